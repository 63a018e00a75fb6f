"""Episode input pipeline on the GPU.

The reference builds every episode tensor on the host, one image at a time
(evaluation_util/data/dataset.py:36-40 `Resize((S,S)) -> ToTensor -> Normalize(0.5,0.5)` on PIL images,
coco.py:36-46 `F.interpolate(nearest)` on the class masks, main_oss.py:100-104 mask -> 3 channels in
{-1,+1} and shots folded into the batch).  At ~80 episodes/s per MI355X that is ~250 bilinear
resizes/s/GPU of PIL work on the critical path.  Here the host only decodes (PIL) and hands over raw
bytes: one pinned staging buffer per batch carries the images, the class masks and Pillow's fixed-point
filter weights (dfw_resample_coeffs) in ONE H2D copy; the resize / normalise / binarise / nearest
kernels (csrc/inputs.hip) run on a side stream while the previous batch is in the UNet, and the
result has exactly the tensor contract of `episodes.make_episode_batch`:

    support_imgs [b*s,3,S,S] fp32 in [-1,1], query_img [b,3,S,S], support_masks [b*s,3,S,S] in {-1,+1},
    query_mask uint8 [b,S,S] in {0,1}, class_id int64 [b]

Values are bit-identical to the reference's host transform (tests/test_preprocess_gpu.py checks them
against PIL / torch themselves).  No CPU fallback: the kernels come from libdiffews_hip.so.

There is one route from bytes to tensors: `InputBatch` / `DeviceImageTransform.batch` turn a whole ragged batch into tensors
with one staging buffer and one dfw_inputs_to_tensor call (three launches whatever the batch); `image()` / `mask()` are a
batch of one.  `support_tensors` builds a support set that way, `EpisodeLoader` whole episodes, and `QueryLoader` (a stream
of queries against one prepared support) what pipeline.segment_queries / segment_classes consume,
`NativeTargets` included; both loaders prefetch through `_Prefetcher`.

`TilePlan` is the host side of tiled segmentation (pipeline.segment_tiled): where the overlapping windows of an image larger
than the processing size lie and how their masks are weighted in the merge (csrc/tiles.hip).
"""
import ctypes as C
import queue
import threading

import numpy as np
import torch

from . import _lib as L


def _align(n, a=16):
    return (n + a - 1) // a * a


_COEF_CACHE = {}


def resample_coeffs(in_size, out_size, filt=L.FILTER_BILINEAR):
    """Pillow's fixed-point weights of one axis, in_size -> out_size, for filter `filt` (L.FILTER_BILINEAR: the input
    side's Resize; L.FILTER_BICUBIC: `Image.resize`'s default, the output side) -> (bounds int32 [out, 2], weights int32
    [out, ksize], ksize).  Cached per (in, out, filter); the arrays are shared, do not write to them."""
    key = (int(in_size), int(out_size), int(filt))
    c = _COEF_CACHE.get(key)
    if c is None:
        lib = L.lib()
        k = lib.dfw_resample_ksize_ex(*key)
        if k <= 0:
            raise ValueError(f"no resample weights for in={in_size} out={out_size} filter={filt}")
        b = np.zeros((key[1], 2), np.int32)
        w = np.zeros((key[1], k), np.int32)
        L.check(lib.dfw_resample_coeffs_ex(*key, b.ctypes.data, w.ctypes.data), "dfw_resample_coeffs_ex")
        c = (b, w, k)
        if len(_COEF_CACHE) < 4096:
            _COEF_CACHE[key] = c
    return c


class DeviceImageTransform:
    """FSSDataset.transform + mask handling for one target size, on `device`.  `size` is the square S of the reference's
    Resize((S, S)) or (out_h, out_w); `self.size` stays the int for a square target and is the pair otherwise.
    device=None: host-only, for `batch`'s layout mode (no GPU needed)."""

    def __init__(self, size, device="cuda"):
        if np.isscalar(size):
            self.out_h = self.out_w = int(size)
        else:
            self.out_h, self.out_w = (int(v) for v in size)
        if self.out_h < 1 or self.out_w < 1:
            raise ValueError(f"target size must be >= 1 x 1, got {size}")
        self.size = self.out_h if self.out_h == self.out_w else (self.out_h, self.out_w)
        self.lib = L.lib()
        # ToTensor + Normalize([0.5],[0.5]) of every byte value, computed by torch (same bits as the reference)
        lut = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
        self.lut = (lut - 0.5) / 0.5
        self.device = None
        if device is not None:
            self.device = torch.device(device)
            if self.device.type == "cuda" and self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            self.lut = self.lut.to(self.device)

    # ---- host side -----------------------------------------------------------------------------
    def coeffs(self, in_size, out_size=None):
        """Pillow's fixed-point bilinear weights for in_size -> out_size (default: out_w); cached, see resample_coeffs."""
        return resample_coeffs(in_size, self.out_w if out_size is None else out_size, L.FILTER_BILINEAR)

    @staticmethod
    def as_rgb_bytes(img):
        """PIL image / ndarray -> contiguous uint8 [H, W, 3] (coco.py:82 `.convert('RGB')`)."""
        if hasattr(img, "convert"):
            img = np.asarray(img.convert("RGB"))
        img = np.ascontiguousarray(img)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("image must be uint8 [H, W, 3] RGB")
        return img

    @staticmethod
    def as_mask(mask):
        mask = np.ascontiguousarray(np.asarray(mask))
        if mask.ndim != 2:
            raise ValueError("mask must be a 2-D class-id map")
        if mask.dtype != np.uint8:
            mask = mask.astype(np.int32)
        return mask

    # ---- device side: one staging buffer, one H2D copy, one library call (three launches); one item = a batch of one
    def image(self, img):
        """-> fp32 [3, out_h, out_w] in [-1, 1]."""
        return self.batch([img])["images"][0]

    def mask(self, mask_ids, class_sample):
        """-> (+-1 fp32 [3,S,S], uint8 {0,1} [S,S]) for class id `class_sample` (coco.py:74-75: the PNG stores it + 1)."""
        r = self.batch([], [mask_ids], [class_sample + 1])
        return r["pm1"][0], r["bin"][0]

    @torch.no_grad()
    def batch(self, images, masks=(), mask_class=(), want_pm1=True, want_bin=True, guard=0, buffers=None):
        """`images` (PIL / uint8 [H, W, 3], any sizes) and class-id maps `masks` (mask j is on where id == mask_class[j])
        -> dict(images fp32 [n, 3, out_h, out_w] or None, pm1 fp32 [m1, 3, out_h, out_w] in +-1 or None, bin uint8
        [m2, out_h, out_w] in 0/1 or None, layout = the InputBatch, staged = the device copy of its bytes).
        want_pm1 / want_bin: one bool or one per mask; pm1 / bin hold the masks that asked for them, in order.  Tables,
        image bytes, weights and mask ids travel in ONE pinned buffer and one H2D copy on the current stream; one
        dfw_inputs_to_tensor call: three launches whatever the batch.  guard / buffers: see InputBatch (tests put
        sentinels around every item).  On a host-only transform (device=None) nothing is launched: returns the
        InputBatch, its bytes staged in the numpy buffer `.host`."""
        lay = InputBatch((self.out_h, self.out_w), [self.as_rgb_bytes(x) for x in images], [self.as_mask(m) for m in masks],
                         mask_class, want_pm1, want_bin, guard=guard)
        if self.device is None:
            lay.host = np.zeros(max(lay.total, 16), np.uint8)
            lay.fill(lay.host)
            return lay
        host = torch.empty(max(lay.total, 16), dtype=torch.uint8, pin_memory=True)
        lay.fill(host.numpy())
        dev = host.to(self.device, non_blocking=True)                       # the one H2D copy
        out = lay.run(dev, self.lut, torch.cuda.current_stream(self.device).cuda_stream, **(buffers or {}))
        out.update(layout=lay, staged=dev)
        return out


class TilePlan:
    """Overlapping windows that cover an image at its own resolution, and the weights of their merge (pure host: no GPU).

    img_hw = (h, w); tile = (th, tw), the processing size (need not be square); overlap = the minimum overlap of
    neighbouring windows in pixels, 0 <= overlap <= min(th, tw) // 2.  Per axis of length L with tile length S: L == S gives
    one window at 0, otherwise n = 1 + ceil((L - S) / (S - overlap)) windows at o_i = (i * (L - S)) // (n - 1) -- the first
    at 0, the last ending at the border, neighbours at most S - overlap apart, no padding anywhere.  L < S is a ValueError
    (pipeline.segment_stream is the route that resizes), as are more than MAX_ORIGINS windows on an axis: the table travels
    by value in the kernel arguments.  Windows are numbered row-major, t = iy * nx + ix, T = ny * nx.

    ramp (default max(1, overlap)), 1 <= ramp <= min(th, tw) // 2: the weight of pixel (dy, dx) of a window is
    min(dy + 1, th - dy, ramp) * min(dx + 1, tw - dx, ramp); ramp = 1 is the plain mean of the windows over a pixel."""
    MAX_ORIGINS = 64

    def __init__(self, img_hw, tile, overlap, ramp=None):
        self.img_h, self.img_w = (int(v) for v in img_hw)
        self.tile_h, self.tile_w = (int(tile), int(tile)) if np.isscalar(tile) else (int(v) for v in tile)
        small = min(self.tile_h, self.tile_w)
        if small < 1:
            raise ValueError(f"tile must be >= 1 x 1, got {tile}")
        self.overlap = int(overlap)
        if not 0 <= self.overlap <= small // 2:
            raise ValueError(f"overlap must be in 0..{small // 2} (half the tile's short side), got {overlap}")
        self.ramp = max(1, self.overlap) if ramp is None else int(ramp)
        if not 1 <= self.ramp <= max(1, small // 2):
            raise ValueError(f"ramp must be in 1..{max(1, small // 2)}, got {ramp}")
        self.ys = self.axis_origins(self.img_h, self.tile_h, self.overlap, "height")
        self.xs = self.axis_origins(self.img_w, self.tile_w, self.overlap, "width")
        self.ny, self.nx = len(self.ys), len(self.xs)
        self.T = self.ny * self.nx

    @classmethod
    def axis_origins(cls, L_, S, overlap, what="axis"):
        if L_ < S:
            raise ValueError(f"image {what} {L_} is smaller than the tile's {S}: tiling never pads or resizes -- use "
                             "segment_stream, the route that resizes the query to the processing size")
        if L_ == S:
            return [0]
        n = 1 + -(-(L_ - S) // (S - overlap))
        if n > cls.MAX_ORIGINS:
            raise ValueError(f"image {what} {L_} needs {n} windows of {S} with overlap {overlap}; at most {cls.MAX_ORIGINS} "
                             "per axis (the table travels in the kernel arguments)")
        return [(i * (L_ - S)) // (n - 1) for i in range(n)]

    def origin(self, t):
        """(y, x) of window t's first pixel."""
        return self.ys[t // self.nx], self.xs[t % self.nx]

    def window_bytes(self, nclass=1):
        """Bytes of the [N, T, 3, th, tw] buffer segment_tiled keeps the windows' seg_u8 in: 3 * th * tw per window and class."""
        return 3 * self.tile_h * self.tile_w * self.T * int(nclass)

    def candidate_table(self, candidates, nsets):
        """The table of ops.tiles_labels_cand for per-window candidate classes: `candidates` is T sequences of set indices,
        the classes window t is segmented against (sorted here; a window may have none, and so may all of them).
        ValueError for a number of lists other than T, a duplicate within a list, an index outside [0, nsets), nsets > 254
        (a label is a byte).  Returns dict(tab int32 [T + 1 + max(E, 1)] = offsets off[0..T] then the class of every
        entry, E = the number of (window, class) entries, sets = the sorted lists, a tuple of tuples)."""
        nsets = int(nsets)
        if not 1 <= nsets <= 254:
            raise ValueError(f"candidate_table: a label is a byte, nsets must be in 1..254, got {nsets}")
        candidates = list(candidates)
        if len(candidates) != self.T:
            raise ValueError(f"candidate_table: {len(candidates)} candidate lists for {self.T} windows")
        sets, off, cls = [], [0], []
        for t, cand in enumerate(candidates):
            cs = sorted(int(c) for c in (cand.tolist() if isinstance(cand, (torch.Tensor, np.ndarray)) else cand))
            for c in cs:
                if not 0 <= c < nsets:
                    raise ValueError(f"candidate_table: window {t} names set {c} of {nsets}")
            if len(set(cs)) != len(cs):
                raise ValueError(f"candidate_table: window {t} names a set twice ({cs})")
            sets.append(tuple(cs))
            cls += cs
            off.append(len(cls))
        E = len(cls)
        return dict(tab=torch.tensor(off + cls + [0] * (max(E, 1) - E), dtype=torch.int32), E=E, sets=tuple(sets))

    def candidates_from_labels(self, label_map, min_pixels=1, margin=0):
        """Per-window candidate lists from a label map of ANY size: label_map uint8 [lh, lw], 0 and 255 ignored, 1 + c =
        class c (a coarse pass' labels, or a ground truth).  Window t's footprint in the map is rows (y0 * lh) // h up to
        ceil((y0 + th) * lh / h) and the columns alike -- at least one pixel, grown by `margin` map pixels on every side,
        clipped to the map; at (lh, lw) = (h, w) and margin 0 it is the window's exact crop.  Returns T lists: the
        ascending classes with at least `min_pixels` pixels inside the footprint."""
        lm = np.asarray(label_map.cpu() if torch.is_tensor(label_map) else label_map)
        if lm.dtype != np.uint8 or lm.ndim != 2 or lm.size == 0:
            raise ValueError(f"candidates_from_labels: label_map must be a non-empty uint8 [lh, lw], got {lm.dtype} {lm.shape}")
        lh, lw = lm.shape
        margin, min_pixels = int(margin), max(1, int(min_pixels))
        if margin < 0:
            raise ValueError(f"candidates_from_labels: margin must be >= 0, got {margin}")

        def span(o, tile, full, n):
            a, b = (o * n) // full, -(-((o + tile) * n) // full)
            b = max(b, a + 1)
            return max(0, a - margin), min(n, b + margin)
        out = []
        for t in range(self.T):
            y0, x0 = self.origin(t)
            ya, yb = span(y0, self.tile_h, self.img_h, lh)
            xa, xb = span(x0, self.tile_w, self.img_w, lw)
            n = np.bincount(lm[ya:yb, xa:xb].ravel(), minlength=256)
            out.append([c - 1 for c in range(1, 255) if n[c] >= min_pixels])
        return out

    def c_struct(self):
        """The dfw_tile_plan of this plan (a fresh ctypes record)."""
        p = L.TilePlan()
        p.img_h, p.img_w, p.tile_h, p.tile_w = self.img_h, self.img_w, self.tile_h, self.tile_w
        p.ny, p.nx, p.ramp = self.ny, self.nx, self.ramp
        p.ys[:self.ny] = self.ys
        p.xs[:self.nx] = self.xs
        return p


class InputBatch:
    """Byte layout of one ragged batch for dfw_inputs_to_tensor: the two item tables (ctypes arrays `img_items` /
    `mask_items`: the host mirrors the library validates) and ONE staging buffer of `total` bytes holding
    [image table][mask table][per image: RGB bytes, x bounds, x weights, y bounds, y weights][per mask: ids].

    out_hw      (out_h, out_w) every item goes to
    images      uint8 [H, W, 3] arrays; masks: 2-D uint8 / int32 class-id maps (DeviceImageTransform.as_rgb_bytes / as_mask)
    mask_class  one int or one per mask: on where id == value
    want_pm1 / want_bin   one bool or one per mask.  A mask that wants neither is staged only (no table item, no
                launch): its bytes travel with the batch for a later reader (QueryLoader's native ground truth).
    guard       bytes left free after every item in tmp / dst / pm1 / bin (tests put sentinels there)

    `mask_src` holds every mask's (byte offset in the staging buffer, element size).  Every staging and tmp offset is
    16-byte aligned.  The outputs are dense tensors: item i of dst lies at i * dst_stride with dst_stride = 12 * out_h *
    out_w (+ guard, rounded up to 16, when guard > 0), pm1 alike, bin with out_h * out_w; they are 16-byte aligned
    whenever out_h * out_w is a multiple of 16."""

    def __init__(self, out_hw, images, masks=(), mask_class=(), want_pm1=True, want_bin=True, guard=0):
        oh, ow = (int(v) for v in out_hw)
        images, masks = list(images), list(masks)
        m = len(masks)
        per = lambda v, what: [v] * m if np.isscalar(v) else _n(list(v), m, what)
        cls = [int(c) for c in per(mask_class if m else 0, "mask_class")]
        pm1 = [bool(v) for v in per(want_pm1, "want_pm1")]
        bn = [bool(v) for v in per(want_bin, "want_bin")]
        self.out_hw, self.guard, self.n_img = (oh, ow), int(guard), len(images)
        used = [j for j in range(m) if pm1[j] or bn[j]]
        self.n_mask = len(used)
        self.img_items = (L.InputImageItem * max(self.n_img, 1))()
        self.mask_items = (L.InputMaskItem * max(self.n_mask, 1))()
        self.img_table_off = 0
        self.mask_table_off = _align(C.sizeof(L.InputImageItem) * self.n_img)
        off = self.mask_table_off + _align(C.sizeof(L.InputMaskItem) * self.n_mask)
        pad = (lambda n: _align(n + self.guard)) if self.guard else (lambda n: n)
        self.dst_stride, self.pm1_stride, self.bin_stride = pad(12 * oh * ow), pad(12 * oh * ow), pad(oh * ow)
        self.parts, tmp = [], 0
        for i, im in enumerate(images):
            H, W = im.shape[:2]
            it = self.img_items[i]
            xb, xw, it.xk = resample_coeffs(W, ow, L.FILTER_BILINEAR)
            yb, yw, it.yk = resample_coeffs(H, oh, L.FILTER_BILINEAR)
            it.H, it.W = H, W
            offs = []
            for arr in (im, xb, xw, yb, yw):
                offs.append(off)
                self.parts.append((off, arr))
                off = _align(off + arr.nbytes)
            it.src_off, it.xb_off, it.xc_off, it.yb_off, it.yc_off = offs
            it.tmp_off, it.dst_off = tmp, i * self.dst_stride
            tmp = _align(tmp + 3 * H * ow + self.guard)
        self.mask_src, self.pm1_index, self.bin_index = [], [], []
        for j, mk in enumerate(masks):
            self.mask_src.append((off, mk.dtype.itemsize))
            self.parts.append((off, mk))
            if pm1[j] or bn[j]:
                it = self.mask_items[used.index(j)]
                it.H, it.W, it.elem, it.class_value, it.src_off = mk.shape[0], mk.shape[1], mk.dtype.itemsize, cls[j], off
                it.pm1_off = len(self.pm1_index) * self.pm1_stride if pm1[j] else -1
                it.bin_off = len(self.bin_index) * self.bin_stride if bn[j] else -1
                if pm1[j]:
                    self.pm1_index.append(j)
                if bn[j]:
                    self.bin_index.append(j)
            off = _align(off + mk.nbytes)
        self.total, self.tmp_bytes = off, tmp
        self.dst_bytes = self.n_img * self.dst_stride
        self.pm1_bytes = len(self.pm1_index) * self.pm1_stride
        self.bin_bytes = len(self.bin_index) * self.bin_stride
        self.host = None

    def fill(self, hv):
        """Write the tables and every staged array into the numpy uint8 view `hv` (>= total bytes)."""
        if self.n_img:
            n = C.sizeof(L.InputImageItem) * self.n_img
            hv[:n] = np.frombuffer(self.img_items, dtype=np.uint8)[:n]
        if self.n_mask:
            n = C.sizeof(L.InputMaskItem) * self.n_mask
            hv[self.mask_table_off:self.mask_table_off + n] = np.frombuffer(self.mask_items, dtype=np.uint8)[:n]
        for off, arr in self.parts:
            hv[off:off + arr.nbytes] = arr.reshape(-1).view(np.uint8)

    def args(self, staged, staged_bytes, lut, tmp=(None, 0), dst=(None, 0), pm1=(None, 0), bin=(None, 0)):
        """The dfw_inputs_args of this batch for base addresses given as (address, bytes) pairs."""
        a = L.InputsArgs()
        a.image_items, a.image_items_host, a.n_img = staged + self.img_table_off, C.addressof(self.img_items), self.n_img
        a.mask_items, a.mask_items_host, a.n_mask = staged + self.mask_table_off, C.addressof(self.mask_items), self.n_mask
        a.out_h, a.out_w = self.out_hw
        a.staged, a.staged_bytes, a.lut = staged, staged_bytes, lut
        (a.tmp, a.tmp_bytes), (a.dst, a.dst_bytes), (a.pm1, a.pm1_bytes), (a.bin, a.bin_bytes) = tmp, dst, pm1, bin
        return a

    def run(self, staged, lut, stream, tmp=None, dst=None, pm1=None, bin=None):
        """One dfw_inputs_to_tensor call on `stream` over `staged` (uint8 device tensor holding fill()'s bytes from its
        start).  tmp / dst / pm1 / bin: caller-owned contiguous uint8 device buffers of at least tmp_bytes / dst_bytes /
        pm1_bytes / bin_bytes (fresh ones otherwise).  Returns dict(images, pm1, bin): strided views of those buffers,
        None where the batch has nothing of the kind."""
        dev, (oh, ow) = staged.device, self.out_hw
        if self.n_img + self.n_mask == 0:
            return dict(images=None, pm1=None, bin=None)

        def buf(given, n):
            if n == 0:
                return None
            if given is None:
                return torch.empty(n, dtype=torch.uint8, device=dev)
            assert given.dtype == torch.uint8 and given.is_contiguous() and given.numel() >= n and given.device == dev
            return given
        tmp, dst, pm1, bin = buf(tmp, self.tmp_bytes), buf(dst, self.dst_bytes), buf(pm1, self.pm1_bytes), buf(bin, self.bin_bytes)
        pair = lambda t: (None, 0) if t is None else (t.data_ptr(), t.numel())
        a = self.args(staged.data_ptr(), staged.numel(), lut.data_ptr(), pair(tmp), pair(dst), pair(pm1), pair(bin))
        L.check(L.lib().dfw_inputs_to_tensor(C.byref(a), stream), "dfw_inputs_to_tensor")

        def planes(t, n, stride):
            if t is None:
                return None
            f = t[:n * stride].view(torch.float32)
            return f.as_strided((n, 3, oh, ow), (stride // 4, oh * ow, ow, 1))
        bins = None
        if bin is not None:
            bins = bin.as_strided((len(self.bin_index), oh, ow), (self.bin_stride, ow, 1))
        return dict(images=planes(dst, self.n_img, self.dst_stride),
                    pm1=planes(pm1, len(self.pm1_index), self.pm1_stride), bin=bins)


def _n(v, n, what):
    if len(v) != n:
        raise ValueError(f"{what} must be one value or one per mask ({n}), got {len(v)}")
    return v


@torch.no_grad()
def support_tensors(images, class_maps, class_values, size, device="cuda"):
    """n annotated examples -- decoded images of any sizes, their class-id maps and the id (one int, or one per example)
    that marks the object -- -> (support_imgs fp32 [n, 3, S, S] in [-1, 1], support_masks fp32 [n, 3, S, S] in +-1)
    through DeviceImageTransform.batch: one H2D copy and three launches for the whole set.  Feed them to
    pipeline.prepare_support, or to prepare_support_classes after a view to [N, s, 3, S, S] (classes of different
    sizes: after a split into N tensors [s_c, 3, S, S])."""
    images, class_maps = list(images), list(class_maps)
    if not images or len(images) != len(class_maps):
        raise ValueError("support_tensors needs as many class-id maps as images, and at least one")
    r = DeviceImageTransform(size, device).batch(images, class_maps, class_values, want_pm1=True, want_bin=False)
    return r["images"], r["pm1"]


class NativeTargets:
    """Per-query native sizes (and ground truth) of one ragged batch, staged for ops.seg_native: the dfw_native_item
    table, Pillow's bicubic weights of every axis and -- when given as host arrays -- the ground truth, laid out in ONE
    pinned buffer and copied to `device` in one H2D copy on the current stream.

    src_hw       (Hs, Ws) of the seg_u8 the batch will be resized from
    sizes        [(h, w)] per query
    gt           optional list of host arrays [h, w], uint8 or integer (staged as int32): 0/1 masks with 255 = ignore, or
                 class-id maps
    gt_device    instead of gt: (uint8 device tensor, [byte offset per query], [element size 1 | 4 per query]) -- ground
                 truth already on the device (the EpisodeLoader's staged class-id maps); the tensor is kept alive here
    class_value  int or one per query: foreground where id == class_value (1 for a 0/1 mask; coco.py:74-75)
    ignore_value pixels with this id are dropped from the counts; -1 = none, 255 = PASCAL's boundary (pascal.py)
    guard        bytes left free after every image in tmp and the packed outputs (tests put sentinels there)
    device=None  builds the host layout only (`host` is then a numpy buffer): no GPU needed.

    All offsets are 16-byte aligned.  tmp / out_u8 / pred are not allocated here: ops.seg_native sizes them from
    tmp_bytes / u8_bytes / pred_bytes."""

    def __init__(self, src_hw, sizes, gt=None, gt_device=None, class_value=1, ignore_value=-1, device="cuda", guard=0):
        Hs, Ws = (int(v) for v in src_hw)
        sizes = [(int(h), int(w)) for h, w in sizes]
        b = len(sizes)
        if b < 1 or Hs < 1 or Ws < 1:
            raise ValueError("NativeTargets needs at least one query and a positive source size")
        if any(h < 1 or w < 1 for h, w in sizes):
            raise ValueError(f"native sizes must be >= 1 x 1, got {sizes}")
        if gt is not None and gt_device is not None:
            raise ValueError("give the ground truth either as host arrays (gt) or as staged device bytes (gt_device)")
        cls = [int(class_value)] * b if np.isscalar(class_value) else [int(c) for c in class_value]
        if len(cls) != b:
            raise ValueError("class_value must be one int or one per query")
        if gt is not None:
            if len(gt) != b:
                raise ValueError("gt must hold one array per query")
            gt = [DeviceImageTransform.as_mask(g) for g in gt]
            for g, hw in zip(gt, sizes):
                if g.shape != hw:
                    raise ValueError(f"ground truth of shape {g.shape} for a query of native size {hw}")
        self.src_hw, self.sizes, self.b, self.guard = (Hs, Ws), sizes, b, int(guard)
        self.items = (L.NativeItem * b)()          # host mirror: what dfw_seg_native validates
        off, parts = _align(C.sizeof(self.items)), []
        tmp = u8 = pr = 0
        for i, (h, w) in enumerate(sizes):
            it = self.items[i]
            xb, xw, it.xk = resample_coeffs(Ws, w, L.FILTER_BICUBIC)
            yb, yw, it.yk = resample_coeffs(Hs, h, L.FILTER_BICUBIC)
            it.h, it.w = h, w
            offs = []
            for arr in (xb, xw, yb, yw):
                offs.append(off)
                parts.append((off, arr))
                off = _align(off + arr.nbytes)
            it.xb_off, it.xc_off, it.yb_off, it.yc_off = offs
            it.tmp_off, it.u8_off, it.pred_off = tmp, u8, pr
            tmp = _align(tmp + 3 * Hs * w + self.guard)
            u8 = _align(u8 + 3 * h * w + self.guard)
            pr = _align(pr + h * w + self.guard)
            it.gt_elem, it.class_value, it.ignore_value = 1, cls[i], int(ignore_value)
        self.tmp_bytes, self.u8_bytes, self.pred_bytes = tmp, u8, pr
        self.has_gt = gt is not None or gt_device is not None
        self._gt_keep = None
        if gt is not None:
            for it, g in zip(self.items, gt):
                it.gt_off, it.gt_elem = off, g.dtype.itemsize
                parts.append((off, g))
                off = _align(off + g.nbytes)
        self.total = off
        if gt_device is not None:
            buf, offs, elems = gt_device
            if buf.dtype != torch.uint8 or not buf.is_contiguous() or len(offs) != b or len(elems) != b:
                raise ValueError("gt_device = (contiguous uint8 device tensor, b byte offsets, b element sizes)")
            for it, o, e in zip(self.items, offs, elems):
                if e not in (1, 4) or o < 0 or o + it.h * it.w * e > buf.numel():
                    raise ValueError("staged ground truth leaves its buffer or has an element size other than 1 / 4")
                it.gt_off, it.gt_elem = int(o), int(e)
            self._gt_keep = buf
        if device is None:
            self.device, self.dev = None, None
            self.host = np.zeros(self.total, np.uint8)
            hv = self.host
        else:
            self.device = torch.device(device)
            self.host = torch.empty(self.total, dtype=torch.uint8, pin_memory=True)
            hv = self.host.numpy()
        hv[:C.sizeof(self.items)] = np.frombuffer(self.items, dtype=np.uint8)
        for o, arr in parts:
            hv[o:o + arr.nbytes] = arr.reshape(-1).view(np.uint8)
        if device is not None:
            self.dev = self.host.to(self.device, non_blocking=True)     # the one H2D copy

    @property
    def gt_base(self):
        """(device tensor the gt offsets refer to, its bytes) or (None, 0)."""
        if not self.has_gt:
            return None, 0
        buf = self._gt_keep if self._gt_keep is not None else self.dev
        return buf, buf.numel()


class _Prefetcher:
    """Host items -> device batches, prefetched on a side stream: everything EpisodeLoader and QueryLoader share.

    A producer thread (`self._thread`) draws `batch` items at a time (the last batch may be short), lays them out as one
    InputBatch and stages it in one of depth + 2 slots -- one with the consumer, `depth` queued, one being staged: one
    pinned buffer, one H2D copy and one dfw_inputs_to_tensor call on the side stream.  A slot owns its staging (`host`,
    `dev`), scratch (`tmp`) and output (`dst`, `pm1`, `bin`) buffers; the outputs are sized once for a full batch, the
    others grow on demand.  Three events order a slot's reuse:
      copied   the H2D copy has left the pinned bytes: the producer waits for it ON THE CPU before refilling them
      release  the consumer's work on the slot's previous batch: the side stream waits for it before overwriting
      event    the batch is complete: the consumer's stream waits for it before the batch is handed out
    So a batch's tensors stay valid for the work enqueued on the consumer's stream before the NEXT batch is drawn.
    The producer allocates slots and pinned buffers and synchronises `copied` while the consumer may be capturing a
    graph: that is why pipeline._replay captures with capture_error_mode="thread_local".

    A subclass says how items become an InputBatch (`_plan`), how many outputs of each kind a full batch has (`_outputs`),
    what NativeTargets go with a batch (`_native`) and what is yielded (`_result`).  device=None: host-only, for
    `host_batch` (no GPU needed); such a loader does not iterate."""

    def __init__(self, src, size, batch, device, depth):
        self.src, self.b, self.depth = src, int(batch), int(depth)
        if self.b < 1 or self.depth < 1:
            raise ValueError(f"{type(self).__name__} needs batch >= 1 and depth >= 1")
        self.tf = DeviceImageTransform(size, device)
        self.device = self.tf.device
        self.stream = None if self.device is None else torch.cuda.Stream(device=self.device)
        self._slots = [None] * (self.depth + 2)
        self._thread = None

    def host_batch(self, items):
        """Host-only layout of one batch of source dicts: (InputBatch with its bytes in the numpy buffer `.host`,
        NativeTargets(device=None) whose gt offsets refer to that buffer)."""
        lay, ctx = self._plan(items)
        lay.host = np.zeros(max(lay.total, 16), np.uint8)
        lay.fill(lay.host)
        return lay, self._native(lay, ctx, torch.from_numpy(lay.host), None)

    def _slot(self, i, lay):
        s = self._slots[i]
        if s is None:
            plane = self.tf.out_h * self.tf.out_w
            s = dict(host=None, dev=None, tmp=None, event=torch.cuda.Event(), release=torch.cuda.Event(), released=False,
                     copied=torch.cuda.Event(), staged=False)
            for name, n in zip(("dst", "pm1", "bin"), self._outputs()):
                nbytes = n * plane * (1 if name == "bin" else 12)
                s[name] = torch.empty(nbytes, dtype=torch.uint8, device=self.device) if n else None
            self._slots[i] = s
        if s["host"] is None or s["host"].numel() < lay.total:
            if s["dev"] is not None:
                s["dev"].record_stream(self.stream)   # still read by kernels queued on the side stream
            s["host"] = torch.empty(int(lay.total * 1.25) + 64, dtype=torch.uint8, pin_memory=True)
            s["dev"] = torch.empty(s["host"].numel(), dtype=torch.uint8, device=self.device)
        if s["tmp"] is None or s["tmp"].numel() < lay.tmp_bytes:
            if s["tmp"] is not None:
                s["tmp"].record_stream(self.stream)
            s["tmp"] = torch.empty(int(lay.tmp_bytes * 1.25), dtype=torch.uint8, device=self.device)
        return s

    def _stage(self, i, items, index):
        """Decode-side work for one batch (runs in the producer thread): pack, copy, launch."""
        lay, ctx = self._plan(items)
        sl = self._slot(i, lay)
        if sl["staged"]:
            # The H2D copy of this slot's PREVIOUS batch reads the same pinned bytes asynchronously; stream
            # waits order GPU work only, and a consumer that never synchronises lets this thread run several
            # batches ahead of the GPU.  Block here (CPU) until that copy has left the host buffer.
            sl["copied"].synchronize()
        lay.fill(sl["host"].numpy())
        with torch.cuda.stream(self.stream):
            if sl["released"]:          # the consumer's work on this buffer set's previous batch
                self.stream.wait_event(sl["release"])
            sl["dev"][:lay.total].copy_(sl["host"][:lay.total], non_blocking=True)
            sl["copied"].record(self.stream)
            sl["staged"] = True
            r = lay.run(sl["dev"], self.tf.lut, self.stream.cuda_stream, tmp=sl["tmp"], dst=sl["dst"], pm1=sl["pm1"],
                        bin=sl["bin"])
            out = self._result(items, index, lay, ctx, r, sl["dev"])    # may stage NativeTargets: on the side stream too
            sl["event"].record(self.stream)
        out["_slot"] = sl
        return out

    def __iter__(self):
        if self.device is None:
            raise RuntimeError(f"a host-only {type(self).__name__} (device=None) lays batches out (host_batch) only")
        q = queue.Queue(maxsize=self.depth)
        stop = threading.Event()
        nslots = self.depth + 2

        def put(out):           # every put gives up once the consumer has left: the thread ends, the slots go
            while not stop.is_set():
                try:
                    q.put(out, timeout=0.1)
                    return
                except queue.Full:
                    continue

        def produce():
            try:
                torch.cuda.set_device(self.device)
                buf, i, pos = [], 0, 0
                for e in self.src:
                    if stop.is_set():
                        return
                    buf.append(e)
                    if len(buf) == self.b:
                        put(self._stage(i % nslots, buf, range(pos, pos + len(buf))))
                        buf, i, pos = [], i + 1, pos + self.b
                if buf and not stop.is_set():
                    put(self._stage(i % nslots, buf, range(pos, pos + len(buf))))
                put(None)
            except BaseException as ex:  # surfaced in the consumer
                put(ex)

        self._thread = threading.Thread(target=produce, daemon=True)
        self._thread.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                sl = item.pop("_slot")
                torch.cuda.current_stream(self.device).wait_event(sl["event"])
                yield item
                # the generator resumes here when the NEXT batch is drawn: everything the consumer has enqueued on this
                # batch since lies before the event the side stream waits for before it overwrites the slot
                sl["release"].record(torch.cuda.current_stream(self.device))
                sl["released"] = True
        finally:
            stop.set()


class EpisodeLoader(_Prefetcher):
    """Host episodes -> device batches, prefetched on a side stream (protocol and buffer lifetime: _Prefetcher).

    `episodes` yields dicts with the raw material of DatasetCOCO.load_frame (coco.py:77-107):
        query_img, support_imgs (list): PIL images or uint8 [H,W,3] arrays
        query_mask, support_masks (list): class-id maps [H,W] (uint8 / int)
        class_id: the sampled class (masks hold class_id + 1)
    Iterating yields dicts like episodes.make_episode_batch plus `class_id` [b]: views of the slot's buffers, the first
    b * nshot images the supports (episode * nshot + shot), the rest the queries.

    native=True: every batch also carries `native`, a NativeTargets for pipeline.run_episodes(native=...) /
    ops.seg_native: each query's own h x w, its class id + 1 as the foreground value, `ignore_value` (-1: none, 255:
    PASCAL's boundary) and, as ground truth, the query's raw class-id map where it already sits in this batch's staged
    bytes -- no second copy, so `native` is valid exactly as long as the batch's tensors are.
    """

    def __init__(self, episodes, size, batch, nshot, device="cuda", depth=2, native=False, ignore_value=-1):
        super().__init__(episodes, size, batch, device, depth)
        self.s, self.native, self.ignore_value = int(nshot), bool(native), int(ignore_value)

    def layout(self, eps):
        """The InputBatch of one batch of episode dicts: support images (episode * nshot + shot) then query images; masks
        in the same order, on where id == class_id + 1, the supports' to +-1 planes, the queries' to 0/1 bytes."""
        tf, n_sup = self.tf, len(eps) * self.s
        for e in eps:
            if len(e["support_imgs"]) != self.s or len(e["support_masks"]) != self.s:
                raise ValueError("episode does not hold nshot support images / masks")
        images = [tf.as_rgb_bytes(x) for e in eps for x in e["support_imgs"]] + [tf.as_rgb_bytes(e["query_img"]) for e in eps]
        masks = [tf.as_mask(m) for e in eps for m in e["support_masks"]] + [tf.as_mask(e["query_mask"]) for e in eps]
        cls = [int(e["class_id"]) + 1 for e in eps for _ in range(self.s)] + [int(e["class_id"]) + 1 for e in eps]
        sup = [True] * n_sup + [False] * len(eps)
        return InputBatch((tf.out_h, tf.out_w), images, masks, cls, want_pm1=sup, want_bin=[not v for v in sup])

    def _plan(self, eps):
        return self.layout(eps), None

    def _outputs(self):
        return self.b * (self.s + 1), self.b * self.s, self.b

    def _native(self, lay, ctx, staged, device):
        nb = len(lay.bin_index)                         # the queries: last among the images and among the maps
        imgs, maps = lay.img_items[lay.n_img - nb:lay.n_img], lay.mask_items[lay.n_mask - nb:lay.n_mask]
        for im, m in zip(imgs, maps):
            if (im.H, im.W) != (m.H, m.W):
                raise ValueError(f"query image {(im.H, im.W)} and query mask {(m.H, m.W)} differ in size")
        return NativeTargets(lay.out_hw, [(m.H, m.W) for m in maps], gt_device=(staged, *zip(*lay.mask_src[-nb:])),
                             class_value=[m.class_value for m in maps], ignore_value=self.ignore_value, device=device)

    def _result(self, eps, index, lay, ctx, r, staged):
        n_sup = len(eps) * self.s
        out = dict(support_imgs=r["images"][:n_sup], query_img=r["images"][n_sup:], support_masks=r["pm1"],
                   query_mask=r["bin"], class_id=torch.tensor([int(e["class_id"]) for e in eps], dtype=torch.long))
        if self.native:
            out["native"] = self._native(lay, ctx, staged, self.device)
        return out


class QueryLoader(_Prefetcher):
    """Host queries -> device batches for pipeline.segment_queries / segment_classes, prefetched on a side stream
    (protocol and buffer lifetime: _Prefetcher): the input half of "segment a stream of images against the same few
    annotated examples".

    `queries` yields dicts with
        query_img: PIL image or uint8 [H, W, 3] array, any size
        gt (optional): class-id map or label map [H, W] (uint8 / int) of the same size; all queries of a batch carry
                       one, or none does
    Iterating yields dicts with
        query_img  fp32 [b, 3, out_h, out_w] in [-1, 1]
        native     NativeTargets for the b queries' own sizes; with `gt` its ground truth is read IN PLACE from the
                   batch's staged bytes (gt_device: no second copy), with `ignore_value` (-1: none, 255: PASCAL's
                   boundary) and the query's class value as foreground (1 without class_value); without `gt` it carries
                   sizes only and the native counts are None
        query_mask (only with class_value and gt) uint8 [b, out_h, out_w]: gt == class value, nearest-resized, so
                   r["counts"] at the processing size works too
        index      positions of the batch's queries in the stream (list of int)
        route      (only with `route`) the set index of each of the batch's queries (list of int), for
                   pipeline.segment_routed
        candidates (only with `candidates`) the candidate set indices of each of the batch's queries (list of lists), for
                   pipeline.segment_candidates; then also
        query_labels (only when every query of the batch carries `labels`) uint8 HOST tensor [b, out_h, out_w]: the
                   queries' label maps, which are already at the processing size (ValueError for another size, or when
                   only some queries of a batch carry one)
    class_value: one int, or a callable on the query dict.
    route: a callable on the query dict that gives the index of the support set the query goes to.
    candidates: a callable on the query dict that gives the indices of the support sets the query is segmented against.
    """

    def __init__(self, queries, size, batch, device="cuda", depth=2, class_value=None, ignore_value=-1, route=None,
                 candidates=None):
        super().__init__(queries, size, batch, device, depth)
        self.class_value, self.ignore_value, self.route = class_value, int(ignore_value), route
        self.candidates = candidates

    def layout(self, qs):
        """(InputBatch, per-query class values, has_gt) of one batch of query dicts: the images, then the ground-truth
        maps -- with class_value each also a mask item with a 0/1 destination, without it staged only."""
        tf = self.tf
        images = [tf.as_rgb_bytes(q["query_img"]) for q in qs]
        with_gt = [q.get("gt") is not None for q in qs]
        if any(with_gt) and not all(with_gt):
            raise ValueError("either every query of a batch carries `gt` or none does")
        gts, cls = [], [1] * len(qs)
        if all(with_gt):
            gts = [tf.as_mask(q["gt"]) for q in qs]
            for im, g in zip(images, gts):
                if im.shape[:2] != g.shape:
                    raise ValueError(f"query image {im.shape[:2]} and its gt {g.shape} differ in size")
            if self.class_value is not None:
                cls = [int(self.class_value(q)) if callable(self.class_value) else int(self.class_value) for q in qs]
        want_bin = self.class_value is not None
        lay = InputBatch((tf.out_h, tf.out_w), images, gts, cls if gts else (), want_pm1=False, want_bin=want_bin)
        return lay, cls, bool(gts)

    def _plan(self, qs):
        lay, cls, has_gt = self.layout(qs)
        return lay, (cls, has_gt)

    def _outputs(self):
        return self.b, 0, self.b if self.class_value is not None else 0

    def _native(self, lay, ctx, staged, device):
        cls, has_gt = ctx
        gt_device = (staged, *zip(*lay.mask_src)) if has_gt else None
        return NativeTargets(lay.out_hw, [(it.H, it.W) for it in lay.img_items[:lay.n_img]], gt_device=gt_device,
                             class_value=cls, ignore_value=self.ignore_value, device=device)

    def _result(self, qs, index, lay, ctx, r, staged):
        out = dict(query_img=r["images"], native=self._native(lay, ctx, staged, self.device), index=list(index))
        if r["bin"] is not None:
            out["query_mask"] = r["bin"]
        if self.route is not None:
            out["route"] = [int(self.route(q)) for q in qs]
        if self.candidates is not None:
            out["candidates"] = [[int(c) for c in self.candidates(q)] for q in qs]
            have = [q.get("labels") is not None for q in qs]
            if any(have) and not all(have):
                raise ValueError("either every query of a batch carries `labels` or none does")
            if all(have):
                maps = [torch.as_tensor(np.asarray(q["labels"])).to(torch.uint8) for q in qs]
                for m in maps:
                    if tuple(m.shape) != (self.tf.out_h, self.tf.out_w):
                        raise ValueError(f"`labels` is a label map at the processing size {(self.tf.out_h, self.tf.out_w)}, "
                                         f"got {tuple(m.shape)}")
                out["query_labels"] = torch.stack(maps)
        return out
