"""Episode input pipeline on the GPU.

The reference builds every episode tensor on the host, one image at a time
(evaluation_util/data/dataset.py:36-40 `Resize((S,S)) -> ToTensor -> Normalize(0.5,0.5)` on PIL images,
coco.py:36-46 `F.interpolate(nearest)` on the class masks, main_oss.py:100-104 mask -> 3 channels in
{-1,+1} and shots folded into the batch).  At ~80 episodes/s per MI355X that is ~250 bilinear
resizes/s/GPU of PIL work on the critical path.  Here the host only decodes (PIL) and hands over raw
bytes: one pinned staging buffer per batch carries the images, the class masks and Pillow's fixed-point
filter weights (dfw_resample_coeffs) in ONE H2D copy; the resize / normalise / binarise / nearest
kernels (csrc/preprocess.hip) run on a side stream while the previous batch is in the UNet, and the
result has exactly the tensor contract of `episodes.make_episode_batch`:

    support_imgs [b*s,3,S,S] fp32 in [-1,1], query_img [b,3,S,S], support_masks [b*s,3,S,S] in {-1,+1},
    query_mask uint8 [b,S,S] in {0,1}, class_id int64 [b]

Values are bit-identical to the reference's host transform (tests/test_preprocess_gpu.py checks them
against PIL / torch themselves).  No CPU fallback: the kernels come from libdiffews_hip.so.
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
    """FSSDataset.transform + mask handling for one target size, on `device`."""

    def __init__(self, size, device="cuda"):
        self.size = int(size)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = L.lib()
        # ToTensor + Normalize([0.5],[0.5]) of every byte value, computed by torch (same bits as the reference)
        lut = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
        self.lut = ((lut - 0.5) / 0.5).to(self.device)

    # ---- host side -----------------------------------------------------------------------------
    def coeffs(self, in_size):
        """Pillow's fixed-point bilinear weights for in_size -> self.size (cached, see resample_coeffs)."""
        return resample_coeffs(in_size, self.size, L.FILTER_BILINEAR)

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

    def plan(self, images, masks):
        """Byte layout of one staging buffer: [(image, xb, xw, yb, yw) ...][mask ...] -> (items, total)."""
        off, items = 0, []
        for im in images:
            H, W = im.shape[:2]
            xb, xw, xk = self.coeffs(W)
            yb, yw, yk = self.coeffs(H)
            parts = []
            for arr in (im, xb, xw, yb, yw):
                parts.append((off, arr))
                off = _align(off + arr.nbytes)
            items.append(("image", H, W, xk, yk, parts))
        for m in masks:
            items.append(("mask", m.shape[0], m.shape[1], m.dtype.itemsize, 0, [(off, m)]))
            off = _align(off + m.nbytes)
        return items, off

    # ---- device side ---------------------------------------------------------------------------
    def launch(self, items, dev_base, img_out, tmp, mask_pm1, mask_bin, mask_class, stream):
        """Kernels for a staged batch: image i -> img_out[i]; mask j -> mask_pm1[j] / mask_bin[j] (either
        may be None per entry)."""
        S, ii, mi = self.size, 0, 0
        for kind, H, W, a, b, parts in items:
            if kind == "image":
                args = L.ImageArgs()
                p = [dev_base + o for o, _ in parts]
                args.src, args.H, args.W, args.out_h, args.out_w = p[0], H, W, S, S
                args.xbounds, args.xcoef, args.xk = p[1], p[2], a
                args.ybounds, args.ycoef, args.yk = p[3], p[4], b
                args.tmp, args.dst, args.lut = tmp.data_ptr(), img_out[ii].data_ptr(), self.lut.data_ptr()
                L.check(self.lib.dfw_image_to_tensor(C.byref(args), stream), "dfw_image_to_tensor")
                ii += 1
            else:
                pm1, bn = mask_pm1[mi], mask_bin[mi]
                L.check(self.lib.dfw_mask_to_tensor(dev_base + parts[0][0], a, H, W, int(mask_class[mi]), S, S,
                                                    pm1.data_ptr() if pm1 is not None else None,
                                                    bn.data_ptr() if bn is not None else None, stream),
                        "dfw_mask_to_tensor")
                mi += 1

    # ---- one-shot convenience (tests, single images) ---------------------------------------------
    @torch.no_grad()
    def image(self, img):
        im = self.as_rgb_bytes(img)
        out = torch.empty(1, 3, self.size, self.size, dtype=torch.float32, device=self.device)
        self._run([im], [], out, [], [], [])
        return out[0]

    @torch.no_grad()
    def mask(self, mask_ids, class_sample):
        """-> (+-1 fp32 [3,S,S], uint8 {0,1} [S,S]) for class id `class_sample` (coco.py:74-75: the
        PNG stores class_sample + 1)."""
        m = self.as_mask(mask_ids)
        pm1 = torch.empty(3, self.size, self.size, dtype=torch.float32, device=self.device)
        bn = torch.empty(self.size, self.size, dtype=torch.uint8, device=self.device)
        self._run([], [m], None, [pm1], [bn], [class_sample + 1])
        return pm1, bn

    def _run(self, images, masks, img_out, mask_pm1, mask_bin, mask_class):
        items, total = self.plan(images, masks)
        host = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
        fill_staging(host, items)
        dev = host.to(self.device, non_blocking=True)
        hmax = max([im.shape[0] for im in images], default=1)
        tmp = torch.empty(hmax * self.size * 3, dtype=torch.uint8, device=self.device)
        self.launch(items, dev.data_ptr(), img_out, tmp, mask_pm1, mask_bin, mask_class,
                    torch.cuda.current_stream().cuda_stream)


def fill_staging(host, items):
    hv = host.numpy()
    for _, _, _, _, _, parts in items:
        for off, arr in parts:
            hv[off:off + arr.nbytes] = arr.reshape(-1).view(np.uint8)


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


class EpisodeLoader:
    """Host episodes -> device batches, prefetched on a side stream.

    `episodes` yields dicts with the raw material of DatasetCOCO.load_frame (coco.py:77-107):
        query_img, support_imgs (list): PIL images or uint8 [H,W,3] arrays
        query_mask, support_masks (list): class-id maps [H,W] (uint8 / int)
        class_id: the sampled class (masks hold class_id + 1)
    Iterating yields dicts like episodes.make_episode_batch plus `class_id` [b].  A batch's tensors are
    recycled: they stay valid for the work enqueued on the consumer's stream before the NEXT batch is
    drawn (the producer's side stream waits on an event recorded at that point before overwriting).
    depth + 2 buffer sets: one with the consumer, `depth` queued, one being staged.

    native=True: every batch also carries `native`, a NativeTargets for pipeline.run_episodes(native=...) /
    ops.seg_native: each query's own h x w, its class id + 1 as the foreground value, `ignore_value` (-1: none, 255:
    PASCAL's boundary) and, as ground truth, the query's raw class-id map where it already sits in this batch's staged
    bytes -- no second copy, so `native` is valid exactly as long as the batch's tensors are.
    """

    def __init__(self, episodes, size, batch, nshot, device="cuda", depth=2, native=False, ignore_value=-1):
        self.src, self.b, self.s, self.depth = episodes, int(batch), int(nshot), int(depth)
        self.native, self.ignore_value = bool(native), int(ignore_value)
        self.tf = DeviceImageTransform(size, device)
        self.device = self.tf.device
        self.stream = torch.cuda.Stream(device=self.device)
        self._slots = [None] * (self.depth + 2)

    def _slot(self, i, total, hmax, nb):
        S, dev, s = self.tf.size, self.device, self._slots[i]
        if s is None or s["b"] != nb:
            s = dict(b=nb, host=None, dev=None, tmp=None,
                     sup=torch.empty(nb * self.s, 3, S, S, dtype=torch.float32, device=dev),
                     qry=torch.empty(nb, 3, S, S, dtype=torch.float32, device=dev),
                     smask=torch.empty(nb * self.s, 3, S, S, dtype=torch.float32, device=dev),
                     qmask=torch.empty(nb, S, S, dtype=torch.uint8, device=dev),
                     event=torch.cuda.Event(), release=torch.cuda.Event(), released=False,
                     copied=torch.cuda.Event(), staged=False)
            self._slots[i] = s
        if s["host"] is None or s["host"].numel() < total:
            if s["dev"] is not None:
                s["dev"].record_stream(self.stream)   # still read by kernels queued on the side stream
            s["host"] = torch.empty(int(total * 1.25) + 64, dtype=torch.uint8, pin_memory=True)
            s["dev"] = torch.empty(s["host"].numel(), dtype=torch.uint8, device=self.device)
        need = hmax * S * 3
        if s["tmp"] is None or s["tmp"].numel() < need:
            if s["tmp"] is not None:
                s["tmp"].record_stream(self.stream)
            s["tmp"] = torch.empty(int(need * 1.25), dtype=torch.uint8, device=self.device)
        return s

    def _stage(self, i, eps):
        """Decode-side work for one batch (runs in the producer thread): pack, copy, launch."""
        tf, nb = self.tf, len(eps)
        images, masks, mclass, pm1, bins = [], [], [], [], []
        for e in eps:                                   # support images batch-major episode*nshot + shot
            if len(e["support_imgs"]) != self.s or len(e["support_masks"]) != self.s:
                raise ValueError("episode does not hold nshot support images / masks")
            images += [tf.as_rgb_bytes(x) for x in e["support_imgs"]]
        images += [tf.as_rgb_bytes(e["query_img"]) for e in eps]
        for e in eps:
            masks += [tf.as_mask(m) for m in e["support_masks"]]
            mclass += [int(e["class_id"]) + 1] * self.s
        masks += [tf.as_mask(e["query_mask"]) for e in eps]
        mclass += [int(e["class_id"]) + 1 for e in eps]
        items, total = tf.plan(images, masks)
        sl = self._slot(i, total, max(im.shape[0] for im in images), nb)
        if sl["staged"]:
            # The H2D copy of this slot's PREVIOUS batch reads the same pinned bytes asynchronously; stream
            # waits order GPU work only, and a consumer that never synchronises lets this thread run several
            # batches ahead of the GPU.  Block here (CPU) until that copy has left the host buffer.
            sl["copied"].synchronize()
        fill_staging(sl["host"], items)
        n_sup = nb * self.s
        img_out = [sl["sup"][j] for j in range(n_sup)] + [sl["qry"][j] for j in range(nb)]
        pm1 = [sl["smask"][j] for j in range(n_sup)] + [None] * nb
        bins = [None] * n_sup + [sl["qmask"][j] for j in range(nb)]
        with torch.cuda.stream(self.stream):
            if sl["released"]:          # the consumer's work on this buffer set's previous batch
                self.stream.wait_event(sl["release"])
            sl["dev"][:total].copy_(sl["host"][:total], non_blocking=True)
            sl["copied"].record(self.stream)
            sl["staged"] = True
            tf.launch(items, sl["dev"].data_ptr(), img_out, sl["tmp"], pm1, bins, mclass, self.stream.cuda_stream)
            native = None
            if self.native:
                qm = items[-nb:]                     # the queries' class-id maps, last in the staging plan
                for im, it in zip(images[-nb:], qm):
                    if im.shape[:2] != (it[1], it[2]):
                        raise ValueError(f"query image {im.shape[:2]} and query mask {(it[1], it[2])} differ in size")
                native = NativeTargets((tf.size, tf.size), [(it[1], it[2]) for it in qm],
                                       gt_device=(sl["dev"], [it[5][0][0] for it in qm], [it[3] for it in qm]),
                                       class_value=mclass[-nb:], ignore_value=self.ignore_value, device=self.device)
            sl["event"].record(self.stream)
        cid = torch.tensor([int(e["class_id"]) for e in eps], dtype=torch.long)
        out = dict(support_imgs=sl["sup"], query_img=sl["qry"], support_masks=sl["smask"], query_mask=sl["qmask"],
                   class_id=cid, _slot=sl)
        if native is not None:
            out["native"] = native
        return out

    def __iter__(self):
        q = queue.Queue(maxsize=self.depth)
        stop = threading.Event()

        def produce():
            try:
                torch.cuda.set_device(self.device)
                buf, i = [], 0
                for e in self.src:
                    buf.append(e)
                    if len(buf) == self.b:
                        out = self._stage(i % (self.depth + 2), buf)
                        buf, i = [], i + 1
                        while not stop.is_set():
                            try:
                                q.put(out, timeout=0.1)
                                break
                            except queue.Full:
                                continue
                        if stop.is_set():
                            return
                if buf and not stop.is_set():
                    q.put(self._stage(i % (self.depth + 2), buf))
                q.put(None)
            except BaseException as ex:  # surfaced in the consumer
                q.put(ex)

        th = threading.Thread(target=produce, daemon=True)
        th.start()
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
                sl["release"].record(torch.cuda.current_stream(self.device))
                sl["released"] = True
        finally:
            stop.set()
