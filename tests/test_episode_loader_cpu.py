"""CPU test of the EpisodeLoader's staging layout in its host-only mode (device=None): the order of images and maps, which
map goes where, the in-place ground truth of its NativeTargets, and the numpy emulation of the device tables over the
staged bytes against Pillow and torch themselves (exact).  The layout checks and the emulation are
tests/test_query_loader_cpu.py's."""
import numpy as np
import pytest
import torch

import query_loader_ref as qr
from test_query_loader_cpu import _check_layout, _emulate, lib  # noqa: F401 -- `lib` is the fixture that builds

OUT = (64, 64)
NSHOT = 2


def _episodes(n, seed=11):
    """n episodes of NSHOT shots: every image and map of another size from qr.source_sizes (a query and its map share
    theirs), maps uint8 / int64 in turn."""
    rs = np.random.RandomState(seed)
    sizes, k, eps = qr.source_sizes(OUT), 0, []

    def one():
        nonlocal k
        h, w = sizes[k % len(sizes)]
        k += 1
        return (rs.randint(0, 256, (h, w, 3)).astype(np.uint8),
                rs.choice([0, 3, 4, 8, 255], size=(h, w)).astype(np.uint8 if k % 2 else np.int64))
    for e in range(n):
        q, sup = one(), [one() for _ in range(NSHOT)]
        sup[0] = (sup[0][0], sup[0][1][:-1] if sup[0][1].shape[0] > 1 else sup[0][1])      # a support map need not match
        eps.append(dict(query_img=q[0], query_mask=q[1], support_imgs=[s[0] for s in sup],
                        support_masks=[s[1] for s in sup], class_id=[2, 7][e % 2]))
    return eps


@pytest.mark.parametrize("n", [2, 1], ids=["full", "short"])
def test_episode_loader_host_layout(lib, n):
    from diffews_amd.input_pipeline import EpisodeLoader, InputBatch
    eps = _episodes(n)
    ld = EpisodeLoader(eps, OUT[0], 2, NSHOT, device=None, native=True, ignore_value=255)
    lay, native = ld.host_batch(eps)
    assert isinstance(ld.layout(eps), InputBatch)
    images = [x for e in eps for x in e["support_imgs"]] + [e["query_img"] for e in eps]
    masks = [m for e in eps for m in e["support_masks"]] + [e["query_mask"] for e in eps]
    cls = [e["class_id"] + 1 for e in eps for _ in range(NSHOT)] + [e["class_id"] + 1 for e in eps]
    n_sup = n * NSHOT
    # order, destinations, class values
    assert _check_layout(lay, images, masks, 0) == (n_sup, n)
    assert lay.n_img == n_sup + n and lay.n_mask == n_sup + n
    assert lay.pm1_index == list(range(n_sup)) and lay.bin_index == list(range(n_sup, n_sup + n))
    assert [it.class_value for it in lay.mask_items[:lay.n_mask]] == cls
    assert [it.dst_off for it in lay.img_items[:lay.n_img]] == [i * 12 * OUT[0] * OUT[1] for i in range(n_sup + n)]
    # the staged bytes through the tables == Pillow / torch
    got_img, got_pm1, got_bin = _emulate(lay, ld.tf.lut)
    for i, im in enumerate(images):
        assert torch.equal(got_img[i], qr.host_image(im, OUT)), (i, im.shape)
    for j, (m, c) in enumerate(zip(masks, cls)):
        ref = qr.host_mask(m, c, OUT)
        if j < n_sup:
            assert np.array_equal(got_pm1[j * lay.pm1_stride], (ref[None].repeat(3, 1, 1) * 2 - 1).numpy()), j
        else:
            assert np.array_equal(got_bin[(j - n_sup) * lay.bin_stride], ref.to(torch.uint8).numpy()), j
    assert len(got_pm1) == n_sup and len(got_bin) == n
    # native: the queries' sizes, their maps in place
    assert native.b == n and native.has_gt and native.src_hw == OUT
    assert native.sizes == [e["query_img"].shape[:2] for e in eps]
    for it, (off, elem), e in zip(native.items, lay.mask_src[n_sup:], eps):
        assert (it.gt_off, it.gt_elem) == (off, elem) and it.gt_off % 16 == 0
        assert (it.class_value, it.ignore_value) == (e["class_id"] + 1, 255)
        g = e["query_mask"] if e["query_mask"].dtype == np.uint8 else e["query_mask"].astype(np.int32)
        assert bytes(lay.host[it.gt_off:it.gt_off + it.h * it.w * it.gt_elem]) == g.tobytes()
    # a query and its map must agree in size; an episode must hold NSHOT shots
    bad = _episodes(1)
    bad[0]["query_mask"] = np.zeros((3, 3), np.uint8)
    with pytest.raises(ValueError, match="size"):
        ld.host_batch(bad)
    bad = _episodes(1)
    bad[0]["support_imgs"] = bad[0]["support_imgs"][:1]
    with pytest.raises(ValueError, match="nshot"):
        ld.host_batch(bad)
    with pytest.raises(RuntimeError):
        iter(ld).__next__()
