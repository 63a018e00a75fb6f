"""GPU tests of the one input-transform route: the per-item C entry points (dfw_image_to_tensor / dfw_mask_to_tensor, no
longer called by the package, here through ctypes) against Pillow / torch themselves; the prefetching loaders' producer
thread ending when the consumer leaves early; the EpisodeLoader's batch in three launches.  Bytes: every comparison is
exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import query_loader_ref as qr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("out_hw", qr.OUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_per_item_entry_points_equal_pillow_and_torch(hip_lib, out_hw):
    """One dfw_image_to_tensor call per image and dfw_mask_to_tensor calls per class-id map of qr.ragged (1 x 1, 2 x 3, a
    700 x 20 strip, the identity, ...; uint8 and int32 maps): every map with both class values and with +-1 only, 0/1
    only and both destinations."""
    from diffews_amd.input_pipeline import DeviceImageTransform
    d = qr.ragged(out_hw)
    lut = DeviceImageTransform(out_hw).lut
    assert {m.dtype for m in d["masks"]} == {np.dtype(np.uint8), np.dtype(np.int32)}
    for i, (im, ref) in enumerate(zip(d["images"], d["ref_images"])):
        assert torch.equal(qr.per_item_image(im, out_hw, lut).cpu(), ref), (i, im.shape)
    for j, m in enumerate(d["masks"]):
        for value in qr.CLASS_VALUES:
            ref = d["ref_masks"][j] if value == d["mask_class"][j] else qr.host_mask(m, value, out_hw)
            for want_pm1, want_bin in ((True, False), (False, True), (True, True)):
                pm1, bn = qr.per_item_mask(m, value, out_hw, lut.device, want_pm1, want_bin)
                assert (pm1 is not None) == want_pm1 and (bn is not None) == want_bin
                if want_pm1:
                    assert torch.equal(pm1.cpu(), ref[None].repeat(3, 1, 1) * 2 - 1), (j, value)
                if want_bin:
                    assert torch.equal(bn.cpu().float(), ref), (j, value)


def _small_sources(n, seed):
    rs = np.random.RandomState(seed)
    sizes = [(9, 13), (20, 7), (32, 32), (5, 40)]
    out = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        out.append((rs.randint(0, 256, (h, w, 3)).astype(np.uint8), rs.randint(0, 3, (h, w)).astype(np.uint8)))
    return out


@pytest.mark.parametrize("kind", ["episodes", "queries"])
def test_producer_ends_when_the_consumer_leaves(hip_lib, kind):
    """depth = 1, batch = 1, 8 sources, and a consumer that breaks out after the first batch while the queue is full: the
    producer thread gives up its pending put and ends (bounded by one staging plus the 0.1 s put poll; the 5 s only
    guard against a hang)."""
    from diffews_amd.input_pipeline import EpisodeLoader, QueryLoader
    src = _small_sources(8, seed=4)
    if kind == "episodes":
        loader = EpisodeLoader([dict(query_img=im, query_mask=m, support_imgs=[im], support_masks=[m], class_id=0)
                                for im, m in src], 32, 1, 1, depth=1)
    else:
        loader = QueryLoader([dict(query_img=im, gt=m) for im, m in src], 32, 1, depth=1, class_value=1)
    n = 0
    for bt in loader:
        assert bt["query_img"].shape == (1, 3, 32, 32)
        n += 1
        break
    assert n == 1
    loader._thread.join(timeout=5)
    assert not loader._thread.is_alive()
    torch.cuda.synchronize()


def test_episode_batch_in_three_launches(hip_lib):
    """An EpisodeLoader batch's layout, captured as test_three_launches_whatever_the_batch captures a plain batch: three
    kernel nodes for 1 episode x 1 shot and for 2 episodes x 3 shots, none of them a memset node; the replay gives the
    loader's own tensors' values (Pillow / torch)."""
    from diffews_amd.input_pipeline import EpisodeLoader
    S, nodes = 32, []
    for b, nshot in ((1, 1), (2, 3)):
        src = _small_sources(b * (nshot + 1), seed=b)
        eps = [dict(query_img=src[e][0], query_mask=src[e][1], support_imgs=[x[0] for x in src[b + e * nshot:][:nshot]],
                    support_masks=[x[1] for x in src[b + e * nshot:][:nshot]], class_id=1) for e in range(b)]
        ld = EpisodeLoader(eps, S, b, nshot)
        lay = ld.layout(eps)
        host = torch.empty(lay.total, dtype=torch.uint8, pin_memory=True)
        lay.fill(host.numpy())
        staged = host.cuda()
        lay.run(staged, ld.tf.lut, torch.cuda.current_stream().cuda_stream)       # warms the allocator
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = lay.run(staged, ld.tf.lut, torch.cuda.current_stream().cuda_stream)
        n = C.c_int32(0)
        assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(n)) == 0
        nodes.append(n.value)
        graph.instantiate()
        graph.replay()
        torch.cuda.synchronize()
        assert out["images"].shape == (b * (nshot + 1), 3, S, S) and out["pm1"].shape == (b * nshot, 3, S, S)
        assert out["bin"].shape == (b, S, S)
        for e in range(b):
            assert torch.equal(out["images"][b * nshot + e].cpu(), qr.host_image(eps[e]["query_img"], (S, S)))
            assert torch.equal(out["bin"][e].cpu().float(), qr.host_mask(eps[e]["query_mask"], 2, (S, S)))
            for k in range(nshot):
                assert torch.equal(out["images"][e * nshot + k].cpu(), qr.host_image(eps[e]["support_imgs"][k], (S, S)))
                ref = qr.host_mask(eps[e]["support_masks"][k], 2, (S, S))
                assert torch.equal(out["pm1"][e * nshot + k].cpu(), ref[None].repeat(3, 1, 1) * 2 - 1)
    assert nodes == [3, 3], nodes
