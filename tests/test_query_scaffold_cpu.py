"""Host-side bookkeeping the five bank-backed routes share (pipeline._query_context, _run_query_step, _touch_query_graph,
_graph_key), on a pipeline object without models: the eviction rule of the captured query steps, the order of the
argument checks, and the shape of the graph keys.  The bit-for-bit GPU tests compare the routes' outputs; these pin what
they cannot see."""
import pytest
import torch

from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise as P


def _fake_pipe(**attrs):
    """A pipeline that has no scheduler, UNet or VAE (tests/test_candidates_native_cpu.py::_fake_pipe): reading one is an
    AttributeError."""
    pipe = object.__new__(P)
    pipe.device = "cpu"
    for k, v in attrs.items():
        setattr(pipe, k, v)
    return pipe


def _supports(nsets=3, shots=2):
    from diffews_amd import config
    from diffews_amd.unet import SupportBank, SupportBankSet, bank_layout
    cfg = config.get("tiny_unet")
    dt, hw, key = torch.bfloat16, (8, 8), (1.0, "folded", 1)
    layout = bank_layout(cfg, *hw)
    kv = lambda n: [torch.zeros(n, t, c, dtype=dt) for t, c in layout]
    return (SupportBank(kv(shots), kv(shots), shots, hw, dt, dt, key, 1, layout),
            SupportBankSet(kv(nsets * shots), kv(nsets * shots), nsets, shots, hw, dt, dt, key, 1, layout))


# ------------------------------------------------------------------------------------------------ eviction

def _q(i):
    return ("queries", i, (1, 3, 64, 64), False)


EPISODES = ((4, 3, 64, 64), (2, 3, 64, 64), True, (0.25, 0.0, False))      # a run_episodes-style key: k[0] is a shape


def test_known_key_moves_to_the_end_and_nothing_is_dropped():
    pipe = _fake_pipe(MAX_QUERY_GRAPHS=4, _graphs={_q(0): "a", EPISODES: "e", _q(1): "b", _q(2): "c", _q(3): "d"})
    pipe._touch_query_graph(_q(1))
    assert list(pipe._graphs) == [_q(0), EPISODES, _q(2), _q(3), _q(1)] and pipe._graphs[_q(1)] == "b"
    pipe._touch_query_graph(_q(1))                                         # already last
    assert list(pipe._graphs) == [_q(0), EPISODES, _q(2), _q(3), _q(1)]


def test_new_key_drops_exactly_the_oldest_query_key():
    pipe = _fake_pipe(MAX_QUERY_GRAPHS=4, _graphs={EPISODES: "e", _q(0): "a", _q(1): "b", _q(2): "c", _q(3): "d"})
    pipe._touch_query_graph(_q(9))               # the caller (_replay) inserts the new key; room is made for exactly one
    assert list(pipe._graphs) == [EPISODES, _q(1), _q(2), _q(3)]
    pipe._graphs[_q(9)] = "n"
    pipe._touch_query_graph(_q(1))                                         # least recently used is now _q(2)
    pipe._touch_query_graph(_q(10))
    assert list(pipe._graphs) == [EPISODES, _q(3), _q(9), _q(1)]


def test_below_the_limit_nothing_is_dropped():
    pipe = _fake_pipe(MAX_QUERY_GRAPHS=4, _graphs={_q(0): "a", _q(1): "b", EPISODES: "e"})
    pipe._touch_query_graph(_q(2))
    assert list(pipe._graphs) == [_q(0), _q(1), EPISODES]
    pipe._graphs[_q(2)] = "c"
    pipe._touch_query_graph(_q(3))                                         # three query keys: the fourth still fits
    assert list(pipe._graphs) == [_q(0), _q(1), EPISODES, _q(2)]


def test_other_graphs_are_never_counted_or_dropped():
    others = {EPISODES: "e", ((8, 3, 64, 64), (2, 3, 64, 64), False, (0.0, 0.5, True)): "f", ("segmented", 1): "g"}
    pipe = _fake_pipe(MAX_QUERY_GRAPHS=2, _graphs={**others, _q(0): "a"})
    pipe._touch_query_graph(_q(1))               # one query key of two allowed: five graphs in all, nothing goes
    assert list(pipe._graphs) == list(others) + [_q(0)]
    pipe._graphs[_q(1)] = "b"
    pipe._touch_query_graph(_q(2))
    assert list(pipe._graphs) == list(others) + [_q(1)]


def test_limit_of_one_drops_every_other_query_key():
    pipe = _fake_pipe(MAX_QUERY_GRAPHS=1, _graphs={_q(0): "a", EPISODES: "e", _q(1): "b", _q(2): "c"})
    pipe._touch_query_graph(_q(3))
    assert list(pipe._graphs) == [EPISODES]
    pipe._graphs[_q(3)] = "d"
    pipe._touch_query_graph(_q(3))
    assert list(pipe._graphs) == [EPISODES, _q(3)]


# ------------------------------------------------------------------------------------------------ error order

@pytest.mark.parametrize("wrong", ["bank", "object", "none"])
def test_wrong_support_type_raises_before_any_model_is_read(wrong):
    """segment_classes raises TypeError, segment_routed and segment_candidates(_native) ValueError, for a SupportBank, an
    arbitrary object and None -- on a pipeline without scheduler / unet / vae, so a check that moved behind the first use of
    one shows as AttributeError."""
    support = {"bank": _supports()[0], "object": object(), "none": None}[wrong]
    q = torch.zeros(1, 3, 64, 64)
    with pytest.raises(TypeError, match="SupportBankSet"):
        P.segment_classes(_fake_pipe(), support, q)
    with pytest.raises(ValueError, match="segment_routed needs a SupportBankSet"):
        P.segment_routed(_fake_pipe(), support, q, (0,))
    with pytest.raises(ValueError, match="segment_candidates needs a SupportBankSet"):
        P.segment_candidates(_fake_pipe(), support, q, [(0,)])
    with pytest.raises(ValueError, match="segment_candidates needs a SupportBankSet"):
        P.segment_candidates_native(_fake_pipe(), support, q, [(0,)], object())
    with pytest.raises(ValueError, match="NativeTargets"):                 # and this one before the type of `support`
        P.segment_candidates_native(_fake_pipe(), support, q, [(0,)], None)


def test_right_support_type_goes_on_to_the_scheduler():
    """With a SupportBankSet the next thing every route does is read the scheduler: the fake has none."""
    _, sets = _supports()
    q = torch.zeros(1, 3, 64, 64)
    for call in (lambda p: P.segment_classes(p, sets, q), lambda p: P.segment_routed(p, sets, q, (0,)),
                 lambda p: P.segment_candidates(p, sets, q, [(0,)]), lambda p: P.segment_queries(p, sets.bank(0), q)):
        with pytest.raises(AttributeError, match="scheduler"):
            call(_fake_pipe())


# ------------------------------------------------------------------------------------------------ key shape

class _Sched:
    timesteps = [torch.tensor(1.0)]

    def set_timesteps(self, n, device=None):
        assert n == 1

    def z0_is_neg_v(self, t):
        return self.ok


def _stub_pipe(monkeypatch, z0_is_neg_v=True):
    """A pipeline whose models are stubs that answer the preamble only, and whose runner records what it is handed."""
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda t: t)           # no accelerator here: the tables stay pageable
    sched = _Sched()
    sched.ok = z0_is_neg_v
    dt = torch.bfloat16
    unet = type("U", (), dict(dtype=dt, residual_dtype=dt, _weights_id=1, _fold_key=lambda self, tt, prompt: (1.0, "folded", 1)))()
    vae = type("V", (), dict(config={"block_out_channels": [1, 1, 1, 1]}, residual_dtype=torch.float32))()
    pipe = _fake_pipe(scheduler=sched, unet=unet, vae=vae, test_timestep=1, fold_conditioning=False, use_graph=False,
                      empty_text_embed=torch.zeros(1, 2, 4), _graphs={}, calls=[])

    def record(key_head, step, ins, tt, folded, captured, finish):
        pipe.calls.append(dict(head=key_head, ins=ins, tt=tt, folded=folded, captured=captured))
        return {}
    pipe._run_query_step = record
    return pipe


def test_key_heads_of_the_five_routes(monkeypatch):
    """What _run_query_step receives from one call per route: the head of the graph key, value for value what the tests and
    tools that read _graphs by position rely on, and the static inputs in the order their H2D copies are issued."""
    pipe = _stub_pipe(monkeypatch)
    bank, sets = _supports()
    q, gt = torch.zeros(2, 3, 64, 64), torch.zeros(2, 64, 64, dtype=torch.uint8)
    shape, flags = (2, 3, 64, 64), (0.25, 0.0, False)
    assert pipe._vae_factor == 8

    pipe.segment_queries(bank, q, gt)
    pipe.segment_queries(bank, q, None, r_threshold=0.0, threshold=0.5, batch_max=True, captured=True)
    pipe.segment_classes(sets, q, gt, max_batch=7)
    pipe.segment_routed(sets, q, (2, 0), gt)
    pipe.segment_candidates(sets, q, [(2, 0), (1,)], None, entry_batch=2, labels="local")
    pipe.segment_candidates_native(sets, q, [(2, 0), (1,)], object(), None, gt, entry_batch=4)
    heads = [c["head"] for c in pipe.calls]
    assert heads[0] == ("queries", bank.uid, shape, True, flags)
    assert heads[1] == ("queries", bank.uid, shape, False, (0.0, 0.5, True)) and pipe.calls[1]["captured"] is True
    assert heads[2] == ("queries", "classes", sets.uid, shape, True, flags, 7)
    assert heads[3] == ("queries", "routed", sets.uid, shape, True, flags) and heads[3][:3] == ("queries", "routed", sets.uid)
    # E_pad, entry_batch, labels, nlabels (local: the longest list), gt given, (r_threshold, threshold)
    assert heads[4] == ("queries", "candidates", sets.uid, shape, 4, 2, "local", 2, False, (0.25, 0.0))
    assert heads[5] == ("queries", "candidates", sets.uid, shape, 4, 4, "set", 3, True, (0.25, 0.0))
    assert all(h[0] == "queries" for h in heads) and all(c["captured"] is None for c in pipe.calls[2:])
    assert [list(c["ins"]) for c in pipe.calls] == [["query_img", "gt"]] * 3 + [["query_img", "gt", "table"]] + \
        [["query_img", "gt", "entries", "rows", "tab"]] * 2
    assert pipe.calls[3]["ins"]["table"].tolist() == [[4, 2], [0, 2]]
    assert pipe.calls[1]["ins"]["gt"] is None and pipe.calls[0]["ins"]["gt"].dtype == torch.uint8
    assert all(c["ins"]["query_img"].dtype == torch.float32 and c["folded"] is False for c in pipe.calls)


def test_graph_key_is_head_plus_the_common_tail(monkeypatch):
    pipe = _stub_pipe(monkeypatch)
    pipe._fold_key = (1.0, 123, 0)
    head = ("queries", "routed", 5, (2, 3, 64, 64), True, (0.25, 0.0, False))
    assert pipe._graph_key(head, torch.tensor(1.0), True) == head + (1.0, True, (1.0, 123, 0), torch.bfloat16, torch.float32)
    episodes = ((4, 3, 64, 64), (2, 3, 64, 64), True, (0.25, 0.0, False))    # run_episodes: shapes, with_gt, flags in 0..3
    key = pipe._graph_key(episodes, 1.0, False)
    assert key[:4] == episodes and key[4:] == (1.0, False, (1.0, 123, 0), torch.bfloat16, torch.float32)
    del pipe._fold_key
    assert pipe._graph_key((), 2, False)[2] is None


def test_preamble_order_after_the_type_check(monkeypatch):
    """Scheduler restriction (with the route's name) before the route's own argument errors, those before the stale-handle
    check."""
    bank, sets = _supports()
    q = torch.zeros(2, 3, 64, 64)
    pipe = _stub_pipe(monkeypatch, z0_is_neg_v=False)
    for name, call in (("segment_queries", lambda: pipe.segment_queries(bank, q)),
                       ("segment_classes", lambda: pipe.segment_classes(sets, q)),
                       ("segment_routed", lambda: pipe.segment_routed(sets, q, (0, 99))),
                       ("segment_candidates", lambda: pipe.segment_candidates(sets, q, [(0,)]))):
        with pytest.raises(NotImplementedError, match=name + " needs the one-step scheduler"):
            call()
    pipe = _stub_pipe(monkeypatch)
    stale = torch.zeros(2, 3, 32, 32)                                      # another resolution than the supports'
    with pytest.raises(ValueError, match="a route of 3 entries for 2 queries"):
        pipe.segment_routed(sets, stale, (0, 1, 2))
    with pytest.raises(ValueError, match="route_table"):
        pipe.segment_routed(sets, stale, (0, 99))
    with pytest.raises(ValueError, match="1 candidate lists for 2 queries"):
        pipe.segment_candidates(sets, stale, [(0,)])
    with pytest.raises(ValueError, match="candidate_tables"):
        pipe.segment_candidates(sets, stale, [(0, 0), ()])
    for call in (lambda: pipe.segment_queries(bank, stale), lambda: pipe.segment_classes(sets, stale),
                 lambda: pipe.segment_routed(sets, stale, (0, 1)), lambda: pipe.segment_candidates(sets, stale, [(0,), ()])):
        with pytest.raises(ValueError, match=r"mismatch: latent \(h, w\)"):
            call()
    assert pipe.calls == []
