"""The stream-ordering harness without a device (tests/stream_stall.py): the inventory of the product's ordering sites
against the table, the cap on rows that are not cut, and the proxy and the witness on fake stream and event classes."""
import importlib.util
import os
import re
import types

import pytest

import stream_stall as ss

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------ inventory

def test_every_ordering_site_of_the_product_is_a_row_with_a_scenario():
    """An AST scan of diffews_amd/*.py finds every wait_event, wait_stream, .synchronize(, record_stream,
    non_blocking=True and pin_memory call; each is a row of EDGES, in its file, with a scenario the GPU file runs.  A site
    added later without a row fails here with its file and line."""
    found = ss.package_sites()
    assert len(found) >= 40 and {s.kind for s in found} == set(ss.KINDS)
    rows = {e.name: e for e in ss.EDGES}
    assert len(rows) == len(ss.EDGES), "a name twice in EDGES"
    missing = [repr(s) for s in found if s.name not in rows]
    assert not missing, "ordering sites without a row in tests/stream_stall.py EDGES:\n" + "\n".join(missing)
    stale = sorted(set(rows) - {s.name for s in found})
    assert not stale, f"rows of EDGES that name no site of the product: {stale}"
    for s in found:
        assert rows[s.name].file == s.file, (repr(s), rows[s.name].file)
    with open(os.path.join(HERE, "test_stream_order_gpu.py")) as f:
        tests = set(re.findall(r"^def test_(s\d+)_", f.read(), flags=re.M))
    for e in ss.EDGES:
        assert e.stalled in ss.SCENARIOS and e.stalled.lower() in tests, f"{e.name}: no test runs scenario {e.stalled}"
        assert e.protects.strip(), e.name


def test_a_search_by_name_finds_no_more_than_the_scan():
    """Every NAME token of the sources (comments and strings are no tokens of that kind) that is one of the six words lies
    on a line of a site the AST scan found: the scan misses no spelling of a call."""
    import glob
    import tokenize
    lines = {(s.file, ln) for s in ss.package_sites() for ln in range(s.lineno, s.end_lineno + 1)}
    words = {"wait_event", "wait_stream", "synchronize", "record_stream", "non_blocking", "pin_memory"}
    seen = 0
    for path in sorted(glob.glob(os.path.join(ss.PACKAGE, "*.py"))):
        with open(path, "rb") as f:
            for tok in tokenize.tokenize(f.readline):
                if tok.type == tokenize.NAME and tok.string in words:
                    seen += 1
                    assert (os.path.basename(path), tok.start[0]) in lines, f"{path}:{tok.start[0]}: {tok.line.strip()}"
    assert seen >= len(ss.EDGES)


def test_names_are_qualified_and_counted_in_source_order():
    names = [s.name for s in ss.package_sites()]
    for n in ("_Prefetcher._stage:synchronize#0", "_Prefetcher._stage:wait_event#0", "_Prefetcher.__iter__:wait_event#0",
              "GradBucketReducer._fire:wait_event#0", "GradBucketReducer.finish:wait_stream#0",
              "UNetTrainer._resolve_overflow:synchronize#0", "ScoreBuffers.stage:synchronize#0"):
        assert names.count(n) == 1, n
    seg = [s for s in ss.package_sites() if s.function == "UNetTrainer.forward_backward_segmented" and s.kind == "wait_stream"]
    assert [s.ordinal for s in seg] == [0, 1, 2] and seg[0].lineno < seg[1].lineno < seg[2].lineno


def test_cap_on_rows_that_are_not_cut():
    """Every row is cut or carries one of the two reasons; a wait written in the product's own code is cut at its own site
    unless a device synchronize joins it (the warm-up streams); everything else is cut through the wait that protects it or
    lives in torch's caching allocators."""
    assert ss.REASONS == ("allocator", "joined-by-device-sync")
    for e in ss.EDGES:
        kind = e.name.split(":")[1].split("#")[0]
        assert (e.cut is None) != (e.reason is None), f"{e.name}: a row is either cut or says why not"
        if e.cut is None:
            assert e.reason in ss.REASONS, e.name
            assert e.reason == ("joined-by-device-sync" if kind in ss.WAITS else "allocator"), e.name
        else:
            scenario, edge = e.cut
            assert scenario in ss.SCENARIOS and edge in ss.CUTTABLE
            assert edge.split(":")[1].split("#")[0] in ss.WAITS
            if kind in ss.WAITS:
                assert edge == e.name, f"{e.name}: a wait is cut at its own site"
    joined = [e for e in ss.EDGES if e.reason == "joined-by-device-sync"]
    for e in joined:              # only the warm-ups in front of a capture
        assert e.name.split(":")[0] in ("MarigoldPipelineRGBLatentNoise._replay", "UNetTrainer.forward_backward_captured",
                                        "UNetTrainer.forward_backward_segmented"), e.name
    assert len(ss.CUTTABLE) == 7
    with open(os.path.join(HERE, "test_stream_order_gpu.py")) as f:
        text = f.read()
    for edge in ss.CUTTABLE:
        assert edge in text or any(f"ss.{k}" in text for k, v in vars(ss).items() if v == edge), f"no test cuts {edge}"


# ------------------------------------------------------------------------------------------------ the proxy on fakes

class _World:
    """A fake torch with streams and events that write down what is done to them."""

    def __init__(self):
        w = self
        self.calls, self.current, self.capturing, self.done = [], None, False, False

        class Stream:
            count = 0

            def __new__(cls, device=None, priority=0, stream_id=None, device_index=0, device_type=0):
                self = object.__new__(cls)                  # like torch's: complete when __new__ returns
                if stream_id is None:
                    Stream.count += 1
                    stream_id = Stream.count
                self.stream_id, self.device_index, self.device_type = stream_id, device_index, device_type
                return self

            def __repr__(self):
                return f"<stream {self.stream_id}>"

            def __eq__(self, other):
                return isinstance(other, Stream) and other.stream_id == self.stream_id

            __hash__ = None

            def wait_event(self, event):
                w.calls.append(("wait_event", self.stream_id))

            def wait_stream(self, stream):
                w.calls.append(("wait_stream", self.stream_id, stream.stream_id))

            def synchronize(self):
                w.calls.append(("stream.synchronize", self.stream_id))

        class Event:
            def record(self, stream=None):
                w.calls.append(("record", None if stream is None else stream.stream_id))

            def synchronize(self):
                w.calls.append(("event.synchronize",))

            def query(self):
                return w.done

        class _Ctx:
            def __init__(self, s):
                self.s = s

            def __enter__(self):
                self.prev, w.current = w.current, self.s
                w.calls.append(("enter", self.s.stream_id))

            def __exit__(self, *exc):
                w.current = self.prev
                w.calls.append(("exit", self.s.stream_id))

        self.default = Stream(stream_id=0)
        self.current = self.default
        self.Stream, self.Event = Stream, Event
        self.cuda = types.SimpleNamespace(
            Stream=Stream, Event=Event, stream=_Ctx, current_stream=lambda device=None: w.current,
            synchronize=lambda device=None: w.calls.append(("cuda.synchronize",)),
            is_current_stream_capturing=lambda: w.capturing, is_available=lambda: False)
        self.float32 = "float32"

    def stall(self, stream, ms):
        self.calls.append(("stall", stream.stream_id, ms))


PRODUCT = '''
torch = None


class Tensor:
    def record_stream(self, stream):
        self.recorded = stream


class Loader:
    def __init__(self):
        self.stream = torch.cuda.Stream(device=None)
        self.other = torch.cuda.Stream()
        self.ev = torch.cuda.Event()
        self.dtype = torch.float32

    def stage(self, t):
        self.ev.synchronize()
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(self.ev)
            self.stream.wait_event(
                self.ev)
            self.ev.record(self.stream)
        with torch.cuda.stream(self.other):
            self.other.synchronize()
        t.record_stream(self.stream)
        torch.cuda.current_stream().wait_stream(self.stream)
        torch.cuda.synchronize()

    def boom(self):
        with torch.cuda.stream(self.stream):
            raise KeyError("boom")
'''
NAMES = ["Loader.stage:synchronize#0", "Loader.stage:wait_event#0", "Loader.stage:wait_event#1", "Loader.stage:synchronize#1",
         "Loader.stage:wait_stream#0", "Loader.stage:synchronize#2"]


@pytest.fixture()
def fake(tmp_path):
    pkg = tmp_path / "fakepkg"
    pkg.mkdir()
    path = pkg / "product.py"
    path.write_text(PRODUCT)
    spec = importlib.util.spec_from_file_location("stream_order_fake_product", str(path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    world = _World()
    mod.torch = world
    order = ss.Order(real=world, stall=world.stall, package=str(pkg), cuttable=set(NAMES))
    return types.SimpleNamespace(mod=mod, world=world, order=order)


def test_proxy_names_call_sites(fake):
    """Qualified.function:primitive#ordinal, ordinals in source order; events, streams and the device synchronise under one
    primitive; a call that spans two lines is found; everything is passed on to the real classes."""
    with fake.order.installed(fake.mod), fake.order.run():
        ld = fake.mod.Loader()
        assert isinstance(ld.stream, fake.world.Stream) and isinstance(ld.ev, fake.world.Event) and ld.dtype == "float32"
        ld.stage(fake.mod.Tensor())
    assert fake.order.log == NAMES
    kinds = [c[0] for c in fake.world.calls if c[0] not in ("enter", "exit", "record")]
    assert kinds == ["event.synchronize", "wait_event", "wait_event", "stream.synchronize", "wait_stream", "cuda.synchronize"]
    assert ("wait_stream", 0, ld.stream.stream_id) in fake.world.calls       # current_stream() was wrapped, not replaced
    assert not any(c[0] == "stall" for c in fake.world.calls) and fake.order.witness is None
    # a call from outside the package is not an edge
    ld.stream.wait_event(ld.ev)
    ld.ev.synchronize()
    assert fake.order.log == NAMES


@pytest.mark.parametrize("which", range(len(NAMES)))
def test_proxy_cuts_exactly_one_site_for_one_run(fake, which):
    with fake.order.installed(fake.mod):
        ld = fake.mod.Loader()
        with fake.order.run():
            ld.stage(fake.mod.Tensor())
        full = [c for c in fake.world.calls if c[0] not in ("enter", "exit", "record")]
        del fake.world.calls[:]
        with fake.order.run(cut=NAMES[which]):
            ld.stage(fake.mod.Tensor())
        assert fake.order.cut_hits == 1 and fake.order.log == NAMES       # a cut edge is still logged
        got = [c for c in fake.world.calls if c[0] not in ("enter", "exit", "record")]
        assert got == full[:which] + full[which + 1:]
        del fake.world.calls[:]
        with fake.order.run():                                                 # the cut ended with its run
            ld.stage(fake.mod.Tensor())
        assert [c for c in fake.world.calls if c[0] not in ("enter", "exit", "record")] == full
    with pytest.raises(AssertionError):
        with fake.order.run(cut="Loader.stage:wait_event#7"):
            pass


def test_proxy_stalls_on_entry_for_the_named_stream_only(fake):
    with fake.order.installed(fake.mod):
        ld = fake.mod.Loader()
        with fake.order.run(stalls=[(ld.stream, 30.0)]):
            ld.stage(fake.mod.Tensor())
            ld.stage(fake.mod.Tensor())
            w = fake.order.witness
        sid, oid = ld.stream.stream_id, ld.other.stream_id
        calls = fake.world.calls
        assert [c for c in calls if c[0] == "stall"] == [("stall", sid, 30.0)] * 2
        i = calls.index(("stall", sid, 30.0))
        assert calls[i + 1] == ("enter", sid)                                    # the stall comes BEFORE the entry
        assert calls[calls.index(("exit", sid)) + 1] == ("record", sid)          # the witness behind the first delayed work
        assert sum(1 for c in calls if c == ("record", sid)) == 3                # two of the product, ONE witness
        assert ("stall", oid, 30.0) not in calls
        assert fake.order.stalled_ms == 60.0 and fake.order.stall_count == 2
        w.held("the end of the run")                                             # the fake device has done nothing yet
        fake.world.done = True
        with pytest.raises(ss.StallDidNotBite, match="the stall did not bite"):
            w.held("the end of the run")
        # nothing is stalled while the stream captures, and nothing after the run
        del calls[:]
        fake.world.capturing = True
        with fake.order.run(stalls=[(ld.stream, 30.0)]):
            ld.stage(fake.mod.Tensor())
        fake.world.capturing = False
        with fake.order.run():
            ld.stage(fake.mod.Tensor())
        assert not any(c[0] == "stall" for c in calls)


def test_stalls_are_bounded(fake):
    with pytest.raises(AssertionError):
        ss.stall(None, ss.MAX_STALL_MS + 1)
    with pytest.raises(AssertionError):
        ss.stall(None, 0)
    with fake.order.run():
        for _ in range(8):
            fake.order.enqueue_stall(fake.world.default, 250.0)
        with pytest.raises(AssertionError, match="of stalls in one test"):
            fake.order.enqueue_stall(fake.world.default, 1.0)
    fake.order.new_test()
    fake.order.enqueue_stall(fake.world.default, 1.0)
    assert fake.order.stalled_ms == 1.0
    assert ss.stall_length(0.5) == ss.MIN_STALL_MS and ss.stall_length(10.0) == 40.0 and ss.stall_length(62.5) == 250.0
    with pytest.raises(ss.ScenarioTooLarge):
        ss.stall_length(63.0)


def test_proxy_keeps_record_stream_working(fake):
    """The proxy's streams ARE streams of the real class: what record_stream and event.record receive needs no unwrapping."""
    with fake.order.installed(fake.mod), fake.order.run():
        ld = fake.mod.Loader()
        t = fake.mod.Tensor()
        ld.stage(t)
    assert isinstance(t.recorded, fake.world.Stream) and t.recorded == ld.stream
    assert type(fake.order.wrap(fake.world.default)) is fake.order.Stream and fake.order.wrap(fake.world.default) == fake.world.default
    assert fake.order.wrap(ld.stream) is ld.stream and fake.order.wrap(None) is None


def test_new_streams_are_drawn_again_until_they_are_apart(fake):
    """With `apart` set, a new stream that shares a hardware queue with one of those streams (here: the same id modulo 4,
    asked both ways) is dropped and another one drawn; a view of an existing stream is not probed; twelve in a row fail."""
    asked = []

    def independent(a, b):
        asked.append((a.stream_id, b.stream_id))
        return a.stream_id % 4 != b.stream_id % 4
    order = ss.Order(real=fake.world, stall=fake.world.stall, independent=independent)
    first = order.Stream()                                    # nothing to keep apart from: not probed
    assert first.stream_id == 1 and not asked
    order.new_test(apart=[fake.world.default, first])         # ids 0 and 1
    s = order.Stream(device=None)
    assert s.stream_id == 2 and order.rejected == 0 and asked == [(2, 0), (0, 2), (2, 1), (1, 2)]
    fake.world.Stream.count = 3
    t = order.Stream()                                        # 4 shares with 0, 5 with 1
    assert t.stream_id == 6 and order.rejected == 2 and isinstance(t, fake.world.Stream)
    del asked[:]
    assert order.wrap(fake.world.default).stream_id == 0 and not asked
    order.new_test(apart=[fake.world.default])
    assert order.rejected == 0
    with pytest.raises(AssertionError, match="share a hardware queue"):
        order2 = ss.Order(real=fake.world, stall=fake.world.stall, independent=lambda a, b: False)
        order2.new_test(apart=[fake.world.default])
        order2.Stream()


def test_proxy_restores_the_module_globals_after_an_exception(fake):
    with pytest.raises(KeyError):
        with fake.order.installed(fake.mod), fake.order.run(cut=NAMES[0]):
            assert fake.mod.torch is fake.order.torch
            fake.mod.Loader().boom()
    assert fake.mod.torch is fake.world and fake.order.cut is None and fake.order.stalls == []
    assert fake.world.current is fake.world.default                              # the stream context was left as well
    with pytest.raises(AttributeError):
        fake.order.torch.cuda = None
    with pytest.raises(AttributeError):
        fake.order.torch.cuda.Stream = None


def test_proxy_is_inert_when_not_installed(fake):
    ld = fake.mod.Loader()
    with fake.order.run(cut=NAMES[1], stalls=[(ld.stream, 30.0)]):
        ld.stage(fake.mod.Tensor())
    assert type(ld.stream) is fake.world.Stream and fake.order.log == [] and fake.order.cut_hits == 0
    assert not any(c[0] == "stall" for c in fake.world.calls)
    assert len([c for c in fake.world.calls if c[0] == "wait_event"]) == 2


def test_the_real_modules_hold_the_real_torch():
    import torch
    for m in ss.product_modules():
        assert m.__dict__["torch"] is torch, m.__name__
    order = ss.Order()
    with pytest.raises(KeyError):
        with order.installed(*ss.product_modules()):
            assert all(m.torch is order.torch for m in ss.product_modules())
            assert order.torch.float32 is torch.float32 and order.torch.cuda.is_available is torch.cuda.is_available
            assert issubclass(order.torch.cuda.Stream, torch.cuda.Stream) and issubclass(order.torch.cuda.Event, torch.cuda.Event)
            raise KeyError
    for m in ss.product_modules():
        assert m.__dict__["torch"] is torch, m.__name__


def test_witness_reports_a_stall_that_did_not_bite():
    class Done:
        def record(self, stream):
            self.stream = stream

        def query(self):
            return True

    class Pending(Done):
        def query(self):
            return False

    w = ss.witness("side", "batch 0", event_class=Done)
    assert w.event.stream == "side"
    with pytest.raises(ss.StallDidNotBite, match="the stall did not bite: batch 0 had completed"):
        w.held("the first clone")
    ss.witness("side", event_class=Pending).held()
