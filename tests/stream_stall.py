"""Stream-ordering harness: stall one stream, cut one edge, require the same bytes.

The product orders its streams, and the host against the device, with events, `wait_stream`, host `synchronize()`,
`record_stream` and pinned buffers that outlive an asynchronous copy.  A missing edge is no error: it is rare, silently
wrong pixels, counts or gradients under load.  This module makes the bad interleaving certain instead of likely:

  * `stall(stream, ms)` enqueues a delay of fixed length on a stream (`torch.cuda._sleep`: a one-thread kernel that spins
    for a COUNT of clock ticks; it polls no memory and waits for no flag, so it cannot hang).  Ticks per millisecond are
    calibrated once per process with two timed calls.  One stall is at most MAX_STALL_MS, one test enqueues at most
    MAX_TOTAL_MS (Order.new_test() opens the budget): asking for more is an AssertionError, never a longer wait.
  * `Order` owns a proxy that takes the place of the module global `torch` in input_pipeline, train, objects, pipeline and
    ops (`with order.installed(*modules): ...`, the pattern of tests/launch_guard.py: the globals are restored on any
    exception).  It forwards everything unchanged except `cuda.Stream`, `cuda.Event`, `cuda.stream`, `cuda.current_stream`
    and `cuda.synchronize`.  Streams and events are SUBCLASSES of torch's, so `record_stream(stream)`,
    `event.record(stream)` and `torch.cuda.stream(stream)` keep working.
      - name: every `wait_event`, `wait_stream` and `synchronize` (of an event, a stream or the device) issued from a file
        of the package is identified by its call site, `Qualified.function:primitive#ordinal`, the ordinal counted per
        function and primitive in source order from the AST (`sites()`): `_Prefetcher._stage:synchronize#0`,
        `GradBucketReducer.finish:wait_stream#0`.  A call from anywhere else (a test, torch itself) is passed through.
      - log: `order.log` holds the names a run passed through, in order.
      - cut: `with order.run(cut=name)` turns exactly that edge into a no-op until the block ends.
      - apart: a new stream is drawn again until it shares no hardware queue with the streams the test names
        (`independent()`): two streams on one queue are serialised and neither a stall nor a cut shows between them.
      - stall on entry: `with order.run(stalls=[(stream, ms)])` enqueues a stall on `stream` every time product code
        enters `with torch.cuda.stream(stream)`, BEFORE the entry, so that what the product enqueues there runs late
        while the host goes on; when the block is left for the first time an event is recorded on the stream behind that
        delayed work: `order.witness`.
  * `Witness`: a stalled run means nothing if the host did not run ahead of the device.  `witness.held(what)` requires
    `event.query() is False` at the moment the host has enqueued what must race with the delayed work; otherwise it raises
    StallDidNotBite ("the stall did not bite").  Such a run fails, it never passes.
  * `EDGES`: one row per ordering site of the product -- what it protects, the scenario of
    tests/test_stream_order_gpu.py that exercises it under a stall, and either the scenario that cuts it or the reason it
    is not cut.  tests/test_stream_order_cpu.py requires a row for every site the AST scan finds.

A cut run exists to produce wrong BYTES and must never produce a fault: see SAFETY at the table.
"""
import ast
import contextlib
import glob
import os
import sys
import threading

import torch as _torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PACKAGE = os.path.join(ROOT, "diffews_amd")

MODULES = ("input_pipeline", "train", "objects", "pipeline", "ops")
WAITS = ("wait_event", "wait_stream", "synchronize")            # the primitives the proxy names, logs and cuts
KINDS = WAITS + ("record_stream", "non_blocking", "pin_memory")   # what the inventory lists

MIN_STALL_MS = 20.0
MAX_STALL_MS = 250.0
MAX_TOTAL_MS = 2000.0
HOST_FACTOR = 4.0          # host time jitters on a shared slice of CPUs
PROBE_MS = 2.0             # the stall of independent()
STREAM_ATTEMPTS = 12       # streams the proxy draws at most until one shares no hardware queue with `apart`


class StallDidNotBite(AssertionError):
    pass


class ScenarioTooLarge(AssertionError):
    pass


# ------------------------------------------------------------------------------------------------ call sites from the AST

class Site:
    __slots__ = ("file", "function", "kind", "ordinal", "lineno", "end_lineno")

    def __init__(self, file, function, kind, ordinal, lineno, end_lineno):
        self.file, self.function, self.kind, self.ordinal = file, function, kind, ordinal
        self.lineno, self.end_lineno = lineno, end_lineno

    @property
    def name(self):
        return f"{self.function}:{self.kind}#{self.ordinal}"

    def __repr__(self):
        return f"{self.file}:{self.lineno} {self.name}"


def _kinds_of(call):
    """The inventory kinds of one ast.Call: by the attribute called and by its keywords."""
    kinds = []
    if isinstance(call.func, ast.Attribute) and call.func.attr in ("wait_event", "wait_stream", "synchronize",
                                                                   "record_stream", "pin_memory"):
        kinds.append(call.func.attr)
    for kw in call.keywords:
        if kw.arg in ("non_blocking", "pin_memory") and isinstance(kw.value, ast.Constant) and kw.value.value is True:
            kinds.append(kw.arg)
    return kinds


def sites(path):
    """Every ordering site of one source file, in source order: a list of Site.  The function is qualified by the classes
    and functions around it ("_Prefetcher._stage"; a nested function "outer.inner"; lambdas and comprehensions belong to
    the function that holds them; module level is "<module>")."""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    found = []

    def walk(node, qual):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                walk(child, qual + [child.name])
                continue
            if isinstance(child, ast.Call):
                for kind in _kinds_of(child):
                    found.append((child.lineno, child.col_offset, ".".join(qual) or "<module>", kind, child.end_lineno))
            walk(child, qual)

    walk(tree, [])
    found.sort()
    out, count = [], {}
    for lineno, _, function, kind, end in found:
        k = count.get((function, kind), 0)
        count[(function, kind)] = k + 1
        out.append(Site(os.path.basename(path), function, kind, k, lineno, end))
    return out


def package_sites(package=PACKAGE):
    """sites() of every .py file of the package directory, by file name."""
    return [s for p in sorted(glob.glob(os.path.join(package, "*.py"))) for s in sites(p)]


class _SiteIndex:
    """(file path, line) of a frame -> the name of the wait issued there."""

    def __init__(self, package):
        self.package = os.path.realpath(package)
        self._files = {}

    def covers(self, filename):
        return os.path.dirname(os.path.realpath(filename)) == self.package

    def name(self, filename, lineno, kind):
        path = os.path.realpath(filename)
        if path not in self._files:
            self._files[path] = [s for s in sites(path) if s.kind in WAITS]
        hits = [s for s in self._files[path] if s.kind == kind and s.lineno <= lineno <= s.end_lineno]
        if len(hits) != 1:
            raise AssertionError(f"{filename}:{lineno}: {len(hits)} `{kind}` call sites on this line; the harness needs one")
        return hits[0].name


# ------------------------------------------------------------------------------------------------ the delay

_ticks_per_ms = None
CALIBRATION = {}         # what the two timed calls measured: ticks and milliseconds of each, ticks per millisecond


def ticks_per_ms():
    """Clock ticks of `torch.cuda._sleep` per millisecond on the current device: two timed calls, once per process."""
    global _ticks_per_ms
    if _ticks_per_ms is None:
        _torch.cuda._sleep(1000)               # first launch: code object load, not timed
        _torch.cuda.synchronize()
        counts, times = (2_000_000, 10_000_000), []
        for c in counts:
            e0, e1 = _torch.cuda.Event(enable_timing=True), _torch.cuda.Event(enable_timing=True)
            e0.record()
            _torch.cuda._sleep(c)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        rate = (counts[1] - counts[0]) / (times[1] - times[0]) if times[1] > times[0] else 0.0
        if not 1e3 <= rate <= 1e7:             # 1 MHz .. 10 GHz: anything else is no clock
            raise AssertionError(f"stall calibration: {counts} ticks took {times} ms")
        CALIBRATION.update(ticks=counts, ms=tuple(times), ticks_per_ms=rate)
        _ticks_per_ms = rate
    return _ticks_per_ms


def stall(stream, ms):
    """Enqueue a delay of `ms` milliseconds on `stream`: bounded by a tick count, at most MAX_STALL_MS."""
    if not 0 < ms <= MAX_STALL_MS:
        raise AssertionError(f"one stall is at most {MAX_STALL_MS} ms, asked for {ms}")
    ticks = int(ms * ticks_per_ms())
    with _torch.cuda.stream(stream):
        _torch.cuda._sleep(ticks)


def independent(a, b, ms=None):
    """True when work on stream `b` completes while stream `a` is held up: the two do not share a hardware queue.  The HIP
    runtime maps its streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default) and two streams on one queue run
    one after the other, so a stall on one delays the other as well: a stalled run between such a pair proves nothing
    and a cut run between them changes nothing.  One short stall on `a`, one empty kernel on `b`, one host wait for `b`."""
    ms = PROBE_MS if ms is None else ms
    ea, eb = _torch.cuda.Event(), _torch.cuda.Event()
    stall(a, ms)
    ea.record(a)
    with _torch.cuda.stream(b):
        _torch.cuda._sleep(1)
    eb.record(b)
    eb.synchronize()
    free = ea.query() is False
    ea.synchronize()
    return free


def stall_length(t_host_ms):
    """max(MIN_STALL_MS, HOST_FACTOR x the quiet run's host enqueue time); ScenarioTooLarge above MAX_STALL_MS: a stall
    that may not bite is not run, the scenario has to shrink."""
    ms = max(MIN_STALL_MS, HOST_FACTOR * float(t_host_ms))
    if ms > MAX_STALL_MS:
        raise ScenarioTooLarge(f"the host needs {t_host_ms:.1f} ms to enqueue this scenario: a stall of {ms:.0f} ms is above "
                               f"the cap of {MAX_STALL_MS:.0f} ms -- shrink the scenario")
    return ms


# ------------------------------------------------------------------------------------------------ the witness

class Witness:
    """An event behind delayed work.  held(): the host got where it is while that work was still pending."""

    def __init__(self, event, what="the delayed work"):
        self.event, self.what = event, what

    def held(self, at="here"):
        if self.event.query() is not False:
            raise StallDidNotBite(f"the stall did not bite: {self.what} had completed when the host reached {at}; "
                                  "the run proves nothing about the order")


def witness(stream, what="the delayed work", event_class=None):
    ev = (event_class or _torch.cuda.Event)()
    ev.record(stream)
    return Witness(ev, what)


# ------------------------------------------------------------------------------------------------ the proxy

class _CudaProxy:
    def __init__(self, order):
        object.__setattr__(self, "_order", order)

    def __getattr__(self, name):
        return getattr(self._order.real.cuda, name)

    def __setattr__(self, name, value):
        raise AttributeError("the torch.cuda proxy is read-only")

    @property
    def Stream(self):
        return self._order.Stream

    @property
    def Event(self):
        return self._order.Event

    def current_stream(self, device=None):
        return self._order.wrap(self._order.real.cuda.current_stream(device))

    def stream(self, stream):
        return self._order._entered(stream)

    def synchronize(self, device=None):
        if self._order._passes("synchronize"):
            self._order.real.cuda.synchronize(device)


class _TorchProxy:
    """Stands in for the module global `torch`: everything is the real torch's except `cuda`."""

    def __init__(self, order):
        object.__setattr__(self, "_order", order)
        object.__setattr__(self, "cuda", _CudaProxy(order))

    def __getattr__(self, name):
        return getattr(self._order.real, name)

    def __setattr__(self, name, value):
        raise AttributeError("the torch proxy is read-only")


class Order:
    """The proxy, its plan (one cut, stalls on entry) and its log.  real: the torch it stands in front of (tests of the
    harness pass a fake without a device); stall: the function that enqueues a delay; package: the directory whose files
    count as product code; cuttable: the edge names run(cut=) accepts (default: those the table cuts).

    apart: streams every NEW stream of the proxy's class must not share a hardware queue with (independent(), both ways):
    the product's side and comm streams are drawn again until they can really run beside the consumer's stream, and a test
    draws its own further streams with `order.Stream()`.  Empty: any stream will do."""

    def __init__(self, real=_torch, stall=stall, package=PACKAGE, cuttable=None, independent=independent):
        self.real, self._stall, self._index, self._cuttable = real, stall, _SiteIndex(package), cuttable
        self._independent, self.apart, self.rejected = independent, [], 0
        self.cut, self.cut_hits, self.log, self.stalls = None, 0, [], []
        self.witness, self.stalled_ms, self.stall_count = None, 0.0, 0
        self._lock = threading.Lock()
        order = self

        class Stream(real.cuda.Stream):
            def __new__(cls, *args, **kw):
                s = super().__new__(cls, *args, **kw)
                if "stream_id" in kw or not order.apart or real.cuda.is_current_stream_capturing():
                    return s                      # a view of an existing stream, or nobody to keep apart from
                for _ in range(STREAM_ATTEMPTS):
                    order.stalled_ms += 2 * PROBE_MS * len(order.apart)
                    if all(order._independent(s, t) and order._independent(t, s) for t in order.apart):
                        return s
                    order.rejected += 1
                    s = super().__new__(cls, *args, **kw)
                raise AssertionError(f"{STREAM_ATTEMPTS} new streams in a row share a hardware queue with one of {order.apart}")

            def wait_event(self, event):
                if order._passes("wait_event"):
                    super().wait_event(event)

            def wait_stream(self, stream):
                if order._passes("wait_stream"):
                    super().wait_stream(stream)

            def synchronize(self):
                if order._passes("synchronize"):
                    super().synchronize()

        class Event(real.cuda.Event):
            def synchronize(self):
                if order._passes("synchronize"):
                    super().synchronize()

        self.Stream, self.Event = Stream, Event
        self.torch = _TorchProxy(self)

    # ---- naming, logging, cutting
    def _passes(self, kind):
        """Called by an overridden primitive: names the call site two frames up.  False when that edge is cut."""
        f = sys._getframe(2)
        if not self._index.covers(f.f_code.co_filename):
            return True
        name = self._index.name(f.f_code.co_filename, f.f_lineno, kind)
        self.log.append(name)
        if name == self.cut:
            self.cut_hits += 1
            return False
        return True

    def wrap(self, s):
        """The stream `s` as an instance of the proxy's Stream class (the same device stream, not a new one)."""
        if s is None or isinstance(s, self.Stream):
            return s
        return self.Stream(stream_id=s.stream_id, device_index=s.device_index, device_type=s.device_type)

    # ---- stall on entry
    @contextlib.contextmanager
    def _entered(self, stream):
        ms = next((m for s, m in self.stalls if stream is not None and s == stream), None)
        if ms is not None and not self.real.cuda.is_current_stream_capturing():
            self.enqueue_stall(stream, ms)
        with self.real.cuda.stream(stream):
            yield
        if ms is not None and self.witness is None:
            self.witness = witness(stream, "the first work enqueued behind a stall on entry", self.real.cuda.Event)

    def enqueue_stall(self, stream, ms):
        """stall(stream, ms), counted against MAX_TOTAL_MS (the tests' own stalls go through here too)."""
        with self._lock:
            if self.stalled_ms + ms > MAX_TOTAL_MS:
                raise AssertionError(f"more than {MAX_TOTAL_MS:.0f} ms of stalls in one test ({self.stalled_ms:.0f} + {ms:.0f})")
            self.stalled_ms += ms
            self.stall_count += 1
        self._stall(stream, ms)

    def new_test(self, apart=()):
        """The budget of MAX_TOTAL_MS is one test's: every run of the test counts against it.  apart: see the class."""
        self.stalled_ms, self.apart, self.rejected = 0.0, list(apart), 0

    # ---- one run
    @contextlib.contextmanager
    def run(self, cut=None, stalls=()):
        """One run under a plan: `cut` (an edge name or None) and `stalls` ((stream, ms) pairs, stalled on entry).  The
        log, the witness and the run's counters start empty (the stall budget is the test's); the plan ends with the block."""
        if cut is not None and cut not in (CUTTABLE if self._cuttable is None else self._cuttable):
            raise AssertionError(f"{cut} is not an edge the table allows to cut")
        self.cut, self.cut_hits, self.log, self.stalls = cut, 0, [], list(stalls)
        self.witness, self.stall_count = None, 0
        try:
            yield self
        finally:
            self.cut, self.stalls = None, []

    @contextlib.contextmanager
    def installed(self, *modules):
        saved = [(m, m.__dict__["torch"]) for m in modules]
        for m, _ in saved:
            m.torch = self.torch
        try:
            yield self
        finally:
            for m, real in saved:
                m.torch = real


def product_modules():
    import importlib
    return [importlib.import_module(f"diffews_amd.{m}") for m in MODULES]


# ------------------------------------------------------------------------------------------------ the table
#
# SAFETY of a cut run on a shared device.  It must produce wrong bytes, never a fault, by construction:
#   * the test keeps a reference to every buffer of the scenario until it ends, so nothing is unmapped;
#   * data that crosses a cut edge is pixels, floats or a flag -- tables that cross one are byte-identical in every batch
#     (S1 cuts use sources of ONE size: item tables and resampling weights are the same in every batch, a torn or stale
#     buffer holds valid tables with the wrong pixels) or valid for the same tensors (S4: the same number of planes);
#   * no cut run passes NativeTargets, candidate tables or routing tables through the cut edge.
# A cut that cannot meet this is not run: its row carries a reason and counts as uncut.

SCENARIOS = {
    "S1": "the prefetcher through EpisodeLoader and QueryLoader, consumer never synchronises",
    "S2": "GradBucketReducer on a flat fp32 buffer, then through UNetTrainer.forward_backward",
    "S3": "the overflow word of UNetTrainer.optimizer_step / _resolve_overflow",
    "S4": "ScoreBuffers.stage: two object_scores calls back to back",
    "S5": "host buffers behind asynchronous copies, the host overwrites or drops them at once",
    "S6": "NativeTargets staged on the loader's stream, consumed on the stalled main stream, dropped, restaged",
    "S7": "captured training steps: warm-up on a side stream, static-input copies in front of a replay",
}
REASONS = ("allocator", "joined-by-device-sync")


class Edge:
    """name: the site; protects: what goes wrong without it; stalled: the scenario that exercises it under a stall;
    cut: (scenario, edge cut there) or None; reason: why it is not cut (one of REASONS) or None."""
    __slots__ = ("name", "file", "protects", "stalled", "cut", "reason")

    def __init__(self, name, file, protects, stalled, cut=None, reason=None):
        self.name, self.file, self.protects, self.stalled, self.cut, self.reason = name, file, protects, stalled, cut, reason


_COPIED, _RELEASE, _EVENT = "_Prefetcher._stage:synchronize#0", "_Prefetcher._stage:wait_event#0", "_Prefetcher.__iter__:wait_event#0"
_FIRE, _FINISH = "GradBucketReducer._fire:wait_event#0", "GradBucketReducer.finish:wait_stream#0"
_OVERFLOW, _PLANES = "UNetTrainer._resolve_overflow:synchronize#0", "ScoreBuffers.stage:synchronize#0"
_PIPE = "MarigoldPipelineRGBLatentNoise."
_PINNED = "the pinned source is dropped or reused by the host as soon as the call returns; the caching host allocator " \
          "keeps the block until the copy's event has completed"
_WARM = "the warm-up on a side stream sees the inputs and is finished before the capture: the device synchronize that " \
        "follows joins every stream, a cut changes nothing"

EDGES = [
    # ---- input_pipeline.py
    Edge("DeviceImageTransform.batch:pin_memory#0", "input_pipeline.py", _PINNED, "S5", reason="allocator"),
    Edge("DeviceImageTransform.batch:non_blocking#0", "input_pipeline.py", _PINNED, "S5", reason="allocator"),
    Edge("NativeTargets.__init__:pin_memory#0", "input_pipeline.py", "the pinned table goes with the object, possibly "
         "before the copy ran: " + _PINNED, "S5", reason="allocator"),
    Edge("NativeTargets.__init__:non_blocking#0", "input_pipeline.py", "item and weight tables staged on the current stream; "
         "they would cross a cut edge as tables", "S6", reason="allocator"),
    Edge("_Prefetcher._slot:record_stream#0", "input_pipeline.py", "a slot's old `dev` is freed on regrowth while kernels "
         "queued on the side stream still read it", "S1", reason="allocator"),
    Edge("_Prefetcher._slot:pin_memory#0", "input_pipeline.py", "a slot's old pinned buffer is dropped on regrowth while "
         "its copy may be pending: " + _PINNED, "S1", reason="allocator"),
    Edge("_Prefetcher._slot:record_stream#1", "input_pipeline.py", "a slot's old `tmp` is freed on regrowth while the "
         "resize queued on the side stream still uses it", "S1", reason="allocator"),
    Edge(_COPIED, "input_pipeline.py", "`copied`: the host refills a slot's pinned bytes only after the previous H2D copy "
         "has left them", "S1", cut=("S1", _COPIED)),
    Edge(_RELEASE, "input_pipeline.py", "`release`: the side stream overwrites a slot only after the consumer's work on "
         "its previous batch", "S1", cut=("S1", _RELEASE)),
    Edge("_Prefetcher._stage:non_blocking#0", "input_pipeline.py", "the copy that reads the pinned bytes asynchronously: "
         "what `copied` protects", "S1", cut=("S1", _COPIED)),
    Edge(_EVENT, "input_pipeline.py", "`event`: the consumer's stream reads a batch only when the side stream has "
         "finished it", "S1", cut=("S1", _EVENT)),
    # ---- objects.py
    Edge("ScoreBuffers.__init__:pin_memory#0", "objects.py", "the pinned plane table, overwritten by the next call",
         "S4", cut=("S4", _PLANES)),
    Edge(_PLANES, "objects.py", "the pinned plane table is overwritten only after the previous copy out of it", "S4",
         cut=("S4", _PLANES)),
    Edge("ScoreBuffers.stage:non_blocking#0", "objects.py", "the copy that reads the pinned plane table asynchronously",
         "S4", cut=("S4", _PLANES)),
    # ---- ops.py
    Edge("_native_setup:record_stream#0", "ops.py", "targets staged on the loader's stream, read on the consumer's and "
         "dropped: the block must not be handed out again before that read (skipped while capturing: the graph's inputs "
         "are held by the caller)", "S6", reason="allocator"),
    # ---- pipeline.py
    Edge(_PIPE + "_run_query_step:non_blocking#0", "pipeline.py", "pinned host tables of the eager step: " + _PINNED, "S5",
         reason="allocator"),
    Edge(_PIPE + "segment_routed:pin_memory#0", "pipeline.py", "the route table: " + _PINNED, "S5", reason="allocator"),
    Edge(_PIPE + "_segment_candidates:pin_memory#0", "pipeline.py", "candidate rows: " + _PINNED, "S5", reason="allocator"),
    Edge(_PIPE + "_segment_candidates:pin_memory#1", "pipeline.py", "candidate table: " + _PINNED, "S5", reason="allocator"),
    Edge(_PIPE + "_segment_candidates:pin_memory#2", "pipeline.py", "candidate entries: " + _PINNED, "S5",
         reason="allocator"),
    Edge(_PIPE + "_segment_candidates:non_blocking#0", "pipeline.py", "entry sets, a pageable source: the copy is "
         "synchronous for the host", "S5", reason="allocator"),
    Edge(_PIPE + "_tile_stage:pin_memory#0", "pipeline.py", "image and ground truth of a tiled call: " + _PINNED, "S5",
         reason="allocator"),
    Edge(_PIPE + "_tile_stage:non_blocking#0", "pipeline.py", "image and ground truth of a tiled call: " + _PINNED, "S5",
         reason="allocator"),
    Edge(_PIPE + "segment_tiled:pin_memory#0", "pipeline.py", "per-window candidate table: " + _PINNED, "S5",
         reason="allocator"),
    Edge(_PIPE + "segment_tiled:non_blocking#0", "pipeline.py", "per-window candidate table: " + _PINNED, "S5",
         reason="allocator"),
    Edge(_PIPE + "_replay:wait_stream#0", "pipeline.py", _WARM, "S5", reason="joined-by-device-sync"),
    Edge(_PIPE + "_replay:wait_stream#1", "pipeline.py", _WARM, "S5", reason="joined-by-device-sync"),
    Edge(_PIPE + "_replay:synchronize#0", "pipeline.py", _WARM + "; itself a host wait in front of a capture, which a cut "
         "would turn into a capture of a busy device", "S5", reason="joined-by-device-sync"),
    Edge(_PIPE + "_replay:non_blocking#0", "pipeline.py", "static-input copies in front of a replay: same-stream order for "
         "a device source, for a pinned host source " + _PINNED, "S5", reason="allocator"),
    # ---- train.py
    Edge("UNetTrainer._build:pin_memory#0", "train.py", "the pinned found-inf word", "S3", cut=("S3", _OVERFLOW)),
    Edge("UNetTrainer.forward_backward_captured:wait_stream#0", "train.py", _WARM, "S7", reason="joined-by-device-sync"),
    Edge("UNetTrainer.forward_backward_captured:wait_stream#1", "train.py", _WARM, "S7", reason="joined-by-device-sync"),
    Edge("UNetTrainer.forward_backward_captured:synchronize#0", "train.py", _WARM, "S7", reason="joined-by-device-sync"),
    Edge("UNetTrainer.forward_backward_captured:non_blocking#0", "train.py", "static-input copies in front of a replay, "
         "device to device: same-stream order; the sources are held by the caching allocator's stream order", "S7",
         reason="allocator"),
    Edge("UNetTrainer.forward_backward_segmented:wait_stream#0", "train.py", _WARM, "S7", reason="joined-by-device-sync"),
    Edge("UNetTrainer.forward_backward_segmented:wait_stream#1", "train.py", _WARM, "S7", reason="joined-by-device-sync"),
    Edge("UNetTrainer.forward_backward_segmented:synchronize#0", "train.py", _WARM, "S7", reason="joined-by-device-sync"),
    Edge("UNetTrainer.forward_backward_segmented:wait_stream#2", "train.py", "joins the side stream after the segments "
         "were CAPTURED on it: since the device synchronize above nothing has been executed there", "S7",
         reason="joined-by-device-sync"),
    Edge("UNetTrainer.forward_backward_segmented:non_blocking#0", "train.py", "static-input copies in front of a replay, "
         "device to device: same-stream order", "S7", reason="allocator"),
    Edge(_OVERFLOW, "train.py", "the host reads the found-inf word only after its D2H copy", "S3", cut=("S3", _OVERFLOW)),
    Edge("UNetTrainer.optimizer_step:non_blocking#0", "train.py", "the D2H copy of the found-inf word into pinned memory",
         "S3", cut=("S3", _OVERFLOW)),
    Edge(_FIRE, "train.py", "a bucket's collective starts on `comm` only after the bucket's last writer", "S2",
         cut=("S2", _FIRE)),
    Edge("GradBucketReducer._fire:record_stream#0", "train.py", "the bf16 wire buffer is allocated on the compute stream's "
         "pool and used on `comm`", "S2", reason="allocator"),
    Edge(_FINISH, "train.py", "the compute stream reads the reduced gradient only after `comm` has finished", "S2",
         cut=("S2", _FINISH)),
]

CUTTABLE = frozenset(e.cut[1] for e in EDGES if e.cut is not None)
