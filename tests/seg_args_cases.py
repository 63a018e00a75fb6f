"""The overlap matrix every object stage's entry point is held against (csrc/seg_args.h: one buffer table, one checker),
on host memory: every call here is refused before a launch, or is made to be.  Used by the test_every_refusal.. tests of
dfw_seg_components, _holes, _rle, _contours, _match, _scores, _boundary and _boundary_counts.

A stage describes itself with `valid() -> (args struct, the arrays behind its pointers)`, a fully valid call; `call(args)
-> return code`; and two dicts {field: (extent in bytes, required alignment in bytes)} of the buffers the call reads and
of those it writes, the workspace ("ws", where the stage has one) among the latter with the extent its query returns."""
import numpy as np

DFW_EINVAL, DFW_ESHAPE, DFW_EWORKSPACE = -1, -2, -4


def _arrays(keep):
    return list(keep.values()) if isinstance(keep, dict) else list(keep)


def _arena(fields, tail=0):
    """Every buffer of `fields` back to back in ONE allocation, each padded only to its alignment, so that neighbours of
    equal alignment touch: (the array, {field: address}).  `tail` bytes are added to the last address."""
    total = sum(n + al for n, al in fields.values()) + 64 + tail
    raw = np.zeros(total, np.uint8)
    at, where = raw.ctypes.data + (-raw.ctypes.data % 16), {}
    for name, (nbytes, align) in fields.items():
        at += -at % align
        where[name] = at
        at += nbytes
    last = list(fields)[-1]
    where[last] += tail
    assert where[last] + fields[last][0] <= raw.ctypes.data + total
    return raw, where


def check_overlap_rule(call, valid, inputs, outputs):
    """The matrix.  Refusals, each DFW_EINVAL: every output on every input, at the input's start and on its last byte;
    every output on every other output's last byte; every input inside an output.  Accepted by the overlap stage: two
    inputs on each other, and all buffers touching end to start -- shown with one misaligned pointer, which is only
    looked at once no overlap was found (DFW_ESHAPE), and, where there is a workspace, by making it the only thing wrong
    (DFW_EWORKSPACE).  The order: the workspace before overlap, overlap before alignment.  Nothing is written."""
    kept = []

    def fresh(*more):
        a, keep = valid()
        arrays = _arrays(keep) + list(more)
        kept.append((arrays, [np.array(v) for v in arrays]))             # a valid call is never made: it would launch
        return a

    def code(**moved):
        a = fresh()
        for field, (onto, shift) in moved.items():
            setattr(a, field, getattr(a, onto) + shift)
        return call(a)

    for out in outputs:
        for inp, (nbytes, _) in inputs.items():
            for shift in (0, nbytes - 1):
                assert code(**{out: (inp, shift)}) == DFW_EINVAL, (out, inp, shift)
        for other, (nbytes, _) in outputs.items():
            if other != out:
                assert code(**{out: (other, nbytes - 1)}) == DFW_EINVAL, (out, other)
    for inp in inputs:
        for out, (nbytes, _) in outputs.items():
            assert code(**{inp: (out, nbytes // 2)}) == DFW_EINVAL, (inp, out)

    # one pointer off its alignment and nothing else wrong: the answer that shows a call got past the overlap stage
    odd = next(f for f in reversed(list(outputs)) if outputs[f][1] > 1)
    assert code(**{odd: (odd, 1)}) == DFW_ESHAPE, odd
    names = list(inputs)
    for i, f in enumerate(names):
        for g in names[i + 1:]:
            small, large = (f, g) if inputs[f][0] <= inputs[g][0] else (g, f)   # stay inside the larger one's allocation
            assert code(**{small: (large, 0), odd: (odd, 1)}) == DFW_ESHAPE, (small, large)
    # all buffers touching: the misaligned one goes last, one byte behind its place, so it still touches nothing
    fields = {**inputs, **{f: v for f, v in outputs.items() if f != odd}, odd: outputs[odd]}
    for tail, want in ((1, DFW_ESHAPE),) + (((0, DFW_EWORKSPACE),) if "ws" in outputs else ()):
        raw, where = _arena(fields, tail)
        a = fresh(raw)
        for f, at in where.items():
            setattr(a, f, at)
        if want == DFW_EWORKSPACE:
            a.ws_bytes = outputs["ws"][0] - 1                             # the workspace is the only thing wrong
        assert call(a) == want, ("arena", tail)

    # the order of the house
    first_out, first_in = next(iter(outputs)), next(iter(inputs))
    if "ws" in outputs:
        a = fresh()
        setattr(a, first_out, getattr(a, first_in))
        a.ws_bytes = 0
        assert call(a) == DFW_EWORKSPACE
    assert code(**{odd: (first_in, 1)}) == DFW_EINVAL                     # on an input AND off its alignment
    assert all(np.array_equal(v, was) for arrays, before in kept for v, was in zip(arrays, before)), "a refused call wrote"
