"""Poisoned allocations: hold every returned byte independent of what an uninitialised buffer held.

dicp_amd allocates every output, gradient and workspace from Python, most of them with torch.empty / torch.empty_like, and leaves it to the kernels
to write each element before anything reads it.  A fresh process starts on zeroed pages and the caching allocator then hands back whatever the last
test left, so a missed store (a pad row, columns 3:6 of a six-column gradient, a cloud of 0 rows, a counter read before its first write) passes by
luck.  poisoned() takes the luck away: while it is active torch.empty and torch.empty_like return buffers whose every byte is `byte`.

Two patterns, both mandatory (PATTERNS):

    0xFF   float16/32/64 NaN                         signed integers -1 (uint8 255)         bool true (raw byte 0xFF)
    0xFE   float32 -1.7e38, float64 -5.3e303         -16843010 (int32), -72340172838076674  bool true (raw byte 0xFE)
           (float16 0xFEFE has all exponent bits     (int64), uint8 254
           set: NaN again)

NaN alone is not enough: fminf, v_min_f32 and every where(x < y) swallow it, so a running minimum that starts from garbage hides a NaN; a huge
negative finite value wins every such minimum and shows in every sum.

There is deliberately NO positive pattern.  On a shared GPU, positive garbage read as a count becomes a long loop and read as an index becomes a
wild address; a negative value ends a signed loop at once and the kernels' (unsigned)idx < rows compares reject a negative index, while the missing
write still shows through the output.  The tests exist to show value dependence through outputs, not to see what a kernel does with a garbage count.

hold(probe, exact=..., atomic=...) runs a probe clean, under 0xFF and under 0xFE and compares what the user gets back (see its docstring).
"""
import contextlib

import numpy as np
import torch

PATTERNS = (0xFF, 0xFE)
_REAL_EMPTY = torch.empty                       # (bound at import, before any patch: the fill's own 0-element handle is not an allocation)


class Tally:
    """What one poisoned() block replaced: allocations filled, bytes filled, calls passed through (0 elements, or a stream that is capturing)."""

    def __init__(self, byte):
        self.byte, self.allocations, self.bytes, self.passed = byte, 0, 0, 0

    def __repr__(self):
        return "poison 0x%02X: %d buffers, %d bytes (%d passed through)" % (self.byte, self.allocations, self.bytes, self.passed)


def _capturing(t):
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


def _fill(t, tally):
    if not isinstance(t, torch.Tensor) or t.numel() == 0 or _capturing(t):
        tally.passed += 1
        return t
    store = t.untyped_storage()                 # (a fresh buffer owns its storage: every byte of it, whatever the strides of the tensor)
    raw = _REAL_EMPTY(0, dtype=torch.uint8, device=t.device).set_(store)
    raw.fill_(tally.byte)
    tally.allocations += 1
    tally.bytes += raw.numel()
    return t


@contextlib.contextmanager
def poisoned(monkeypatch, byte):
    """Replace torch.empty and torch.empty_like on the torch module (the only two uninitialised allocation forms dicp_amd uses;
    tests/test_poison_host.py::test_sources_use_patched_forms_only keeps it so) by versions that call the real function and then fill the result,
    through a uint8 view of its storage, with `byte` repeated.  A tensor of 0 elements is returned as it is, and while the current stream is
    capturing the call passes through untouched.  -> Tally (allocations, bytes); the real functions are back on exit, also after an exception."""
    assert 0 <= byte <= 0xFF
    tally = Tally(byte)
    real_empty, real_like = torch.empty, torch.empty_like

    def empty(*args, **kwargs):
        return _fill(real_empty(*args, **kwargs), tally)

    def empty_like(*args, **kwargs):
        return _fill(real_like(*args, **kwargs), tally)

    with monkeypatch.context() as mp:
        mp.setattr(torch, "empty", empty)
        mp.setattr(torch, "empty_like", empty_like)
        yield tally


def raw_bytes(t):
    """The bytes of a CPU tensor as a uint8 numpy array (bool through its uint8 view), for bitwise comparison."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return t.numpy().reshape(-1).view(np.uint8)


def _first_differences(a, b, limit=6):
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype == torch.bool:
        a, b = a.view(torch.uint8), b.view(torch.uint8)
    an, bn = a.numpy(), b.numpy()
    same = (an == bn) | ((an != an) & (bn != bn)) if an.dtype.kind == "f" else an == bn
    where = np.argwhere(~same)
    return "%d of %d elements differ; first: %s" % (len(where), an.size, ", ".join(
        "%s clean %r poisoned %r" % (tuple(int(i) for i in ix), an[tuple(ix)].item(), bn[tuple(ix)].item()) for ix in where[:limit]))


def hold(probe, exact=None, atomic=None, monkeypatch=None, masks=None, label=None):
    """Run `probe` (no arguments; builds its inputs from a fixed seed; returns {name: CPU tensor} of every tensor the user gets back, forward
    outputs and gradients; None values are dropped) three times: clean, under 0xFF, under 0xFE.

      * patch took: each poisoned run filled more than 0 buffers; the count and the bytes are printed.
      * exact (names; None = every returned name that is not in `atomic`): the three runs give the same bytes.  No tolerance.
      * atomic {name: check}: gradients the kernels add with float atomics, whose order of addition is free.  Each poisoned run is finite
        wherever the clean run is finite, and check(value, outputs_of_that_run) -- the operator's existing bound against its existing
        reference -- is called on the clean and on both poisoned values.  Integer and bool outputs can never be listed here.
      * masks {name: bool tensor}: elements a docstring declares unspecified (True = compared); the caller quotes the sentence next to it.

    Every returned name must be in exactly one of the two sets.  -> the clean outputs."""
    import pytest
    atomic = dict(atomic or {})
    masks = dict(masks or {})
    what = label or getattr(probe, "__name__", "probe")
    runs = {}
    own = monkeypatch is None
    mp = pytest.MonkeyPatch() if own else monkeypatch
    try:
        runs["clean"] = {k: v for k, v in probe().items() if v is not None}
        for byte in PATTERNS:
            with poisoned(mp, byte) as tally:
                out = probe()
                if torch.cuda.is_available() and torch.cuda.is_initialized():
                    torch.cuda.synchronize()
            print("%s: %r" % (what, tally))
            assert tally.allocations > 0 and tally.bytes > 0, "%s: no torch.empty / torch.empty_like call was replaced under 0x%02X" % (what, byte)
            runs[byte] = {k: v for k, v in out.items() if v is not None}
    finally:
        if own:
            mp.undo()
    clean = runs["clean"]
    names = set(clean)
    assert names, what + ": the probe returned nothing"
    exact = names - set(atomic) if exact is None else set(exact)
    assert exact | set(atomic) == names and not (exact & set(atomic)), \
        "%s: returned %s, exact %s, atomic %s" % (what, sorted(names), sorted(exact), sorted(atomic))
    for k in atomic:
        assert clean[k].dtype.is_floating_point, "%s: %s is %s: integer and bool outputs are exact" % (what, k, clean[k].dtype)
    for k, v in clean.items():
        assert not v.is_cuda, "%s: %s is not on the CPU" % (what, k)
    failures = []
    for byte in PATTERNS:
        got = runs[byte]
        assert set(got) == names, "%s: under 0x%02X the probe returned %s, clean %s" % (what, byte, sorted(got), sorted(names))
        for k in sorted(names):
            a, b = clean[k], got[k]
            if a.shape != b.shape or a.dtype != b.dtype:
                failures.append("%s [%s] 0x%02X: %s %s, clean %s %s" % (what, k, byte, tuple(b.shape), b.dtype, tuple(a.shape), a.dtype))
                continue
            if k in exact:
                if k in masks:
                    keep = masks[k].expand_as(a)
                    fill = torch.zeros((), dtype=a.dtype)
                    a, b = torch.where(keep, a, fill), torch.where(keep, b, fill)
                if not np.array_equal(raw_bytes(a), raw_bytes(b)):
                    failures.append("%s [%s] follows the poison 0x%02X: %s" % (what, k, byte, _first_differences(a, b)))
            else:
                bad = torch.isfinite(a) & ~torch.isfinite(b)
                if bad.any():
                    failures.append("%s [%s] 0x%02X: %d elements are finite clean and not finite poisoned, first %s" % (
                        what, k, byte, int(bad.sum()), [tuple(int(i) for i in ix) for ix in bad.nonzero()[:6]]))
    assert not failures, "\n".join(failures)
    for k, check in atomic.items():
        for tag in ("clean",) + PATTERNS:
            check(runs[tag][k], runs[tag])
    return clean
