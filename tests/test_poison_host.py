"""tests/poison.py on the CPU: both patterns read back as documented for every dtype dicp_amd allocates, the patch is undone on exit (also after an
exception), the counters count, hold() refuses a value that follows the poison, and the sources under dicp_amd/ use no uninitialised allocation
form the helper does not replace."""
import glob
import os
import re
import struct
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool]
F32_FE = struct.unpack("<f", b"\xfe" * 4)[0]
F64_FE = struct.unpack("<d", b"\xfe" * 8)[0]
EXPECT = {                                      # (byte, dtype) -> value of every element; None = NaN
    (0xFF, torch.float16): None, (0xFF, torch.float32): None, (0xFF, torch.float64): None,
    (0xFF, torch.int32): -1, (0xFF, torch.int64): -1, (0xFF, torch.uint8): 255,
    (0xFE, torch.float16): None, (0xFE, torch.float32): F32_FE, (0xFE, torch.float64): F64_FE,
    (0xFE, torch.int32): -0x01010102, (0xFE, torch.int64): -0x0101010101010102, (0xFE, torch.uint8): 254,
}


def test_the_finite_pattern_is_huge_and_negative():
    assert -1.8e38 < F32_FE < -1.6e38 and -5.5e303 < F64_FE < -5.2e303


@pytest.mark.parametrize("byte", poison.PATTERNS, ids=hex)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_patterns_read_back(monkeypatch, dtype, byte):
    with poison.poisoned(monkeypatch, byte) as tally:
        a = torch.empty(5, 7, dtype=dtype)
        b = torch.empty_like(torch.zeros(3, 2, dtype=dtype))
        c = torch.empty((4,), dtype=dtype, device="cpu")
    assert tally.allocations == 3 and tally.bytes == (35 + 6 + 4) * a.element_size()
    for t in (a, b, c):
        assert t.dtype == dtype
        if dtype == torch.bool:
            assert t.all() and (t.view(torch.uint8) == byte).all()      # true under both; the raw byte tells the patterns apart
            continue
        want = EXPECT[(byte, dtype)]
        if want is None:
            assert torch.isnan(t).all()
        else:
            assert (t == want).all(), (t.flatten()[0].item(), want)
            assert want < 0 or dtype == torch.uint8
        assert (poison.raw_bytes(t) == byte).all()


def test_zero_elements_and_non_contiguous(monkeypatch):
    base = torch.zeros(6, 4, 3).permute(2, 0, 1)                        # dense, not contiguous: empty_like keeps its strides
    sliced = torch.zeros(8, 6)[:, ::2]                                  # not dense: empty_like makes it contiguous
    with poison.poisoned(monkeypatch, 0xFF) as tally:
        z = torch.empty(0, 3)
        zl = torch.empty_like(torch.zeros(4, 0))
        p = torch.empty_like(base)
        s = torch.empty_like(sliced)
    assert z.shape == (0, 3) and zl.shape == (4, 0) and tally.passed == 2
    assert p.shape == base.shape and p.stride() == base.stride() and torch.isnan(p).all()
    assert s.shape == sliced.shape and torch.isnan(s).all()
    assert tally.allocations == 2 and tally.bytes == 4 * (72 + 24)


def test_restored_on_exit_and_after_an_exception(monkeypatch):
    real, real_like = torch.empty, torch.empty_like
    with poison.poisoned(monkeypatch, 0xFE):
        assert torch.empty is not real and torch.empty_like is not real_like
    assert torch.empty is real and torch.empty_like is real_like
    with pytest.raises(KeyError):
        with poison.poisoned(monkeypatch, 0xFF):
            assert torch.empty is not real
            raise KeyError("inside")
    assert torch.empty is real and torch.empty_like is real_like


def test_counters_count(monkeypatch):
    with poison.poisoned(monkeypatch, 0xFF) as tally:
        assert (tally.allocations, tally.bytes) == (0, 0)
        torch.empty(10, dtype=torch.float64)
        assert (tally.allocations, tally.bytes) == (1, 80)
        torch.empty_like(torch.zeros(3, dtype=torch.int32))
        assert (tally.allocations, tally.bytes) == (2, 92)
        torch.zeros(100)                                                # not an uninitialised form: not counted
        assert (tally.allocations, tally.bytes) == (2, 92)
    torch.empty(10)                                                     # outside: not counted
    assert tally.allocations == 2


def _probe_of(missing):
    def probe():
        g = torch.Generator().manual_seed(3)
        x = torch.randn(6, 3, generator=g)
        out = torch.empty(8, 3)
        out[:6] = 2 * x
        if "pad" not in missing:
            out[6:] = 0
        n = torch.empty(2, dtype=torch.int64)
        n[0] = 6
        if "count" not in missing:
            n[1] = 0
        low = torch.empty(())
        if "min" not in missing:
            low.fill_(float("inf"))
        low = torch.minimum(low, x.min())                              # (a NaN start is swallowed by where(x < y); -1.7e38 wins)
        low = torch.where(x.min() < low, x.min(), low)
        return dict(out=out, n=n, low=low.reshape(1), none=None)
    return probe


def test_hold_passes_a_complete_writer_and_refuses_each_missed_store():
    clean = poison.hold(_probe_of(()))
    assert set(clean) == {"out", "n", "low"}
    for missing, name in (("pad", "out"), ("count", "n"), ("min", "low")):
        with pytest.raises(AssertionError, match=r"\[%s\] follows the poison" % name):
            poison.hold(_probe_of((missing,)))
    assert torch.empty.__module__ != poison.__name__                   # hold() undoes its own patch


def test_hold_masks_exactly_the_elements_named():
    def probe():
        out = torch.empty(4)
        out[1:] = torch.tensor([1.0, 2.0, 3.0])
        return dict(out=out)
    with pytest.raises(AssertionError, match=r"\[out\] follows the poison"):
        poison.hold(probe)
    poison.hold(probe, masks={"out": torch.tensor([False, True, True, True])})
    with pytest.raises(AssertionError, match=r"\[out\] follows the poison"):
        poison.hold(probe, masks={"out": torch.tensor([True, False, True, True])})


def test_hold_atomic_outputs_are_finite_and_checked():
    seen, calls = [], []

    def probe(complete=True):
        calls.append(1)
        g = torch.empty(4)
        g[:3] = 1.0 + 1e-7 * len(calls)                                 # (an order-of-addition difference: allowed on an atomic output)
        if complete or len(calls) == 1:                                 # the incomplete writer: its first (clean) run happens to see 0
            g[3] = 0.0
        return dict(g=g, idx=torch.arange(3))

    poison.hold(probe, atomic={"g": lambda v, outs: seen.append((v, outs["idx"]))})
    assert len(seen) == 3 and len(calls) == 3
    with pytest.raises(AssertionError, match=r"\[g\] follows the poison"):
        poison.hold(probe)                                              # the same drift on an exact output is a failure
    del calls[:]
    with pytest.raises(AssertionError, match="finite clean and not finite poisoned"):
        poison.hold(lambda: probe(complete=False), atomic={"g": lambda v, o: None})

    def bound(v, outs):
        assert (v[3] == 0).all(), "held to the reference"
    del calls[:]
    with pytest.raises(AssertionError, match="held to the reference"):  # 0xFE is finite: the operator's own bound catches it
        poison.hold(lambda: dict(g=torch.nan_to_num(probe(complete=False)["g"], nan=0.0)), atomic={"g": bound})
    with pytest.raises(AssertionError, match="integer and bool outputs are exact"):
        poison.hold(lambda: dict(idx=torch.arange(3), e=torch.empty(1) * 0), exact=["e"], atomic={"idx": lambda v, o: None})


FORBIDDEN = {
    "new_empty": re.compile(r"\.new_empty\s*\("),
    "new_empty_strided": re.compile(r"\.new_empty_strided\s*\("),
    "empty_strided": re.compile(r"\bempty_strided\s*\("),
    "resize_": re.compile(r"\.resize_\s*\("),
    "empty_permuted": re.compile(r"\bempty_permuted\s*\("),
    "from torch import": re.compile(r"^\s*from\s+torch\s+import\b", re.M),
    "a bound name for torch.empty": re.compile(r"=\s*torch\.empty(_like)?\s*($|[^\w(])", re.M),
}


def test_sources_use_patched_forms_only():
    """poisoned() replaces torch.empty and torch.empty_like as attributes of the torch module.  Any other way to obtain uninitialised memory in
    dicp_amd/ would escape it: extend tests/poison.py before adding one."""
    files = sorted(glob.glob(os.path.join(ROOT, "dicp_amd", "**", "*.py"), recursive=True))
    assert len(files) > 20
    found, sites = [], 0
    for path in files:
        with open(path) as f:
            text = f.read()
        sites += len(re.findall(r"\btorch\.empty(?:_like)?\s*\(", text))
        for name, rx in FORBIDDEN.items():
            for m in rx.finditer(text):
                found.append("%s:%d uses %s" % (os.path.relpath(path, ROOT), text.count("\n", 0, m.start()) + 1, name))
    assert not found, "allocation forms tests/poison.py does not replace (extend the helper, then this list):\n" + "\n".join(found)
    assert sites > 100, "expected the package's torch.empty / torch.empty_like sites, found %d" % sites
