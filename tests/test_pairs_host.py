"""CPU checks of dicp_amd/_pairs.py, what register.py and compat.py share: the packed-pair record's way back to the original rows, the
shaping of the results, and the one number check.  Hand-written tensors; no GPU, no library call."""
import pytest
import torch

from dicp_amd._pairs import _Pairs, _finish, _mask_idx, _number

LIVE = torch.tensor([[1, 0, 1, 1, 0, 0], [0, 0, 0, 0, 0, 0]], dtype=torch.bool)         # one cloud with live rows 0, 2, 3; one with none


def _record():
    return _Pairs(None, LIVE, None, None, LIVE.sum(dim=1).to(torch.int32), None)


def test_unpack_puts_packed_position_k_on_the_kth_live_row_and_zero_elsewhere():
    pk = _record()
    for dtype in (torch.float32, torch.float64, torch.int32, torch.int64):
        packed = torch.tensor([[11, 12, 13, -7, -8, -9], [21, 22, 23, 24, 25, 26]]).to(dtype)     # (past P: whatever a kernel left there)
        out = pk.unpack(packed)
        assert out.dtype == dtype
        assert torch.equal(out, torch.tensor([[11, 0, 12, 13, 0, 0], [0, 0, 0, 0, 0, 0]]).to(dtype))
    assert pk._pos is not None and _record()._pos is None           # built on the first use, not before


def test_keep_holds_back_exactly_the_ranks_below_keep():
    pk = _record()
    rank = torch.tensor([[2, 0, 1, 0, 0, 0], [0, 1, 2, 3, 4, 5]], dtype=torch.int32)         # packed: row 0 has rank 2, row 2 rank 0, row 3 rank 1
    idx = torch.tensor([[5, 6, 7, 8, 9, 10], [1, 2, 3, 4, 5, 6]])
    for keep, rows in ((1, [2]), (2, [2, 3]), (3, [0, 2, 3]), (10 ** 12, [0, 2, 3])):
        kept, idx_kept = pk.keep(rank, keep, idx)
        want = torch.zeros_like(LIVE)
        want[0, rows] = True
        assert torch.equal(kept, want)
        assert idx_kept.dtype == idx.dtype and torch.equal(idx_kept, torch.where(want, idx, torch.tensor(-1)))
    assert torch.equal(_mask_idx(LIVE, idx.int()), torch.tensor([[5, -1, 7, 8, -1, -1], [-1] * 6], dtype=torch.int32))


def test_finish_squeezes_the_per_row_outputs_of_a_single_pair_only():
    outs = [torch.zeros(1, 4, 4), torch.zeros(1, 6), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 4, 4)]
    shapes = lambda res: [tuple(t.shape) for t in res]  # noqa: E731
    assert shapes(_finish("single", False, outs, 2)) == [(4, 4), (6,), (1,), (1, 4, 4)]
    assert shapes(_finish("single", False, outs, len(outs))) == [(4, 4), (6,), (), (4, 4)]
    assert shapes(_finish("batch", False, outs, 2)) == shapes(_finish("batch", True, outs, len(outs))) == shapes(outs)
    res = _finish("single", True, outs, 2)
    assert isinstance(res, tuple) and all(not t.is_cuda for t in res)


def _ok(value, *a, **kw):
    _number(value, "op", "v must be right", *a, **kw)
    return True


def _bad(value, *a, **kw):
    with pytest.raises(ValueError) as e:
        _number(value, "op", "v must be right", *a, **kw)
    assert str(e.value) == "op: v must be right, got %r" % (value,)
    return True


def test_number_check_at_every_kind_of_boundary():
    inf, nan = float("inf"), float("nan")
    # a finite number > 0: both ends open
    assert _ok(0.1, 0.0, inf, True, True) and _ok(1, 0.0, inf, True, True) and _ok(5e-324, 0.0, inf, True, True)
    for v in (0, 0.0, -1.0, inf, nan, "0.1", None, True, torch.tensor(0.1)):
        assert _bad(v, 0.0, inf, True, True)
    # a finite number >= 0: a closed lower end, an open upper end
    assert _ok(0, 0.0, inf, hi_open=True) and _ok(0.0, 0.0, inf, hi_open=True) and _ok(-0.0, 0.0, inf, hi_open=True)
    assert _bad(-5e-324, 0.0, inf, hi_open=True) and _bad(inf, 0.0, inf, hi_open=True) and _bad(nan, 0.0, inf, hi_open=True)
    # (0, 1]: an open lower end, a closed upper end; None allowed
    assert _ok(1, 0.0, 1.0, lo_open=True, none_ok=True) and _ok(1.0, 0.0, 1.0, lo_open=True) and _ok(None, 0.0, 1.0, lo_open=True, none_ok=True)
    assert _bad(0.0, 0.0, 1.0, lo_open=True) and _bad(1.0000000000000002, 0.0, 1.0, lo_open=True) and _bad(None, 0.0, 1.0, lo_open=True)
    # >= 0 with no upper end: +inf passes, a NaN does not
    assert _ok(inf, 0.0, none_ok=True) and _ok(None, 0.0, none_ok=True) and _bad(nan, 0.0, none_ok=True) and _bad(-1, 0.0, none_ok=True)
    # an int in [1, 8]
    assert _ok(1, 1, 8, integer=True) and _ok(8, 1, 8, integer=True)
    for v in (0, 9, 1.0, True, None, "1", nan, inf, torch.tensor(1)):
        assert _bad(v, 1, 8, integer=True)
    # an int >= 1 with no upper end; None or any int
    assert _ok(10 ** 400, 1, integer=True) and _bad(0, 1, integer=True)
    assert _ok(-10 ** 400, integer=True, none_ok=True) and _ok(None, integer=True, none_ok=True)
    assert _bad(1.5, integer=True, none_ok=True) and _bad(True, integer=True, none_ok=True) and _bad(False, 0.0, 1.0)
    # a message with parts: put together for a refused value only
    _number(3, "op", "%s", 1, 8, integer=True, fmt=("never", "formatted"))
    with pytest.raises(ValueError) as e:
        _number(9, "op", "%s must be an int in [%d, %d]", 1, 8, integer=True, fmt=("v", 1, 8))
    assert str(e.value) == "op: v must be an int in [1, 8], got 9"
