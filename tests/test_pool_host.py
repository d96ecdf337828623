"""CPU checks of pool_neighbors (dicp_amd/group.py) that need no GPU.

The pool rules of ``dicp_amd/csrc/dicp_group.h`` -- the lines the HIP kernels run -- are compiled with g++ through
tests/hostcheck/pool_check.cpp, run in a serial loop and held to the numpy restatement tests/pool_ref.py: the maximum (with its argmax)
and the sum bit for bit, the counts exactly, the mean within (k + 2) u sum|f| / count of a float64 evaluation.  The inputs are asserted to
hold what they promise, the comparison is shown to refuse four deliberately wrong restatements, and the argument checks of the entry
points and of the Python front run before any device work.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib
from dicp_amd.group import pool_neighbors

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import group_ref as gr  # noqa: E402
import hostbuild  # noqa: E402
import pool_ref as pr  # noqa: E402

DTYPES = [np.float32, np.float64]
SFX = {np.float32: "f32", np.float64: "f64"}
ISFX = {np.int64: "i64", np.int32: "i32"}
CODE = {"sum": 0, "mean": 1, "max": 2}
KS = (1, 3, 8, 32)
CS = (1, 33)
N_Q, M_ROWS, ROWS = 120, 257, 200


@pytest.fixture(scope="module")
def check():
    lib = hostbuild.build("pool_check.cpp", "pool_check", ("-Wall",))
    for s in SFX.values():
        for w in ISFX.values():
            getattr(lib, "pc_pool_%s_%s" % (s, w)).restype = None
        getattr(lib, "pc_mean_grad_" + s).restype = None
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _table(m, C, dtype, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random((m, C)) * 2 - 1) * 10.0 ** rng.integers(-2, 3, size=(m, C))).astype(dtype)


def _header(check, f, idx, reduce, rows):
    n, k = idx.shape
    C = f.shape[1]
    out, arg, cnt = np.empty((n, C), dtype=f.dtype), np.empty((n, C), dtype=np.int32), np.empty(n, dtype=np.int32)
    f, idx = np.ascontiguousarray(f), np.ascontiguousarray(idx)
    getattr(check, "pc_pool_%s_%s" % (SFX[f.dtype.type], ISFX[idx.dtype.type]))(_ptr(f), _ptr(idx), int(rows), CODE[reduce], n, k, C, _ptr(out), _ptr(arg), _ptr(cnt))
    if reduce != "max":
        assert (arg == -1).all()
    return out, arg, cnt


def test_inputs_hold_what_they_promise():
    for k in KS:
        for it in (np.int64, np.int32):
            kinds = gr.idx_kinds(gr.make_idx(N_Q, k, M_ROWS, ROWS, 7 + k, it), M_ROWS, ROWS)
            assert all(kinds.values()), (k, kinds)
    for dtype in DTYPES:
        for C in (3, 33):
            f = pr.make_tie_table(M_ROWS, C, dtype, 5)
            assert set(np.unique(np.abs(f[np.isfinite(f)]))) == {0.0, 1.0, 2.0} and np.isinf(f).any() and np.signbit(f[f == 0]).any() and not np.signbit(f[f == 0]).all()
            t = pr.tie_kinds(f, gr.make_idx(N_Q, 8, M_ROWS, ROWS, 6), ROWS)
            assert t["tied_maximum"] >= t["queries"] * C // 4 and t["signed_zero_tie"] >= 1, t
        f, idx, where = pr.make_nan_case(N_Q, 8, M_ROWS, 3, dtype, 9)
        assert {0, 1, 2} <= set(where.tolist()) and (where == -1).any()
        live = gr.live_slots(idx, M_ROWS, M_ROWS)
        for i in np.flatnonzero(where >= 0):
            ls = np.flatnonzero(live[i])
            nans = [s for s in ls if np.isnan(f[idx[i, s], 0])]
            assert nans[0] == (ls[0], ls[len(ls) // 2], ls[-1])[where[i]]
        assert any(sum(np.isnan(f[idx[i, s], 0]) for s in np.flatnonzero(live[i])) == 2 for i in np.flatnonzero(where == 0))


@pytest.mark.parametrize("it", [np.int64, np.int32])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rules_match_reference(check, dtype, it):
    """fails without the pool rules of dicp_group.h.  max and sum bit for bit with argmax and counts; the mean within its bound -- the
    restatement itself first (at most 0.64 of the bound), then the header"""
    worst = 0.0
    for k in KS:
        for C in CS:
            idx = gr.make_idx(N_Q, k, M_ROWS, ROWS, 13 * k + C, it)
            f = _table(M_ROWS, C, dtype, k + C)
            for reduce in ("max", "sum"):
                assert pr.same_result(_header(check, f, idx, reduce, ROWS), pr.pool_ref(f, idx, reduce, ROWS)), (reduce, k, C)
            ref = pr.pool_ref(f, idx, "mean", ROWS)
            r = pr.mean_ratio(ref[0], f, idx, ROWS)
            worst = max(worst, r)
            assert r <= 0.64, (k, C, r)
            out, arg, cnt = _header(check, f, idx, "mean", ROWS)
            assert pr.mean_ratio(out, f, idx, ROWS) <= 1.0 and np.array_equal(cnt, ref[2]) and (out[cnt == 0] == 0).all(), (k, C)
    print("restatement: mean %.3f of its bound" % worst)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_and_nans(check, dtype):
    for C in (3, 33):
        f = pr.make_tie_table(M_ROWS, C, dtype, 21 + C)
        idx = gr.make_idx(N_Q, 8, M_ROWS, ROWS, 22)
        assert pr.same_result(_header(check, f, idx, "max", ROWS), pr.pool_ref(f, idx, "max", ROWS))
        assert pr.same_result(_header(check, f, idx, "sum", ROWS), pr.pool_ref(f, idx, "sum", ROWS), nan_ok=True)
        f, idx, where = pr.make_nan_case(N_Q, 8, M_ROWS, C, dtype, 23 + C)
        got = _header(check, f, idx, "max", M_ROWS)
        assert pr.same_result(got, pr.pool_ref(f, idx, "max", M_ROWS))
        assert np.isnan(got[0][where >= 0]).all() and not np.isnan(got[0][where < 0]).any()
        assert (got[1][where >= 0] == (M_ROWS - 3 + where[where >= 0])[:, None]).all()        # the FIRST NaN's row


def test_only_the_last_slot_live(check):
    f = _table(M_ROWS, 3, np.float32, 1)
    idx = np.full((4, 8), -1, dtype=np.int64)
    idx[:3, 7] = [0, 5, ROWS - 1]
    for reduce in pr.REDUCES:
        out, arg, cnt = _header(check, f, idx, reduce, ROWS)
        assert gr.same_bits(out[:3], f[[0, 5, ROWS - 1]] + np.float32(0)) and (out[3] == 0).all() and cnt.tolist() == [1, 1, 1, 0]
        if reduce == "max":
            assert (arg[:3] == np.array([0, 5, ROWS - 1])[:, None]).all() and (arg[3] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_comparison_refuses_wrong_restatements(dtype):
    """`>=` in place of `>`, a lost slot, a NaN that does not propagate, argmax as the slot number: each differs from the definition on
    the inputs of this file, so a kernel that made the same mistake would be refused"""
    idx = gr.make_idx(N_Q, 8, M_ROWS, ROWS, 31)
    ties = pr.make_tie_table(M_ROWS, 3, dtype, 32)
    good = pr.pool_ref(ties, idx, "max", ROWS)
    assert pr.same_result(good, pr.pool_ref(ties, idx, "max", ROWS))
    assert not pr.same_result(pr.pool_ref(ties, idx, "max", ROWS, tie=">="), good)
    assert not pr.same_result(pr.pool_ref(ties, idx, "max", ROWS, argmax_row=False), good)
    plain = _table(M_ROWS, 3, dtype, 33)
    for reduce in ("max", "sum"):
        assert not pr.same_result(pr.pool_ref(plain, idx, reduce, ROWS, lose_slot=True), pr.pool_ref(plain, idx, reduce, ROWS))
    near = (0.5 + np.random.default_rng(34).random((M_ROWS, 3))).astype(dtype)          # one sign, a factor of 3: a lost term is far outside the bound
    lost = pr.pool_ref(near, idx, "mean", ROWS, lose_slot=True)
    assert pr.mean_ratio(pr.pool_ref(near, idx, "mean", ROWS)[0], near, idx, ROWS) <= 1.0 and pr.mean_ratio(lost[0], near, idx, ROWS) > 1.0
    f, nidx, where = pr.make_nan_case(N_Q, 8, M_ROWS, 3, dtype, 35)
    assert not pr.same_result(pr.pool_ref(f, nidx, "max", M_ROWS, nan_propagates=False), pr.pool_ref(f, nidx, "max", M_ROWS))


@pytest.mark.parametrize("dtype", DTYPES)
def test_mean_gradient_quotient(check, dtype):
    g = _table(1, 400, dtype, 3)[0]
    cnt = np.random.default_rng(4).integers(1, 33, size=400).astype(np.int32)
    out = np.empty_like(g)
    getattr(check, "pc_mean_grad_" + SFX[dtype])(_ptr(g), _ptr(cnt), 400, _ptr(out))
    assert gr.same_bits(out, (g / cnt.astype(dtype)).astype(dtype))


def test_entry_points_reject_bad_arguments():
    """an unknown reduce, nulls, MAX without argmax and the reverse, k = 33, C = 0, misaligned pointers: refused before any launch"""
    _lib.build()
    lib = _lib.load()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)

    def call(fn, good, **kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return fn(*a)
    # dicp_pool_forward(dtype, features, idx, idx64, rows, reduce, N, n, m, k, C, out, argmax, counts, stream)
    good = [0, one, one, 1, None, 2, 1, 10, 20, 4, 3, one, one, one, None]
    fwd = lib.dicp_pool_forward
    assert [call(fwd, good, **{a: None}) for a in ("a1", "a2", "a11", "a13")] == [1] * 4
    assert call(fwd, good, a5=3) == 4 and call(fwd, good, a5=-1) == 4 and call(fwd, good, a3=2) == 4 and call(fwd, good, a0=7) == 3
    assert call(fwd, good, a12=None) == 1                                                   # MAX without argmax
    assert call(fwd, good, a5=0) == 4 and call(fwd, good, a5=1) == 4                        # SUM / MEAN with argmax
    assert call(fwd, good, a9=33) == 2 and call(fwd, good, a9=0) == 2 and call(fwd, good, a10=0) == 2 and call(fwd, good, a6=0) == 2
    assert [call(fwd, good, **{a: odd}) for a in ("a1", "a2", "a4", "a11", "a12", "a13")] == [5] * 6
    assert call(fwd, [1, one, one, 0, None, 0, 1, 10, 20, 4, 3, one, None, one, None], a1=ctypes.c_void_p(260)) == 5      # float64 at 4 mod 8
    # dicp_pool_backward(dtype, grad_out, idx, idx64, rows, reduce, argmax, counts, N, n, m, k, C, grad_features, stream)
    good = [0, one, one, 1, None, 2, one, one, 1, 10, 20, 4, 3, one, None]
    bwd = lib.dicp_pool_backward
    assert [call(bwd, good, **{a: None}) for a in ("a1", "a2", "a13", "a6")] == [1] * 4
    assert call(bwd, good, a5=1, a6=None, a7=None) == 1                                     # MEAN without counts
    assert call(bwd, good, a5=0) == 4 and call(bwd, good, a5=9) == 4 and call(bwd, good, a0=2) == 3 and call(bwd, good, a3=-1) == 4
    assert call(bwd, good, a11=33) == 2 and call(bwd, good, a12=0) == 2
    assert [call(bwd, good, **{a: odd}) for a in ("a1", "a2", "a6", "a7", "a13")] == [5] * 5
    assert lib.dicp_abi_version() == 11


F, I = torch.zeros(20, 4), torch.zeros(10, 3, dtype=torch.int64)


def test_bad_arguments_raise():
    for reduce in ("min", "MAX", "", None, 2, b"max"):
        with pytest.raises(ValueError):
            pool_neighbors(F, I, reduce)
    for reduce in ("mean", "sum"):
        with pytest.raises(ValueError):
            pool_neighbors(F, I, reduce, return_argmax=True)
    bad = [(torch.zeros(20, 0), I), (F, torch.zeros(10, 0, dtype=torch.int64)), (F, torch.zeros(10, 33, dtype=torch.int64)), (F, torch.zeros(10, 3)),
           (F, torch.zeros(10, 3, dtype=torch.int16)), (F.to(torch.float16), I), (F.long(), I), ("abc", I), (F, np.zeros((10, 3), dtype=np.int64)),
           (F, torch.zeros(2, 10, 3, dtype=torch.int64)), (torch.zeros(2, 20, 4), I), ([F], I), (F, [I]), ([F, F], [I]),
           ([F, F.double()], [I, I]), (torch.zeros(0, 4), I), (F, torch.zeros(0, 3, dtype=torch.int64)), ([], []), (F, torch.zeros(10, dtype=torch.int64))]
    for f, i in bad:
        for reduce in pr.REDUCES:
            with pytest.raises(ValueError):
                pool_neighbors(f, i, reduce)
    with pytest.raises(ValueError):
        pool_neighbors([F], [I], rows=[20])
    with pytest.raises(ValueError):
        pool_neighbors(F, I, rows=[20])
    for rows in ([21, 3], [-1, 3], [1.0, 2.0], [3]):
        with pytest.raises(ValueError):
            pool_neighbors(torch.zeros(2, 20, 4), torch.zeros(2, 10, 3, dtype=torch.int64), rows=rows)


def test_valid_arguments_pass_the_checks():
    """what the refusals above leave through reaches the device (and, without one, its error)"""
    calls = [lambda: pool_neighbors(torch.zeros(20, 1), torch.zeros(10, 1, dtype=torch.int32), "max", return_argmax=True, return_counts=True),
             lambda: pool_neighbors(torch.zeros(2, 20, 4, dtype=torch.float64), torch.zeros(2, 10, 32, dtype=torch.int64), "mean", rows=torch.tensor([20, 0]), return_counts=True),
             lambda: pool_neighbors([F, torch.zeros(5, 4)], [I, torch.zeros(7, 3, dtype=torch.int64)], "sum")]
    for c in calls:
        if torch.cuda.is_available():
            c()
        else:
            with pytest.raises(RuntimeError, match="no HIP device"):
                c()
