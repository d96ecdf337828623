"""CPU checks of invert_neighbors and of the deterministic feature gradients (dicp_amd/group.py) that need no GPU.

The rules of ``dicp_amd/csrc/dicp_inverse.h`` -- the lines the HIP kernels run -- are compiled with g++ through
tests/hostcheck/inverse_check.cpp, run in a serial loop and held to the numpy restatement tests/inverse_ref.py bit for bit: the sort key
with its liveness and the offsets rule, and every operator's gradient -- the list walk with its clamps and its entry check, the chunked
sum, the first-of-query rule of the maximum -- in float32 and float64, with int32 and int64 indices, element by element and in the 16-byte
packs of the wide form.  The inputs are asserted to hold what they promise; the comparison is shown to refuse five deliberately wrong
restatements; garbage offsets / slots leave every access inside the arrays (guard regions); and the argument checks of the five entry
points and of the Python front run before any device work.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib
from dicp_amd.group import DET_CHUNK, group_points, interpolate_features, invert_neighbors, pool_neighbors

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import group_ref as gr  # noqa: E402
import hostbuild  # noqa: E402
import inverse_ref as ir  # noqa: E402
import pool_ref as pr  # noqa: E402

DTYPES = [np.float32, np.float64]
ITYPES = [np.int64, np.int32]
SFX = {np.float32: "f32", np.float64: "f64"}
ISFX = {np.int64: "i64", np.int32: "i32"}
OPCODE = {"group": 0, "sum": 1, "mean": 2, "max": 3, "interp": 4}
EPS = 1e-8
D = DET_CHUNK


@pytest.fixture(scope="module")
def check():
    lib = hostbuild.build("inverse_check.cpp", "inverse_check", ("-Wall",))
    for w in ISFX.values():
        getattr(lib, "ic_invert_" + w).restype = None
        for s in SFX.values():
            fn = getattr(lib, "ic_det_%s_%s" % (s, w))
            fn.restype = None
            fn.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_double] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _table(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random(shape) * 2 - 1) * 10.0 ** rng.integers(-2, 3, size=shape)).astype(dtype)


def _header_invert(check, idx, m, rows):
    n, k = idx.shape
    off, slots = np.full(m + 1, -7, dtype=np.int32), np.full(n * k, -7, dtype=np.int32)
    getattr(check, "ic_invert_" + ISFX[idx.dtype.type])(_ptr(np.ascontiguousarray(idx)), int(rows), n, k, m, _ptr(off), _ptr(slots))
    return off, slots


def _case(op, n, k, m, rows, C, dtype, it, seed, idx=None):
    """the arguments of one operator's gradient on one cloud: a dict for det_grad_ref / _header_det"""
    idx = ir.make_idx(n, k, m, rows, seed, it) if idx is None else idx.astype(it)
    a = {"op": op, "idx": idx, "m": m, "rows": rows, "g": _table((n, k, C) if op == "group" else (n, C), dtype, seed + 1)}
    if op in ("mean", "max"):
        f = pr.make_tie_table(m, C, dtype, seed + 2) if op == "max" else _table((m, C), dtype, seed + 2)
        _, a["argmax"], a["counts"] = pr.pool_ref(f, np.where(ir.slot_rows(idx, m, rows) >= 0, idx, -1).astype(np.int64), op, rows)
    if op == "interp":
        a["d2"], a["eps"] = gr.make_d2(n, k, seed + 3, dtype), EPS
    a["offsets"], a["slots"] = ir.invert_ref(idx, m, rows)
    return a


def _ref(a, **kw):
    return ir.det_grad_ref(a["op"], a["g"], a["idx"], a["m"], a["rows"], a["offsets"], a["slots"], a.get("argmax"), a.get("counts"), a.get("d2"), a.get("eps"), **kw)


def _header_det(check, a, packs=1, offsets=None, slots=None, out=None):
    g, idx = np.ascontiguousarray(a["g"]), np.ascontiguousarray(a["idx"])
    n, k = idx.shape
    C = g.shape[-1]
    out = np.full((a["m"], C), 7, dtype=g.dtype) if out is None else out
    off = a["offsets"] if offsets is None else offsets
    sl = a["slots"] if slots is None else slots
    if packs != 1:
        assert C % (16 // g.itemsize) == 0 and g.ctypes.data % 16 == 0 and out.ctypes.data % 16 == 0
    getattr(check, "ic_det_%s_%s" % (SFX[g.dtype.type], ISFX[idx.dtype.type]))(
        OPCODE[a["op"]], packs, _ptr(g), _ptr(idx), _ptr(a.get("argmax")), _ptr(a.get("counts")), _ptr(a.get("d2")), float(a.get("eps", 0.0)),
        n, k, C, int(a["rows"]), a["m"], _ptr(off), _ptr(sl), _ptr(out))
    return out


def test_chunk_constant(check):
    assert check.ic_chunk() == D and 16 <= D <= 256 and D & (D - 1) == 0
    assert [check.ic_passes(m) for m in (1, 254, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 31 - 2)] == [1, 1, 1, 2, 2, 3, 3, 4, 4]


def test_inputs_hold_what_they_promise():
    for k in (3, 8):
        for it in ITYPES:
            idx = ir.make_idx(120, k, 257, 200, 7 + k, it)
            assert all(gr.idx_kinds(np.where(np.abs(idx.astype(np.int64)) < 2 ** 31, idx, -1), 257, 200).values())
            assert all(ir.idx_kinds(idx, 257, 200).values()), ir.idx_kinds(idx, 257, 200)
    idx = ir.make_degree_idx(200, 8, 40, {3: D - 1, 5: D, 7: D + 1, 9: 3 * D + 5, 11: 1}, 1)
    off, _ = ir.invert_ref(idx, 40)
    assert {j: int(off[j + 1] - off[j]) for j in (3, 5, 7, 9, 11, 12)} == {3: D - 1, 5: D, 7: D + 1, 9: 3 * D + 5, 11: 1, 12: 0}


@pytest.mark.parametrize("it", ITYPES)
def test_index_matches_reference(check, it):
    """fails without dicp_inverse.h: the key (liveness on the index's full width, empty slots last) and the offsets from the sorted keys"""
    for n, k, m, rows in [(120, 8, 257, 200), (63, 3, 2000, 2000), (1, 1, 1, 1), (1, 1, 1, 0), (50, 32, 7, 5), (701, 8, 257, 257)]:
        idx = ir.make_idx(n, k, m, rows, n + k, it)
        if n == 701:
            idx[:] = rows - 1
        off, slots = _header_invert(check, idx, m, rows)
        roff, rslots = ir.invert_ref(idx, m, rows)
        assert np.array_equal(off, roff) and np.array_equal(slots, rslots), (n, k, m)
        live = int((ir.slot_rows(idx, m, rows) >= 0).sum())
        assert off[0] == 0 and (off[rows:] == live).all() and (slots[live:] == -1).all() and (np.diff(off) >= 0).all()
        for j in np.flatnonzero(np.diff(off) > 1)[:20]:
            assert (np.diff(slots[off[j]:off[j + 1]]) > 0).all()


@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", ir.OPS)
def test_gradients_match_reference(check, op, dtype, it):
    """bit for bit, element by element and in packs"""
    for n, k, m, rows, C in [(120, 8, 60, 50, 3), (63, 3, 257, 200, 8), (40, 32, 12, 9, 4)]:
        a = _case(op, n, k, m, rows, C, dtype, it, 11 * n + C)
        ref = _ref(a)
        assert gr.same_bits(_header_det(check, a), ref), (n, k, C)
        if C % (16 // np.dtype(dtype).itemsize) == 0:
            assert gr.same_bits(_header_det(check, a, packs=16), ref), (n, k, C)
        deg = np.diff(a["offsets"])
        assert (deg == 0).any() and (ref[deg == 0] == 0).all() and not np.signbit(ref[deg == 0]).any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", ir.OPS)
def test_list_lengths_around_a_chunk(check, op, dtype):
    """lists shorter than one chunk, of exactly D, D + 1 and several chunks (with a remainder and without)"""
    degrees = {3: D - 1, 5: D, 7: D + 1, 9: 3 * D + 5, 11: 1, 13: 4 * D}
    idx = ir.make_degree_idx(2 * D + 40, 8, 40, degrees, 5)
    a = _case(op, idx.shape[0], 8, 40, 40, 3, dtype, np.int64, 70, idx=idx)
    if op == "max":
        a["argmax"] = np.where(np.random.default_rng(1).integers(0, 4, size=a["argmax"].shape) > 0, a["argmax"], -1).astype(np.int32)
    ref = _ref(a)
    assert gr.same_bits(_header_det(check, a), ref)
    assert (ref[[3, 5, 7, 9, 13]] != 0).all() if op != "max" else (ref[[3, 5, 7, 9, 13]] != 0).any(1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_comparison_refuses_wrong_restatements(dtype):
    """a wrong chunk size, descending entry order, a lost entry, a duplicate counted twice in the maximum, an int64 index truncated to 32
    bits: each differs from the definition on the inputs of this file, so a kernel that made the same mistake would be refused"""
    degrees = {3: D - 1, 5: D, 7: D + 1, 9: 3 * D + 5, 11: D // 2}
    idx = ir.make_degree_idx(2 * D + 40, 8, 40, degrees, 6)
    a = _case("sum", idx.shape[0], 8, 40, 40, 3, dtype, np.int64, 80, idx=idx)
    good = _ref(a)
    assert gr.same_bits(good, _ref(a))
    for Dw in (D // 2, 2 * D):
        bad = _ref(a, D=Dw)
        assert not gr.same_bits(bad, good) and gr.same_bits(bad[[11]], good[[11]])        # a list inside both chunk sizes agrees
    assert not gr.same_bits(_ref(a, wrong="descending"), good)
    assert not gr.same_bits(_ref(a, wrong="lose_entry"), good)
    b = _case("max", 120, 8, 60, 50, 3, dtype, np.int64, 81)
    row = ir.slot_rows(b["idx"], 60, 50)
    twice = [(i, c) for i in range(120) for c in range(3) if b["argmax"][i, c] >= 0 and (row[i] == b["argmax"][i, c]).sum() >= 2]
    assert twice                                            # a query naming its argmax row in several slots
    assert not gr.same_bits(_ref(b, wrong="max_counts_duplicates"), _ref(b))
    c = _case("group", 120, 8, 60, 50, 3, dtype, np.int64, 82)
    toff, tslots = ir.invert_ref(c["idx"], 60, 50, truncate=True)                            # the index such a kernel would build, and its walk
    assert not np.array_equal(toff, c["offsets"]) and not np.array_equal(tslots, c["slots"])
    assert not gr.same_bits(_ref(dict(c, offsets=toff, slots=tslots), wrong="truncate_index"), _ref(c))


@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("op", ir.OPS)
def test_garbage_index_stays_in_range(check, op, it):
    """offsets / slots that are negative, huge, non-monotone, or name slots of other rows: every array sits between guard regions --
    NaN around the cotangent, a pattern around the output -- the output holds no NaN that a read outside would bring, and the guards
    are unchanged; a slot number naming another row contributes nothing"""
    n, k, m, rows, C = 40, 8, 30, 25, 3
    a = _case(op, n, k, m, rows, C, np.float32, it, 90)
    rng = np.random.default_rng(91)
    G = 4096
    gbuf = np.full(a["g"].size + 2 * G, np.nan, dtype=np.float32)
    gbuf[G:-G] = a["g"].reshape(-1)
    a["g"] = gbuf[G:-G].reshape(a["g"].shape)
    obuf = np.full(m * C + 2 * G, 12345.0, dtype=np.float32)
    big = [-1, -2 ** 31, 2 ** 31 - 1, n * k, n * k + 1, -5, 10 ** 9]
    for trial in range(6):
        off = rng.choice(big + list(range(n * k)), size=m + 1).astype(np.int32)              # any order: hi < lo among them
        sl = rng.choice(big + list(range(n * k)), size=n * k).astype(np.int32)
        if trial == 0:
            off, sl = a["offsets"].copy(), rng.permutation(a["slots"]).astype(np.int32)      # valid lists, entries naming other rows
        out = obuf[G:-G].reshape(m, C)
        out[:] = 7
        _header_det(check, a, offsets=off, slots=sl, out=out)
        assert (obuf[:G] == 12345.0).all() and (obuf[-G:] == 12345.0).all()
        assert not np.isnan(out).any()
        want = ir.det_grad_ref(op, a["g"], a["idx"], m, rows, off, sl, a.get("argmax"), a.get("counts"), a.get("d2"), a.get("eps"))
        assert gr.same_bits(out, want)


# ------------------------------------------------------------------ the entry points' status codes
NULL, SHAPE, DTYPE, ENUM, ALIGN = 1, 2, 3, 4, 5
F32, F64 = _lib.F32, _lib.F64
BIG = 1 << 62


def P(addr):
    return ctypes.c_void_p(addr)


OK = P(4096)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def entry(fn, good):
    def call(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        assert a != list(good), "a valid call would launch"
        return fn(*a)
    return call


def all_equal(call, positions, value, code, **kw):
    got = {i: call(**dict(kw, **{"a%d" % i: value})) for i in positions}
    assert got == {i: code for i in positions}


def test_invert_neighbors_codes(lib):
    # (idx, idx64, rows, N, n, m, k, offsets, slots, workspace, workspace_bytes, stream)
    need = lib.dicp_invert_neighbors_workspace_bytes(2, 100, 70, 8)
    assert need > 0 and need % 256 == 0 and need <= 2 * (4 * 4 * 800 + 4 * 256) + 5 * 256
    f = entry(lib.dicp_invert_neighbors, [OK, 1, None, 2, 100, 70, 8, OK, OK, OK, need, None])
    all_equal(f, (0, 7, 8, 9), None, NULL)
    assert f(a1=2) == ENUM and f(a1=-1) == ENUM
    assert f(a3=0) == SHAPE and f(a4=0) == SHAPE and f(a5=0) == SHAPE and f(a6=0) == SHAPE and f(a6=33) == SHAPE
    assert f(a4=1 << 26, a6=32, a10=BIG) == SHAPE                                            # n k = 2^31
    assert f(a4=(1 << 26) - 1, a6=32, a3=1, a10=BIG, a7=P(4098)) == ALIGN                    # n k = 2^31 - 32 passes
    assert f(a10=need - 1) == SHAPE and f(a10=need, a7=P(4098)) == ALIGN
    assert f(a0=P(4096 + 4)) == ALIGN and f(a0=P(4096 + 2), a1=0) == ALIGN and f(a0=P(4096 + 4), a1=0, a7=P(4098)) == ALIGN
    all_equal(f, (2, 7, 8), P(4096 + 2), ALIGN)
    assert f(a9=P(4096 + 128)) == ALIGN                                                      # the workspace: 256 bytes
    assert f(a0=None, a1=2) == NULL and f(a1=2, a3=0) == ENUM and f(a6=33, a7=P(4098)) == SHAPE
    assert lib.dicp_invert_neighbors_workspace_bytes(2, 100, 70, 33) == 0 and lib.dicp_invert_neighbors_workspace_bytes(2, 1 << 26, 70, 32) == 0
    assert lib.dicp_invert_neighbors_workspace_bytes(0, 100, 70, 8) == 0 and lib.dicp_invert_neighbors_workspace_bytes(2, 100, 0, 8) == 0


def test_group_backward_det_codes(lib):
    # (dtype, grad_out, idx, idx64, rows, N, n, m, k, C, offsets, slots, grad_features, stream)
    f = entry(lib.dicp_group_backward_det, [F32, OK, OK, 1, None, 2, 100, 70, 8, 3, OK, OK, OK, None])
    all_equal(f, (1, 2, 10, 11, 12), None, NULL)
    assert f(a0=2) == DTYPE and f(a3=2) == ENUM
    assert f(a5=0) == SHAPE and f(a6=0) == SHAPE and f(a7=0) == SHAPE and f(a8=0) == SHAPE and f(a8=33) == SHAPE and f(a9=0) == SHAPE
    assert f(a6=1 << 26, a8=32) == SHAPE and f(a6=(1 << 26) - 1, a8=32, a1=P(4098)) == ALIGN
    all_equal(f, (1, 12, 4, 10, 11), P(4096 + 2), ALIGN)
    all_equal(f, (1, 12), P(4096 + 4), ALIGN, a0=F64)
    assert f(a2=P(4096 + 4)) == ALIGN and f(a2=P(4096 + 4), a3=0, a1=P(4098)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a5=0) == DTYPE and f(a8=33, a1=P(4098)) == SHAPE


def test_pool_backward_det_codes(lib):
    # (dtype, grad_out, idx, idx64, rows, reduce, argmax, counts, N, n, m, k, C, offsets, slots, grad_features, stream)
    f = entry(lib.dicp_pool_backward_det, [F32, OK, OK, 1, None, 2, OK, OK, 2, 100, 70, 8, 3, OK, OK, OK, None])
    all_equal(f, (1, 2, 13, 14, 15, 6), None, NULL)
    assert f(a5=1, a6=None, a7=None) == NULL                                                 # MEAN without counts
    assert f(a5=0) == ENUM and f(a5=1) == ENUM and f(a5=3) == ENUM and f(a5=-1) == ENUM      # SUM / MEAN with argmax; unknown
    assert f(a0=2) == DTYPE and f(a3=2) == ENUM
    assert f(a8=0) == SHAPE and f(a9=0) == SHAPE and f(a10=0) == SHAPE and f(a11=0) == SHAPE and f(a11=33) == SHAPE and f(a12=0) == SHAPE
    assert f(a9=1 << 26, a11=32) == SHAPE and f(a9=(1 << 26) - 1, a11=32, a1=P(4098)) == ALIGN
    all_equal(f, (1, 15, 4, 6, 7, 13, 14), P(4096 + 2), ALIGN)
    all_equal(f, (1, 15), P(4096 + 4), ALIGN, a0=F64)
    assert f(a2=P(4096 + 4)) == ALIGN
    assert f(a5=0, a6=None, a7=None, a1=P(4098)) == ALIGN and f(a5=1, a6=None, a1=P(4098)) == ALIGN
    assert f(a1=None, a5=9) == NULL and f(a5=9, a0=2) == ENUM and f(a0=2, a8=0) == DTYPE and f(a11=33, a1=P(4098)) == SHAPE


def test_interpolate_backward_det_codes(lib):
    # (dtype, grad_out, idx, idx64, rows, d2, eps, N, n, m, k, C, offsets, slots, grad_features, stream)
    f = entry(lib.dicp_interpolate_backward_det, [F32, OK, OK, 1, None, OK, 1e-8, 2, 100, 70, 8, 3, OK, OK, OK, None])
    all_equal(f, (1, 2, 5, 12, 13, 14), None, NULL)
    assert f(a0=2) == DTYPE and f(a3=2) == ENUM
    assert f(a7=0) == SHAPE and f(a8=0) == SHAPE and f(a9=0) == SHAPE and f(a10=0) == SHAPE and f(a10=33) == SHAPE and f(a11=0) == SHAPE
    assert f(a8=1 << 26, a10=32) == SHAPE and f(a8=(1 << 26) - 1, a10=32, a1=P(4098)) == ALIGN
    for eps in (0.0, -1.0, float("inf"), float("nan")):
        assert f(a6=eps) == SHAPE
    all_equal(f, (1, 5, 14, 4, 12, 13), P(4096 + 2), ALIGN)
    all_equal(f, (1, 5, 14), P(4096 + 4), ALIGN, a0=F64)
    assert f(a2=P(4096 + 4)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a7=0) == DTYPE and f(a6=0.0, a1=P(4098)) == SHAPE
    assert lib.dicp_abi_version() == _lib.ABI_VERSION


# ------------------------------------------------------------------ the Python front
F, I = torch.zeros(20, 4), torch.zeros(10, 3, dtype=torch.int64)
OFF, SL = torch.zeros(21, dtype=torch.int32), torch.full((30,), -1, dtype=torch.int32)


def _ops():
    return [lambda **kw: group_points(F, I, **kw), lambda **kw: pool_neighbors(F, I, "max", **kw), lambda **kw: pool_neighbors(F, I, "mean", **kw),
            lambda **kw: interpolate_features(F, I, torch.zeros(10, 3), **kw)]


def test_bad_deterministic_and_inverse_raise():
    for op in _ops():
        for det in (1, 0, None, "yes", torch.tensor(True)):
            with pytest.raises(ValueError):
                op(deterministic=det)
        bad = [OFF, (OFF,), (OFF, SL, SL), (OFF.long(), SL), (OFF, SL.float()), (OFF[:-1], SL), (OFF, SL[:-1]), (OFF[None], SL[None]), (OFF.numpy(), SL.numpy()),
               [(OFF, SL)], "abc", (SL, OFF)]
        for inv in bad:
            with pytest.raises(ValueError):
                op(inverse=inv)
    Fb, Ib = torch.zeros(2, 20, 4), torch.zeros(2, 10, 3, dtype=torch.int64)
    for inv in [(OFF, SL), (OFF[None], SL[None]), [(OFF, SL), (OFF, SL)], (OFF.expand(2, 21), SL.expand(2, 30)[:, :29])]:
        with pytest.raises(ValueError):
            group_points(Fb, Ib, inverse=inv)
    for inv in [(OFF, SL), [(OFF, SL)], [(OFF, SL), (OFF[:7], SL[:21])], [(OFF, SL), (OFF[:6], SL[:20])], [(OFF, SL), OFF]]:
        with pytest.raises(ValueError):
            pool_neighbors([F, F[:5]], [I, I[:7]], "sum", inverse=inv)


def test_bad_invert_arguments_raise():
    bad = [(I, 0), (I, -3), (I, 2.0), (I, True), (I, None), (I, [20]), (I, 2 ** 31 - 1), (I.float(), 20), (I.to(torch.int16), 20), (torch.zeros(10, 0, dtype=torch.int64), 20),
           (torch.zeros(10, 33, dtype=torch.int64), 20), (torch.zeros(10, dtype=torch.int64), 20), (torch.zeros(0, 3, dtype=torch.int64), 20), (I.numpy(), 20),
           ([I], 20), ([I], [20, 20]), ([I, I], [20]), ([I], [-1]), ([I], [2.0]), ([], []), ([I, I.int()], [20, 20]), ([I, I[None]], [20, 20])]
    for idx, m in bad:
        with pytest.raises(ValueError):
            invert_neighbors(idx, m)
    with pytest.raises(ValueError):
        invert_neighbors(I, 20, rows=[20])                  # rows need a padded batch
    with pytest.raises(ValueError):
        invert_neighbors([I], [20], rows=[20])
    for rows in ([21, 3], [-1, 3], [1.0, 2.0], [3], [[3, 3]]):
        with pytest.raises(ValueError):
            invert_neighbors(torch.zeros(2, 10, 3, dtype=torch.int64), 20, rows=rows)


def test_valid_arguments_pass_the_checks():
    """what the refusals above leave through reaches the device (and, without one, its error)"""
    Fg = F.clone().requires_grad_(True)
    calls = [lambda: invert_neighbors(I, 20), lambda: invert_neighbors(I.int()[None].expand(2, 10, 3), 20, rows=torch.tensor([20, 0])),
             lambda: invert_neighbors([I, I[:7]], [20, 0]),
             lambda: group_points(Fg, I, deterministic=True), lambda: pool_neighbors(Fg, I, "sum", inverse=(OFF, SL)),
             lambda: interpolate_features([F, F[:5]], [I, I[:7]], [torch.zeros(10, 3), torch.zeros(7, 3)], inverse=[(OFF, SL), (OFF[:6], SL[:21])])]
    for c in calls:
        if torch.cuda.is_available():
            c()
        else:
            with pytest.raises(RuntimeError, match="no HIP device"):
                c()
