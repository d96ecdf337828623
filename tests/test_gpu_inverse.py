"""invert_neighbors and the deterministic feature gradients of group_points / pool_neighbors / interpolate_features on the MI355X.

The inverted index against its numpy restatement (tests/inverse_ref.py) bit for bit -- every n x m x k of the feature tests, both index
widths, ragged rows, the three input forms, every kind of empty slot, hubs, one case past every tile and grid stride -- and the gradients
that walk it against the restatement of their order of summation, bit for bit for group_points and pool_neighbors; interpolate_features,
whose weights are held to a bound, against the atomic path where every row is named once (bit for bit), against float64 within the
bound of the atomic path, and against the same call with the non-finite slots emptied.  Then reproducibility, no host synchronisation,
a captured graph, and the README chain run twice."""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.ICP import ICP
from dicp_amd.ball import ball_query
from dicp_amd.fps import sample_farthest_points
from dicp_amd.group import DET_CHUNK, group_points, interpolate_features, invert_neighbors, pool_neighbors
from dicp_amd.knn import knn_points
from dicp_amd.voxel import voxel_downsample

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_ref as gr  # noqa: E402
import inverse_ref as ir  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
NS, MS, KS = (1, 63, 700), (1, 257, 2000), (1, 3, 8, 32)
CS = (1, 3, 4, 16, 33, 64, 65, 130)
EPS = 1e-8
D = DET_CHUNK


def _table(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random(shape) * 2 - 1) * 10.0 ** rng.integers(-2, 3, size=shape)).astype(dtype)


def _dev(a, misalign=False):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misalign:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _np(t):
    return t.detach().cpu().numpy()


def _rows_of(m):
    return [m * 3 // 4, m]


def _idx_batch(n, k, m, it, seed):
    rows = _rows_of(m)
    return np.stack([ir.make_idx(n, k, m, rows[b], seed + b, it) for b in range(2)]), rows


def _hold_index(idx, m, rows, got):
    off, slots = (_np(t) for t in got)
    assert off.dtype == np.int32 and slots.dtype == np.int32 and off.shape == (idx.shape[0], m + 1) and slots.shape == (idx.shape[0], idx.shape[1] * idx.shape[2])
    for b in range(idx.shape[0]):
        roff, rslots = ir.invert_ref(idx[b], m, None if rows is None else rows[b])
        assert np.array_equal(off[b], roff) and np.array_equal(slots[b], rslots), b


# ------------------------------------------------------------------ 1. the inverted index
@pytest.mark.parametrize("k", KS)
def test_index_matches_reference(k):
    """every n x m at this k, both index widths, with ragged rows and without; the tables hold -1, other negatives, values in [rows, m),
    values >= m, int64 values whose low 32 bits are a live row, and duplicates inside a query (inverse_ref.make_idx; asserted in
    tests/test_inverse_host.py)"""
    for a, n in enumerate(NS):
        for c, m in enumerate(MS):
            for it in (np.int64, np.int32):
                idx, rows = _idx_batch(n, k, m, it, 100 * k + 10 * a + c)
                _hold_index(idx, m, rows, invert_neighbors(_dev(idx), m, rows=torch.tensor(rows, dtype=torch.int32).cuda()))
                _hold_index(idx, m, None, invert_neighbors(_dev(idx), m))


@pytest.mark.parametrize("it", [np.int64, np.int32])
def test_index_input_forms_agree(it):
    n, m, k = 63, 257, 8
    idx, rows = _idx_batch(n, k, m, it, 7)
    ns = [40, n]
    idx[0, ns[0]:] = -1
    idd, rd = _dev(idx), torch.tensor(rows, dtype=torch.int32).cuda()
    off, slots = invert_neighbors(idd, m, rows=rd)
    _hold_index(idx, m, rows, (off, slots))
    coff, cslots = invert_neighbors(torch.from_numpy(idx), m, rows=torch.tensor(rows))
    assert not coff.is_cuda and not cslots.is_cuda and torch.equal(coff, off.cpu()) and torch.equal(cslots, slots.cpu())
    lists = invert_neighbors([idd[b, :ns[b]] for b in range(2)], rows)
    assert isinstance(lists, list) and len(lists) == 2
    for b in range(2):
        lo, ls = lists[b]
        assert lo.is_cuda and lo.shape == (rows[b] + 1,) and ls.shape == (ns[b] * k,)
        assert torch.equal(lo, off[b, :rows[b] + 1]) and torch.equal(ls, slots[b, :ns[b] * k])
        assert (off[b, rows[b]:] == lo[-1]).all() and (slots[b, ns[b] * k:] == -1).all()
    so, ss = invert_neighbors(idd[1], m)                                                          # a single cloud: the one whose table is all live
    assert so.shape == (m + 1,) and ss.shape == (n * k,) and torch.equal(so, off[1]) and torch.equal(ss, slots[1])


@pytest.mark.parametrize("it", [np.int64, np.int32])
def test_index_of_hubs(it):
    """every slot naming row 0, and every slot naming row rows[b] - 1: 701 x 8 on 257 rows (in-degree 5608, one digit bucket)"""
    n, m, k = 701, 257, 8
    rows = [200, m]
    idx = np.stack([np.zeros((n, k), dtype=it), np.zeros((n, k), dtype=it)])
    _hold_index(idx, m, rows, invert_neighbors(_dev(idx), m, rows=torch.tensor(rows, dtype=torch.int32).cuda()))
    idx = np.stack([np.full((n, k), rows[b] - 1, dtype=it) for b in range(2)])
    off, slots = invert_neighbors(_dev(idx), m, rows=torch.tensor(rows, dtype=torch.int32).cuda())
    _hold_index(idx, m, rows, (off, slots))
    assert torch.equal(slots[0], torch.arange(n * k, dtype=torch.int32, device="cuda")) and int(off[0, rows[0] - 1]) == 0 and int(off[0, rows[0]]) == n * k


def test_index_beyond_a_tile_and_three_digits():
    """N = 3, n = 5000, k = 32: 160000 slots a cloud are 40 tiles of 4096 and 625 workgroups of the flat kernels a cloud; m = 70000 needs
    three 8-bit digits (both ping-pong directions of the sort), and the digit scan takes 10 tiles per thread group"""
    N, n, k, m = 3, 5000, 32, 70000
    rng = np.random.default_rng(3)
    idx = rng.integers(-2, m + 5, size=(N, n, k))
    idx[1, :, :16] = 69999                                   # a hub of 80000 in the last row
    rows = [m, m, 1234]
    _hold_index(idx, m, rows, invert_neighbors(_dev(idx), m, rows=torch.tensor(rows, dtype=torch.int32).cuda()))


# ------------------------------------------------------------------ 2. deterministic gradients against the restatement
def _cot(shape, tdt, seed):
    gen = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=gen, dtype=torch.float64) + 0.5) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).to(tdt).cuda()


def _det_grads(f, idx, rows, cen, seed, misalign=False, inverse=None, ops=("group", "group_c", "sum", "mean", "max")):
    """the deterministic gradients into the features of one batch (N, ...) -> {op: (g_features (N, m, C), cotangent, argmax, counts)}.
    The cotangent holds NaN / inf at empty slots (group) and at queries without a live slot (pool)."""
    dtype = f.dtype.type
    tdt = TORCH[dtype]
    N, m, C = f.shape
    n, k = idx.shape[1:]
    idd = _dev(idx)
    rd = torch.tensor(rows, dtype=torch.int32).cuda() if rows is not None else None
    live = torch.from_numpy(np.stack([ir.slot_rows(idx[b], m, None if rows is None else rows[b]) >= 0 for b in range(N)])).cuda()
    kw = {"deterministic": True} if inverse is None else {"inverse": inverse}
    res = {}
    for o, op in enumerate(ops):
        fd = _dev(f, misalign).requires_grad_(True)
        if op.startswith("group"):
            g = _cot((N, n, k, C), tdt, seed + o)
            g = torch.where(live[..., None], g, torch.full_like(g, float("nan") if o % 2 else float("inf")))
            out = group_points(fd, idd, rows=rd, centers=_dev(cen) if op == "group_c" else None, **kw)
            am = cnt = None
        else:
            g = _cot((N, n, C), tdt, seed + o)
            g = torch.where(live.any(2)[..., None], g, torch.full_like(g, float("nan") if o % 2 else float("-inf")))
            r = pool_neighbors(fd, idd, op, rows=rd, return_argmax=op == "max", return_counts=True, **kw)
            out, am, cnt = r[0], (r[1] if op == "max" else None), r[-1]
        if misalign:
            buf = torch.empty(g.numel() + 1, dtype=g.dtype, device="cuda")
            gv = buf[1:].view(g.shape)
            gv.copy_(g)
            g = gv
        out.backward(g)
        res[op] = (_np(fd.grad), _np(g), None if am is None else _np(am), None if cnt is None else _np(cnt))
    return res


def _hold_det(f, idx, rows, cen, seed, misalign=False, ops=("group", "group_c", "sum", "mean", "max")):
    N, m, C = f.shape
    res = _det_grads(f, idx, rows, cen, seed, misalign, ops=ops)
    for op, (gf, g, am, cnt) in res.items():
        for b in range(N):
            rb = None if rows is None else rows[b]
            off, slots = ir.invert_ref(idx[b], m, rb)
            want = ir.det_grad_ref("group" if op.startswith("group") else op, g[b], idx[b], m, rb, off, slots, None if am is None else am[b], None if cnt is None else cnt[b])
            assert gr.same_bits(gf[b], want), (op, b)
            deg = np.diff(off)
            assert np.isfinite(gf[b]).all() and (gf[b][deg == 0] == 0).all() and not np.signbit(gf[b][deg == 0]).any()
    return res


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CS)
def test_gradients_match_reference(C, dtype):
    """group_points with and without centers, pool_neighbors sum / mean / max: bit for bit, both index widths; n, m and k going round"""
    o = CS.index(C)
    n, m, k = (63, 200)[o % 2], (257, 700)[(o // 2) % 2], KS[1 + o % 3]
    for it in (np.int64, np.int32):
        idx, rows = _idx_batch(n, k, m, it, 300 + C)
        _hold_det(_table((2, m, C), dtype, 310 + C), idx, rows, _table((2, n, min(3, C)), dtype, 320 + C), 330 + C)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_from_a_misaligned_base(dtype):
    for C in (16, 64):
        idx, rows = _idx_batch(63, 8, 257, np.int64, 400 + C)
        _hold_det(_table((2, 257, C), dtype, 410 + C), idx, rows, _table((2, 63, 3), dtype, 420), 430 + C, misalign=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [3, 64])
def test_gradient_of_a_hub(C, dtype):
    """700 x 8 slots on row 5 of 257 (in-degree 5600: 87 chunks and a remainder) and one query without a live slot"""
    n, m, k = 701, 257, 8
    idx = np.full((1, n, k), 5, dtype=np.int64)
    idx[0, 700] = -1
    _hold_det(_table((1, m, C), dtype, 1), idx, None, _table((1, n, 3), dtype, 3), 600 + C)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lists_around_a_chunk_and_a_row_named_twice(dtype):
    """lists of D - 1, D, D + 1 and several chunks; under max, queries naming their argmax row in several slots send its cotangent once"""
    degrees = {3: D - 1, 5: D, 7: D + 1, 9: 3 * D + 5, 11: 1, 13: 4 * D}
    n, k, m = 2 * D + 40, 8, 40
    idx = ir.make_degree_idx(n, k, m, degrees, 5)[None]
    for C in (3, 64):
        _hold_det(_table((1, m, C), dtype, 700 + C), idx, None, _table((1, n, 3), dtype, 701), 710 + C)
    twice = np.stack([ir.make_idx(63, 8, 20, 20, 720 + b, np.int64) for b in range(2)])           # 20 rows, 8 slots: many repeats
    twice[:, ::3, 5] = twice[:, ::3, 2]
    f = _table((2, 20, 4), dtype, 730)
    res = _hold_det(f, twice, None, None, 740, ops=("max",))
    gf, g, am, _ = res["max"]
    row = np.stack([ir.slot_rows(twice[b], 20) for b in range(2)])
    named = (row[:, :, :, None] == am[:, :, None, :]) & (am[:, :, None, :] >= 0)                   # (N, n, k, C)
    assert (named.sum(2) >= 2).any()
    once = np.zeros((2, 20, 4), dtype=np.float64)
    for b, i, c in zip(*np.nonzero(am >= 0)):
        once[b, am[b, i, c], c] += g[b, i, c]
    u = float(np.finfo(dtype).eps)
    assert np.allclose(gf, once, rtol=0, atol=64 * u * np.abs(g[np.isfinite(g)]).max() * 63)       # a term counted twice is off by about |g| >= 0.5


# ------------------------------------------------------------------ 3. interpolate_features
def _interp_grads(f, idx, d2, rows, g, **kw):
    fd = _dev(f).requires_grad_(True)
    rd = torch.tensor(rows, dtype=torch.int32).cuda() if rows is not None else None
    interpolate_features(fd, _dev(idx), _dev(d2), eps=EPS, rows=rd, **kw).backward(g)
    return _np(fd.grad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [3, 64])
def test_every_row_named_once_equals_the_atomic_path(C, dtype):
    """0 + t is exact: where no row is named twice the deterministic gradients of all three operators are the atomic path's, bit for bit"""
    n, m, k = 63, 2000, 8
    rng = np.random.default_rng(800 + C)
    idx = np.stack([rng.permutation(m)[:n * k].reshape(n, k) for _ in range(2)]).astype(np.int64)
    idx[:, ::7, 3] = -1
    rows = _rows_of(m)
    f, d2 = _table((2, m, C), dtype, 801), np.stack([gr.make_d2(n, k, 802 + b, dtype) for b in range(2)])
    g = _cot((2, n, C), TORCH[dtype], 803)
    assert gr.same_bits(_interp_grads(f, idx, d2, rows, g, deterministic=True), _interp_grads(f, idx, d2, rows, g))
    idd, rd = _dev(idx), torch.tensor(rows, dtype=torch.int32).cuda()
    for op in ("group", "sum", "mean", "max"):
        got = []
        for det in (True, False):
            fd = _dev(f).requires_grad_(True)
            if op == "group":
                group_points(fd, idd, rows=rd, deterministic=det).backward(_cot((2, n, k, C), TORCH[dtype], 804))
            else:
                pool_neighbors(fd, idd, op, rows=rd, deterministic=det).backward(g)
            got.append(_np(fd.grad))
        assert gr.same_bits(got[0], got[1]) and (got[0] != 0).any(), op


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,k,C,it", [(700, 257, 8, 3, np.int64), (63, 2000, 3, 1, np.int32), (700, 257, 32, 33, np.int32), (63, 257, 8, 64, np.int64), (701, 257, 8, 64, np.int64)])
def test_interpolate_gradient_within_the_atomic_bound(n, m, k, C, it, dtype):
    """within (D_in + k + 8) u sum|terms| of the float64 sum of the terms w_s g[i, c] (test_gpu_group.py's _hold_gf: it holds for any
    order of summation), D_in the row's in-degree; rows nobody names exactly 0; a slot with a non-finite d2 sends nothing"""
    u = float(np.finfo(dtype).eps) / 2
    idx, rows = _idx_batch(n, k, m, it, 900 + C)
    if n == 701:
        idx[:] = 5                                           # the hub
    d2 = np.stack([gr.make_d2(n, k, 910 + b, dtype) for b in range(2)])
    d2[:, ::5, 0] = np.nan                                   # (make_d2 has +inf)
    f = _table((2, m, C), dtype, 920)
    g = _cot((2, n, C), TORCH[dtype], 930)
    got = _interp_grads(f, idx, d2, rows, g, deterministic=True)
    gn = _np(g).astype(np.float64)
    for b in range(2):
        live, r, R, w = gr._interp_weights(idx[b], d2[b].astype(np.float64), float(dtype(EPS)), m, rows[b], np.float64)
        assert (~np.isfinite(d2[b]) & (ir.slot_rows(idx[b], m, rows[b]) >= 0)).any()
        terms = np.where(live[..., None], w[..., None] * gn[b][:, None, :], 0.0)                  # (n, k, C)
        dest = np.where(live, idx[b], 0).reshape(-1)
        ref, mag, deg = np.zeros((m, C)), np.zeros((m, C)), np.zeros(m)
        np.add.at(ref, dest, terms.reshape(-1, C))
        np.add.at(mag, dest, np.abs(terms).reshape(-1, C))
        np.add.at(deg, dest, live.reshape(-1).astype(np.float64))
        err = np.abs(got[b].astype(np.float64) - ref)
        bound = (deg[:, None] + k + 8) * u * mag
        assert np.isfinite(got[b]).all() and (err <= bound).all(), float((err - bound).max())
        assert (got[b][deg == 0] == 0).all()
    short = all(np.diff(ir.invert_ref(idx[b], m, rows[b])[0]).max() <= D for b in range(2))
    assert short or n != 63
    if short:                                                # lists within one chunk: emptying the non-finite slots moves no chunk boundary
        emptied = np.where(np.isfinite(d2), idx, -1).astype(it)
        assert gr.same_bits(got, _interp_grads(f, emptied, np.where(np.isfinite(d2), d2, 1).astype(dtype), rows, g, deterministic=True))


# ------------------------------------------------------------------ 4. reproducibility
def _all_grads(f, idx, d2, cen, rows, seed, **kw):
    """the bytes of every gradient of the three operators (features, centers, d2)"""
    tdt = TORCH[f.dtype.type]
    N, n, k = idx.shape
    C = f.shape[2]
    idd, rd = _dev(idx), torch.tensor(rows, dtype=torch.int32).cuda() if rows is not None else None
    out = []
    fd, cd = _dev(f).requires_grad_(True), _dev(cen).requires_grad_(True)
    group_points(fd, idd, rows=rd, centers=cd, **kw).backward(_cot((N, n, k, C), tdt, seed))
    out += [fd.grad, cd.grad]
    for op in ("sum", "mean", "max"):
        fd = _dev(f).requires_grad_(True)
        pool_neighbors(fd, idd, op, rows=rd, **kw).backward(_cot((N, n, C), tdt, seed + 1))
        out.append(fd.grad)
    fd, dd = _dev(f).requires_grad_(True), _dev(d2).requires_grad_(True)
    interpolate_features(fd, idd, dd, eps=EPS, rows=rd, **kw).backward(_cot((N, n, C), tdt, seed + 2))
    out += [fd.grad, dd.grad]
    return [_np(t).tobytes() for t in out]


@pytest.mark.parametrize("hub", [False, True])
def test_runs_repeat(hub):
    """five calls give identical bytes for every gradient; deterministic=True and inverse= give the same bytes, one inverse shared by
    the three operators"""
    if hub:
        n, m, k, C, rows = 701, 257, 8, 64, None
        idx = np.full((1, n, k), 5, dtype=np.int64)
        idx[0, 700] = -1
        N = 1
    else:
        n, m, k, C = 700, 2000, 8, 64
        idx, rows = _idx_batch(n, k, m, np.int64, 11)
        N = 2
    f, cen = _table((N, m, C), np.float32, 12), _table((N, n, 3), np.float32, 13)
    d2 = np.stack([gr.make_d2(n, k, 14 + b, np.float32, near=True) for b in range(N)])
    runs = [_all_grads(f, idx, d2, cen, rows, 15, deterministic=True) for _ in range(5)]
    assert all(r == runs[0] for r in runs[1:])
    inv = invert_neighbors(_dev(idx), m, rows=torch.tensor(rows, dtype=torch.int32).cuda() if rows is not None else None)
    assert _all_grads(f, idx, d2, cen, rows, 15, inverse=inv) == runs[0]
    assert _all_grads(f, idx, d2, cen, rows, 15, inverse=inv, deterministic=True) == runs[0]


def test_list_form_with_inverse():
    """the lists' pairs go back in as they came out"""
    n, m, k, C = 63, 257, 8, 6
    idx, rows = _idx_batch(n, k, m, np.int64, 21)
    ns = [40, n]
    f = _table((2, m, C), np.float32, 22)
    idl, fl = [_dev(idx[b, :ns[b]]) for b in range(2)], [_dev(f[b, :rows[b]]) for b in range(2)]
    inv = invert_neighbors(idl, rows)
    got = []
    for kw in ({"deterministic": True}, {"inverse": inv}):
        leaves = [t.clone().requires_grad_(True) for t in fl]
        outs = pool_neighbors(leaves, idl, "sum", **kw)
        sum((o * (b + 1.5)).sum() for b, o in enumerate(outs)).backward()
        got.append([_np(t.grad) for t in leaves])
    for b in range(2):
        assert gr.same_bits(got[0][b], got[1][b]) and (got[0][b] != 0).any()
        off, slots = ir.invert_ref(idx[b, :ns[b]], rows[b])
        want = ir.det_grad_ref("sum", np.full((ns[b], C), b + 1.5, dtype=np.float32), idx[b, :ns[b]], rows[b], None, off, slots)
        assert gr.same_bits(got[0][b], want)


# ------------------------------------------------------------------ 5. no host synchronisation
def test_no_host_synchronisation():
    n, m, k, C = 700, 2000, 8, 64
    idx, rows = _idx_batch(n, k, m, np.int64, 31)
    f, cen = _table((2, m, C), np.float32, 32), _table((2, n, 3), np.float32, 33)
    d2 = np.stack([gr.make_d2(n, k, 34 + b, np.float32, near=True) for b in range(2)])
    fd, idd, dd, cd, rd = _dev(f).requires_grad_(True), _dev(idx), _dev(d2).requires_grad_(True), _dev(cen).requires_grad_(True), torch.tensor(rows, dtype=torch.int32).cuda()
    invert_neighbors(idd, m, rows=rd)                       # (the library is loaded)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        inv = invert_neighbors(idd, m, rows=rd)
        a = group_points(fd, idd, rows=rd, centers=cd, deterministic=True)
        p = pool_neighbors(fd, idd, "max", rows=rd, inverse=inv)
        i = interpolate_features(fd, idd, dd, eps=EPS, rows=rd, deterministic=True)
        (a.sum() + p.sum() + i.sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    _hold_index(idx, m, rows, inv)
    assert torch.isfinite(fd.grad).all() and (fd.grad != 0).any() and (dd.grad != 0).any() and (cd.grad != 0).any()


# ------------------------------------------------------------------ 6. a captured graph
@pytest.mark.parametrize("C", [3, 64])
def test_captured_forward_and_backward(C):
    """forward + backward of the three operators with deterministic=True (the index built inside the backward) captured once, replayed
    on new data in the same buffers behind synchronisations; the replayed gradients equal the restatement (interpolate_features: the
    eager call on the same data, which section 3 holds)"""
    N, n, m, k = 2, 63, 257, 8
    rows = _rows_of(m)
    rd = torch.tensor(rows, dtype=torch.int32).cuda()

    def data(seed):
        idx, _ = _idx_batch(n, k, m, np.int64, seed)
        return {"f": _dev(_table((N, m, C), np.float32, seed + 1)), "idx": _dev(idx), "g": _cot((N, n, C), torch.float32, seed + 2), "g4": _cot((N, n, k, C), torch.float32, seed + 3),
                "d2": _dev(np.stack([gr.make_d2(n, k, seed + 4 + b, np.float32, near=True) for b in range(N)])), "cen": _dev(_table((N, n, 3), np.float32, seed + 6))}

    def run(x):
        outs = {}
        f, cen = x["f"].detach().requires_grad_(True), x["cen"].detach().requires_grad_(True)
        outs["group"], outs["centers"] = torch.autograd.grad(group_points(f, x["idx"], rows=rd, centers=cen, deterministic=True), [f, cen], x["g4"])
        for op in ("sum", "mean", "max"):
            f = x["f"].detach().requires_grad_(True)
            r = pool_neighbors(f, x["idx"], op, rows=rd, return_argmax=op == "max", return_counts=True, deterministic=True)
            outs[op], = torch.autograd.grad(r[0], [f], x["g"])
            outs[op + "_aux"] = (r[1] if op == "max" else None, r[-1])
        f, d2 = x["f"].detach().requires_grad_(True), x["d2"].detach().requires_grad_(True)
        outs["interp"], outs["d2"] = torch.autograd.grad(interpolate_features(f, x["idx"], d2, eps=EPS, rows=rd, deterministic=True), [f, d2], x["g"])
        return outs

    static = data(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = run(static)
    for seed in (20, 30):
        fresh = data(seed)
        for key, t in fresh.items():
            static[key].copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(fresh)
        idx = _np(fresh["idx"])
        for b in range(N):
            off, slots = ir.invert_ref(idx[b], m, rows[b])
            assert gr.same_bits(_np(cap["group"][b]), ir.det_grad_ref("group", _np(fresh["g4"][b]), idx[b], m, rows[b], off, slots))
            for op in ("sum", "mean", "max"):
                am, cnt = cap[op + "_aux"]
                want = ir.det_grad_ref(op, _np(fresh["g"][b]), idx[b], m, rows[b], off, slots, None if am is None else _np(am[b]), _np(cnt[b]))
                assert gr.same_bits(_np(cap[op][b]), want), (op, seed, b)
        for key in ("interp", "d2", "centers", "group", "sum", "mean", "max"):
            assert gr.same_bits(_np(cap[key]), _np(eager[key])) and (cap[key] != 0).any(), (key, seed)


# ------------------------------------------------------------------ 7. the chain
def test_chain_gradients_repeat():
    """voxel -> FPS -> ball -> pool -> knn -> interpolate -> ICP(weight=) with deterministic=True on the feature operators, twice: the
    gradient of a scalar taken straight after interpolate_features (the part of the chain these operators own: no y-side atomics of
    knn_points / ball_query in its path) reaches the network's parameters with identical bytes; the ICP runs on the weights"""
    rng = np.random.default_rng(21)
    scan = torch.from_numpy((rng.random((2, 3000, 3)) * 4.0).astype(np.float32)).cuda()
    target = scan + 0.02
    rows = torch.tensor([3000, 2400], dtype=torch.int32).cuda()
    lin0 = torch.from_numpy(rng.standard_normal((16, 3)).astype(np.float32)).cuda()
    head0 = torch.from_numpy(rng.standard_normal(16).astype(np.float32)).cuda()

    def once():
        lin, head = lin0.clone().requires_grad_(True), head0.clone().requires_grad_(True)
        cloud, crow = voxel_downsample(scan, 0.3, rows=rows)
        pts, _, prow = sample_farthest_points(cloud, 500, rows=crow, return_rows=True)
        centres, _, erow = sample_farthest_points(pts, 64, rows=prow, return_rows=True)
        _, idx = ball_query(centres, pts, 0.6, 16, x_rows=erow, y_rows=prow)
        per_point = torch.tanh((pts.detach()[:, :, None, :] * lin).sum(-1))                    # (2, ~500, 16): the user's per-point layer
        inv = invert_neighbors(idx, per_point.shape[1], rows=prow)
        pooled = pool_neighbors(per_point, idx, "max", rows=prow, inverse=inv) + pool_neighbors(per_point, idx, "mean", rows=prow, inverse=inv)
        centre_w = torch.sigmoid((pooled * head).sum(-1, keepdim=True))                         # (2, 64, 1)
        d3, i3 = knn_points(pts, centres, k=3, x_rows=prow, y_rows=erow)
        w = interpolate_features(centre_w, i3, d3.detach(), eps=EPS, rows=erow, deterministic=True)
        gl, gh = torch.autograd.grad((w * w).sum(), [lin, head], retain_graph=True)
        T0 = torch.eye(4, dtype=torch.float32, device="cuda").repeat(2, 1, 1)
        icp = ICP(icp_type="pt2pt", differentiable=True, max_iterations=3, tolerance=1e-12)
        out = icp.icp(pts.detach(), target, T0, weight=w[..., 0], source_rows=prow, target_rows=rows)
        out["T"].sum().backward()
        assert torch.isfinite(lin.grad).all() and (lin.grad != 0).any()
        return _np(gl).tobytes(), _np(gh).tobytes(), _np(w).tobytes(), (gl != 0).any().item() and (gh != 0).any().item()
    a, b = once(), once()
    assert a[3] and b[3] and a[:3] == b[:3]
