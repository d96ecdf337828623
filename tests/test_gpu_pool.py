"""pool_neighbors on the MI355X against its definition (dicp_amd/group.py).

The forward of every kernel form (narrow rows; wide rows with 16-byte packs in lane groups of 8, 16, 32 and 64 lanes, rows wider than a
wave, their misaligned fallback and the scalar form of odd widths; both dtypes, both index widths; two cases beyond every grid stride)
against the numpy restatement tests/pool_ref.py -- the maximum with its argmax, the sum and the counts bit for bit, the mean within
(k + 2) u sum|f| / count of float64; tables of ties and of NaNs; every input form against the others; the gradients against an autograd
graph in torch float64 built from the restatement's argmax and liveness, with the module's bound (D + k + 8) u sum|terms| that one lost
or doubled term breaks; the compositions a user writes today; reproducibility; no host synchronisation; and the chain
voxel -> FPS -> ball -> linear map -> pool -> sigmoid -> knn -> interpolate -> ICP(weight=) -> backward."""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.ICP import ICP
from dicp_amd.ball import ball_query
from dicp_amd.fps import sample_farthest_points
from dicp_amd.group import group_points, interpolate_features, pool_neighbors
from dicp_amd.knn import knn_points
from dicp_amd.voxel import voxel_downsample

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_ref as gr  # noqa: E402
import pool_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
NS, MS, KS = (1, 63, 700), (1, 257, 2000), (1, 3, 8, 32)
# narrow (1, 3, 4, 6; 16 in float32, 31 in float32); the first wide width of float64 (16) and of float32 (32); packs that are no power of
# two (36: 9 float32 packs in a group of 16); a group of exactly one wave (256 float32: 64 packs; 130 scalar lanes loop); more than a
# wave (260: 65 packs); odd widths in the scalar form (31 float64, 33, 65, 130)
CS = (1, 3, 4, 6, 16, 31, 32, 33, 36, 64, 65, 130, 256, 260)
# the wide forward: a grid-stride loop of at most MAX_BLOCKS workgroups of WAVES waves, WAVE / G queries a wave (csrc/group.hip)
MAX_BLOCKS, WAVES, WAVE = 2048, 4, 64


def _group_lanes(C, dtype):
    """G of a wide row whose accesses are 16-byte packs: the smallest power of two >= min(packs, WAVE), at least 8"""
    packs, g = C * np.dtype(dtype).itemsize // 16, 8
    while g < min(packs, WAVE):
        g *= 2
    return g


def _u(dtype):
    return float(np.finfo(dtype).eps) / 2


def _table(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random(shape) * 2 - 1) * 10.0 ** rng.integers(-2, 3, size=shape)).astype(dtype)


def _dev(a, misalign=False):
    """the array on the device; misalign: as a contiguous view that starts one element into its allocation (no 16-byte base)"""
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


def _rows_dev(rows):
    return torch.tensor(rows, dtype=torch.int32).cuda() if rows is not None else None


def _batch(n, m, k, C, dtype, it, seed):
    """two clouds, the first with fewer live rows than the table holds: features, idx, rows"""
    rows = [m * 3 // 4, m]
    f = _table((2, m, C), dtype, seed)
    idx = np.stack([gr.make_idx(n, k, m, rows[b], seed + 10 + b, it) for b in range(2)])
    return f, idx, rows


def _pool(fd, idd, reduce, rd):
    """-> numpy (out, argmax or None, counts)"""
    if reduce == "max":
        out, arg, cnt = pool_neighbors(fd, idd, "max", rows=rd, return_argmax=True, return_counts=True)
        return _np(out), _np(arg), _np(cnt)
    out, cnt = pool_neighbors(fd, idd, reduce, rows=rd, return_counts=True)
    return _np(out), None, _np(cnt)


def _hold_forward(f, idx, rows, misalign=False, reduces=pr.REDUCES, nan_ok=False):
    """every reduce of one batch against the restatement, cloud by cloud"""
    fd, idd, rd = _dev(f, misalign), _dev(idx), _rows_dev(rows)
    for reduce in reduces:
        out, arg, cnt = _pool(fd, idd, reduce, rd)
        for b in range(f.shape[0]):
            rb = None if rows is None else rows[b]
            want = pr.pool_ref(f[b], idx[b], reduce, rb)
            got = (out[b], None if arg is None else arg[b], cnt[b])
            if reduce == "mean":
                ratio = pr.mean_ratio(out[b], f[b], idx[b], rb)
                assert ratio <= 1.0 and np.array_equal(cnt[b], want[2]) and cnt[b].dtype == np.int32 and (out[b][cnt[b] == 0] == 0).all(), (reduce, b, ratio)
            else:
                assert pr.same_result(got, want, nan_ok=nan_ok and reduce == "sum"), (reduce, b)


# ------------------------------------------------------------------ 1. the forward of every form
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CS)
def test_forward_matches_reference(C, dtype):
    """every reduce at every k, with n, m and the index width going round (each of n, m at every k over the C's)"""
    for a, k in enumerate(KS):
        o = a + CS.index(C)
        n, m, it = NS[o % 3], MS[(o // 3 + a) % 3], (np.int64, np.int32)[o % 2]
        _hold_forward(*_batch(n, m, k, C, dtype, it, 1000 * C + k))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_shape_at_two_widths(dtype):
    """n x m in full, narrow (C = 3) and wide with idle lanes in every group (C = 36), int32 and int64 by turns"""
    for i, n in enumerate(NS):
        for j, m in enumerate(MS):
            _hold_forward(*_batch(n, m, 8, 3, dtype, (np.int64, np.int32)[(i + j) % 2], 50 + 3 * i + j))
            _hold_forward(*_batch(n, m, 3, 36, dtype, (np.int32, np.int64)[(i + j) % 2], 70 + 3 * i + j))


@pytest.mark.parametrize("dtype", DTYPES)
def test_misaligned_base_takes_the_scalar_form(dtype):
    for C in (16, 64):
        _hold_forward(*_batch(63, 257, 8, C, dtype, np.int64, 90 + C), misalign=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [3, 64])
def test_ties_and_nans(C, dtype):
    """ties keep the lowest slot (+0 and -0 tie), the argmax is a row, +-inf are values; the first NaN wins and stays"""
    n, m, k = 63, 257, 8
    rows = [m * 3 // 4, m]
    f = np.stack([pr.make_tie_table(m, C, dtype, 3 + b) for b in range(2)])
    idx = np.stack([gr.make_idx(n, k, m, rows[b], 5 + b) for b in range(2)])
    t = pr.tie_kinds(f[1], idx[1], rows[1])
    assert t["tied_maximum"] >= t["queries"] * C // 4 and t["signed_zero_tie"] >= 1
    _hold_forward(f, idx, rows, reduces=("max", "sum"), nan_ok=True)
    cases = [pr.make_nan_case(n, k, m, C, dtype, 7 + b) for b in range(2)]
    f, idx = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    assert all({0, 1, 2} <= set(c[2].tolist()) for c in cases)
    _hold_forward(f, idx, None, reduces=("max",))
    out, arg = pool_neighbors(_dev(f), _dev(idx), "max", return_argmax=True)
    out, arg = _np(out), _np(arg)
    for b, (_, _, where) in enumerate(cases):
        assert np.isnan(out[b][where >= 0]).all() and not np.isnan(out[b][where < 0]).any()
        assert (arg[b][where >= 0] == (m - 3 + where[where >= 0])[:, None]).all()


@pytest.mark.parametrize("C", [3, 64])
def test_only_the_last_slot_live(C):
    for k in (8, 32):
        f = _table((1, 257, C), np.float32, k)
        idx = np.full((1, 5, k), -1, dtype=np.int64)
        idx[0, :4, k - 1] = [0, 5, 256, 5]
        _hold_forward(f, idx, None)
        out, arg, cnt = _pool(_dev(f), _dev(idx), "max", None)
        assert gr.same_bits(out[0, :4], f[0, [0, 5, 256, 5]]) and (arg[0, :4] == np.array([0, 5, 256, 5])[:, None]).all() and cnt[0].tolist() == [1, 1, 1, 1, 0]
        assert (out[0, 4] == 0).all() and (arg[0, 4] == -1).all()


# ------------------------------------------------------------------ 2. beyond every grid stride
def _big_wide():
    """N = 2, n = 17000, m = 20000, C = 64, k = 4: 34000 queries, more than the 32768 that 2048 workgroups of 16 hold; 35 MB gathered"""
    N, n, m, C, k = 2, 17000, 20000, 64, 4
    rng = np.random.default_rng(5)
    f = rng.standard_normal((N, m, C)).astype(np.float32)
    rows = [15000, m]
    idx = rng.integers(-1, m, size=(N, n, k))
    idx[:, 17] = -1                                         # a query without a live slot in each cloud
    return f, idx, rows


def _big_narrow():
    n, m, k, C = 100000, 5000, 3, 3
    f, idx, rows = _batch(n, m, k, C, np.float32, np.int64, 800)
    return f, idx, rows


def test_beyond_every_grid_stride_wide():
    f, idx, rows = _big_wide()
    per_workgroup = WAVES * (WAVE // _group_lanes(64, np.float32))
    assert per_workgroup == 16 and f.shape[0] * idx.shape[1] > MAX_BLOCKS * per_workgroup
    assert f.shape[0] * idx.shape[1] * idx.shape[2] * 64 * 4 < 40e6
    _hold_forward(f, idx, rows)
    for reduce in pr.REDUCES:
        _grad_case(f, idx, rows, reduce, 700)


def test_beyond_every_grid_stride_narrow():
    """N n C = 600000 (query, channel) elements and N n k C = 1.8 M (query, slot, channel) elements: more than 2048 x 256 each"""
    f, idx, rows = _big_narrow()
    assert f.shape[0] * idx.shape[1] * 3 > MAX_BLOCKS * 256
    _hold_forward(f, idx, rows)
    for reduce in pr.REDUCES:
        _grad_case(f, idx, rows, reduce, 801)


# ------------------------------------------------------------------ 3. input forms
@pytest.mark.parametrize("dtype", DTYPES)
def test_input_forms_agree(dtype):
    n, m, k, C = 63, 257, 8, 6
    f, idx, rows = _batch(n, m, k, C, dtype, np.int64, 7)
    ns = [40, n]
    for b in range(2):
        idx[b, ns[b]:] = -1                                  # (what the neighbour operators give query rows past their cloud's count)
    fd, idd, rd = _dev(f), _dev(idx), _rows_dev(rows)
    for reduce in pr.REDUCES:
        kw = dict(return_argmax=reduce == "max", return_counts=True)
        batch = pool_neighbors(fd, idd, reduce, rows=rd, **kw)
        assert isinstance(batch, tuple) and len(batch) == (3 if reduce == "max" else 2)
        assert batch[0].shape == (2, n, C) and batch[-1].shape == (2, n) and batch[-1].dtype == torch.int32
        alone = pool_neighbors(fd, idd, reduce, rows=rd)
        assert isinstance(alone, torch.Tensor) and gr.same_bits(_np(alone), _np(batch[0]))
        cpu = pool_neighbors(torch.from_numpy(f), torch.from_numpy(idx), reduce, rows=torch.tensor(rows), **kw)
        lists = pool_neighbors([fd[b, :rows[b]] for b in range(2)], [idd[b, :ns[b]] for b in range(2)], reduce, **kw)
        for o, (bt, ct, lt) in enumerate(zip(batch, cpu, lists)):
            bt = _np(bt)
            assert not ct.is_cuda and gr.same_bits(ct.numpy(), bt), (reduce, o)
            assert isinstance(lt, list) and len(lt) == 2
            for b in range(2):
                assert lt[b].is_cuda and lt[b].shape[0] == ns[b] and gr.same_bits(_np(lt[b]), bt[b, :ns[b]]), (reduce, o, b)
                if rows[b] == m:                             # a single cloud has no rows argument: the cloud whose table is all live
                    single = pool_neighbors(fd[b], idd[b], reduce, **kw)[o]
                    assert single.shape == bt[b].shape and gr.same_bits(_np(single), bt[b]), (reduce, o, b)
            past = bt[0, ns[0]:]
            assert (past == (-1 if (reduce == "max" and o == 1) else 0)).all()


# ------------------------------------------------------------------ 4. gradients
def _grad_case(f, idx, rows, reduce, seed, nan_at_empty=False):
    """g_features of one reduce on one batch (N, ...) against a torch float64 graph built from the restatement's argmax and liveness.
    Every element within (D + k + 8) u sum|terms|, D the row's in-degree (the live slots that name it); rows nobody names exactly 0."""
    dtype = f.dtype.type
    tdt, u = TORCH[dtype], _u(dtype)
    N, m, C = f.shape
    n, k = idx.shape[1:]
    gen = torch.Generator().manual_seed(seed)
    g = ((torch.rand((N, n, C), generator=gen, dtype=torch.float64) + 0.5) * (torch.randint(0, 2, (N, n, C), generator=gen) * 2 - 1)).to(tdt).cuda()
    idd, rd = _dev(idx), _rows_dev(rows)
    lim = rd.view(-1, 1, 1) if rd is not None else m
    live = (idd >= 0) & (idd < lim)
    any_live = live.any(2)
    assert live.any() and (~any_live).any()
    safe = idd.clamp(min=0, max=m - 1).long()
    bi = torch.arange(N, device="cuda")[:, None, None]
    zero = torch.zeros((), dtype=torch.float64, device="cuda")

    fd = _dev(f).requires_grad_(True)
    out = pool_neighbors(fd, idd, reduce, rows=rd)
    out.backward(torch.where(any_live[..., None], g, torch.full_like(g, float("nan"))) if nan_at_empty else g)
    got = fd.grad.reshape(N * m, C).double()

    fa = _dev(f).double().requires_grad_(True)
    gz = torch.where(any_live[..., None], g.double(), zero)
    ci = torch.arange(C, device="cuda")
    if reduce == "max":
        arg = torch.from_numpy(np.stack([pr.pool_ref(f[b], idx[b], "max", None if rows is None else rows[b])[1] for b in range(N)])).cuda().long()
        assert ((arg >= 0) == any_live[..., None]).all()
        dest, mask, terms = arg.clamp(min=0)[:, :, None, :], (arg >= 0)[:, :, None, :], gz[:, :, None, :]          # (N, n, 1, C)
        picked = fa[bi, dest[:, :, 0, :], ci]                                                                       # (N, n, C)
        (torch.where(mask[:, :, 0, :], picked, zero) * gz).sum().backward()
    else:
        cnt = live.sum(2, keepdim=True).clamp(min=1).double()
        per = gz / cnt if reduce == "mean" else gz
        dest, mask, terms = safe[..., None].expand(N, n, k, C), live[..., None].expand(N, n, k, C), per[:, :, None, :].expand(N, n, k, C)
        gathered = torch.where(live[..., None], fa[bi, safe], zero).sum(2)
        ((gathered / cnt if reduce == "mean" else gathered) * gz).sum().backward()
    flat = ((dest + bi[..., None] * m) * C + ci).reshape(-1)
    t = torch.where(mask, terms, zero).reshape(-1)
    ref = torch.zeros(N * m * C, dtype=torch.float64, device="cuda").index_add_(0, flat, t).reshape(N * m, C)
    ab = torch.zeros(N * m * C, dtype=torch.float64, device="cuda").index_add_(0, flat, t.abs()).reshape(N * m, C)
    deg = torch.zeros(N * m, dtype=torch.float64, device="cuda").index_add_(0, (safe + bi * m).reshape(-1), live.reshape(-1).double())[:, None]
    # (scaffolding only: both sides are torch's own float64 sums of the same `deg` terms, added with atomics in an order that changes from run to run; each is
    #  within (deg - 1) 2^-53 sum|terms| of the exact sum, so any two orders agree elementwise within twice that)
    assert ((fa.grad.reshape(N * m, C) - ref).abs() <= 2 * deg * 2.0 ** -53 * ab).all()
    assert torch.isfinite(got).all()
    assert (got[(deg == 0).expand_as(got)] == 0).all() and ((deg == 0).any() or m == 1)
    bound = (deg + k + 8) * u * ab
    assert ((got - ref).abs() <= bound).all(), (reduce, float(((got - ref).abs() - bound).max()))
    assert (ref != 0).any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,k,C,it", [(700, 257, 8, 3, np.int64), (63, 2000, 3, 1, np.int32), (700, 2000, 32, 33, np.int32), (63, 257, 8, 64, np.int64),
                                        (63, 257, 3, 130, np.int64), (1, 1, 1, 16, np.int64)])
def test_gradients(n, m, k, C, it, dtype):
    f, idx, rows = _batch(n, m, k, C, dtype, it, 400 + C)
    if n == 1:                                              # one query per cloud: a live one and an empty one
        idx[0, 0, 0], idx[1, 0, 0], rows = 0, -1, [1, 1]
    for reduce in pr.REDUCES:
        _grad_case(f, idx, rows, reduce, 500 + C, nan_at_empty=(C % 2 == 1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [3, 64])
def test_gradient_of_one_row_everybody_points_at(C, dtype):
    """700 x 8 slots on row 5 of 257 (in-degree 5600) and one query without a live slot; every other row's gradient is exactly 0"""
    n, m, k = 701, 257, 8
    idx = np.full((1, n, k), 5, dtype=np.int64)
    idx[0, 700] = -1
    f = _table((1, m, C), dtype, 1)
    for reduce in pr.REDUCES:
        _grad_case(f, idx, None, reduce, 600 + C, nan_at_empty=True)


# ------------------------------------------------------------------ 5. what users write today
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [3, 64])
def test_equals_group_then_reduce(C, dtype):
    """group_points -> masked_fill(-inf) -> amax(2) is pool_neighbors("max") bit for bit where a query has a live slot (the maximum of
    finite, distinct-or-equal values is one of them whatever the order).  The masked sum adds the same terms in another order: both are
    within (k - 1) u sum|f| of the exact sum, so within 2 (k - 1) u sum|f| of each other."""
    n, m, k = 700, 2000, 8
    f, idx, rows = _batch(n, m, k, C, dtype, np.int64, 40 + C)
    fd, idd, rd = _dev(f), _dev(idx), _rows_dev(rows)
    live = (idd >= 0) & (idd < rd.view(-1, 1, 1))
    grouped = group_points(fd, idd, rows=rd)
    has = live.any(2)
    assert has.any() and (~has).any()
    theirs = grouped.masked_fill(~live[..., None], float("-inf")).amax(2)
    ours = pool_neighbors(fd, idd, "max", rows=rd)
    assert torch.equal(ours[has], theirs[has]) and (ours[~has] == 0).all()
    s_theirs, s_ours = grouped.sum(2).double(), pool_neighbors(fd, idd, "sum", rows=rd).double()
    mag = grouped.double().abs().sum(2)
    assert ((s_ours - s_theirs).abs() <= 2 * (k - 1) * _u(dtype) * mag).all()


# ------------------------------------------------------------------ 6. reproducibility, no host synchronisation
def test_runs_repeat():
    f, idx, rows = _batch(700, 2000, 8, 64, np.float32, np.int64, 11)
    runs = []
    for _ in range(2):
        fd, idd, rd = _dev(f), _dev(idx), _rows_dev(rows)
        res = []
        for reduce in pr.REDUCES:
            res += [x for x in _pool(fd, idd, reduce, rd) if x is not None]
        runs.append([x.tobytes() for x in res])
    assert runs[0] == runs[1]


@pytest.mark.parametrize("C", [3, 64])
def test_no_host_synchronisation(C):
    f, idx, rows = _batch(700, 2000, 8, C, np.float32, np.int64, 12)
    fd, idd, rd = _dev(f).requires_grad_(True), _dev(idx), _rows_dev(rows)
    pool_neighbors(fd, idd, "max", rows=rd)                 # (the library is loaded)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        mx, arg, cnt = pool_neighbors(fd, idd, "max", rows=rd, return_argmax=True, return_counts=True)
        mean = pool_neighbors(fd, idd, "mean", rows=rd)
        total = pool_neighbors(fd, idd, "sum", rows=rd)
        (mx.sum() + mean.sum() + total.sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for b in range(2):
        assert pr.same_result((_np(mx[b]), _np(arg[b]), _np(cnt[b])), pr.pool_ref(f[b], idx[b], "max", rows[b]))
    assert torch.isfinite(fd.grad).all() and (fd.grad != 0).any()


# ------------------------------------------------------------------ 7. the chain
def test_chain_to_icp_weights():
    rng = np.random.default_rng(21)
    scan = torch.from_numpy((rng.random((2, 3000, 3)) * 4.0).astype(np.float32)).cuda()
    target = scan + 0.02
    rows = torch.tensor([3000, 2400], dtype=torch.int32).cuda()
    cloud, crow = voxel_downsample(scan, 0.3, rows=rows)
    pts, _, prow = sample_farthest_points(cloud, 500, rows=crow, return_rows=True)                 # the two clouds of about 500 points
    centres, _, erow = sample_farthest_points(pts, 64, rows=prow, return_rows=True)
    d2, idx = ball_query(centres, pts, 0.6, 16, x_rows=erow, y_rows=prow)
    lin = torch.linspace(-1.0, 1.0, 3, device="cuda").requires_grad_(True)                          # the user's "MLP": one linear map, per point
    feat = (pts * lin).sum(-1, keepdim=True)                                                        # (2, 500, 1)
    pooled, arg, cnt = pool_neighbors(feat, idx, "max", rows=prow, return_argmax=True, return_counts=True)   # (2, 64, 1): nothing grouped
    assert pooled.shape == (2, 64, 1) and arg.shape == (2, 64, 1) and cnt.shape == (2, 64)
    fn, idn = _np(feat), _np(idx)
    for b in range(2):
        assert pr.same_result((_np(pooled[b]), _np(arg[b]), _np(cnt[b])), pr.pool_ref(fn[b], idn[b], "max", int(prow[b])))
        assert (_np(cnt[b])[:int(erow[b])] >= 1).all()                                              # (a centre is its own neighbour)
    centre_w = torch.sigmoid(pooled - (centres * lin).sum(-1, keepdim=True))                        # max_s(f_s - centre) = max_s(f_s) - centre
    centre_w.retain_grad()
    d3, i3 = knn_points(pts, centres, k=3, x_rows=prow, y_rows=erow)
    w = interpolate_features(centre_w, i3, d3, eps=1e-8, rows=erow)                                 # (2, 500, 1)
    assert w.shape == (2, 500, 1)
    T0 = torch.eye(4, dtype=torch.float32, device="cuda").repeat(2, 1, 1)
    icp = ICP(icp_type="pt2pt", differentiable=True, max_iterations=3, tolerance=1e-12)
    out = icp.icp(pts.detach(), target, T0, weight=w[..., 0], source_rows=prow, target_rows=rows)
    out["T"].sum().backward()
    gw = centre_w.grad
    assert torch.isfinite(gw).all() and (gw != 0).any() and torch.isfinite(lin.grad).all() and (lin.grad != 0).any()
