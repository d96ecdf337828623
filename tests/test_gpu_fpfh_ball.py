"""fpfh_features_ball / compute_fpfh(whole_ball=True, at=) on the MI355X (dicp_amd/fpfh.py; csrc/fpfh_ball.hip) against the numpy
restatement tests/fpfh_ball_ref.py: the pair counts integer for integer, the descriptor bit for bit, float32 and float64.

1  tile and wave edges: m in {1, 2, 63, 64, 65, 300}, two clouds of different row counts per call, dead rows and extra columns holding
   NaN, c in {3, 6}, balls of about 4, 40 and 150 rows;
2  the layouts of the coverage claim (tests/iss_ball_cases.py), the wide-count lattice, a cloud with no rows;
3  single clouds, lists and CPU tensors against the batch, no gradient, int32 counts;
4  `at`: arange, a shuffled list with dead, out-of-range and duplicate entries, the index of compute_iss_keypoints;
5  compute_fpfh with and without the new arguments;  6  a captured graph;  7  poisoned allocations;
8  the cross-check with the k-slot form where every ball fits 32 slots;  9  the end-to-end registration from keypoint descriptors.

Where a grid's plan enlarged an edge or went flat, the reference takes the edges from the library's own plan (read back from the CellGrid
the front end builds); tests/iss_ball_ref.py asserts that the simple rule is used wherever the plan did not.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import iss as iss_module
from dicp_amd.ICP import ICP
from dicp_amd.ball import ball_query
from dicp_amd.fpfh import compute_fpfh, fpfh_features, fpfh_features_ball
from dicp_amd.iss import compute_iss_keypoints
from dicp_amd.match import match_features
from dicp_amd.normals import estimate_normals
from dicp_amd.register import ransac_correspondences

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_ball_cases as fbc  # noqa: E402
import fpfh_ball_ref as fbr  # noqa: E402
import fpfh_cases as fc  # noqa: E402
import fpfh_ref as fr  # noqa: E402
import iss_ball_cases as ibc  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def device_plans(Pd, rows_t, radius):
    """the plans of the grid the front end builds for this batch and radius -> [(edges (3,), enlarged, flat)] per cloud (csrc/dicp_ball.h:
    BallPlan -- o[3], s[3], R, r2 of T, then hi[3] int64, wy, wz, cnt, flat int32)"""
    grid = iss_module._ball_grid(Pd, rows_t, radius)
    raw = host(grid.plans)
    dt = host(Pd).dtype
    ts = dt.itemsize
    out = []
    for b in range(raw.shape[0]):
        f = raw[b, :8 * ts].copy().view(dt)
        ints = raw[b, 8 * ts + 24:8 * ts + 40].copy().view(np.int32)
        edges, R, flat = f[3:6], f[6], bool(ints[3])
        out.append((edges, flat or bool((edges != R).any()), flat))
    return out


def rows_tensor(rows):
    return None if rows is None else torch.tensor(np.asarray(rows), dtype=torch.int32).cuda()


def reference(P, Nn, rows, radius):
    plans = device_plans(dev(P), rows_tensor(rows), radius)
    return fbr.fpfh_ball_ref_batch(P, Nn, radius, rows, plans=[p if (p[1] or p[2]) else None for p in plans])


def check(P, Nn, rows, radius):
    """fpfh_features_ball on one batch against the reference -> the reference"""
    ref = reference(P, Nn, rows, radius)
    out, spfh = fpfh_features_ball(dev(P), dev(Nn), radius, rows=rows_tensor(rows), return_spfh=True)
    assert out.shape == P.shape[:2] + (33,) and out.dtype == dev(P).dtype and not out.requires_grad
    assert spfh.shape == out.shape and spfh.dtype == torch.int32 and spfh.is_contiguous()
    assert np.array_equal(host(spfh).astype(np.int64), ref["cnt"])
    assert fr.same_bits(host(out), ref["out"])
    return ref


def padded(clouds, cols):
    """clouds [(points (m_b, 3), normals (m_b, 3), rows_b)] -> P (N, m, cols), Nn (N, m, 3) with NaN in pad rows and extra columns, rows (N,)"""
    m = max(c[0].shape[0] for c in clouds)
    P = np.full((len(clouds), m, cols), np.nan, dtype=clouds[0][0].dtype)
    Nn = np.full((len(clouds), m, 3), np.nan, dtype=clouds[0][0].dtype)
    for b, (pts, nrm, r) in enumerate(clouds):
        P[b, :r, :3] = pts[:r, :3]
        Nn[b, :r] = nrm[:r]
    return P, Nn, np.array([c[2] for c in clouds], dtype=np.int32)


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 300])
def test_tile_edges(dtype, m):
    for q, members in enumerate((4, 40, 150)):
        a, na = fbc.cloud(100 * m + q, m, dtype, dead=m >= 63)
        b, nb = fbc.cloud(100 * m + q + 50, m, dtype)
        P, Nn, rows = padded([(a, na, m), (b, nb, m - m // 3)], 3 if q % 2 == 0 else 6)
        r = ibc.ball_radius(a, members) if m > 2 else 5.0
        ref = check(P, Nn, rows, r)
        pairs = ref["cnt"][..., :fr.BINS].sum(axis=-1)
        if m == 300:
            assert abs(np.median(pairs[0][pairs[0] > 0]) - members) <= 0.5 * members           # (the ball holds what the case says)
            assert (members <= 31) == (pairs.max() <= 31)                                       # 40 and 150: beyond the k-slot form
        if m >= 63:
            for i in fbc.DEAD_ROWS:
                assert not ref["cnt"][0, i].any() and not ref["out"][0, i].any()
            assert pairs[0, 10] > 0 and pairs[0, 10] == pairs[0, 11]                           # the duplicates: not near each other, one ball
            assert not ref["cnt"][1, m - m // 3:].any() and not ref["out"][1, m - m // 3:].any()
        if m == 2:
            assert (pairs == 1).all()


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ibc.LAYOUT_NAMES)
def test_layouts(dtype, name):
    pts, r1, _ = ibc.layouts(dtype)[name]
    plans = device_plans(dev(pts[None]), None, r1)
    assert (plans[0][1], plans[0][2]) == (name in ("two clusters", "far outlier", "flat"), name == "flat")
    ref = check(pts[None], fbc.normals(41, pts.shape[0], dtype)[None], None, r1)
    assert ref["cnt"].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_wide_count_and_a_cloud_with_no_rows(dtype):
    """399 pairs a row in three channels (a byte counter would hold 143), beside a cloud with rows = 0"""
    P, Nn = fbc.wide_lattice(dtype)
    Pb, Nb, rows = padded([(P, Nn, 400), (P, Nn, 0)], 3)
    ref = check(Pb, Nb, rows, fbc.WIDE_RADIUS)
    expect = np.zeros((400, 33), np.int64)
    expect[:, list(fbc.WIDE_CHANNELS)] = 399
    assert np.array_equal(ref["cnt"][0], expect) and (ref["out"][0] == np.where(expect > 0, 200.0, 0.0)).all()
    assert not ref["cnt"][1].any() and not ref["out"][1].any()


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("dtype", DTYPES)
def test_forms(dtype):
    rows = [90, 61, 75]
    P, Nn, rw = padded([fbc.cloud(51 + b, 90, dtype, dead=True) + (r,) for b, r in enumerate(rows)], 4)
    r = 0.5
    ref = check(P, Nn, rw, r)
    assert ref["cnt"][..., :fr.BINS].sum(-1).max() > 12
    for b, n in enumerate(rows):
        out, spfh = fpfh_features_ball(dev(P[b, :n]), dev(Nn[b, :n]), r, return_spfh=True)
        assert out.shape == (n, 33) and fr.same_bits(host(out), ref["out"][b, :n])
        assert spfh.shape == (n, 33) and spfh.dtype == torch.int32 and np.array_equal(host(spfh), ref["cnt"][b, :n])
    outs, counts = fpfh_features_ball([dev(P[b, :n]) for b, n in enumerate(rows)], [dev(Nn[b, :n]) for b, n in enumerate(rows)], r, return_spfh=True)
    assert isinstance(outs, list) and all(fr.same_bits(host(o), ref["out"][b, :n]) for b, (o, n) in enumerate(zip(outs, rows)))
    assert all(np.array_equal(host(o), ref["cnt"][b, :n]) and o.dtype == torch.int32 for b, (o, n) in enumerate(zip(counts, rows)))
    out_c, spfh_c = fpfh_features_ball(torch.from_numpy(P), torch.from_numpy(Nn), r, rows=torch.tensor(rows), return_spfh=True)
    assert not out_c.is_cuda and not spfh_c.is_cuda and fr.same_bits(out_c.numpy(), ref["out"]) and np.array_equal(spfh_c.numpy(), ref["cnt"])
    x, n = dev(P[0]).requires_grad_(True), dev(Nn[0]).requires_grad_(True)
    out = fpfh_features_ball(x, n, r)
    assert not out.requires_grad and fr.same_bits(host(out), ref["out"][0])
    assert not compute_fpfh(x, n, r, whole_ball=True, at=torch.tensor([1, 2]).cuda()).requires_grad


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("itype", [np.int32, np.int64])
def test_at(dtype, itype):
    rows = [90, 61]
    P, Nn, rw = padded([fbc.cloud(71 + b, 90, dtype, dead=True) + (r,) for b, r in enumerate(rows)], 3)
    r = 0.5
    Pd, Nd, rt = dev(P), dev(Nn), rows_tensor(rw)
    ref = check(P, Nn, rw, r)
    full = ref["out"]
    ar = np.broadcast_to(np.arange(90, dtype=itype), (2, 90))
    got, spfh = fpfh_features_ball(Pd, Nd, r, rows=rt, at=dev(ar), return_spfh=True)
    assert fr.same_bits(host(got), full) and np.array_equal(host(spfh), ref["cnt"])            # arange: the full call; the counts cover every row
    at = np.stack([fbc.at_entries(90, n, itype, seed=b) for b, n in enumerate(rows)])
    want = np.stack([fbr.at_ref(full[b], at[b], n) for b, n in enumerate(rows)])
    got = fpfh_features_ball(Pd, Nd, r, rows=rt, at=dev(at))
    assert got.shape == at.shape + (33,) and got.dtype == Pd.dtype and fr.same_bits(host(got), want)
    live = (at.astype(np.int64) >= 0) & (at.astype(np.int64) < rw[:, None])
    assert want[live].any() and not want[~live].any() and (~live).sum() >= 10
    one = fpfh_features_ball(Pd[1, :61], Nd[1, :61], r, at=dev(at[1]))                         # a single cloud: m = 61, `rows` is the cloud
    assert one.shape == (at.shape[1], 33) and fr.same_bits(host(one), fbr.at_ref(full[1, :61], at[1], 61))
    lists = fpfh_features_ball([Pd[0], Pd[1, :61]], [Nd[0], Nd[1, :61]], r, at=[dev(at[0][:7]), dev(at[1])])
    assert [tuple(o.shape) for o in lists] == [(7, 33), (at.shape[1], 33)]
    assert fr.same_bits(host(lists[0]), want[0][:7]) and fr.same_bits(host(lists[1]), want[1])
    cpu = fpfh_features_ball(torch.from_numpy(P), torch.from_numpy(Nn), r, rows=torch.tensor(rows), at=torch.from_numpy(at))
    assert not cpu.is_cuda and fr.same_bits(cpu.numpy(), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_at_the_iss_keypoints(dtype):
    """the `index` of compute_iss_keypoints(whole_ball=True, return_index=True) goes in unchanged: (N, m) int64, -1 past rows_out"""
    rows = [400, 333]
    P, Nn, rw = padded([fbc.cloud(61 + b, 400, dtype) + (r,) for b, r in enumerate(rows)], 3)
    Pd, Nd, rt = dev(P), dev(Nn), rows_tensor(rw)
    _, kp_rows, index = compute_iss_keypoints(Pd, 0.45, 0.3, rows=rt, return_index=True, whole_ball=True)
    assert index.shape == (2, 400) and index.dtype == torch.int64 and int(kp_rows.min()) >= 3
    full = host(fpfh_features_ball(Pd, Nd, 0.5, rows=rt))
    got = compute_fpfh(Pd, Nd, 0.5, rows=rt, whole_ball=True, at=index)
    ix = host(index)
    assert got.shape == (2, 400, 33) and fr.same_bits(host(got), np.stack([fbr.at_ref(full[b], ix[b], rows[b]) for b in range(2)]))
    for b in range(2):
        n = int(kp_rows[b])
        assert host(got[b, :n]).any(axis=1).all() and not host(got[b, n:]).any() and fr.same_bits(host(got[b, :n]), full[b][ix[b, :n]])


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("dtype", DTYPES)
def test_compute_fpfh(dtype):
    rows = [300, 211]
    P, Nn, rw = padded([fbc.cloud(81 + b, 300, dtype, dead=True) + (r,) for b, r in enumerate(rows)], 6)
    Pd, Nd, rt = dev(P), dev(Nn), rows_tensor(rw)
    r = ibc.ball_radius(P[0], 40)
    want = fpfh_features_ball(Pd, Nd, r, rows=rt)
    assert torch.equal(compute_fpfh(Pd, Nd, r, rows=rt, whole_ball=True), want)
    assert torch.equal(compute_fpfh(Pd, Nd, r, k=3, rows=rt, whole_ball=True), want)           # k is ignored
    # without the new arguments: the k-slot path as before, the bits of fpfh_features on ball_query's index
    idx = ball_query(Pd, Pd, r, k=32, x_rows=rt, y_rows=rt)[1]
    slot = fpfh_features(Pd, Nd, idx, rows=rt, radius=r)
    assert torch.equal(compute_fpfh(Pd, Nd, r, rows=rt), slot) and torch.equal(compute_fpfh(Pd, Nd, r, k=32, rows=rt, whole_ball=False), slot)
    assert not torch.equal(slot, want)                                                         # 40 rows a ball: the 32 slots truncate


# ------------------------------------------------------------------ 6
def test_captured_call():
    rows = [400, 333]

    def data(seed):
        P, Nn, rw = padded([fbc.cloud(seed + b, 400, np.float32, dead=True) + (r,) for b, r in enumerate(rows)], 3)
        at = np.stack([fbc.at_entries(400, r, np.int64, seed=seed + b) for b, r in enumerate(rows)])
        return {"P": dev(P), "N": dev(Nn), "rows": torch.tensor(rw, dtype=torch.int32).cuda(), "at": dev(at)}

    def run(s):
        out, spfh = fpfh_features_ball(s["P"], s["N"], 0.4, rows=s["rows"], return_spfh=True)
        return out, spfh, fpfh_features_ball(s["P"], s["N"], 0.4, rows=s["rows"], at=s["at"])
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
        captured = run(static)
    for seed in (20, 30):
        fresh = data(seed)
        for key, t in fresh.items():
            static[key].copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(fresh)
        torch.cuda.synchronize()
        assert all(fr.same_bits(host(c), host(e)) for c, e in zip(captured, eager))
        assert int(captured[1][..., :11].sum(-1).max()) > 32 and bool(captured[2].any())


# ------------------------------------------------------------------ 7
@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_allocations(dtype):
    """every returned byte -- the descriptors, the int32 counts, an `at` result -- is independent of what the uninitialised buffers
    (outputs, workspace, grid) held; all names exact"""
    rows = [90, 0, 61]
    P, Nn, rw = padded([fbc.cloud(91 + b, 90, dtype, dead=r > 0) + (r,) for b, r in enumerate(rows)], 6)
    at = np.stack([fbc.at_entries(90, r if r else 90, np.int64, seed=b) for b, r in enumerate(rows)])       # (the cloud without rows: every entry dead)

    def probe():
        x, n, rt = dev(P), dev(Nn), rows_tensor(rw)
        out, spfh = fpfh_features_ball(x, n, 0.5, rows=rt, return_spfh=True)
        picked = compute_fpfh(x, n, 0.5, rows=rt, whole_ball=True, at=dev(at))
        return dict(out=out.cpu(), spfh=spfh.cpu(), picked=picked.cpu())
    clean = poison.hold(probe, label="fpfh_features_ball")
    assert (clean["out"][0] != 0).any() and (clean["out"][1] == 0).all() and (clean["spfh"][2] != 0).any() and (clean["picked"][1] == 0).all()
    assert (clean["picked"][0] != 0).any()


# ------------------------------------------------------------------ 8
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", [31, 32])
def test_cross_check_with_the_k_slot_form(dtype, seed):
    """On tests/iss_ball_cases.py's cross_scene (radius 1.3) every ball holds at most 31 other rows, so compute_fpfh(k=32) -- ball_query,
    then fpfh_features -- sees the SAME near rows as the whole-ball form: the pair counts must be equal integer for integer on EVERY row,
    and with them s_j and every term t_j = fl(fl(1 / r2_j) s_j[ch]) of the weighted sum.  The two forms differ only in the ORDER in which
    they add these non-negative terms (distance order against grid order).

    The bound (fbc.cross_bound), derived -- not fitted.  u = 2^-53, gamma_j = j u / (1 - j u), n the largest number of terms (with seeded
    random normals every near row is a pair, asserted in tests/test_fpfh_ball_host.py: n is the largest pair count).
      acc: a recursive sum of n non-negative terms in any order is within gamma_(n-1) of the exact sum A, relatively.
      S: the 11 sums of a feature added in one fixed order: within gamma_10 of the sum of the computed acc, so within gamma_(n+9) of the
        exact S* = sum A.
      u[ch] = fl(acc fl(100 / S)): two more roundings.  The exact value u* = 100 A / S* is at most 100, and each form's u is
        u* (1 + theta) with |theta| <= gamma_((n-1) + 2 + (n+9)) = gamma_(2n+10): the forms are within 2 * 100 gamma_(2n+10) of each other.
      out = fl(u + s_i) <= 200 with the same s_i on both sides: one rounding each, 2 * 200 u.
    200 gamma_(2n+10) + 400 u = (400 n + 2400) u up to second order, below 100 * 4 * gamma_(n+12) = (400 n + 4800) u (1 + ...): the bound.
    In float32 each side is then rounded once to the output dtype: + 2 * 2^-24 * 200.
    tests/test_fpfh_ball_host.py asserts the same bound on the two numpy references alone (1.4e-14 in float64, 0 in float32)."""
    P, r = ibc.cross_scene(seed, dtype)
    Nn = fbc.normals(seed, P.shape[0], dtype)
    Pd, Nd = dev(P[None]), dev(Nn[None])
    idx = ball_query(Pd, Pd, r, k=ibc.K)[1]
    out_k, spfh_k = fpfh_features(Pd, Nd, idx, radius=r, return_spfh=True)
    assert torch.equal(compute_fpfh(Pd, Nd, r, k=ibc.K), out_k)
    out_b, spfh_b = fpfh_features_ball(Pd, Nd, r, return_spfh=True)
    assert spfh_k.dtype == torch.uint8 and spfh_b.dtype == torch.int32
    assert torch.equal(spfh_k.to(torch.int32), spfh_b)                                         # every row, none left out
    n = int(spfh_b[..., :11].sum(-1).max())
    assert 16 < n <= ibc.K - 1
    bound = fbc.cross_bound(n, dtype)
    diff = np.abs(host(out_k).astype(np.float64) - host(out_b).astype(np.float64)).max()
    print("seed %d %s: |out difference| max %.3g, bound %.3g" % (seed, np.dtype(dtype).name, diff, bound))
    assert diff <= bound


# ------------------------------------------------------------------ 9
E2E_CPU_SHARE = 0.748             # profiles/r36_fpfh_ball_edges.txt: the share the numpy references alone reach on this scene at radius 1.2


def rotation_error(R, C_true):
    Rm = np.asarray(R, dtype=np.float64).reshape(3, 3)
    return float(np.arccos(np.clip((np.trace(Rm @ C_true.T) - 1.0) / 2.0, -1.0, 1.0)))


def test_end_to_end_registration_from_keypoint_descriptors():
    """The scene of tests/test_gpu_fpfh.py's end-to-end test (m = 1500, the source an 85 % subset turned by 1 rad, 2 mm noise), with the
    whole-ball descriptor at radius 1.2.  scripts/fpfh_ball_edges.py measured with the numpy references alone, on the CPU, before any
    threshold here was fixed (profiles/r36_fpfh_ball_edges.txt): E2E_CPU_SHARE of the mutual matches on all points within 0.15 of the true
    row (0.546 for the k-slot form), and 34 right matches of 49 among the whole-ball ISS keypoints.  The GPU run uses estimate_normals, so
    it must reach half the share; the k = 32 form at the same radius must reach LESS than the whole ball: the reason the feature exists.
    Then the chain without any (N, m, 32) index: ISS keypoints (whole ball) -> descriptors AT them -> matches -> RANSAC -> ICP."""
    P = fc.scene(0, 1500)
    mv = fc.moved_copy(P, seed=0, keep=0.85, angle=1.0, noise=0.002, axis=fc.E2E_AXIS)
    y, x = dev(P.astype(np.float32)), dev(mv["x"].astype(np.float32))
    ny = estimate_normals(y, k=16, viewpoint=torch.tensor(fc.VIEWPOINT, dtype=torch.float32))
    nx = estimate_normals(x, k=16, viewpoint=torch.tensor(fc.VIEWPOINT @ mv["R"].T + mv["t"], dtype=torch.float32))
    truth = P[mv["src"]]

    def share(fx, fy):
        got = host(match_features(fx, fy, mutual=True)[0])
        live = got >= 0
        err = np.linalg.norm(P[np.where(live, got, 0)] - truth, axis=1)
        return int(live.sum()), float((err[live] <= 0.15).mean())
    n_b, share_b = share(compute_fpfh(x, nx, 1.2, whole_ball=True), compute_fpfh(y, ny, 1.2, whole_ball=True))
    n_k, share_k = share(compute_fpfh(x, nx, 1.2, k=32), compute_fpfh(y, ny, 1.2, k=32))
    print("radius 1.2, all points: whole ball %d mutual matches, %.3f within 0.15 (CPU reference %.3f); k = 32: %d, %.3f"
          % (n_b, share_b, E2E_CPU_SHARE, n_k, share_k))
    assert n_b >= 100 and share_b >= 0.5 * E2E_CPU_SHARE
    assert share_k < share_b
    # descriptors only AT the keypoints
    kx, kx_rows, ix = compute_iss_keypoints(x[None], 0.8, 0.4, return_index=True, whole_ball=True)
    ky, ky_rows, iy = compute_iss_keypoints(y[None], 0.8, 0.4, return_index=True, whole_ball=True)
    fx = compute_fpfh(x[None], nx[None], 1.2, whole_ball=True, at=ix)
    fy = compute_fpfh(y[None], ny[None], 1.2, whole_ball=True, at=iy)
    idx, _ = match_features(fx, fy, x_rows=kx_rows, y_rows=ky_rows, mutual=True)
    got, rows_x, rows_y = host(idx)[0], host(ix)[0], host(iy)[0]
    live = got >= 0
    err = np.linalg.norm(P[rows_y[np.where(live, got, 0)]] - truth[np.where(rows_x >= 0, rows_x, 0)], axis=1)
    print("keypoints %d / %d, mutual matches %d, right %d" % (int(kx_rows[0]), int(ky_rows[0]), int(live.sum()), int((err[live] <= 0.15).sum())))
    thr = 0.15
    T0, inl = ransac_correspondences(kx, ky, idx, thr, hypotheses=4096, seed=7, refine=2, x_rows=kx_rows)
    C_true, r_true = mv["R"].T, -mv["R"].T @ mv["t"]
    T0h = host(T0[0]).astype(np.float64)
    moved = mv["x"] @ T0h[:3, :3].T + T0h[:3, 3]
    worst = float(np.linalg.norm(moved - truth, axis=1).max())
    print("RANSAC on the keypoint matches: %d inliers; the worst true pair is %.4f apart under its pose (threshold %.2f)" % (int(inl.sum()), worst, thr))
    assert worst <= thr
    out = ICP(icp_type="pt2pt", max_iterations=30, tolerance=1e-9).icp(x[None], y[None], T_init=T0)
    Th = host(out["T"][0]).astype(np.float64)
    e_rot, e_t = rotation_error(Th[:3, :3], C_true), float(np.linalg.norm(Th[:3, 3] - r_true))
    print("ICP on all points from that pose: %.3g rad, %.3g m" % (e_rot, e_t))
    assert e_rot < 1e-2 and e_t < 5e-2
