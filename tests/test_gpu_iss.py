"""iss_saliency / iss_keypoints / compute_iss_keypoints on the MI355X (dicp_amd/iss.py; csrc/iss.hip) against the numpy restatement
tests/iss_ref.py: eigenvalues, saliency and counts bit for bit, the keypoint mask exactly.

1  shapes at the edges of the kernels' tiles: m in {1, 2, 63, 64, 65, 300, 1500} x k in {1, 2, 7, 8, 31, 32}, float32 and float64, int64
   and int32 indices, two clouds of different row counts per call, radii None / cutting about half the slots / cutting all of them, dead
   rows holding NaN and garbage indices in every cloud, extra point columns holding NaN;
2  the designed clouds of tests/iss_cases.py (duplicates, exactly planar and collinear neighbourhoods, the count at min_neighbors and one
   below, a ratio exactly at gamma, a row alone with itself, non-finite neighbours) and a cloud with no rows;
3  an idx straight from ball_query, from knn_points(method="grid") cut by the radii, nms_idx different from idx; single clouds, lists and
   CPU tensors against the batch; no gradient;
4  compute_iss_keypoints against its three steps, its index, its gradient;  5  a call in a captured graph;
6  the cube-corner scene;  7  end to end: keypoints in front of match_features -> ransac_correspondences -> ICP.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.ball import ball_query
from dicp_amd.filter import select_rows
from dicp_amd.fpfh import compute_fpfh
from dicp_amd.ICP import ICP
from dicp_amd.iss import compute_iss_keypoints, iss_keypoints, iss_saliency
from dicp_amd.knn import knn_points
from dicp_amd.match import match_features, ransac_correspondences
from dicp_amd.normals import estimate_normals

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_cases as fc  # noqa: E402
import iss_cases as ic  # noqa: E402
import iss_ref as ir  # noqa: E402
from ransac_ref import rotation_error  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
M_CASES = (1, 2, 63, 64, 65, 300, 1500)
K_CASES = (1, 2, 7, 8, 31, 32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(P, idx, rows, r1=None, r2=None, itype=np.int64, nms=None, ref=None, **params):
    """both front ends on one batch against the reference (computed here unless given) -> the reference"""
    idx_t = ic.index_dtype(idx, itype)
    nms_t = None if nms is None else ic.index_dtype(nms, itype)
    if ref is None:
        ref = ir.keypoints_ref_batch(P, idx_t, rows, nms_idx=nms_t, salient_radius=r1, non_max_radius=r2, **params)
    rows_t = None if rows is None else torch.tensor(np.asarray(rows), dtype=torch.int32).cuda()
    Pd, Id = dev(P), dev(idx_t)
    sal, eig, cnt = iss_saliency(Pd, Id, rows=rows_t, radius=r1, return_eigenvalues=True, return_counts=True, **params)
    assert sal.shape == P.shape[:2] and eig.shape == P.shape[:2] + (3,) and cnt.shape == sal.shape and cnt.dtype == torch.int32
    assert sal.dtype == Pd.dtype and eig.dtype == Pd.dtype and not sal.requires_grad and not eig.requires_grad
    mask, sal2 = iss_keypoints(Pd, Id, rows=rows_t, salient_radius=r1, non_max_radius=r2, nms_idx=None if nms is None else dev(nms_t),
                               return_saliency=True, **params)
    assert mask.dtype == torch.bool and mask.shape == sal.shape and not mask.requires_grad
    got = dict(eig=host(eig), sal=host(sal), count=host(cnt), mask=host(mask))
    for key in ("count", "eig", "sal", "mask"):
        assert ir.same_bits(got[key], ref[key]), key
    assert ir.same_bits(host(sal2), ref["sal"])
    return ref


# ------------------------------------------------------------------ 1
ITYPES = (np.int64, np.int32)


def top_slot_members(c, radius):
    """how many rows of one cloud (a dict of iss_cases) have a member in their LAST slot, by the reference"""
    P, ok, rows = ir._cloud(c["points"], c["rows"])
    return int(ir.members(P, ok, c["idx"], rows, radius)[0][:, -1].sum())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", M_CASES)
def test_tile_edges(dtype, m):
    """Every (m, k) runs one of the three radii in one of the two index dtypes, chosen by the positions of m AND k, so that every k meets
    every radius and both dtypes over the m; k = 7 and k = 32 (an odd k, and the largest: bit 31 of the member mask, the last row of the
    transposed slots) at m >= 65 run no cut and the half cut in BOTH dtypes whatever that choice was.  Without a cut and with 2 <= k <= m the
    last slot of some row holds a member: asserted, so the top slot is held to the reference."""
    mi = M_CASES.index(m)
    for q, k in enumerate(K_CASES):
        a = ic.random_cloud(100 * m + k, m, k, dtype, cols=3 + q % 3)
        b = ic.random_cloud(100 * m + k + 50, m, k, dtype, rows=m - m // 3, cols=3 + q % 3, planar=True)
        P, idx, rows = ic.pad_batch([a, b])
        radii = (None, ic.median_radius(a, 0.5), 1e-6)                  # no cut / about half the slots / all of them
        pick, it = ((q + mi) % 3, (q + mi) % 2) if m >= 63 else (0, q % 2)
        runs = [(pick, it)]
        if m >= 65 and k in (7, 32):
            runs = [(sel, t) for sel in (0, 1) for t in (it, 1 - it)] + ([(2, it)] if pick == 2 else [])
        refs = {}
        for sel, t in runs:
            r1 = radii[sel]
            refs[sel] = ref = check(P, idx, rows, r1, None if r1 is None else 0.8 * r1, itype=ITYPES[t], ref=refs.get(sel))
            if sel == 0 and m >= 63 and 2 <= k <= m:
                assert top_slot_members(a, None) > 0                                     # slot k - 1 of some row is live
            if sel == 1 and m >= 63 and k >= 7:
                assert ref["count"][0].max() > 2 and (0 not in refs or ref["count"][0].sum() < refs[0]["count"][0].sum())     # a cut, not all
            if sel != 2 and m >= 300 and k >= 7:
                assert (ref["sal64"] > 0).sum() > 20 and ref["mask"].sum() >= 2          # (the case is not empty)
            if sel == 2 and m >= 63:
                assert ref["count"].max() <= 2 and not ref["mask"].any()
        if m == 300 and k in (8, 31):
            check(P, idx, rows, radii[pick], None if radii[pick] is None else 0.8 * radii[pick], itype=ITYPES[1 - it], ref=refs[pick])


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", DTYPES)
def test_designed_clouds(dtype):
    d = ic.designed(dtype)
    names = list(d)
    empty = dict(ic.random_cloud(9, 12, 12, dtype), rows=0)                        # a cloud with no rows
    P, idx, rows = ic.pad_batch(list(d.values()) + [empty])
    assert rows[-1] == 0
    ref = check(P, idx, rows)
    check(P, idx, rows, itype=np.int32, ref=ref)
    sal, cnt, mask, eig = ref["sal64"], ref["count"], ref["mask"], ref["eig"].astype(np.float64)
    b = names.index("duplicates")
    assert sal[b, 0] > 0 and sal[b, 0] == sal[b, 1] and list(np.flatnonzero(mask[b])) == [0]       # equal saliency, one keypoint: the lower row
    b = names.index("planar")
    assert eig[b, 0, 0] == 0.0 and eig[b, 0, 1] > 0 and not sal[b].any() and not mask[b].any()
    b = names.index("collinear")
    assert eig[b, 0, 0] == 0.0 and eig[b, 0, 1] == 0.0 and eig[b, 0, 2] > 0 and not mask[b].any()
    b = names.index("counts")
    assert list(cnt[b, [0, 5]]) == [5, 4] and sal[b, 0] > 0 and sal[b, 5] == 0 and list(np.flatnonzero(mask[b])) == [0]
    four = check(P, idx, rows, min_neighbors=4)
    assert four["sal64"][b, 5] > 0 and list(np.flatnonzero(four["mask"][b])) == [0, 5]
    b = names.index("only_itself")
    assert list(cnt[b, :6]) == [1, 1, 0, 0, 0, 0] and not eig[b].any() and not mask[b].any()
    b = names.index("non_finite")
    assert cnt[b, 0] == 9 and sal[b, 0] > 0 and mask[b, 0]
    assert not cnt[-1].any() and not eig[-1].any() and not sal[-1].any() and not mask[-1].any()
    b = names.index("ratio")                                                       # a ratio exactly at gamma fails the strict test
    assert eig[b, 0, 1] == 0.25 * eig[b, 0, 2] and eig[b, 0, 0] == 0.25 * eig[b, 0, 1]
    for g21, g32, salient in ((0.25, 0.5, False), (0.5, 0.25, False), (0.5, 0.5, True)):
        at = check(P, idx, rows, gamma21=g21, gamma32=g32)
        assert bool(at["sal64"][b, 0] > 0) == salient and bool(at["mask"][b, 0]) == salient


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("dtype", DTYPES)
def test_idx_of_the_searches(dtype):
    clouds = [ic.random_cloud(31 + b, 700, 1, dtype, rows=r, garbage=False) for b, r in enumerate((700, 520))]
    P, _, rows = ic.pad_batch(clouds)
    Pd, rw = dev(P), torch.tensor(rows).cuda()
    r1, r2 = 0.3, 0.2
    _, idx_ball = ball_query(Pd, Pd, r1, k=24, x_rows=rw, y_rows=rw)
    _, idx_knn = knn_points(Pd, Pd, 24, x_rows=rw, y_rows=rw, method="grid")
    assert (idx_ball >= 0).sum() > 3 * 700 and (idx_ball == -1).any()
    ref = check(P, host(idx_ball), rows, r1, r2)
    assert ref["mask"].sum() >= 4
    hybrid = check(P, host(idx_knn), rows, r1, r2)                  # the k nearest, cut by the recomputed distances: the same members
    if dtype == np.float64:                                         # (float32: the search's own d2 decides at the rim of the ball)
        assert np.array_equal(hybrid["count"], ref["count"])
    _, idx_small = ball_query(Pd, Pd, r2, k=9, x_rows=rw, y_rows=rw)
    other = check(P, host(idx_ball), rows, r1, None, nms=host(idx_small))           # a second index, another k, for the suppression
    assert ir.same_bits(other["sal"], ref["sal"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_forms(dtype):
    rows = [90, 61, 75]
    clouds = [ic.random_cloud(51 + b, 90, 12, dtype, rows=r) for b, r in enumerate(rows)]
    P, idx, rw = ic.pad_batch(clouds)
    r1, r2 = 0.6, 0.45
    ref = check(P, idx, rw, r1, r2)
    assert ref["mask"].sum() >= 3
    kw = dict(salient_radius=r1, non_max_radius=r2, return_saliency=True)
    for b, r in enumerate(rows):
        mask, sal = iss_keypoints(dev(P[b, :r]), dev(idx[b, :r]), **kw)
        assert mask.shape == (r,) and np.array_equal(host(mask), ref["mask"][b, :r]) and ir.same_bits(host(sal), ref["sal"][b, :r])
        eig = iss_saliency(dev(P[b, :r]), dev(idx[b, :r]), radius=r1, return_eigenvalues=True)[1]
        assert eig.shape == (r, 3) and ir.same_bits(host(eig), ref["eig"][b, :r])
    lists = [[dev(a[b, :r]) for b, r in enumerate(rows)] for a in (P, idx)]
    masks, sals = iss_keypoints(*lists, **kw)
    assert isinstance(masks, list) and all(np.array_equal(host(o), ref["mask"][b, :r]) for b, (o, r) in enumerate(zip(masks, rows)))
    assert all(ir.same_bits(host(o), ref["sal"][b, :r]) for b, (o, r) in enumerate(zip(sals, rows)))
    mask_c, sal_c = iss_keypoints(torch.from_numpy(P), torch.from_numpy(idx), rows=torch.tensor(rows), **kw)
    assert not mask_c.is_cuda and not sal_c.is_cuda and np.array_equal(mask_c.numpy(), ref["mask"]) and ir.same_bits(sal_c.numpy(), ref["sal"])
    cnt_c = iss_saliency(torch.from_numpy(P), torch.from_numpy(idx), rows=torch.tensor(rows), radius=r1, return_counts=True)[1]
    assert not cnt_c.is_cuda and np.array_equal(cnt_c.numpy(), ref["count"])
    x = dev(P[0]).requires_grad_(True)
    mask, sal = iss_keypoints(x, dev(idx[0]), **kw)
    assert not mask.requires_grad and not sal.requires_grad and ir.same_bits(host(sal), ref["sal"][0])
    assert not iss_saliency(x, dev(idx[0]), radius=r1).requires_grad


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("dtype", DTYPES)
def test_compute_iss_keypoints(dtype):
    rows = [400, 333]
    clouds = [ic.random_cloud(61 + b, 400, 1, dtype, rows=r, cols=4, garbage=False) for b, r in enumerate(rows)]
    P, _, rw = ic.pad_batch(clouds)
    P[..., 3] = np.arange(P.shape[0] * P.shape[1]).reshape(P.shape[:2])            # a column carried along
    Pd, rt = dev(P), torch.tensor(rw).cuda()
    r1, r2, k = 0.35, 0.25, 20
    # the three steps written out
    idx = ball_query(Pd, Pd, r1, k=k, x_rows=rt, y_rows=rt)[1]
    mask = iss_keypoints(Pd, idx, rows=rt, salient_radius=r1, non_max_radius=r2)
    want, want_rows, want_index = select_rows(Pd, mask, rows=rt, return_index=True)
    ref = ir.keypoints_ref_batch(P, host(idx), rw, salient_radius=r1, non_max_radius=r2)
    assert np.array_equal(host(mask), ref["mask"]) and ref["mask"].sum(axis=1).min() >= 3
    got, got_rows, index = compute_iss_keypoints(Pd, r1, r2, k=k, rows=rt, return_index=True)
    assert torch.equal(got, want) and torch.equal(got_rows, want_rows) and torch.equal(index, want_index)
    assert got.shape == Pd.shape and got_rows.dtype == torch.int32 and list(host(got_rows)) == list(ref["mask"].sum(axis=1))
    for b in range(2):                                               # index names the mask's rows in order
        n = int(got_rows[b])
        assert list(host(index[b, :n])) == list(np.flatnonzero(ref["mask"][b])) and bool((index[b, n:] == -1).all())
        assert ir.same_bits(host(got[b, :n]), P[b][ref["mask"][b]]) and not host(got[b, n:]).any()
    two = compute_iss_keypoints(Pd, r1, k=k, rows=rt)               # non_max_radius=None: the salient radius
    assert len(two) == 2 and torch.equal(two[0], compute_iss_keypoints(Pd, r1, r1, k=k, rows=rt)[0])
    single = compute_iss_keypoints(Pd[1, :333], r1, r2, k=k, return_index=True)
    assert single[0].shape == (int(got_rows[1]), 4) and torch.equal(single[0], got[1, :int(got_rows[1])]) and torch.equal(single[2], index[1, :int(got_rows[1])])
    # the gradient reaches exactly the kept rows
    x = Pd.clone().requires_grad_(True)
    out, _ = compute_iss_keypoints(x, r1, r2, k=k, rows=rt)
    assert out.requires_grad
    w = torch.arange(1, out.numel() + 1, dtype=out.dtype, device=out.device).reshape(out.shape)
    (out * w).sum().backward()
    g = host(x.grad)
    assert (g[ref["mask"]] != 0).all() and not g[~ref["mask"]].any()


# ------------------------------------------------------------------ 5
def test_captured_call():
    rows = [400, 333]

    def data(seed):
        clouds = [ic.random_cloud(seed + b, 400, 16, np.float32, rows=r) for b, r in enumerate(rows)]
        P, idx, rw = ic.pad_batch(clouds)
        return {"P": dev(P), "idx": dev(idx), "rows": torch.tensor(rw, dtype=torch.int32).cuda()}

    def run(s):
        sal, eig, cnt = iss_saliency(s["P"], s["idx"], rows=s["rows"], radius=0.5, return_eigenvalues=True, return_counts=True)
        mask = iss_keypoints(s["P"], s["idx"], rows=s["rows"], salient_radius=0.5, non_max_radius=0.4)
        return sal, eig, cnt, mask
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
        assert all(ir.same_bits(host(c), host(e)) for c, e in zip(captured, eager))
        assert captured[3].sum() > 0


# ------------------------------------------------------------------ 6
CORNER_SEEDS = (1, 2, 3, 4, 5)


def test_corner_scene():
    """Three exactly planar faces of the cube [0, 4]^3 meeting at the origin (tests/iss_cases.py: corner_scene), float64, salient and
    non-max radius 0.6, k = 32 (no ball holds more than 27 rows): every row farther than 0.6 from all three edges has saliency exactly 0
    (its neighbourhood lies in one axis-aligned plane: every d along the normal is 0), every keypoint lies within 0.6 of an edge, the
    nearest keypoint to the corner is within 0.6 of it, and there are between 1 and 32 keypoints (tests/iss_ref.py alone, on the CPU:
    7 to 10 a seed).  Seed 0 of this generator is left out: there the reference's nearest keypoint to the corner is 0.90 away -- the
    rows nearer to the corner are suppressed by more salient ones within their ball, which non-maximum suppression allows -- so the
    third property is one of the seeded scenes, not of the detector."""
    scenes = [ic.corner_scene(seed) for seed in CORNER_SEEDS]
    P = np.stack([s[0] for s in scenes])
    Pd = dev(P)
    _, idx, counts = ball_query(Pd, Pd, ic.CORNER_RADIUS, k=32, return_counts=True)
    assert int(counts.max()) <= 27
    ref = check(P, host(idx), None, ic.CORNER_RADIUS, ic.CORNER_RADIUS)
    kp, rows_out, index = compute_iss_keypoints(Pd, ic.CORNER_RADIUS, k=32, return_index=True)
    sal = host(iss_saliency(Pd, idx, radius=ic.CORNER_RADIUS))
    for b, (pts, edge) in enumerate(scenes):
        n = int(rows_out[b])
        rows = host(index[b, :n])
        assert list(rows) == list(np.flatnonzero(ref["mask"][b]))
        assert not sal[b][edge > ic.CORNER_RADIUS].any() and (sal[b] > 0).sum() > n
        assert (edge[rows] <= ic.CORNER_RADIUS).all()
        assert np.linalg.norm(pts[rows], axis=1).min() <= ic.CORNER_RADIUS
        assert 1 <= n <= 32
        print("seed %d: %d keypoints, %d salient rows, the nearest keypoint to the corner %.3f away" %
              (CORNER_SEEDS[b], n, int((sal[b] > 0).sum()), float(np.linalg.norm(pts[rows], axis=1).min())))


# ------------------------------------------------------------------ 7
def test_end_to_end_registration_on_keypoints():
    """The chain of the README on the seeded scene of tests/test_gpu_fpfh.py's last test (m = 1500, the source an 85 % subset, rotated by
    1 rad about a nearly vertical axis, moved metres away, 2 mm of noise): normals -> compute_fpfh -> compute_iss_keypoints -> select_rows
    of the descriptors with the same mask -> match_features -> ransac_correspondences on the KEYPOINTS -> ICP on all points.  It must end
    within the errors the all-points test accepts, 1e-2 rad and 5e-2.  Salient radius 0.8 (the descriptor's), non-max radius 0.4: with
    tests/iss_ref.py and tests/fpfh_ref.py alone, on the CPU, that gives 79 and 93 keypoints, 46 mutual matches, 24 of them within 0.15
    of the true row -- enough for RANSAC on the 1500-point scene as it is."""
    P = fc.scene(0, 1500)
    mv = fc.moved_copy(P, seed=0, keep=0.85, angle=1.0, noise=0.002, axis=fc.E2E_AXIS)
    y, x = dev(P.astype(np.float32)), dev(mv["x"].astype(np.float32))
    vp_y = torch.tensor(fc.VIEWPOINT, dtype=torch.float32)
    vp_x = torch.tensor(fc.VIEWPOINT @ mv["R"].T + mv["t"], dtype=torch.float32)
    ny = estimate_normals(y, k=16, viewpoint=vp_y)
    nx = estimate_normals(x, k=16, viewpoint=vp_x)
    fx, fy = compute_fpfh(x, nx, 0.8, k=32), compute_fpfh(y, ny, 0.8, k=32)
    keys = {}
    for name, pts, f in (("x", x, fx), ("y", y, fy)):
        kp, rows, index = compute_iss_keypoints(pts, 0.8, 0.4, k=32, return_index=True)
        mask = torch.zeros(pts.shape[0], dtype=torch.bool, device=pts.device)
        mask[index] = True
        fk, frows = select_rows(f, mask)
        assert int(frows) == int(rows) == kp.shape[0] and torch.equal(fk, f[index]) and torch.equal(kp, pts[index])
        keys[name] = (kp, fk, host(index))
    (kx, fkx, ix), (ky, fky, iy) = keys["x"], keys["y"]
    assert 20 <= kx.shape[0] <= 1500 // 8 and 20 <= ky.shape[0] <= 1500 // 8          # a few dozen points in place of 1500
    idx, _ = match_features(fkx, fky, mutual=True)
    got = host(idx)
    live = got >= 0
    err = np.linalg.norm(P[iy[np.where(live, got, 0)]] - P[mv["src"][ix]], axis=1)
    print("keypoints %d and %d; mutual matches %d, within 0.15 of the true row: %d" % (kx.shape[0], ky.shape[0], live.sum(), (err[live] <= 0.15).sum()))
    T0, inl = ransac_correspondences(kx, ky, idx, 0.15, hypotheses=4096, seed=7, refine=2)
    C_true, r_true = mv["R"].T, -mv["R"].T @ mv["t"]
    icp = ICP(icp_type="pt2pt", max_iterations=30, tolerance=1e-9)
    out = icp.icp(x[None], y[None], T_init=T0[None])
    Th = host(out["T"][0]).astype(np.float64)
    rot, tr = rotation_error(Th[:3, :3].reshape(-1), C_true), float(np.linalg.norm(Th[:3, 3] - r_true))
    print("RANSAC on the keypoints: %d inliers; ICP from its pose: %.3g rad, %.3g m" % (int(inl.sum()), rot, tr))
    assert rot < 1e-2 and tr < 5e-2
