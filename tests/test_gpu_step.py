"""dicp_step (step_body, csrc/kernels_accumulate.h), dicp_step_bwd (step_bwd_kernel, csrc/kernels_backward.h) and dicp_loop_init called directly
through _lib.call, in float32 and float64, and held to tests/step_ref.py: the float64 model with its derived bounds (safety factor 1), exact
equalities for everything that is a fixed-order sum or a single rounding, and -- for the match certificates -- the two inequalities the motion
bound claims, with no tolerance, plus the exact contents of the next guard launch's work lists.  tests/test_step_ref.py shows on the CPU what
these comparators refuse.  `-m gpu`.

With DICP_STEP_EDGES_OUT=<file> the largest |error| / bound per family and the largest lhs / rhs of the motion inequalities are written there
(profiles/r23_step_edges.txt is one such run)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_ref as S  # noqa: E402

from dicp_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [np.float32, np.float64]
CODE = {np.float32: _lib.F32, np.float64: _lib.F64}
RECORD = {}


def note(T, family, value):
    key = ("float32" if T == np.float32 else "float64", family)
    RECORD[key] = max(RECORD.get(key, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    lines = ["%-8s %-28s %.6g" % (k[0], k[1], v) for k, v in sorted(RECORD.items())]
    print("\n".join(["largest |error| / bound (families) and lhs / rhs (motion):"] + lines))
    out = os.environ.get("DICP_STEP_EDGES_OUT")
    if out and lines:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def to_dev(bufs):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in bufs.items() if v is not None}


def step_call(T, N, scal, bufs, alias=()):
    """dicp_step with the scalar fields `scal` and the buffers `bufs` (numpy, copied to the device; dtype as given) -> every buffer afterwards"""
    dev = to_dev(bufs)
    io = _lib.StepIO(**scal)
    for k, t in dev.items():
        setattr(io, k, t.data_ptr())
    for a, b in alias:
        setattr(io, a, dev[b].data_ptr())
    _lib.call("dicp_step", DEV, CODE[T], ctypes.byref(io), N)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in dev.items()}


def base_bufs(T, N, parts, poses, **kw):
    b = dict(partials=parts, pose_in=poses.astype(T), pose_out=np.full((N, 12), -7, T), delta=np.full((N, 6), -7, T), cost=np.full(N, -7, T),
             areg=np.full((N, 36), -7.0), alive=np.ones(N, T), alive_out=np.full(N, -7, T), converged=np.zeros(N, np.uint8), iterations=np.zeros(N, T),
             matched_ratio=np.zeros(N, T), n_start=np.full(N, 10, T), n_matched=np.full(N, -7, T), n_not_converged=np.zeros(1, np.int32))
    b.update(kw)
    return b


def base_scal(nblk, dim, **kw):
    s = dict(nblk=nblk, iter=0, dim=dim, const_iter=1, tolerance=0.0, rows_per_point=1, n=0, delta_stride=6, cost_stride=1, w_stride=0)
    s.update(kw)
    return s


def io_of(T, dim, pose, **kw):
    io = dict(T=T, dim=dim, iter=0, const_iter=1, tolerance=0.0, pose_in=pose, cost_prev=None, alive=1.0, converged=0, iterations=0.0,
              matched_ratio=0.0, n_start=10.0, weights=False, w_copied=0, frame=None)
    io.update(kw)
    return io


# ------------------------------------------------------------------ 1. forward numerics
NBLK = [1, 2, 3, 15, 16, 17, 31, 32, 33, 64]            # the edges of the 2 x 8 unroll of the reduction


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("nblk", NBLK)
def test_forward_within_the_model(T, dim, nblk):
    rng = np.random.RandomState(1000 * dim + nblk)
    N = 14
    ds = [S.delta_star(rng, S.ANGLES[c % 7], (0.01, 1.0, 50.0)[(c + c // 7) % 3], dim) for c in range(N)]
    parts = np.stack([S.make_partials(rng, nblk, T, dim, ds[c], S.KAPPAS[T][(c + c // 7) % 3]) for c in range(N)])
    poses = np.stack([S.random_pose(rng, T) for _ in range(N)])
    out = step_call(T, N, base_scal(nblk, dim), base_bufs(T, N, parts, poses))
    for c in range(N):
        io = io_of(T, dim, poses[c])
        got = {k: out[k][c] for k in ("cost", "n_matched", "areg", "delta", "pose_out")}
        res = S.hold_forward(got, parts[c], io)
        D = len(S.slots(dim))
        assert np.isfinite(S.solve_bound(np.asarray(got["areg"], dtype=np.float64).reshape(6, 6)[:D, :D], np.ones(1)))      # (the bound says something)
        for k, v in res.items():
            note(T, "fwd " + k, v[1])
        assert all(v[0] for v in res.values()), (dim, nblk, c, res)
        if (c + c // 7) % 3 == 0:                       # (condition 10: the designed step comes out, to the rounding of the blocks)
            np.testing.assert_allclose(out["delta"][c][S.slots(dim)], ds[c][S.slots(dim)], rtol=0, atol=1e-3 * np.abs(ds[c]).max())


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("dim", [2, 3])
def test_forward_ill_conditioned_systems(T, dim):
    """planar normals, all-zero partials, one matched point: only the 1e-12 regulariser keeps the matrix from singular -- the residual is held
    to the backward-error bound, outputs are finite; all-zero partials leave delta = 0 and the pose bit for bit"""
    rng = np.random.RandomState(77 + dim)
    kinds = ["planar", "zeros", "one_point", "planar", "one_point"]
    N = len(kinds)
    parts = np.stack([S.ill_partials(rng, k, T) for k in kinds])
    poses = np.stack([S.random_pose(rng, T) for _ in range(N)])
    out = step_call(T, N, base_scal(3, dim), base_bufs(T, N, parts, poses))
    for c, kind in enumerate(kinds):
        got = {k: out[k][c] for k in ("cost", "n_matched", "areg", "delta", "pose_out")}
        res = S.hold_forward(got, parts[c], io_of(T, dim, poses[c]), ill=True)
        for k, v in res.items():
            note(T, "ill " + k, v[1])
        assert all(v[0] for v in res.values()), (dim, kind, res)
        if kind == "zeros":
            assert np.all(out["delta"][c] == 0) and np.array_equal(out["pose_out"][c], poses[c].astype(T)) and out["cost"][c] == 0


# ------------------------------------------------------------------ 2. bookkeeping
def frames_for(rng, T, N, mode):
    if mode == "none":
        return None
    F = []
    for c in range(N):
        Q = np.eye(3) if (mode == "translation" or c % 2 == 0) else S.rotation(rng)
        F.append(np.concatenate([Q.ravel(), rng.normal(size=3) * 300]))
    return S.rT(np.stack(F), T)


@pytest.mark.parametrize("T", DTYPES)
def test_bookkeeping_table(T):
    """Every row of ICP.py:219-257 the step does on device, per cloud against step_model, all exact: the tolerance at |delta| (1 +- 1e-3) with
    const_iter on and off, iterations / matched_ratio kept when already set, alive = 0 with n_start != 0 (start -> 1), alive_out aliasing alive,
    the carry of the previous cost over an exactly zero one, n_not_converged, the frozen-cloud weight copy with its guard regions, and the
    search pose without a frame, under a translation-only frame and under a rotated one (bit for bit the fma chain of step_ref.frame_pose)."""
    N, nblk, tol = 12, 3, 1e-2
    combos = [(ci, cp, wc, fm, al, n) for ci in (0, 1) for cp in (0, 1) for wc in (0, 1) for fm, al, n in (("none", 0, 1), ("translation", 1, 64), ("mixed", 0, 300))]
    combos += [(0, 1, wc, "mixed", 1, n) for wc in (0, 1) for n in (63, 65)]
    for ci, cp, wc, fm, al, n in combos:
        rng = np.random.RandomState(n + 7 * ci + 3 * cp + wc)
        dim = 2 if n == 64 else 3
        ds, parts = [], []
        for c in range(N):
            d = S.delta_star(rng, 0.3, 1.0, dim)
            d *= tol / np.linalg.norm(d) / (1 + (1e-3 if c % 2 == 0 else -1e-3))          # even clouds: just under the tolerance, odd: just over
            ds.append(d)
            p = S.make_partials(rng, nblk, T, dim, d, 10.0, nmatch=float(7 + c))
            if c % 3 == 0:
                p[:, S.ACC_COST] = 0                                                          # an exactly zero cost
            if c % 4 < 2:
                p[:, S.ACC_SUMW] = 0                                                          # no weight left: the cloud is frozen
            parts.append(p)
        parts = np.stack(parts)
        poses = np.stack([S.random_pose(rng, T) for _ in range(N)])
        frame = frames_for(rng, T, N, fm)
        alive = np.array([0.0 if c in (2, 3, 4, 5) else 1.0 for c in range(N)])
        iters = np.array([9.0 if c in (0, 6) else 0.0 for c in range(N)])
        ratio = np.array([0.25 if c in (0, 8) else 0.0 for c in range(N)])
        n_start = np.array([0.0 if c == 10 else 40.0 + c for c in range(N)])
        conv = np.array([1 if c == 1 else 0 for c in range(N)], np.uint8)
        cost_prev = rng.uniform(1, 2, N) if cp else None
        stride = n + 9
        w_prev, w_cur = rng.uniform(0, 1, (N, stride)), np.full((N, stride), -3.0)
        bufs = base_bufs(T, N, parts, poses, alive=alive.astype(T), iterations=iters.astype(T), matched_ratio=ratio.astype(T), n_start=n_start.astype(T),
                         converged=conv, cost_prev=None if cost_prev is None else cost_prev.astype(T), w_prev=w_prev.astype(T), w_cur=w_cur.astype(T),
                         frame=None if frame is None else frame.astype(T), pose_search_out=np.full((N, 12), -7, T))
        if al:
            del bufs["alive_out"]
        out = step_call(T, N, base_scal(nblk, dim, iter=4, const_iter=ci, tolerance=tol, n=n, w_stride=stride, w_copied=wc), bufs,
                        alias=(("alive_out", "alive"),) if al else ())
        misses = 0
        for c in range(N):
            io = io_of(T, dim, poses[c], iter=4, const_iter=ci, tolerance=tol, cost_prev=None if cost_prev is None else cost_prev[c], alive=alive[c],
                       converged=conv[c], iterations=iters[c], matched_ratio=ratio[c], n_start=n_start[c], weights=True, w_copied=wc,
                       frame=None if frame is None else frame[c])
            ref = S.step_model(parts[c], io)
            what = (ci, cp, wc, fm, al, n, c)
            assert ref["hit"] == (c % 2 == 0), what
            misses += ref["not_converged"]
            assert out["converged"][c] == ref["converged"], what
            assert out["iterations"][c] == ref["iterations"] and out["matched_ratio"][c] == T(ref["matched_ratio"]), (what, out["matched_ratio"][c], ref["matched_ratio"])
            assert out["alive" if al else "alive_out"][c] == ref["alive_out"], what
            assert out["cost"][c] == T(ref["cost"]) and out["n_matched"][c] == ref["n_matched"], what
            if ref["copy"]:
                assert np.array_equal(out["w_cur"][c, :n], w_prev[c, :n].astype(T)), what
            else:
                assert np.all(out["w_cur"][c, :n] == -3), what
            assert np.all(out["w_cur"][c, n:] == -3), what                                  # (rows past n: another cloud's, or nobody's)
            want = S.frame_pose(None if frame is None else frame[c], out["pose_out"][c], T)  # from the kernel's own new pose
            assert np.array_equal(out["pose_search_out"][c].astype(np.float64), want), (what, out["pose_search_out"][c], want)
        assert int(out["n_not_converged"][0]) == misses == N // 2
        assert np.array_equal(out["w_prev"], w_prev.astype(T))


# ------------------------------------------------------------------ 3. the motion bound
def loop_init(T, T_init, src, frame, K):
    N, n = src.shape[:2]
    dev = to_dev(dict(T_init=T_init.astype(T), src=src.astype(T), frame=None if frame is None else frame.astype(T), pose0=np.zeros((N, 12), T), alive0=np.zeros(N, T),
                      n_start=np.zeros(N, T), ps0=np.zeros((N, 12), T), rmax=np.zeros((N, 4), T), dcum=np.full((N, 2 * (K + 1)), -7, T)))
    _lib.call("dicp_loop_init", DEV, CODE[T], P(dev["T_init"]), None, 0.5, 1, N, n, P(dev["pose0"]), P(dev["alive0"]), P(dev["n_start"]), P(dev.get("frame")),
              P(dev["ps0"]), P(dev["src"]), P(dev["rmax"]), P(dev["dcum"]), 2 * (K + 1))
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in dev.items()}


def motion_run(T, frame_mode, K=8, n=500, seed=0):
    """12 clouds (offsets 0 / 300 / 2500 / 25000 x extents 1 / 20 / 100) through dicp_loop_init and K chained dicp_step calls"""
    rng = np.random.RandomState(seed)
    combos = [(off, ext) for off in (0.0, 300.0, 2500.0, 25000.0) for ext in (1.0, 20.0, 100.0)]
    N = len(combos)
    src = np.stack([S.rT(rng.uniform(-0.5, 0.5, (n, 3)) * ext + off * np.array([0.6, -0.64, 0.48]), T) for off, ext in combos])
    frame = None
    if frame_mode != "none":
        F = []
        for c in range(N):
            Q = np.eye(3) if frame_mode == "translation" else S.rT(S.rotation(rng), T).reshape(3, 3)
            F.append(np.concatenate([Q.ravel(), -Q @ S.rT(src[c].mean(0) + rng.normal(size=3), T)]))
        frame = S.rT(np.stack(F), T)
    T_init = np.zeros((N, 4, 4))
    for c, (off, ext) in enumerate(combos):
        T_init[c, :3, :3], T_init[c, :3, 3], T_init[c, 3, 3] = S.rotation(rng, 0.2), rng.normal(size=3) + 0.05 * off, 1.0
    T_init = S.rT(T_init, T)
    st = loop_init(T, T_init, src, frame, K)
    poses, search = [st["pose0"]], [st["ps0"]]
    dcum = st["dcum"]
    sizes = (1e-6, 1e-3, 0.05, 0.3)
    for k in range(K):
        parts = np.stack([S.make_partials(rng, 1, T, 3, S.delta_star(rng, 0.5 * sizes[(k + c) % 4], 0.5 * sizes[(k + c + k // 4) % 4], 3), 10.0) for c in range(N)])
        out = step_call(T, N, base_scal(1, 3, iter=k, dcum_stride=2 * (K + 1)),
                        base_bufs(T, N, parts, poses[-1], frame=frame if frame is None else frame.astype(T), pose_search_out=np.zeros((N, 12), T), rmax=st["rmax"], dcum=dcum))
        dcum = out["dcum"]
        poses.append(out["pose_out"])
        search.append(out["pose_search_out"])
    return src, frame, T_init, np.stack(poses, 1), np.stack(search, 1), dcum.reshape(N, K + 1, 2), st["rmax"]


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("frame_mode", ["none", "translation", "rotated"])
def test_motion_bound_covers_every_point(T, frame_mode):
    """The soundness condition of the match certificates, as the claim itself (step_ref.motion_check, no tolerance): between any two iterations
    j < k no point of the cloud moves further than M_k - M_j, in the world and -- with the roundings of both transformed points against e_j + e_k --
    in the search frame.  M never decreases; e sits at dcum[2k + 1] and is the model's to the rounding of its handful of operations."""
    src, frame, T_init, poses, search, dcum, rmax = motion_run(T, frame_mode)
    for c in range(src.shape[0]):
        fr = None if frame is None else frame[c]
        assert np.array_equal(search[c, 0].astype(np.float64), S.frame_pose(fr, poses[c, 0], T))
        ww, ws = S.motion_check(src[c], poses[c], search[c], dcum[c], T)
        note(T, "motion world lhs/rhs", ww)
        note(T, "motion search lhs/rhs", ws)
        assert ww <= 1.0 and ws <= 1.0, (frame_mode, c, ww, ws)
        M, e = dcum[c, :, 0].astype(np.float64), dcum[c, :, 1].astype(np.float64)
        assert M[0] == 0 and np.all(np.diff(M) >= 0) and np.all(e > 0)
        assert np.linalg.norm(src[c] - rmax[c, 1:].astype(np.float64), axis=1).max() <= float(rmax[c, 0])           # (radius, midpoint) hold the cloud
        model = S.motion_model(poses[c], rmax[c].astype(np.float64), fr, T)
        # e is at most eight roundings of the working precision away from the model's (e_0: eight operations in T, three of them square roots;
        # e_k: a double expression of as many, rounded to T); M gathers as much per step, in whatever order the sums and the fused round-up take
        assert np.all(np.abs(e - model[:, 1]) <= 8 * S.ulp(model[:, 1], T)), (e, model[:, 1])
        assert np.all(np.abs(M - model[:, 0]) <= 8 * np.arange(len(M)) * S.ulp(model[:, 0], T)), (M, model[:, 0])


# ------------------------------------------------------------------ 4. the next guard launch's work list
CC_ROWS = [None, (0, 0, 0, 0, 0, 0, 0), (0, 0, S.CERT_RECERTIFY, 0, 0, 0, 0), (0, 0, 3, 0, 0, 0, 0), (0, 0, -1, 0, 0, 0, 0),             # state as it is (no certified iteration ran)
           (1, 0, 0, 10, 0, 0, 0), (5, 0, 0, 10, 0, 0, 0), (0, 60, 0, 10, 0, 0, 0), (0, 60, 0, 10, 0, 1, 0), (5, 0, -1, 10, 0, 0, 0), (5, 0, -1, 10, 2, 0, 0),
           (5, 0, -1, 10, 16, 0, 0), (0, 60, -1, 10, 0, 1, 0), (1, 0, -1, 10, 0, 0, 0), (0, 0, 3, 10, 4, 0, 0), (0, 0, 1, 10, 4, 0, 0), (0, 0, S.CERT_OFF_FOR_GOOD, 10, 0, 0, 0),
           (0, 0, S.CERT_RECERTIFY, 10, 0, 0, 0), (0, 60, S.CERT_RECERTIFY, 10, 0, 0, 0), (9, 0, S.CERT_RECERTIFY, 10, 0, 1, 0), (0, 0, S.CERT_RECERTIFY, 10, 0, 1, 0),
           (0, 0, 0, 10, 0, 1, 400), (0, 0, 0, 10, 0, 1, 60)]


def guard_call(T, units, rows, cap, have, n, qu=None, seed=0):
    """one dicp_step over clouds 0 .. 8 with the certificates' buffers; qu None: a first call that only finds (M, e) of the new pose"""
    rng = np.random.RandomState(seed)
    N = 9
    parts = np.stack([S.make_partials(rng, 2, T, 3, S.delta_star(rng, 0.01, 0.05, 3), 10.0) for _ in range(N)])
    poses = np.stack([S.random_pose(rng, T) for _ in range(N)])
    rmax = S.rT(np.concatenate([rng.uniform(1, 5, (N, 1)), rng.normal(size=(N, 3)) * 20], axis=1), T)
    dcum = np.zeros((N, 4))
    dcum[:, 0], dcum[:, 1] = rng.uniform(0, 0.2, N), 1e-5
    cc = None
    if rows is not None:
        cc = np.zeros((N, 8), np.int32)
        for c in range(N):
            cc[c, :7] = rows[c]
    slist = None
    if have is not None:
        slist = np.full((N, n), -9, np.int32)
        for c in range(N):
            slist[c, :min(have[c], n)] = np.arange(min(have[c], n))
    bufs = base_bufs(T, N, parts, poses, rmax=rmax.astype(T), dcum=dcum.astype(T), cert_cloud=cc, cert_qu=(np.zeros((N, units)) if qu is None else qu).astype(T),
                     glist=np.full(8 * cap + 32, -777, np.int32), gcount=np.zeros(8, np.int32), cert_scount=None if have is None else np.array(have, np.int32), cert_slist=slist)
    return step_call(T, N, base_scal(2, 3, n=n, dcum_stride=4, cert_units=units, glist_cap=cap), bufs), cc


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("units", [1, 63, 64, 65, 200])
def test_guard_list_is_the_model_set(T, units):
    """Per list (cloud & 7: clouds 0 and 8 share one) the MULTISET of entries is guard_list_model's, gcount holds the totals -- with budgets just
    above, exactly at and just below what is spent, negative marks and NaN; certificates on, off, tried again, and every branch of the per-cloud
    switch (cert_state_model); candidate-set lists at every length around a chunk of 64.  A list that is too short is cut, never overrun."""
    n = 150
    haves = [0, 1, 63, 64, 65, n, n + 5, 130, 2]
    for variant, rows in enumerate([None] + [[CC_ROWS[1 + (9 * v + c) % (len(CC_ROWS) - 1)] for c in range(9)] for v in range(3)]):
        have = haves if variant != 1 else None
        probe, _ = guard_call(T, units, rows, 4096, have, n, seed=variant)
        nxt = probe["dcum"][:, 2:4]
        spent = np.array([S.cert_spent(nxt[c, 0], nxt[c, 1], T) for c in range(9)])
        rng = np.random.RandomState(5 + variant)
        qu = np.zeros((9, units))
        for c in range(9):
            sp = T(spent[c])
            pool = [np.nextafter(sp, T(np.inf)), sp, np.nextafter(sp, T(0)), T(-1.0), T(-sp), T(np.nan), T(2) * sp, T(0), T(0.5) * sp, T(np.inf)]
            qu[c] = [pool[(u + c) % len(pool)] if u < 2 * len(pool) else pool[rng.randint(len(pool))] for u in range(units)]
        for cap in (4096, 5):
            out, cc = guard_call(T, units, rows, cap, have, n, qu=qu, seed=variant)
            assert np.array_equal(out["dcum"], probe["dcum"])
            want = [[] for _ in range(8)]
            for c in range(9):
                state = 0
                if cc is not None:
                    cc_next, state = S.cert_state_model(cc[c], n)
                    assert list(out["cert_cloud"][c]) == cc_next, (variant, c, out["cert_cloud"][c], cc_next)
                ent, sc, upto = S.guard_list_model(c, qu[c], spent[c], state, units, None if have is None else have[c], n)
                want[c & 7] += ent
                if have is not None:
                    assert out["cert_scount"][c] == (have[c] if sc is None else sc), (variant, c, state)
                    h = min(have[c], n)
                    fill = h if upto is None else upto
                    assert np.array_equal(out["cert_slist"][c, :h], np.arange(h)) and np.all(out["cert_slist"][c, h:fill] == -1) and np.all(out["cert_slist"][c, fill:] == -9), (variant, c)
            lists = out["glist"][:8 * cap].reshape(8, cap)
            for li in range(8):
                assert out["gcount"][li] == len(want[li]), (variant, cap, li, out["gcount"], len(want[li]))
                k = min(cap, len(want[li]))
                if k == len(want[li]):
                    assert sorted(lists[li, :k].tolist()) == sorted(want[li]), (variant, cap, li)
                else:                                   # cut at the cap: which entries made it is the atomics' order, but each is one of the set, once
                    got = lists[li, :k].tolist()
                    assert len(set(got)) == k and set(got) <= set(want[li]), (variant, cap, li)
                assert np.all(lists[li, k:] == -777), (variant, cap, li)
            assert np.all(out["glist"][8 * cap:] == -777)


# ------------------------------------------------------------------ 5. backward
def bwd_call(T, N, gin, bp, nblk, dim, pose, delta, areg):
    dev = to_dev(dict(gin=gin, bp=None if bp is None else bp.astype(T), pose=pose.astype(T), delta=delta.astype(T), areg=areg, gs=np.full((N, 36), -7, T), gb=np.full((N, 6), -7, T),
                      gout=np.full((N, 12), -7.0)))
    _lib.call("dicp_step_bwd", DEV, CODE[T], P(dev["gin"]), P(dev.get("bp")), nblk, dim, P(dev["pose"]), P(dev["delta"]), 6, P(dev["areg"]), P(dev["gs"]), P(dev["gb"]), P(dev["gout"]), N)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in dev.items()}


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("nblk", [1, 3, 4, 5, 15, 16, 17, 33])          # the edges of the 4 x 4 unroll of the reduction
def test_backward_within_the_model(T, dim, nblk):
    rng = np.random.RandomState(2000 * dim + nblk)
    N = 15                                              # 14 of the delta family + one singular Areg (an exactly zero pivot)
    sl = S.slots(dim)
    D = len(sl)
    delta = np.stack([S.rT(S.delta_star(rng, S.ANGLES[c % 7], (0.01, 1.0, 50.0)[(c + c // 7) % 3], dim), T) for c in range(N)])
    areg = np.zeros((N, 6, 6))
    for c in range(N):
        areg[c, :D, :D] = S.spd(rng, D, S.KAPPAS[T][(c + c // 7) % 3], scale=10.0 ** rng.uniform(-1, 2)) + 1e-12 * np.eye(D)
    areg[N - 1, D - 1, :] = 0
    areg[N - 1, :, D - 1] = 0
    areg = areg.reshape(N, 36)
    pose = np.stack([S.random_pose(rng, T) for _ in range(N)])
    gin = rng.normal(size=(N, 12)) * 10.0 ** rng.uniform(-2, 2, (N, 1))
    for with_partials in (False, True):
        bp = None
        if with_partials:
            bp = (rng.normal(size=(N, nblk, 16)) * 10.0 ** rng.uniform(-2, 1, (N, nblk, 1))).astype(T)
            bp[:, :, 12:] = np.nan                      # the pad slots hold anything
        out = bwd_call(T, N, gin, bp, nblk, dim, pose, delta, areg)
        for c in range(N):
            got = {"gs": out["gs"][c], "gb": out["gb"][c], "gpose": out["gout"][c]}
            res = S.hold_backward(got, gin[c], None if bp is None else bp[c], dim, pose[c], delta[c], areg[c], T)
            for k, v in res.items():
                note(T, "bwd " + k, v[1])
            assert all(v[0] for v in res.values()), (dim, nblk, with_partials, c, res)
            assert ("singular" in res) == (c == N - 1)


# ------------------------------------------------------------------ 6. the truncated reverse sweep's verdict
# dicp_step_bwd itself runs with the skip arguments off; they are set by dicp_icp_backward.  One iteration of it (k1 = k0 + 1, the atomic form, no
# small-cloud launch: search.m_pad = 0) on a four-point cloud is step_bwd_kernel with SkipArgs followed by an accumulate_bwd whose outputs are not looked at.
def skip_call(T, N, K, k, dim, gin, pose_k, deltas, areg_k, alive_k, skip, mref, eps):
    n = 4
    rng = np.random.RandomState(9)
    poses = np.zeros((K + 1, N, 12))
    poses[k] = pose_k
    areg = np.zeros((K, N, 36))
    areg[k] = areg_k
    alive = np.ones((K + 1, N))
    alive[k] = alive_k
    dev = to_dev(dict(src=rng.normal(size=(N, n, 3)).astype(T), tgt=rng.normal(size=(N, n, 3)).astype(T), poses=poses.astype(T), deltas=deltas.astype(T), areg=areg, alive=alive.astype(T),
                      idx=np.zeros((K, N, n), np.int32), skip=skip.astype(np.int32), mref=mref.astype(np.float64), live=np.zeros(K + 1, np.int32), gpose=gin.astype(np.float64),
                      gtmp=np.full((N, 12), -7.0), gs=np.full((N, 36), -7, T), gb=np.full((N, 6), -7, T), gsrc=np.zeros((N, n, 3), T), bp=np.zeros((N, 1, 16), T)))
    LB = _lib.LoopBuffers(src=dev["src"].data_ptr(), tgt=dev["tgt"].data_ptr(), c=3, K=K, hist_per_iter=1, hist_poses=dev["poses"].data_ptr(), hist_deltas=dev["deltas"].data_ptr(),
                          hist_areg=dev["areg"].data_ptr(), hist_alive=dev["alive"].data_ptr(), hist_idx=dev["idx"].data_ptr(), bwd_skip=dev["skip"].data_ptr(),
                          bwd_mref=dev["mref"].data_ptr(), bwd_live=dev["live"].data_ptr(), bwd_skip_eps=float(eps))
    prm = _lib.WeightParams(mode=_lib.PT2PT, trim_on=0, differentiable=0, loss=_lib.LOSS_NONE, trim_dist=0.0, tanh_k=5.0, loss_delta=1.0, match_thresh=0.0)
    _lib.call("dicp_icp_backward", DEV, CODE[T], ctypes.byref(prm), ctypes.byref(LB), N, n, n, dim, P(dev["gpose"]), P(dev["gtmp"]), 0, P(dev["gs"]), P(dev["gb"]), P(dev["gsrc"]), None, None,
              P(dev["bp"]), k, k + 1)
    torch.cuda.synchronize()
    return {k_: t.cpu().numpy() for k_, t in dev.items()}


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 130])        # earlier iterations the lanes of one wave run over
def test_skip_verdicts(T, dim, k):
    """skip_model's verdicts with the inputs a factor 2 to either side of the threshold; a NaN in Gs / gb or in an earlier delta never ends a sweep;
    not alive -> 1; a cloud already at 2 takes the pass-through only (gC = R gC', gr = gr', gs / gb keep their guard values); mref is raised only
    when m > mref; live_k counts the clouds that take part; the largest earlier step is found wherever it sits among the k before."""
    N, K, eps = 10, 131, (2.0 ** -22 if T == np.float32 else 2.0 ** -40)
    rng = np.random.RandomState(100 * dim + k)
    sl = S.slots(dim)
    D = len(sl)
    deltas = np.zeros((N, K, 6))
    deltas[:, :, sl] = rng.normal(size=(N, K, D)) * 1e-9
    deltas[:, k] = np.stack([S.delta_star(rng, 1e-3, 0.01, dim) for _ in range(N)])
    areg = np.zeros((N, 6, 6))
    for c in range(N):
        areg[c, :D, :D] = S.spd(rng, D, 10.0, scale=4.0)
    pose = np.stack([S.random_pose(rng, T) for _ in range(N)])
    gin = rng.normal(size=(N, 12))
    alive, skip = np.ones(N), np.zeros(N, np.int32)
    alive[3], skip[4] = 0.0, 2
    gin[6, 10] = np.nan                                                 # -> NaN in gb and Gs
    where = {7: 0, 8: k - 1, 9: 64 if k > 64 else k // 2}               # where the largest earlier step sits
    if k:
        deltas[5, k // 2, sl[1]] = np.nan
        for c, at in where.items():
            deltas[c, at, sl[c % D]] = 1e12 * (-1) ** c
    deltas = S.rT(deltas, T)
    model = [S.step_bwd_model(gin[c], None, dim, pose[c], deltas[c, k], areg[c].ravel()) for c in range(N)]
    mref = np.zeros(N)
    for c in range(N):
        if c == 2 or c == 6:
            continue                                                    # (mref 0: anything is above it)
        quiet = np.where(np.abs(deltas[c, :k]) > 1, 0.0, np.nan_to_num(deltas[c, :k]))
        _, m_alone, _ = S.skip_model(model[c]["gs"], model[c]["gb"], areg[c], quiet, dim, True, False, 0.0, eps)
        s = np.sqrt(np.diag(areg[c])[:D])
        worst = max(m_alone, (np.abs(model[c]["gb"][sl]) * s).max() * ((np.abs(quiet[:, sl]).max(0) * s).max() if k else 0.0))
        mref[c] = 16 * worst / eps * (0.5 if c == 1 else 2.0)            # a factor 2 under / over the threshold
    out = skip_call(T, N, K, k, dim, gin, pose, deltas.reshape(N, K * 6).reshape(N, K, 6), areg.reshape(N, 36), alive, skip, mref, eps)
    live = 0
    for c in range(N):
        verdict, mnew, lv = S.skip_model(model[c]["gs"], model[c]["gb"], areg[c], deltas[c, :k], dim, bool(alive[c]), bool(skip[c] == 2), mref[c], eps)
        live += lv
        assert out["skip"][c] == verdict, (dim, k, c, out["skip"][c], verdict)
        if mnew == mref[c]:
            assert out["mref"][c] == mref[c], (dim, k, c)
        else:                                           # raised to this iteration's m: condition 10, the adjoint's bound is ~1e-12 of it
            assert c == 2 and abs(out["mref"][c] - mnew) <= 1e-10 * mnew + S.ulp(mnew, T), (dim, k, c, out["mref"][c], mnew)
        got = {"gs": out["gs"][c], "gb": out["gb"][c], "gpose": out["gtmp"][c]}
        if skip[c] == 2:
            assert np.all(out["gs"][c] == -7) and np.all(out["gb"][c] == -7)
            R = S.so3_exp(deltas[c, k])
            want = np.concatenate([(R @ gin[c, :9].reshape(3, 3)).ravel(), gin[c, 9:]])
            assert np.array_equal(out["gtmp"][c, 9:], gin[c, 9:])
            assert np.all(np.abs(out["gtmp"][c, :9] - want[:9]) <= np.repeat(((2 * S.EXP_U + 6) * S.U64 * np.abs(gin[c, :9].reshape(3, 3)).sum(0))[None, :], 3, 0).ravel())
        elif c != 6:
            res = S.hold_backward(got, gin[c], None, dim, pose[c], deltas[c, k], areg[c].ravel(), T)
            assert all(v[0] for v in res.values()), (dim, k, c, res)
        else:
            assert np.all(np.isnan(out["gb"][c][sl]))
    assert out["live"][k] == live and out["live"].sum() == live
    expect = {0: 2, 1: 0, 2: 0, 3: 1, 4: 2, 5: 0 if k else 2, 6: 0, 7: 0 if k else 2, 8: 0 if k else 2, 9: 0 if k else 2}
    assert {c: int(out["skip"][c]) for c in range(N)} == expect
