"""What the CPU and the GPU tests of dicp_amd.evaluate share: the ctypes front of the g++ build of csrc/dicp_evaluate.h, the comparison
with the numpy restatement tests/evaluate_ref.py, the inputs and the two derived bounds.

THE BOUND OF THE INFORMATION MATRIX (info_bound).  The kernel's matrix and evaluate_ref.info_plain's sum the SAME products -- t_x t_x,
t_x t_y, ... and the coordinates themselves, each rounded once in double; a sign changes no bit -- in two different orders.  A sum of k
terms in any order errs by at most gamma_(k-1) sum |terms|, gamma_k = k u / (1 - k u), u = 2^-53.  An entry of the plain form adds three
values per matched point, 3 count in all; an entry of the kernel's form adds at most 2 count terms (two moment sums of count terms each,
then one more addition; the +0 of the unmatched rows and of the pad lanes change nothing).  So both stand within gamma_(3 count) A of the
exact sum, A = the sum of the |terms| of the entry, and they differ by at most 2 gamma_(3 count) A.  The eigenvalues of a symmetric
matrix move by at most the spectral norm of the perturbation, which is at most the sum over all 36 entries of that bound: the exact
matrix is a Gram matrix (eigenvalues >= 0), so the kernel's are >= -sum(bound).

THE BOUND OF THE SCENE'S RMSE (rmse_bound).  The reference is the float64 numpy brute force on the same arrays.  With u_T the unit
roundoff of the points' dtype, a query coordinate is three fma roundings away from the exact one: |dq_a| <= 3 u_T (1 + 2 u_T) S,
S = max_a sum_k |C_ak| |x_k| + |r_a|, so the query moves by at most 3.01 sqrt(3) u_T S.  The distance to the NEAREST row is 1-Lipschitz
in the query whichever row wins.  d2 is then formed in T from five roundings on non-negative terms, a relative 5 u_T, 2.5 u_T on the
distance itself, which is at most max_distance.  The float64 reference errs in the same way at u = 2^-53.  |rms(a) - rms(b)| <=
max |a_i - b_i| for vectors of one length (the counts are asserted equal), and the two orders of summation of SSE add a relative
n 2^-53 / 2 on the root.  So |rmse - rmse_ref| <= (u_T + 2^-53) (5.3 S + 2.6 max_distance) + n 2^-53 max_distance.

A plain module (no fixtures): the tests put this directory on sys.path and import it.
"""
import ctypes

import numpy as np

import evaluate_ref as er
import fpfh_cases as fc
import hostbuild
import ransac_ref as rr

P_, I = ctypes.c_void_p, ctypes.c_int
SFX = {np.float32: "f32", np.float64: "f64"}
DTYPES = [np.float32, np.float64]
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
CHECKED = ("idx", "d2", "counts", "sums", "fitness", "rmse")


def build():
    lib = hostbuild.build("evaluate_check.cpp", "evaluate_check", ("-Wall", "-ffp-contract=off"))
    for name in ("ec_tile", "ec_terms", "ec_h_max"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = I, []
    for dt, s in SFX.items():
        f = getattr(lib, "ec_run_" + s)
        f.restype = None
        f.argtypes = [P_, I, I, I, P_, I, I, I, P_, I, ctypes.c_float if dt is np.float32 else ctypes.c_double] + [P_] * 7
    return lib


def _ptr(a):
    return a.ctypes.data_as(P_)


def header_run(lib, x, y, T, radius, x_rows=None, y_rows=None):
    """dicp_evaluate_poses' outputs for one cloud from the g++ build -> dict idx (H, n), d2 (H, n), counts (H,), sums (H, 10), fitness (H,),
    rmse (H,), stats (4,): enlarged, flat, live rows, rows visited"""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    dt = x.dtype.type
    T = np.ascontiguousarray(np.asarray(T, dtype=dt).reshape(-1, 4, 4))
    H, n, m = T.shape[0], x.shape[0], y.shape[0]
    out = dict(idx=np.zeros((H, n), np.int64), d2=np.zeros((H, n), dt), counts=np.zeros(H, np.int32), sums=np.zeros((H, er.TERMS)),
               fitness=np.zeros(H), rmse=np.zeros(H), stats=np.zeros(4, np.int64))
    ys = y if m else np.zeros((1, max(y.shape[1], 3)), dt)
    xs = x if n else np.zeros((1, max(x.shape[1], 3)), dt)
    getattr(lib, "ec_run_" + SFX[dt])(_ptr(xs), n, xs.shape[1], n if x_rows is None else int(x_rows), _ptr(ys), m, ys.shape[1],
                                      m if y_rows is None else int(y_rows), _ptr(T), H, dt(radius), *[_ptr(out[k]) for k in CHECKED], _ptr(out["stats"]))
    return out


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def differences(got, ref, names=CHECKED):
    """the names of the checked quantities that are not the restatement's bit for bit (-0.0 and +0.0 differ)"""
    return [k for k in names if not same_bits(got[k], ref[k])]


# ------------------------------------------------------------------ poses
def pose44(C, r, dtype):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = C, r
    return T.astype(dtype)


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


# ------------------------------------------------------------------ the random case: rows of very different magnitudes
def magnitudes_case(seed, n, m, H, dtype, radius=0.05):
    """Target rows scaled by 2^-6 .. 2^6, every source row the pre-image of a target row under pose 0 plus a little noise (so nearly every
    row matches and the terms of a sum differ by orders of magnitude); pose 1 is pose 0 turned a little, pose 2 far off
    -> x (n, 3), y (m, 3), T (H, 4, 4), radius"""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((m, 3)) * 2.0 ** rng.integers(-6, 7, (m, 1))
    C, r = rr.rotation(rng), rng.uniform(-0.5, 0.5, 3)
    to = rng.integers(0, m, n)
    x = (y[to] + 1e-4 * np.abs(y[to]) * rng.standard_normal((n, 3)) - r) @ C           # C^T (y - r)
    poses = [pose44(C, r, dtype), pose44(rr.rotation(rng, 0.002) @ C, r + 0.001, dtype), pose44(rr.rotation(rng, 2.0), r + 3.0, dtype),
             pose44(np.eye(3), np.zeros(3), dtype), pose44(C, r - 0.002, dtype)]
    return x.astype(dtype), y.astype(dtype), np.stack(poses[:H]), radius


# ------------------------------------------------------------------ designed inputs: each sits on a comparison of the definition
def designed(dtype):
    """{name: dict(x, y, T, radius, x_rows, y_rows, expect)}; expect(out) asserts what the definition says about the case, on the
    restatement's, the g++ build's or the kernel's outputs alike (out: idx (H, n), d2 (H, n), counts (H,), fitness, rmse)"""
    dt = dtype
    rng = np.random.default_rng(11)
    eye = pose44(np.eye(3), np.zeros(3), dt)[None]
    cases = {}

    # a target duplicated at two indices: the lower index wins
    y = rng.uniform(-1, 1, (50, 3)).astype(dt)
    y[40], y[33] = y[5], y[12]
    x = np.stack((y[5], y[12], y[40] + dt(1e-3), y[7])).astype(dt)

    def dup(o):
        assert o["idx"][0].tolist() == [5, 12, 5, 7] and o["d2"][0, 0] == 0 and o["d2"][0, 1] == 0 and o["counts"][0] == 4
    cases["duplicate"] = dict(x=x, y=y, T=eye, radius=0.1, expect=dup)

    # d2 == r2 exactly is inside, one ulp beyond is outside (identity pose: q = x exactly; d2 = fl(a a) = r2)
    a = dt(0.3)
    y = np.zeros((3, 3), dt)
    y[1:] = 50.0
    x = np.zeros((4, 3), dt)
    x[0, 0], x[1, 1], x[2, 2], x[3, 0] = a, np.nextafter(a, dt(1)), -a, np.nextafter(-a, dt(-1))

    def edge(o):
        assert o["idx"][0].tolist() == [0, -1, 0, -1] and o["d2"][0, 0] == a * a and o["d2"][0, 2] == a * a
        assert np.isposinf(o["d2"][0, [1, 3]]).all() and o["counts"][0] == 2 and o["fitness"][0] == 0.5
        assert o["rmse"][0] == np.sqrt(np.float64(a * a))
    cases["on_the_radius"] = dict(x=x, y=y, T=eye, radius=float(a), expect=edge)

    # non-finite values: a NaN source row, an inf target row, a NaN pose entry among three poses
    x, y, T, radius = magnitudes_case(3, 300, 200, 3, dt)
    x, y, T = x.copy(), y.copy(), T.copy()
    x[17, 1] = np.nan
    y[::7, 2] = np.inf
    T[1, 1, 2] = np.nan
    T = np.concatenate((T, T[:1]))                              # pose 3 = pose 0: unaffected by its neighbour

    def nonfinite(o):
        assert o["idx"][0, 17] == -1 and not np.isin(o["idx"], np.arange(0, 200, 7)).any()
        assert o["counts"][1] == 0 and o["fitness"][1] == 0 and o["rmse"][1] == 0 and (o["idx"][1] == -1).all() and np.isposinf(o["d2"][1]).all()
        assert o["counts"][0] > 100 and same_bits(o["idx"][3], o["idx"][0]) and same_bits(o["d2"][3], o["d2"][0]) and o["rmse"][3] == o["rmse"][0]
    cases["non_finite"] = dict(x=x, y=y, T=T, radius=radius, expect=nonfinite)

    # zero-size clouds
    x, y, T, radius = magnitudes_case(4, 70, 90, 2, dt)

    def empty(o):
        assert (o["counts"] == 0).all() and (o["fitness"] == 0).all() and (o["rmse"] == 0).all() and (o["idx"] == -1).all()
    cases["no_source_rows"] = dict(x=x, y=y, T=T, radius=radius, x_rows=0, expect=empty)
    cases["no_target_rows"] = dict(x=x, y=y, T=T, radius=radius, y_rows=0, expect=empty)

    # rows past the counts hold NaN and have no influence
    xn, yn = np.concatenate((x[:50], np.full((20, 3), np.nan, dt))), np.concatenate((y[:60], np.full((30, 3), np.nan, dt)))
    short = er.evaluate_ref(x[:50], y[:60], T, radius)

    def past(o):
        assert same_bits(o["idx"][:, :50], short["idx"]) and (o["idx"][:, 50:] == -1).all() and same_bits(o["counts"], short["counts"])
        assert same_bits(o["rmse"], short["rmse"]) and same_bits(o["fitness"], short["fitness"])
    cases["nan_past_the_counts"] = dict(x=xn, y=yn, T=T, radius=radius, x_rows=50, y_rows=60, expect=past)

    # a tiny radius against a huge extent: enlarged cells; the queries sit on target rows
    big = 2.0 ** 40 if dt is np.float64 else 2.0 ** 20
    y = (rng.uniform(-1, 1, (120, 3)) * big).astype(dt)
    y[:40] = rng.uniform(-1, 1, (40, 3)).astype(dt)
    x = y[rng.integers(0, 120, 80)].copy()

    def tiny(o):
        assert o["counts"][0] == 80 and (o["d2"][0] == 0).all() and o["rmse"][0] == 0 and o["fitness"][0] == 1.0
    cases["enlarged_cells"] = dict(x=x, y=y, T=eye, radius=2.0 ** -30 if dt is np.float64 else 2.0 ** -20, expect=tiny, stats=(1, 0))

    # an extent that overflows the dtype: a flat grid, every query scans every live row
    far = dt(np.finfo(dt).max * 0.75)
    y = rng.uniform(-1, 1, (40, 3)).astype(dt)
    y[0], y[1] = far, -far
    x = np.concatenate((y[2:12] + dt(1e-3), y[:2])).astype(dt)

    def flat(o):
        assert o["idx"][0].tolist() == list(range(2, 12)) + [0, 1] and o["counts"][0] == 12
    cases["flat_grid"] = dict(x=x, y=y, T=eye, radius=0.01, expect=flat, stats=(1, 1))

    # a query far outside the cloud (and one past the convertible range of the cells)
    y = rng.uniform(-1, 1, (60, 3)).astype(dt)
    x = np.stack((y[3], y[3] + dt(1e6), np.full(3, np.finfo(dt).max * 0.5, dt), y[9] - dt(1e-3))).astype(dt)

    def outside(o):
        assert o["idx"][0].tolist() == [3, -1, -1, 9] and o["counts"][0] == 2 and o["fitness"][0] == 0.5
    cases["far_outside"] = dict(x=x, y=y, T=eye, radius=0.01, expect=outside)
    return cases


def ref_of(case, wrong=None):
    return er.evaluate_ref(case["x"], case["y"], case["T"], case["radius"], case.get("x_rows"), case.get("y_rows"), wrong=wrong)


# ------------------------------------------------------------------ the information matrix
def info_bound(y, idx):
    """-> (plain (6, 6), bound (6, 6)): the independent accumulation and the largest difference from the kernel's form, entry by entry"""
    L, A = er.info_plain(y, idx)
    k = 3 * int((idx >= 0).sum())
    u = 2.0 ** -53
    return L, 2.0 * (k * u / (1.0 - k * u)) * A


# ------------------------------------------------------------------ the scene
SCENE_DISTANCE = 0.15
SCENE_FITNESS = (1.0, 0.449, 0.011)         # a float64 numpy brute force: the true pose, the pose turned by 0.05 rad about z, the identity
SCENE_RMSE = (0.00344, 0.105, 0.111)


def scene_case(dtype):
    """fpfh_cases.scene(0, 1500) as the target, its moved copy (seed 0, 85 % of the rows, 1 rad, noise 0.002) as the source; the candidates:
    the true inverse motion, the same turned by 0.05 rad about z, the identity -> x (1275, 3), y (1500, 3), T (3, 4, 4)"""
    y = fc.scene(0, 1500)
    mv = fc.moved_copy(y, seed=0, keep=0.85, angle=1.0, noise=0.002)
    Ci, ri = mv["R"].T, -mv["R"].T @ mv["t"]
    Z = rot_z(0.05)
    T = np.stack((pose44(Ci, ri, dtype), pose44(Z @ Ci, Z @ ri, dtype), pose44(np.eye(3), np.zeros(3), dtype)))
    return mv["x"].astype(dtype), y.astype(dtype), T


def brute_force64(x, y, T, max_distance):
    """float64 numpy, plain arithmetic, on the arrays as given -> (fitness, rmse, count) of one pose"""
    x, y, T = x.astype(np.float64), y.astype(np.float64), np.asarray(T, dtype=np.float64)
    q = x[:, :3] @ T[:3, :3].T + T[:3, 3]
    d2 = ((q[:, None, :] - y[None, :, :3]) ** 2).sum(-1).min(axis=1)
    hit = d2 <= max_distance * max_distance
    count = int(hit.sum())
    return count / x.shape[0], float(np.sqrt(d2[hit].sum() / count)) if count else 0.0, count


def rmse_bound(x, T, max_distance, dtype):
    x, T = x.astype(np.float64), np.asarray(T, dtype=np.float64)
    S = float((np.abs(x[:, :3]) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])).max())
    return (U[dtype] + 2.0 ** -53) * (5.3 * S + 2.6 * max_distance) + x.shape[0] * 2.0 ** -53 * max_distance
