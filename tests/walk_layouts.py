"""Shared by the tests of the two walk operators (knn_points / chamfer_distance and estimate_normals): the input layouts whose neighbour lists
leave the kernels' LDS windows, a numpy model of those windows, the brute-force oracles, and the derived gradient bounds.

The kernels (csrc/knn_points.hip, csrc/normals.hip) stage a window of consecutive x-sorted target rows in LDS and take another code path for a
row outside it: a global read in the forward walks, a global atomic instead of an LDS atomic in the backward scatters.  The model below repeats
the kernels' window expressions on the host.  It is only used to PROVE that a test input reaches the code it is meant for (the share of entries
outside the window, windows that hit their cap); it is never the expected value of anything.  tests/test_walk_layouts.py holds its constants to
the sources, so that a retuned window cannot silently turn the out-of-window tests back into in-window tests.

A plain module (no fixtures): the tests put this directory on sys.path and import it.
"""
import numpy as np
import torch

BLOCK = 256                                             # csrc/dicp_common.h
HALO = {np.dtype(np.float32): 1024, np.dtype(np.float64): 512}      # WinHalo, WalkHalo, BwdHalo
U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}   # unit roundoff u_T


def np_dtype(dtype):
    """numpy dtype of a numpy or torch dtype"""
    if isinstance(dtype, torch.dtype):
        return np.dtype({torch.float32: np.float32, torch.float64: np.float64}[dtype])
    return np.dtype(dtype)


def win_rows(dtype):
    """WinRows / BwdRows, and the normals kernels' BLOCK + 2 H"""
    return BLOCK + 2 * HALO[np_dtype(dtype)]


# ---------------------------------------------------------------- seeded builders (float64; the tests cast to the dtype under test)

def wall(n, seed):
    """a wall perpendicular to x: x in +-1e-3, y and z in +-1"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-1e-3, 1e-3, (n, 1)), rng.uniform(-1.0, 1.0, (n, 2))], 1)


def cube(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3))


def two_clusters(n, seed):
    """x alternately in [0, 0.05] and [0.95, 1]: two blocks of sorted queries, each with a narrow start span"""
    rng = np.random.default_rng(seed)
    P = rng.uniform(0.0, 1.0, (n, 3))
    P[:, 0] = np.where(np.arange(n) % 2 == 0, 0.05 * P[:, 0], 0.95 + 0.05 * P[:, 0])
    return P


def edge_m(delta, dtype):
    """200 queries against W + delta targets, W the window's row count for the dtype.  Queries 0 and 1 sit next to the targets with the largest
    and the smallest x, so that the lists use both ends of the sorted cloud: the one row a window of W rows cannot hold is then a kept entry."""
    x, y = cube(200, 0), cube(win_rows(dtype) + delta, 1)
    x[0] = y[np.argmax(y[:, 0])] + np.array([0.0, 1e-3, 1e-3])
    x[1] = y[np.argmin(y[:, 0])] + np.array([0.0, 1e-3, 1e-3])
    return x, y


EDGE_DELTAS = (-1, 0, 1, 257)
KNN_LAYOUTS = ("wall", "sparse_queries", "dense_queries", "two_clusters", "cube_k16") + tuple("edge_m%+d" % d for d in EDGE_DELTAS)
NORMALS_LAYOUTS = ("wall", "cube")


def knn_layout(name, dtype):
    """-> (x (n,3), y (m,3), k), float64"""
    if name == "wall":
        return wall(20000, 0), wall(20000, 1), 8
    if name == "sparse_queries":
        return cube(300, 0), cube(60000, 1), 8
    if name == "dense_queries":
        return cube(60000, 0), cube(300, 1), 8
    if name == "two_clusters":
        return two_clusters(512, 0), cube(40000, 1), 8
    if name == "cube_k16":
        return cube(20000, 0), cube(20000, 1), 16
    if name.startswith("edge_m"):
        return edge_m(int(name[6:]), dtype) + (4,)
    raise KeyError(name)


def normals_layout(name):
    """-> (points (m,3), k), float64"""
    if name == "wall":
        return wall(20000, 0), 16
    if name == "cube":
        return cube(40000, 0), 16
    raise KeyError(name)


# ---------------------------------------------------------------- the window model

def model_neighbours(X, Y, k, chunk=512):
    """(n,3), (m,3) finite -> (n,k) int64 rows of Y, the k nearest in float64 (unordered; -1 beyond m).  For the window model only: the GPU
    tests pass the kernel's own idx instead.  Sorted by x on both sides, so that a chunk of queries only scores the targets within its k-th
    distance in x."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    n, m = X.shape[0], Y.shape[0]
    ke = min(k, m)
    out = np.full((n, k), -1, dtype=np.int64)
    if ke == 0:
        return out
    oy = np.argsort(Y[:, 0], kind="stable")
    Ys, keys = Y[oy], Y[oy, 0]
    ox = np.argsort(X[:, 0], kind="stable")
    r = np.inf
    for a in range(0, n, chunk):
        q = ox[a:a + chunk]
        Q = X[q]
        while True:
            lo = int(np.searchsorted(keys, Q[:, 0].min() - r, "left"))
            hi = int(np.searchsorted(keys, Q[:, 0].max() + r, "right"))
            if hi - lo < ke and (lo, hi) != (0, m):
                r *= 2.0
                continue
            C = Ys[lo:hi]
            d2 = (C[None, :, 0] - Q[:, None, 0]) ** 2
            d2 += (C[None, :, 1] - Q[:, None, 1]) ** 2
            d2 += (C[None, :, 2] - Q[:, None, 2]) ** 2
            part = np.argpartition(d2, ke - 1, axis=1)[:, :ke] if ke < hi - lo else np.broadcast_to(np.arange(hi - lo), (Q.shape[0], hi - lo))
            rk = float(np.sqrt(np.take_along_axis(d2, part, 1).max()))
            if rk <= r or (lo, hi) == (0, m):
                break
            r = rk * 1.001                              # every true neighbour lies within the k-th distance found: one more pass suffices
        out[q, :ke] = oy[lo + part]
        r = rk * 1.5
    return out


class KnnWindows:
    """What knn_points' two kernels do with every kept (query, neighbour) entry, in the original query order:
    kept (n,k) bool; fwd_outside / bwd_outside (n,k) bool; capped_fwd / capped_bwd: blocks whose window hit its cap; rows_bind_fwd: blocks
    whose forward window ends at the cloud's row count (mb the smallest of span[1] + H, mb, wlo + W, strictly below span[1] + H); blocks;
    indegree (m,): entries per target row."""

    def share(self, which):
        return float(getattr(self, which + "_outside").sum()) / max(int(self.kept.sum()), 1)


def knn_windows(X, Y, k, dtype, idx=None):
    """X (n,3), Y (m,3) (the rows taking part; cast to dtype here), idx (n,k) the neighbour lists (the kernel's, or None: the model's own)"""
    dt = np_dtype(dtype)
    H, W = HALO[dt], win_rows(dt)
    Xc, Yc = np.asarray(X).astype(dt), np.asarray(Y).astype(dt)
    n, m = Xc.shape[0], Yc.shape[0]
    if idx is None:
        idx = model_neighbours(Xc, Yc, k)
    idx = np.asarray(idx)
    oy = np.argsort(Yc[:, 0], kind="stable")            # NaN last, as the kernels' sort
    slot = np.empty(m, dtype=np.int64)
    slot[oy] = np.arange(m)
    keys = Yc[oy, 0]
    ox = np.argsort(Xc[:, 0], kind="stable")
    xs = Xc[ox, 0]
    pos = np.searchsorted(keys, xs, "left")
    kept = idx >= 0
    sl = np.where(kept, slot[np.clip(idx, 0, max(m - 1, 0))] if m else -1, -1)[ox]      # sorted query order
    w = KnnWindows()
    fo, bo = np.zeros((n, k), bool), np.zeros((n, k), bool)
    w.capped_fwd = w.capped_bwd = w.rows_bind_fwd = 0
    w.blocks = (n + BLOCK - 1) // BLOCK
    for b in range(w.blocks):
        s = slice(b * BLOCK, min(n, (b + 1) * BLOCK))
        j = sl[s]
        p = pos[s][~np.isnan(xs[s])]                    # NaN-x queries do not contribute to the forward span
        wlo = whi = 0
        if p.size:
            wlo = max(int(p.min()) - H, 0)
            whi = min(int(p.max()) + H, m, wlo + W)
            w.capped_fwd += min(int(p.max()) + H, m) > wlo + W
            w.rows_bind_fwd += m < int(p.max()) + H and m <= wlo + W       # whi = mb: the cloud's row count ends the staged window
        fo[s] = (j >= 0) & ((j < wlo) | (j >= whi))
        u = j[j >= 0]
        wlo = whi = 0
        if u.size:
            wlo = int(u.min())
            whi = min(int(u.max()) + 1, wlo + W)
            w.capped_bwd += int(u.max()) + 1 > wlo + W
        bo[s] = (j >= 0) & ((j < wlo) | (j >= whi))
    w.kept = kept
    w.fwd_outside, w.bwd_outside = np.zeros((n, k), bool), np.zeros((n, k), bool)
    w.fwd_outside[ox], w.bwd_outside[ox] = fo, bo
    w.indegree = np.bincount(idx[kept], minlength=m)
    return w


class NormalsWindows:
    """estimate_normals' backward window: kept (m,k), bwd_outside (m,k) in the original row order; indegree (m,)"""

    def share(self, which="bwd"):
        return float(getattr(self, which + "_outside").sum()) / max(int(self.kept.sum()), 1)


def normals_windows(P, k, dtype, nbr=None):
    dt = np_dtype(dtype)
    H = HALO[dt]
    Pc = np.asarray(P).astype(dt)
    m = Pc.shape[0]
    if nbr is None:
        nbr = model_neighbours(Pc, Pc, k)
    nbr = np.asarray(nbr)
    o = np.argsort(Pc[:, 0], kind="stable")
    slot = np.empty(m, dtype=np.int64)
    slot[o] = np.arange(m)
    kept = nbr >= 0
    j = np.where(kept, slot[np.clip(nbr, 0, m - 1)], -1)
    s0 = (slot // BLOCK) * BLOCK
    wlo = np.maximum(s0 - H, 0)[:, None]
    whi = np.minimum(s0 + BLOCK + H, m)[:, None]
    w = NormalsWindows()
    w.kept = kept
    w.bwd_outside = kept & ((j < wlo) | (j >= whi))
    w.indegree = np.bincount(nbr[kept], minlength=m)
    return w


def check_knn_conditions(name, dtype, w):
    """The conditions a layout has to meet before a test may look at the GPU result (conditions on inputs, not measurements)"""
    f32 = np_dtype(dtype) == np.dtype(np.float32)
    fs, bs = w.share("fwd"), w.share("bwd")
    if name in ("wall", "sparse_queries"):
        assert bs >= 0.5 and 1.0 - bs >= 0.01, (name, bs)
    elif name == "two_clusters" or (name == "cube_k16" and not f32):
        assert bs >= 0.10 and 1.0 - bs >= 0.10, (name, bs)
    elif name == "cube_k16":
        assert bs >= 0.02, (name, bs)
    elif name == "dense_queries":
        assert w.indegree.max() >= 1000, (name, int(w.indegree.max()))
    elif name in ("edge_m-1", "edge_m+0"):
        assert not w.fwd_outside.any() and not w.bwd_outside.any() and w.capped_bwd == 0, name
    elif name == "edge_m+1":
        assert w.fwd_outside.sum() >= 1, name
    elif name == "edge_m+257":
        assert fs >= 0.05 and bs >= 0.05, (name, fs, bs)
    else:
        raise KeyError(name)
    if name not in ("dense_queries", "edge_m-1", "edge_m+0"):
        assert w.capped_bwd >= 1, (name, w.capped_bwd)


def check_normals_conditions(name, dtype, w):
    s = w.share()
    if name == "wall":
        assert s >= 0.5 and 1.0 - s >= 0.01, (name, s)
    elif name == "cube":
        assert s >= 0.10 and 1.0 - s >= 0.10, (name, s)
    else:
        raise KeyError(name)


# ---------------------------------------------------------------- oracles

def knn_oracle(X, Y, k, chunk=256):
    """(n,3), (m,3) numpy in their own dtype -> (d2 (n,k), idx (n,k)): the first min(k, #finite) rows in (d2, index) order, +inf / -1 beyond"""
    n, m = X.shape[0], Y.shape[0]
    d2o = np.full((n, k), np.inf, dtype=X.dtype)
    io = np.full((n, k), -1, dtype=np.int64)
    for a in range(0, n, chunk):
        Q = X[a:a + chunk]
        with np.errstate(invalid="ignore", over="ignore"):
            dx = Y[None, :, 0] - Q[:, None, 0]
            dy = Y[None, :, 1] - Q[:, None, 1]
            dz = Y[None, :, 2] - Q[:, None, 2]
            xx = dx * dx
            yy = dy * dy
            zz = dz * dz
            d2 = (xx + yy) + zz
        d2 = np.where(np.isfinite(d2), d2, np.inf)
        ke = min(k, m)
        kth = np.partition(d2, ke - 1, axis=1)[:, ke - 1] if m else np.full(Q.shape[0], np.inf)
        for r in range(Q.shape[0]):
            cand = np.flatnonzero((d2[r] <= kth[r]) & np.isfinite(d2[r]))
            order = np.lexsort((cand, d2[r, cand]))[:k]
            io[a + r, :len(order)] = cand[order]
            d2o[a + r, :len(order)] = d2[r, cand[order]]
    return d2o, io


def _nearest_d2(x, y, chunk_elems):
    """min_j |x_i - y_j|^2 from explicit differences, differentiable; in chunks of queries when the (n,m,3) differences would be too large:
    the argmin of each chunk without a graph, then the same expression on the chosen pairs (the value and the gradient of min)"""
    n, m = x.shape[0], y.shape[0]
    if chunk_elems is None or n * m <= chunk_elems:
        d = x[:, None, :] - y[None, :, :]
        return (d * d).sum(-1).min(1).values
    rows = max(1, chunk_elems // m)
    with torch.no_grad():
        arg = []
        for a in range(0, n, rows):
            d = x[a:a + rows, None, :] - y[None, :, :]
            arg.append((d * d).sum(-1).argmin(1))
    d = x - y[torch.cat(arg)]
    return (d * d).sum(-1)


def chamfer_oracle(xs, ys, chunk_elems=None):
    """per-cloud float64 Chamfer distance from explicit differences (no cdist): lists of (n_b,3) float64 tensors requiring grad -> (N,)"""
    out = []
    for x, y in zip(xs, ys):
        if x.shape[0] and y.shape[0]:
            out.append(_nearest_d2(x, y, chunk_elems).mean() + _nearest_d2(y, x, chunk_elems).mean())
        elif x.shape[0] or y.shape[0]:
            out.append((x.sum() + y.sum()) * 0 + float("inf"))
        else:
            out.append((x.sum() + y.sum()) * 0)
    return torch.stack(out)


# ---------------------------------------------------------------- knn_points gradients: float64 terms and derived bounds

def knn_grad_terms(X, Y, idx, g, dtype):
    """X (n,3), Y (m,3), g (n,k) in the dtype under test (numpy), idx (n,k) the kernel's lists -> (Sx, Bx, Sy, By, D): the gradients' exact
    values and the bounds on the kernel's error, all from the float64 terms t_ij = 2 g_ij (x_i - y_idx(i,j)) per coordinate.  The inputs are
    representable, so the extended-precision terms below carry errors far under every bound.  The kernel forms them in double.
      x-gradient Sx_i = sum_j t_ij, summed by the kernel in double in list order and rounded once to T:
          Bx = u_T |Sx| + (k + 2) 2^-53 sum_j |t_ij|
      y-gradient Sy_l = -sum t over the entries idx = l, in-degree D_l: each term rounded to T, then summed in T in an unspecified order (LDS
      atomics, the flush into the sorted rows, global atomics, dicp_permute_add_rows into zeros):
          By = (D_l + 2) u_T sum |t|"""
    L = np.longdouble
    u = U[np_dtype(dtype)]
    n, k = idx.shape
    m = Y.shape[0]
    kept = idx >= 0
    yi = Y[np.clip(idx, 0, max(m - 1, 0))].astype(L)                                  # (n,k,3)
    t = 2 * g.astype(L)[:, :, None] * (X.astype(L)[:, None, :] - yi)
    t = np.where(kept[:, :, None], t, L(0))
    Sx = t.sum(1)
    Bx = u * np.abs(Sx) + (k + 2) * 2.0 ** -53 * np.abs(t).sum(1)
    flat = idx[kept]
    order = np.argsort(flat, kind="stable")
    rows, first, cnt = np.unique(flat[order], return_index=True, return_counts=True)
    Sy, Ay, D = np.zeros((m, 3), L), np.zeros((m, 3), L), np.zeros(m, dtype=np.int64)
    if rows.size:
        tk = t[kept][order]
        Sy[rows] = -np.add.reduceat(tk, first, axis=0)
        Ay[rows] = np.add.reduceat(np.abs(tk), first, axis=0)
        D[rows] = cnt
    return Sx, Bx, Sy, ((D + 2) * u)[:, None] * Ay, D


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound elementwise (a NaN is off its bound); -> the largest error / bound ratio, for the record"""
    err = np.abs(got.astype(np.longdouble) - ref)
    bad = ~(err <= bound)
    ratio = np.where(np.isnan(err), np.inf, err / np.where(bound > 0, bound, 1))
    assert not bad.any(), "%s: %d of %d values off their bound, worst error / bound %.4g at %s" % (
        what, int(bad.sum()), err.size, float(ratio[bad].max()), np.unravel_index(int(np.argmax(np.where(bad, ratio, 0))), err.shape))
    return float(ratio.max()) if err.size else 0.0


def knn_grad_check(X, Y, idx, g, gx, gy, dtype, what=""):
    """The kernel's gradients gx (n,3), gy (m,3) against knn_grad_terms; rows of y that no list holds exactly 0.  -> worst ratios (x, y)"""
    Sx, Bx, Sy, By, D = knn_grad_terms(X, Y, idx, g, dtype)
    rx = assert_within(gx, Sx, Bx, what + " x-gradient")
    assert np.all(gy[D == 0] == 0), "%s y-gradient: a row that no list holds is not exactly 0" % what
    ry = assert_within(gy, Sy, By, what + " y-gradient")
    return rx, ry


# ---------------------------------------------------------------- estimate_normals gradient in closed form (float64 numpy)

def normals_grad_closed_form(P, nbr, vp, gn, gc):
    """dL/dP of L = sum gn . n + sum gc curv on the given full neighbourhoods, without autograd, and entry by entry as the backward kernel
    scatters it: -> (c (m,k,3), grad (m,3)) with c[i,j] = (2/k) G_i d_ij the share of query i in the gradient of row nbr[i,j].

    q_j = p_j - p_i, d_j = q_j - mean q, C = (1/k) sum d_j d_j^T = V diag(w) V^T (ascending), n = s v0, curv = w0 / tr C.  First-order
    perturbation of a simple eigenvalue: dv0 = -(C - w0 I)^+ dC v0 = sum_{a>0} v_a (v_a^T dC v0) / (w0 - w_a), dw0 = v0^T dC v0, so
    G = dL/dC = sum_{a>0} (s gn . v_a) / (w0 - w_a) sym(v_a v0^T) + gc (v0 v0^T / tr - w0 I / tr^2); dL/dd_j = (2/k) G d_j, and because
    sum d_j = 0 the mean and the query's own -p_i terms cancel: row nbr[i,j] receives exactly c[i,j]."""
    P = np.asarray(P, np.float64)
    m, k = nbr.shape
    q = P[nbr] - P[:, None, :]
    d = q - q.mean(1, keepdims=True)
    C = np.einsum("mka,mkb->mab", d, d) / k
    w, V = np.linalg.eigh(C)
    v0 = V[:, :, 0]
    s = np.where(np.einsum("ma,ma->m", v0, np.asarray(vp, np.float64)[None, :] - P) < 0, -1.0, 1.0)
    tr = w.sum(1)
    G = gc[:, None, None] * (np.einsum("ma,mb->mab", v0, v0) / tr[:, None, None] - (w[:, 0] / tr ** 2)[:, None, None] * np.eye(3)[None])
    for a in (1, 2):
        va = V[:, :, a]
        coef = s * np.einsum("ma,ma->m", gn, va) / (w[:, 0] - w[:, a])
        M = np.einsum("ma,mb->mab", va, v0)
        G = G + coef[:, None, None] * 0.5 * (M + M.transpose(0, 2, 1))
    c = (2.0 / k) * np.einsum("mab,mkb->mka", G, d)
    grad = np.zeros((m, 3))
    for a in range(3):
        grad[:, a] = np.bincount(nbr.reshape(-1), weights=c[:, :, a].reshape(-1), minlength=m)
    return c, grad
