"""Constructions and a plain float64 model for the refine paths of the matrix-core search (csrc/knn_f16.hip).  numpy only: no GPU, no torch device.

EXACT CLOUDS.  Targets lie on the lattice 8 Z^3 in [-64, 64]^3, queries a multiple of 1/8 (at most 0.5 per axis) off a target, far rows and their queries on
integer coordinates around 2048: every product and partial sum of score() = fma(nx0, y0, fma(nx1, y1, fma(nx2, y2, h))), h = 0.5|y|^2, is then a float32
number (`analyse` checks it), so every search form has to return exactly the float64 answer: argmin 0.5|x - y|^2, lowest index among exact ties.  Exact
ties are planted on purpose: bit-identical copies of a row, and mirror rows c +- 8 e_k around a query at c (six equal scores at three different x).

THE MODEL restates, in float64,
  (a) knn_f16_scale_kernel's rule: the scale s, whether far rows are used, and which rows they are            -> scale_model
  (b) the candidate piece of a row: (r // 128, (r % 32) // 16) by index in the all-pairs form, (sp // 64, (sp % 32) // 16) by sorted position in the sweep
  (c) a query's class: U = certainly without a bound (exact scan), B = certainly bounded and clear, G = neither is certain                -> analyse
  (d) the two counters that follow: AGAIN (queries sent through the second filter pass) and SCAN (queries scored against every row)       -> predict
and `compare` is the one comparator both the GPU tests (kernel results) and the CPU tests (mutated models) go through.

Class B rests on two margins, both taken with a factor 2 to spare: f16_margin's acceptance 4E <= slack evaluated at the true distances holds as 8E <= slack,
and every image row outside the winner's tie set is further than 2^-8 (D_best + 0.5|x|^2) = twice slack >= 8E, while two candidate pieces of the filter
differ by at most 2E.  A query of class B whose tie set touches three or more pieces therefore has three filter minima inside the margin (each is within E
of the same exact score): it is `unsure`; one whose tie set touches one or two is settled from them.
"""
import numpy as np

U = 2.0 ** -24
FAR_MAX = 64
SCAN_MAX = 6
F16_RANGE = 60000.0
UNIT = 128                   # queries of a wave
NO_MUTATION = dict(half="ok", scan_max=SCAN_MAX, far_le=True, tie="index")


def _mut(mut):
    out = dict(NO_MUTATION)
    out.update(mut or {})
    return out


def is_f32(a):
    a = np.asarray(a, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return (a.astype(np.float32).astype(np.float64) == a) | ~np.isfinite(a)


def row_finite(y):
    """Rows whose stored 0.5|y|^2 is finite in float32 (the constructions keep clear of the boundary: values are below 2^13 or at 1e30)."""
    with np.errstate(over="ignore", invalid="ignore"):
        h = 0.5 * (y.astype(np.float64) ** 2).sum(1)
        return np.isfinite(y).all(1) & (h < 3.0e38)


# ------------------------------------------------------------------ (a) the scale kernel's rule
def scale_model(y, mut=None):
    """y (m,3) float32 values -> s, use_far, far (set of rows), image (mask of the rows the image holds), cnt, M2, Minf."""
    mut = _mut(mut)
    y = np.asarray(y, np.float32)
    m = len(y)
    fin = row_finite(y)
    with np.errstate(invalid="ignore"):
        rmax = np.where(fin, np.abs(y.astype(np.float64)).max(1), -1.0)
    Minf = max(0.0, float(rmax.max()))
    cut = Minf / 16.0
    bits = np.ascontiguousarray(y).view(np.uint32)
    rep = np.zeros(m, bool)
    rep[1:] = (bits[1:] == bits[:-1]).all(1)          # (the fourth word, 0.5|y|^2, is a function of the three)
    above = rmax > cut
    cnt = int((above & ~rep).sum())
    M2 = max(0.0, float(rmax[~above].max())) if (~above).any() else 0.0
    use_far = cnt > 0 and (cnt <= FAR_MAX if mut["far_le"] else cnt < FAR_MAX) and M2 > 0 and cnt * 64 <= m
    M = M2 if use_far else Minf
    s = 1.0
    if 0 < M < np.inf:
        s = 2.0 ** int(np.clip(11 - np.frexp(M)[1], -60, 60))
    far = frozenset(np.nonzero(above & ~rep)[0].tolist()) if use_far else frozenset()
    image = fin & ~(above if use_far else np.zeros(m, bool))
    return dict(s=s, use_far=use_far, far=far, nfar=len(far), image=image, finite=fin, cnt=cnt, M2=M2, Minf=Minf)


# ------------------------------------------------------------------ (b) pieces
def piece_ids(pos, form, mut=None):
    """pos: row index (all-pairs form) or sorted position (sweep)."""
    mut = _mut(mut)
    pos = np.asarray(pos)
    big = 128 if form == "brute" else 64
    half = (pos % 32) // 16 if mut["half"] == "ok" else (pos % 64) // 32
    return (pos // big) * 2 + half


def stand_in_tperm(y):
    """A stable sort by x (non-finite keys last): what the CPU tests use where the GPU tests read SweepIndex.tperm back."""
    key = np.asarray(y, np.float64)[:, 0].copy()
    key[~np.isfinite(key)] = np.inf
    return np.argsort(key, kind="stable")


def scored_queries(p, pose):
    """C p + r in float64: the point a search scores (the kernels hold nx = -(C p + r), query_point's fma chain; no pose = the identity's chain, in which
    an infinite coordinate meets the zeros of C: 0 * inf = NaN in every row, so a query with an infinite coordinate is scored as all-NaN by every form)."""
    p = np.asarray(p, np.float64)
    pose = np.concatenate((np.eye(3).reshape(9), np.zeros(3))) if pose is None else np.asarray(pose, np.float64)
    with np.errstate(invalid="ignore"):
        C = pose[:9].reshape(3, 3)
        return C[None, :, 0] * p[:, 0, None] + (C[None, :, 1] * p[:, 1, None] + (C[None, :, 2] * p[:, 2, None] + pose[None, 9:]))


# ------------------------------------------------------------------ the float64 oracle and (c) the classes
def analyse(y, X, sm):
    """y (m,3), X (n,3) scored queries, sm = scale_model(y) -> per query: idx (oracle), ties (list of arrays: ALL rows with the best distance), cls,
    img_ties (rows of the image with the image's best distance), exact (every intermediate of score() is a float32 number)."""
    y64 = np.asarray(y, np.float64)
    fin, img, s = sm["finite"], sm["image"], sm["s"]
    n, m = len(X), len(y64)
    fq = np.isfinite(X).all(1)
    Xf = np.where(fq[:, None], X, 0.0)
    yf = np.where(fin[:, None], y64, 0.0)
    D = np.zeros((n, m))
    for k in range(3):
        D += 0.5 * (Xf[:, k, None] - yf[None, :, k]) ** 2
    D[:, ~fin] = np.inf
    best = D.min(1)
    idx = np.where(np.isfinite(best), D.argmin(1), 0)
    tie_all = (D == best[:, None]) & np.isfinite(best)[:, None]
    # the chain itself, for exactness and for the non-finite queries (float32 arithmetic on non-finite values is the same in every format)
    h = 0.5 * (yf ** 2).sum(1)
    t1 = h[None] - Xf[:, 2, None] * yf[None, :, 2]
    t2 = t1 - Xf[:, 1, None] * yf[None, :, 1]
    t3 = t2 - Xf[:, 0, None] * yf[None, :, 0]
    ok = fin[None, :] & fq[:, None]
    exact = bool((is_f32(h) | ~fin).all() and (is_f32(t1) | ~ok).all() and (is_f32(t2) | ~ok).all() and (is_f32(t3) | ~ok).all()
                 and np.abs(np.where(ok, t3, 0.0)).max(initial=0.0) < 2.0 ** 24)
    for q in np.nonzero(~fq)[0]:
        with np.errstate(invalid="ignore", over="ignore"):
            y32 = np.asarray(y, np.float32)
            nx = (-X[q]).astype(np.float32)
            h32 = np.where(fin, h, np.inf).astype(np.float32)
            sc = nx[0] * y32[:, 0] + (nx[1] * y32[:, 1] + (nx[2] * y32[:, 2] + h32))
            lt = sc < np.inf
        idx[q] = int(np.nonzero(lt & (sc == sc[lt].min()))[0][0]) if lt.any() else 0
        tie_all[q] = False
    # classes, on the image's rows
    Di = np.where(img[None, :], D, np.inf)
    Db = Di.min(1)
    has = np.isfinite(Db)
    tie = (Di == Db[:, None]) & has[:, None]
    gap = np.where(tie, np.inf, Di).min(1) - np.where(has, Db, 0.0)
    hx = 0.5 * (Xf ** 2).sum(1)
    x1 = np.abs(Xf).sum(1)
    Dv = np.where(has, Db, 0.0)
    slack = 2.0 ** -9 * (Dv + hx)
    X2 = np.sqrt(2 * hx)
    Y = X2 + np.sqrt(2 * (Dv + slack))
    phi, hphi = U / s, 3 * 2.0 ** -12 / (s * s)
    E = (32 * U * (X2 * Y + 0.5 * Y * Y) + phi * (x1 + 1.7321 * Y) + hphi) * 1.01
    with np.errstate(invalid="ignore"):
        out = ~fq | (np.abs(Xf) * s > F16_RANGE * 1.01).any(1)
        inside = fq & (np.abs(Xf) * s <= F16_RANGE * 0.99).all(1)
    refused = inside & has & (Dv + hx > 0) & (2.0 ** -8 * (Dv + 2 * hx) < 4 * hphi)       # 4E >= 4 hphi > slack, whatever the filter's own error does to D0
    bounded = inside & has & (8 * E <= slack) & (gap > 2.0 ** -8 * (Dv + hx))
    cls = np.where(out | ~has | refused, "U", np.where(bounded, "B", "G"))
    ratio = np.where(has & (Dv + hx > 0), gap / np.maximum(2.0 ** -8 * (Dv + hx), 1e-300), np.inf)
    return dict(idx=idx.astype(np.int64), tie_all=tie_all, tie=tie, cls=cls, exact=exact, ratio=ratio, Dbest=best)


# ------------------------------------------------------------------ cases
class Case:
    """y (N,m,3) float32 targets, x (N,n,3) float32 queries as the search is handed them, pose (N,12) float32 or None, src_rows / tgt_rows (N) or None.
    branch: what the case is there for; reach: {form: predicate on that form's prediction} (form: "brute", "sweep" = the sweep with qorder None).
    grey: the case holds queries whose class is not certain (the counters are then only bounded)."""

    def __init__(self, name, y, x, branch, pose=None, src_rows=None, tgt_rows=None, reach=None, grey=False):
        self.name, self.branch, self.grey = name, branch, grey
        self.y = np.ascontiguousarray(np.asarray(y, np.float32) + np.float32(0))
        self.x = np.ascontiguousarray(np.asarray(x, np.float32))
        if self.y.ndim == 2:
            self.y, self.x = self.y[None], self.x[None]
        self.pose = None if pose is None else np.ascontiguousarray(np.asarray(pose, np.float32).reshape(-1, 12))
        self.src_rows = None if src_rows is None else np.asarray(src_rows, np.int32)
        self.tgt_rows = None if tgt_rows is None else np.asarray(tgt_rows, np.int32)
        self.reach = reach or {}
        self.N, self.m = self.y.shape[:2]
        self.n = self.x.shape[1]

    def rows(self, c):
        n = self.n if self.src_rows is None else int(min(max(self.src_rows[c], 0), self.n))
        m = self.m if self.tgt_rows is None else int(min(max(self.tgt_rows[c], 1), self.m))
        return n, m

    def __repr__(self):
        return self.name


def predict(case, form, tperm=None, qorder=None, mut=None):
    """(d): what one search of `case` must return and add to the counters.  form "brute" or "sweep"; the sweep needs tperm ((N, >= m): original row per
    sorted position; None = the stand-in) and takes the query order in use (qorder (N,n) or None = by index)."""
    mut = _mut(mut)
    N, n_full = case.N, case.n
    out = dict(idx=np.zeros((N, n_full), np.int64), valid=np.zeros((N, n_full), bool), s=np.zeros(N), nfar=np.zeros(N, np.int64), far=[], again=0, scan=0,
               grey=0, units=[], pieces=[], cls=[], exact=True, ratio=np.inf, unsure=[], tiles=[], tie_reversed=0)
    for c in range(N):
        n, m = case.rows(c)
        y = case.y[c, :m]
        X = scored_queries(case.x[c, :n], None if case.pose is None else case.pose[c])
        exact_pose = bool(is_f32(X).all())
        if form == "brute":
            pos = np.arange(m)
            sm = scale_model(y, mut)
        else:
            tp = stand_in_tperm(y) if tperm is None else np.asarray(tperm[c][:m], np.int64)
            assert sorted(tp.tolist()) == list(range(m)), "tperm is not a permutation of the cloud's rows"
            pos = np.empty(m, np.int64)
            pos[tp] = np.arange(m)
            sm = scale_model(y[tp], mut)                             # the sweep's image is made of the SORTED rows (the repeats rule looks at the row before)
            sm["far"] = frozenset(int(tp[r]) for r in sm["far"])
            sm["image"], sm["finite"] = sm["image"][pos], sm["finite"][pos]
        an = analyse(y, X, sm)
        pid = piece_ids(pos, form, mut)
        q, r = np.nonzero(an["tie"])
        npieces = np.zeros(n, np.int64)
        if len(q):
            pairs = np.unique(q * (int(pid.max()) + 1) + pid[r])
            npieces = np.bincount(pairs // (int(pid.max()) + 1), minlength=n)
        cls = an["cls"]
        unsure = (cls == "B") & (npieces >= 3)
        idx = an["idx"].copy()
        for qq in np.nonzero(an["tie_all"].sum(1) > 1)[0]:
            rows = np.nonzero(an["tie_all"][qq])[0]
            first = rows[np.argmin(pos[rows])]                       # the tie's first row in the sorted order
            out["tie_reversed"] += int(first != idx[qq])
            if mut["tie"] == "sorted" and form == "sweep":
                idx[qq] = first
        order = np.arange(n) if (qorder is None or form == "brute") else np.asarray(qorder[c][:n], np.int64)
        assert sorted(order.tolist()) == list(range(n)), "the query order is not a permutation of the cloud's queries"
        units = [int(unsure[order[u:u + UNIT]].sum()) for u in range(0, n, UNIT)]
        scan = int((cls == "U").sum())
        if form == "brute":
            again = int(unsure.sum())
        else:
            again = sum(t for t in units if t > mut["scan_max"])
            scan += sum(t for t in units if t <= mut["scan_max"])
        out["idx"][c, :n] = idx
        out["valid"][c, :n] = True
        out["s"][c], out["nfar"][c] = sm["s"], sm["nfar"]
        out["far"].append(sm["far"])
        out["again"] += again
        out["scan"] += scan
        out["grey"] += int((cls == "G").sum())
        out["units"].append(units)
        out["pieces"].append(npieces)
        out["cls"].append(cls)
        out["unsure"].append(unsure)
        out["tiles"].append(pos[idx] // 64)
        out["exact"] = out["exact"] and an["exact"] and exact_pose
        out["ratio"] = min(out["ratio"], float(an["ratio"][cls == "B"].min(initial=np.inf)))
    return out


def describe(pred):
    return "AGAIN %d SCAN %d grey %d | unsure per unit %s | s %s nfar %s" % (pred["again"], pred["scan"], pred["grey"], pred["units"], pred["s"].tolist(),
                                                                             pred["nfar"].tolist())


def compare(got, pred, what=""):
    """got: idx (N,n), s (N), nfar (N), far (list of sets), again, scan -- of one search -- against a prediction.  Exact, except that a query whose class
    is not certain (pred['grey'] of them) may have been counted once or not at all; the indices are exact always."""
    v = pred["valid"]
    bad = np.nonzero(np.asarray(got["idx"])[v] != pred["idx"][v])[0]
    assert len(bad) == 0, "%s: %d indices differ from the float64 oracle, first at flat position %d: %d instead of %d" % (
        what, len(bad), bad[0], np.asarray(got["idx"])[v][bad[0]], pred["idx"][v][bad[0]])
    assert np.array_equal(np.asarray(got["s"], np.float64), pred["s"]), "%s: scale %s instead of %s" % (what, got["s"], pred["s"])
    assert np.array_equal(np.asarray(got["nfar"]), pred["nfar"]), "%s: nfar %s instead of %s" % (what, got["nfar"], pred["nfar"])
    assert [frozenset(f) for f in got["far"]] == list(pred["far"]), "%s: far rows %s instead of %s" % (what, got["far"], pred["far"])
    if pred["grey"] == 0:
        assert (got["again"], got["scan"]) == (pred["again"], pred["scan"]), "%s: AGAIN, SCAN = %d, %d instead of %d, %d" % (
            what, got["again"], got["scan"], pred["again"], pred["scan"])
    else:
        extra = got["again"] + got["scan"] - pred["again"] - pred["scan"]
        assert got["again"] >= pred["again"] and got["scan"] >= pred["scan"] and 0 <= extra <= pred["grey"], "%s: AGAIN, SCAN = %d, %d with %d, %d certain and %d grey" % (
            what, got["again"], got["scan"], pred["again"], pred["scan"], pred["grey"])


def as_result(pred):
    """A prediction in the shape of a search's result (the CPU tests feed mutated models through `compare` this way)."""
    return dict(idx=pred["idx"], s=pred["s"], nfar=pred["nfar"], far=pred["far"], again=pred["again"], scan=pred["scan"])


# ------------------------------------------------------------------ constructions
_G = np.arange(-64.0, 65.0, 8.0)
_LATTICE = np.array(np.meshgrid(_G, _G, _G, indexing="ij")).reshape(3, -1).T
_LATTICE = _LATTICE[np.abs(_LATTICE).sum(1) > 0]            # (the origin only in the grey case: a query on it has D + 0.5|x|^2 = 0)
E3 = np.eye(3)


def pool(rng, count, xmax=64.0, exclude=(), x_only=None):
    """`count` distinct lattice points (never the origin), none of `exclude`."""
    P = _LATTICE[_LATTICE[:, 0] <= xmax]
    if x_only is not None:
        P = P[P[:, 0] == x_only]
    if len(exclude):
        ex = {tuple(e) for e in np.asarray(exclude, np.float64).reshape(-1, 3).tolist()}
        P = P[[tuple(p) not in ex for p in P.tolist()]]
    return P[rng.choice(len(P), count, replace=False)]


def near(rng, targets, n, maxoff=4):
    """n queries, each a multiple of 1/8 (at most maxoff / 8 per axis) off a random row of `targets`."""
    t = np.asarray(targets, np.float64)
    return t[rng.integers(0, len(t), n)] + rng.integers(-maxoff, maxoff + 1, (n, 3)) / 8.0


def place(fill, special, m):
    """m rows: special {index: point}, every other index from `fill` in order."""
    y = np.zeros((m, 3))
    free = np.ones(m, bool)
    for i, p in special.items():
        y[i] = p
        free[i] = False
    y[free] = fill[:int(free.sum())]
    return y


def quarter_turn(X, r):
    """(src, pose) with C src + r = X exactly: C a quarter turn about z, r an integer translation."""
    C = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    r = np.asarray(r, np.float64)
    return (np.asarray(X, np.float64) - r) @ C + 0.0, np.concatenate((C.reshape(9), r))


def mirror_rows(c, k=6):
    """The six (k = 6) or three (k = 3: left, middle, right in x) mirror rows around c, in ascending x."""
    c = np.asarray(c, np.float64)
    six = [c - 8 * E3[0], c - 8 * E3[1], c + 8 * E3[1], c - 8 * E3[2], c + 8 * E3[2], c + 8 * E3[0]]
    return six if k == 6 else [six[0], six[2], six[5]]


SIX = [5, 20, 130, 150, 260, 280]          # indices in six pieces of the all-pairs form: (chunk 0, half 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)
HUBS = [np.array(c, np.float64) for c in ((8, -24, 16), (-40, 32, -8), (32, 40, -48), (-16, -48, -32))]
M_BIG = 2304                               # ~135 rows per x: the mirror rows left and right of a hub are tiles apart in the sorted order


def _hub_exclude(hubs):
    return np.array([p for c in hubs for p in mirror_rows(c) + [c]])


def _index_order(k, order):
    """rank[i]: which of the k ascending indices the i-th row in ascending x gets.  asc: the sorted order is the original order; desc: its reverse;
    mid: a row in the middle of the sorted order has the lowest index."""
    if order == "asc":
        return list(range(k))
    if order == "desc":
        return list(range(k))[::-1]
    return [1, 0, 2] if k == 3 else [3, 0, 1, 2, 4, 5]


def _unsure(k):
    return lambda p: sum(int(u.sum()) for u in p["unsure"]) == k


def _pieces_max(k):
    return lambda p: max(int(x.max(initial=0)) for x in p["pieces"]) == k


def _both(*fs):
    return lambda p: all(f(p) for f in fs)


def copies_case(name, idxs, npieces, branch):
    rng = np.random.default_rng(7)
    T = np.array([24.0, -16.0, 40.0])
    y = place(pool(rng, M_BIG, exclude=[T]), {i: T for i in idxs}, M_BIG)
    x = near(rng, y[300:], 160)
    x[3:160:13] = T + rng.integers(-4, 5, (len(range(3, 160, 13)), 3)) / 8.0
    k = len(range(3, 160, 13))
    reach = {"brute": _both(_pieces_max(npieces), _unsure(k if npieces >= 3 else 0))}
    return Case(name, y, x, branch, reach=reach)


def mirror_case(name, k, order, branch):
    rng = np.random.default_rng(11)
    c = HUBS[0]
    rows = mirror_rows(c, k)
    rank = _index_order(k, order)
    where = SIX if k == 6 else SIX[:3]
    y = place(pool(rng, M_BIG, exclude=_hub_exclude([c])), {where[rank[i]]: rows[i] for i in range(k)}, M_BIG)
    x = near(rng, y[300:], 160)
    x[3:160:13] = c
    cnt = len(range(3, 160, 13))
    f = _both(_pieces_max(k) if k == 3 else (lambda p: max(int(v.max()) for v in p["pieces"]) >= 3), _unsure(cnt))
    return Case(name, y, x, branch, reach={"brute": f, "sweep": f})


def rounds_cloud(rng):
    special = {}
    for h, c in enumerate(HUBS):
        rows = mirror_rows(c)
        rank = _index_order(6, ("asc", "desc", "mid", "desc")[h])
        for i in range(6):
            special[SIX[rank[i]] + h] = rows[i]
    return place(pool(rng, M_BIG, exclude=_hub_exclude(HUBS)), special, M_BIG)


def rounds_case(name, waves, branch, posed=False, seed=13):
    """waves: (queries, unsure ones among them) per wave of 128 (the last one may be partial)."""
    rng = np.random.default_rng(seed)
    y = rounds_cloud(rng)
    xs, h = [], 0
    for size, uns in waves:
        w = near(rng, y[400:], size)
        for p in rng.choice(size, uns, replace=False):
            w[p] = HUBS[h % len(HUBS)]
            h += 1
        xs.append(w)
    x = np.concatenate(xs)
    want = [u for _, u in waves]
    reach = {"brute": lambda p: p["units"][0] == want and p["again"] == sum(want) and p["scan"] == 0,
             "sweep": lambda p: p["units"][0] == want and p["again"] == sum(u for u in want if u > SCAN_MAX) and p["scan"] == sum(u for u in want if u <= SCAN_MAX)}
    pose = None
    if posed:
        x, pose = quarter_turn(x, (3, -5, 7))
    return Case(name, y, x, branch, pose=pose, reach=reach)


def size_cases(m):
    rng = np.random.default_rng(1000 + m)
    y = pool(rng, m)
    x = near(rng, y, 513)
    clear = lambda p: p["again"] == 0 and p["scan"] == 0 and p["grey"] == 0
    out = []
    for n in (1, 31, 32, 33, 127, 128, 129, 511, 512, 513):
        xs, pose = x[:n], None
        if n == 129:
            xs, pose = quarter_turn(xs, (-2, 9, 4))
        out.append(Case("sizes m=%d n=%d" % (m, n), y, xs, "every query settled from one piece, at the edges of run / tile / chunk / stage / wave / block",
                        pose=pose, reach={"brute": clear, "sweep": clear}))
    return out


SIZES_M = (1, 16, 17, 32, 33, 64, 65, 127, 128, 129, 511, 512, 513, 1025)


def tgt_rows_case():
    rng = np.random.default_rng(21)
    counts, m_full, n = [1, 63, 64, 65], 200, 130
    ys, xs = [], []
    for cnt in counts:
        y = np.zeros((m_full, 3))
        y[:cnt] = pool(rng, cnt)
        x = near(rng, y[:cnt], n)
        junk = np.concatenate((x, x))[:m_full - cnt].copy()          # rows past the count: the queries themselves (distance 0), NaN, huge values
        junk[1::3] = np.nan
        junk[2::3] = 1e30
        y[cnt:] = junk
        ys.append(y)
        xs.append(x)
    clear = lambda p: p["again"] == 0 and p["scan"] == 0 and p["grey"] == 0
    return Case("tgt_rows 1, 63, 64, 65 of 200", np.array(ys), np.array(xs), "rows past the count (nearer points, NaN, 1e30) change neither the answer nor s",
                tgt_rows=counts, reach={"brute": clear, "sweep": clear})


def src_rows_case():
    rng = np.random.default_rng(22)
    counts, n_full, m = [1, 127, 129, 513], 600, 300
    ys, xs = [], []
    for cnt in counts:
        y = pool(rng, m)
        x = near(rng, y, n_full)
        x[cnt::2] = np.nan
        ys.append(y)
        xs.append(x)
    clear = lambda p: p["again"] == 0 and p["scan"] == 0 and p["grey"] == 0
    return Case("src_rows 1, 127, 129, 513 of 600", np.array(ys), np.array(xs), "queries past the count are never searched, their entries of idx stay untouched",
                src_rows=counts, reach={"brute": clear, "sweep": clear})


def scan_cases():
    out = []
    rng = np.random.default_rng(31)
    y = pool(rng, 300)
    x = near(rng, y, 200)
    big = list(range(2, 200, 17))
    for i, q in enumerate(big):
        x[q, i % 3] = 8192.0 * (1 if i % 2 else -1)
    x[5, 1] = np.nan
    x[6] = np.nan
    x[7, 0] = np.inf
    x[140, 2] = -np.inf
    k = len(big) + 4
    f = lambda p: p["scan"] == k and p["again"] == 0
    out.append(Case("queries beyond the f16 range, NaN and inf beside ordinary ones", y, x, "no bound -> exact scan, in waves that also hold settled queries",
                    reach={"brute": f, "sweep": f}))
    y = np.zeros((100, 3))
    y[0::3], y[1::3], y[2::3] = np.nan, np.inf, 1e30
    y[4] = (1.0, np.nan, 2.0)
    x = near(rng, pool(rng, 50), 140)
    f = lambda p: p["scan"] == 140 and p["again"] == 0 and int(np.abs(p["idx"]).max()) == 0
    out.append(Case("every target row non-finite", y, x, "nothing finite -> every query scanned, idx 0", reach={"brute": f, "sweep": f}))
    y = y.copy()
    y[37] = (16.0, -8.0, 24.0)
    x = near(rng, y[37:38], 140)
    x[9, 0] = 4096.0
    f = lambda p: p["scan"] == 1 and p["again"] == 0 and (p["idx"] == 37).all()
    out.append(Case("one finite target row", y, x, "the scale and every answer come from the one finite row", reach={"brute": f, "sweep": f}))
    return out


BEACON = np.array([64.0, 0.0, 0.0])         # the one image row at x = 64 of a far-row cloud (the others have x <= 48): the clear image winner of every query near x = 2048
FAR0 = np.array([2048.0, 0.0, 0.0])


def far_points(k):
    i = np.arange(k)
    return np.stack((np.full(k, 2048.0), 8.0 * (i % 17) - 64.0, 8.0 * (i // 17) - 32.0), 1)


def far_case(name, m, far_at, beacon_at, branch, use_far, s, far_pts=None, n=200, posed=False, seed=41):
    rng = np.random.default_rng(seed)
    if far_pts is None:
        far_pts = far_points(len(far_at))
        far_pts[0] = FAR0
    special = {int(i): p for i, p in zip(far_at, far_pts)}
    special[beacon_at] = BEACON
    y = place(pool(rng, m, xmax=48.0), special, m)
    x = near(rng, y[[i for i in range(m) if i not in special]], n)
    want4 = None
    if use_far:     # (without far rows the rows near x = 2048 are image rows 8 apart: no query near them is clear)
        fq = list(range(1, n, 9))
        x[fq] = near(rng, far_pts, len(fq))                          # queries inside the f16 range whose answer is a far row
        x[4] = 0.5 * (BEACON + FAR0)                                 # exact tie between the beacon and the far row at (2048, 0, 0)
        x[100] = 0.5 * (BEACON + FAR0)
        want4 = min(beacon_at, int(far_at[0]))
    f = lambda p: bool(p["nfar"][0] > 0) == use_far and p["s"][0] == s and p["again"] == 0 and p["scan"] == 0 and p["grey"] == 0 and (want4 is None or p["idx"][0, 4] == want4)
    pose = None
    if posed:
        x, pose = quarter_turn(x, (16, -3, 1))
    return Case(name, y, x, branch, pose=pose, reach={"brute": f, "sweep": f})


def far_cases():
    out = []
    m = 1324
    out.append(far_case("one far point 300 times", m, list(range(1024, 1324)), 50, "cnt = 1 by the repeats rule; far row wins queries near it; tie far / image, image index lower",
                        True, 16.0, far_pts=np.repeat(FAR0[None], 300, 0)))
    out.append(far_case("64 distinct far rows", 4096, 7 + 64 * np.arange(64), 50, "cnt = 64 = F16_FAR_MAX, cnt * 64 = m: far rows are used", True, 16.0, n=260))
    out.append(far_case("65 distinct far rows", 4160, 7 + 64 * np.arange(65), 50, "cnt = 65 > F16_FAR_MAX: no far rows, the scale covers them", False, 0.5, n=260))
    out.append(far_case("m = 128 with 2 far rows, one at index 0", 128, [0, 77], 50, "cnt * 64 = m; far row at index 0; tie far / image, far index lower", True, 16.0, posed=True))
    out.append(far_case("m = 128 with 3 far rows", 128, [0, 77, 90], 50, "cnt * 64 > m: no far rows", False, 0.5))
    rng = np.random.default_rng(47)
    y = np.zeros((128, 3))
    y[90] = FAR0
    x = rng.integers(-4, 5, (150, 3)) / 8.0
    x[np.abs(x).sum(1) == 0] = 0.125
    x[1::9] = near(rng, FAR0[None], len(range(1, 150, 9)))
    k = 150 - len(range(1, 150, 9))
    f = lambda p: p["nfar"][0] == 0 and p["s"][0] == 0.5 and p["scan"] == k and p["again"] == 0
    out.append(Case("every non-far row at the origin", y, x, "M2 = 0: no far rows; the margin refuses the queries at the origin's rows (4E > slack): scanned",
                    reach={"brute": f, "sweep": f}))
    return out


def sweep_cases():
    out = []
    rng = np.random.default_rng(51)
    y = pool(rng, M_BIG)
    x = near(rng, y, 512)

    def spread(p):      # winners more than the row cache's four tiles from the tile of the unit's middle query
        t = p["tiles"][0]
        return p["again"] == 0 and p["scan"] == 0 and all(np.abs(t[u:u + UNIT] - t[min(u + 64, len(t) - 1)]).max() >= 8 for u in range(0, len(t), UNIT))
    out.append(Case("queries in random x order", y, x, "qorder None: the winners' tiles lie outside the wave's row cache (far_run gather)", reach={"sweep": spread}))
    clear = lambda p: p["again"] == 0 and p["scan"] == 0 and p["grey"] == 0
    for side, sign in (("left", -1.0), ("right", 1.0)):
        edge = y[y[:, 0] == 64.0 * sign]
        x = near(rng, edge, 256)
        x[:, 0] += 2.0 * sign
        out.append(Case("every query %s of all targets" % side, y, x, "the sweep starts at the first / last tile and runs one way", reach={"sweep": clear}))
    y = pool(rng, 280, x_only=8.0)
    out.append(Case("all targets on one x", y, near(rng, y, 200), "no side of the sweep ever ends by x", reach={"sweep": clear, "brute": clear}))
    return out


def tie_loop_case():
    """Two equal scores NEXT to each other in the sorted order, in one 16-row run, whose original order is the reverse: targets on the planes x = 0 and x = 16
    only, the query on x = 8 between the rows L = c - 8 e_x and R = c + 8 e_x.  L has the highest index of its plane and R the lowest of its own, so a sort
    that keeps equal keys in index order puts them at positions 132 and 133; whatever the sort does, the prediction is made from the order read back."""
    rng = np.random.default_rng(71)
    c = np.array([8.0, -24.0, 16.0])
    L, R = c - 8 * E3[0], c + 8 * E3[0]
    left, right = pool(rng, 132, x_only=0.0, exclude=[L]), pool(rng, 139, x_only=16.0, exclude=[R])
    y = np.concatenate((left[:100], R[None], left[100:], right[:67], L[None], right[67:]))          # R at index 100, L at index 200
    assert len(y) == 273 and (y[200] == L).all() and (y[:200, 0] == 0).sum() == 132
    x = near(rng, np.delete(y, [100, 200], 0), 150)
    x[3:150:13] = c
    k = len(range(3, 150, 13))

    def f(p):
        q = np.nonzero(np.isin(np.arange(150), np.arange(3, 150, 13)))[0]
        return p["again"] == 0 and p["scan"] == 0 and (p["pieces"][0][q] == 1).all() and (p["idx"][0, q] == 100).all() and p["tie_reversed"] >= k
    return Case("two equal scores side by side in one run, sorted order the reverse of the original", y, x,
                "sweep: the `ties` loop over a lane's own rows decides by the lowest ORIGINAL index", reach={"sweep": f})


def grey_case():
    rng = np.random.default_rng(61)
    y = place(pool(rng, 300), {17: np.zeros(3)}, 300)
    x = near(rng, np.delete(y, 17, 0), 150)
    x[3:150:31] = 0.0
    k = len(range(3, 150, 31))
    f = lambda p: p["grey"] == k and p["again"] == 0 and p["scan"] == 0
    return Case("queries on a target at the origin", y, x, "D0 + 0.5|x|^2 = 0: the margin refuses; only the indices and 'counted at most once' are held",
                reach={"brute": f, "sweep": f}, grey=True)


def cases():
    out = []
    out += [copies_case("copies in one 16-row run", [3, 9], 1, "tie set in one piece"),
            copies_case("copies in two pieces of one chunk, lowest index in half 0", [5, 20], 2, "two candidate pieces, one chunk"),
            copies_case("copies in two pieces of one chunk, lowest index in half 1", [40, 20], 2, "two candidate pieces, one chunk"),
            copies_case("copies in two chunks, lowest index in half 0", [5, 130], 2, "two candidate pieces, two chunks"),
            copies_case("copies in two chunks, lowest index in half 1", [20, 130], 2, "two candidate pieces, two chunks"),
            copies_case("copies in two pieces that the wrong half would call three", [5, 40, 130], 2, "two candidate pieces; rows 5 and 40 share (chunk 0, half 0)"),
            copies_case("copies in three pieces, lowest index in half 0", [5, 20, 130], 3, "three candidate pieces -> pass 2"),
            copies_case("copies in three pieces, lowest index in half 1", [40, 20, 130], 3, "three candidate pieces -> pass 2"),
            copies_case("copies in six pieces, lowest index in half 0", SIX, 6, "six candidate pieces -> pass 2"),
            copies_case("copies in six pieces, lowest index in half 1", [40] + SIX[1:], 6, "six candidate pieces -> pass 2")]
    for k in (3, 6):
        for order, where in (("asc", "first"), ("mid", "a middle"), ("desc", "last")):
            out.append(mirror_case("mirror ties in %d pieces, lowest index in the %s piece of the sorted order" % (k, where), k, order,
                                   "%d equal scores at three x: pass 2 / scan, tie loop by ORIGINAL index" % k))
    out += [rounds_case("unsure queries per wave 1, 6, 7, 32", [(128, 1), (128, 6), (128, 7), (128, 32)], "sweep: tot <= F16_SCAN_MAX at 6 and at 7; one full round of pass 2"),
            rounds_case("unsure queries per wave 0, 33, 128, 5", [(128, 0), (128, 33), (128, 128), (128, 5)],
                        "rounds 2..4 of pass 2 (rank - 32 rd, qslot scatter-back), waves of one block with 0, 2, 4 and 1 rounds under s_rounds", posed=True),
            rounds_case("two blocks, partial last wave with 40 unsure of 70", [(128, 65), (128, 0), (128, 3), (128, 96), (128, 33), (70, 40)],
                        "a second round in a partial last wave; a second block with fewer waves", seed=14)]
    out += scan_cases() + far_cases() + sweep_cases() + [tie_loop_case(), tgt_rows_case(), src_rows_case(), grey_case()]
    return out


MUTATIONS = {
    "pieces computed with the wrong half": dict(half="wrong"),
    "F16_SCAN_MAX taken as 5": dict(scan_max=5),
    "F16_SCAN_MAX taken as 7": dict(scan_max=7),
    "use_far with cnt < 64": dict(far_le=False),
    "tie rule by sorted position": dict(tie="sorted"),
}
