"""Shared by the tests of the ICP loop's windowed backward (csrc/kernels_backward.h: accumulate_bwd_window_kernel / window_body,
window_reduce_kernel, permute_rows): a numpy model of the window geometry, the seeded match layouts that reach each branch of those kernels, the
conditions that prove they do, a pool of reference points the layouts draw their values from, and a numpy emulation of the pass.

The model repeats the kernels' expressions (window_slots, window_origin, hi = min(lo + WT, m_pad), dicp_padded_targets, the MAXB-block pass and
the 32-window round of the reduce).  It is only used to PROVE that a layout reaches the code it is meant for; it is never the expected value of
anything.  tests/test_icp_window_layouts.py holds its constants and expressions to the sources and its block counts to the library's own host
functions.  The expected values are the float64 per-point terms of tests/point_math_ref.py, summed per target row.

A layout is int arrays only: per cloud (n, m, src_rows, qorder, tperm, spos_ref, spos_A, spos_B).  spos_* are indexed by QUERY, as the kernels read
them; slot s of a cloud holds query qorder[s]; tperm[r] is the original row of sorted row r, the pad rows last (as SweepIndex leaves them).  The
per-point terms depend only on the values (p, y, normal, pose, weight, cotangent), not on where a row sits, so every query and every target row
draws its values from a small pool (`Pool`): the reference is evaluated once on the pool's (source, target) pairs and a slot's term is looked up.

A plain module (no fixtures): the tests put this directory on sys.path and import it.
"""
import numpy as np
import torch

import point_math_ref as R

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
BLOCK = 256                     # csrc/dicp_common.h
KNN_PAD = 64                    # csrc/dicp_common.h: m_pad granularity
WT = {F32: 1536, F64: 768}      # WindowRows<float>, WindowRows<double>
MAXB = 256                      # window_reduce_kernel: window blocks per cloud handled per pass
ROUND = 32                      # window_reduce_kernel: covering windows per round (the 32-bit cover masks)
WR_U = 4                        # window_reduce_kernel: gradient elements per thread
SPB_MAX = 4 * BLOCK             # window_body: SPB


def np_dtype(dtype):
    return R.np_dtype(dtype)


# ---------------------------------------------------------------- the model of the window geometry
def padded_targets(m):
    """dicp_padded_targets"""
    return 0 if m <= 0 else (m + KNN_PAD - 1) // KNN_PAD * KNN_PAD


def window_slots(wt, n, m_pad):
    """window_slots (integer division of non-negative values, as C)"""
    s = (wt - wt // 3) * n // (m_pad if m_pad > 0 else 1)
    s = s // BLOCK * BLOCK
    return BLOCK if s < BLOCK else (4 * BLOCK if s > 4 * BLOCK else s)


def window_blocks(dtype, n, m_pad):
    """dicp_window_blocks"""
    if n <= 0 or m_pad <= 0:
        return 0
    spb = window_slots(WT[np_dtype(dtype)], n, m_pad)
    return (n + spb - 1) // spb


def window_origin(sp_ref_c, qo_c, blk, spb, nc, m_pad, wt):
    """window_origin: sp_ref_c indexed by query, qo_c (slot -> query) or None, nc the cloud's own slots"""
    if m_pad <= wt or nc <= 0:
        return 0
    mid = min(blk * spb + spb // 2, nc - 1)
    q = min(max(int(qo_c[mid]), 0), nc - 1) if qo_c is not None else mid
    ctr = max(int(sp_ref_c[q]), 0)
    return min(max(ctr - wt // 2, 0), m_pad - wt) & ~15


class Geometry:
    """What the model says of one cloud under one set of matches (all per SLOT / per SORTED row):
    spb, bpc, lo (bpc,), hi (bpc,); row (n,) the clamped match of each slot, live (n,), blk (n,), inwin (n,) (False on dead slots), far (n,);
    indegree (m_pad,), cover (m_pad,) windows whose [lo, lo + WT) holds the row, live_cover (m_pad,) those with a live in-window contribution"""


def geometry(dtype, n, m, nc, qorder, spos_ref, spos):
    wt = WT[np_dtype(dtype)]
    m_pad = padded_targets(m)
    g = Geometry()
    g.wt, g.n, g.m, g.m_pad, g.nc = wt, n, m, m_pad, nc
    g.spb = window_slots(wt, n, m_pad)
    g.bpc = (n + g.spb - 1) // g.spb
    g.lo = np.array([window_origin(spos_ref, qorder, b, g.spb, nc, m_pad, wt) for b in range(g.bpc)], dtype=np.int64)
    g.hi = np.minimum(g.lo + wt, m_pad)
    mid = [min(b * g.spb + g.spb // 2, nc - 1) for b in range(g.bpc)] if nc > 0 else []
    g.raw = np.array([int(spos_ref[qorder[s] if qorder is not None else s]) - wt // 2 for s in mid], dtype=np.int64)      # before the clamps
    s = np.arange(n)
    q = np.clip(qorder, 0, n - 1) if qorder is not None else s
    g.live = s < nc
    g.blk = s // g.spb
    g.row = np.clip(spos[q].astype(np.int64), 0, m_pad - 1)            # -1 (no neighbour) -> sorted row 0
    g.inwin = g.live & (g.row >= g.lo[g.blk]) & (g.row < g.hi[g.blk])
    g.far = g.live & ~g.inwin
    g.indegree = np.bincount(g.row[g.live], minlength=m_pad)
    d = np.zeros(m_pad + 1, dtype=np.int64)                             # the reduce holds a row against lo <= r < lo + WT
    np.add.at(d, g.lo, 1)
    np.add.at(d, np.minimum(g.lo + wt, m_pad), -1)
    g.cover = np.cumsum(d)[:m_pad]
    pairs = np.unique(np.stack((g.row[g.inwin], g.blk[g.inwin]), 1), axis=0) if g.inwin.any() else np.zeros((0, 2), dtype=np.int64)
    g.live_cover = np.bincount(pairs[:, 0], minlength=m_pad)
    return g


# ---------------------------------------------------------------- the layouts
class Layout:
    """name, n, m, clouds: [(n, m, src_rows, qorder, tperm, spos_ref, spos_A, spos_B)], alive (N,), planted: whatever the conditions name"""

    def __init__(self, name, n, m, clouds, alive=None, planted=None):
        self.name, self.n, self.m, self.clouds = name, n, m, clouds
        self.N = len(clouds)
        self.alive = np.ones(self.N) if alive is None else np.asarray(alive, dtype=np.float64)
        self.planted = planted or {}
        self.m_pad = padded_targets(m)

    def stack(self, k):
        """field k of every cloud as one (N, ...) int32 array"""
        return np.stack([np.asarray(c[k]) for c in self.clouds]).astype(np.int32)

    src_rows = property(lambda self: np.array([c[2] for c in self.clouds], dtype=np.int32))

    def geometry(self, dtype, b, which):
        c = self.clouds[b]
        return geometry(dtype, c[0], c[1], c[2], c[3], c[5], c[6] if which == "A" else c[7])


def _tperm(rng, m):
    m_pad = padded_targets(m)
    return np.concatenate((rng.permutation(m), m + rng.permutation(m_pad - m))).astype(np.int32)


def _qorder(rng, n, nc=None, identity=False):
    """a cloud's own queries in a random slot order, its pad queries last"""
    nc = n if nc is None else nc
    if identity:
        return np.arange(n, dtype=np.int32)
    return np.concatenate((rng.permutation(nc), nc + rng.permutation(n - nc))).astype(np.int32)


def _by_query(qorder, by_slot):
    out = np.empty_like(by_slot)
    out[qorder] = by_slot
    return out


def _diag(rng, n, m, jitter=300):
    """per slot: a match within +-jitter of the diagonal"""
    ctr = (np.arange(n) * (m / n)).astype(np.int64)
    return np.clip(ctr + rng.integers(-jitter, jitter + 1, n), 0, m - 1)


def _rematch(rng, spos_slot, m, nc):
    """the second set of matches: a fifth of the live slots re-matched anywhere in the cloud (some of them out of their window)"""
    out = spos_slot.copy()
    if nc > 0:
        pick = rng.permutation(nc)[:max(nc // 5, 1)]
        out[pick] = rng.integers(0, m, len(pick))
    return out


def _cloud(rng, n, m, nc, ref_slot, a_slot, identity=False, b_slot=None):
    qo = _qorder(rng, n, nc, identity)
    b_slot = _rematch(rng, np.where(a_slot < 0, 0, a_slot), m, nc) if b_slot is None else b_slot
    f = lambda v: _by_query(qo, np.asarray(v).astype(np.int32))
    return (n, m, nc, qo, _tperm(rng, m), f(ref_slot), f(a_slot), f(b_slot))


def _slot_geometry(dtype, n, m, nc, ref_slot):
    """lo, hi, spb of a cloud whose reference matches are given per slot (identity order: the origins depend on the matches of the middle slots only)"""
    g = geometry(dtype, n, m, nc, None, ref_slot, ref_slot)
    return g.lo, g.hi, g.spb, g.bpc


def diagonal(dtype, seed=1, identity=False, N=2):
    n = m = 5000
    rng = np.random.default_rng(seed)
    clouds = []
    for b in range(N):
        a = _diag(rng, n, m)
        a[::97] = rng.integers(0, m, len(range(0, n, 97)))
        _, _, spb, _ = _slot_geometry(dtype, n, m, n, a)
        keep = np.arange(n) % spb == spb // 2
        a[keep] = _diag(rng, n, m, 0)[keep]                          # (the middle slots place the windows: they stay on the diagonal)
        ref = a.copy()
        if b == 0:
            a[5] = -1                                               # "no neighbour" -> sorted row 0
        clouds.append(_cloud(rng, n, m, n, ref, a, identity))
    return Layout("diagonal", n, m, clouds)


def edges(dtype, seed=2):
    """planted[(cloud, where)] = {kind: slot}: in block 0 (origin clamped to 0), an interior block and the last block (origin clamped to m_pad - WT),
    slots matched exactly to lo - 1, lo, hi - 1, hi of the block's window, to row 0 and to row m - 1 (m = m_pad here: hi - 1 of the last window IS row
    m - 1, and no row hi exists there, as no row lo - 1 exists in block 0)"""
    n, m = 5000, 5056
    rng = np.random.default_rng(seed)
    clouds, planted = [], {}
    for b in range(2):
        a = _diag(rng, n, m, 100)
        lo, hi, spb, bpc = _slot_geometry(dtype, n, m, n, a)
        for where, blk in (("first", 0), ("interior", bpc // 2), ("last", bpc - 1)):
            rows = {"lo-1": lo[blk] - 1, "lo": lo[blk], "hi-1": hi[blk] - 1, "hi": hi[blk], "row0": 0, "rowm-1": m - 1}
            s0, s1 = blk * spb, min(n, (blk + 1) * spb)
            free = [s for s in range(s0, s1) if s != min(s0 + spb // 2, n - 1)]
            slots = rng.permutation(free)[:len(rows)]
            planted[(b, where)] = {}
            for (kind, row), s in zip(rows.items(), slots):
                if 0 <= row < m:
                    a[s] = row
                    planted[(b, where)][kind] = (int(s), int(row))
        clouds.append(_cloud(rng, n, m, n, a, a))
    return Layout("edges", n, m, clouds, planted=planted)


def block_hub(dtype, spb, seed=3):
    """every slot of one block matches one row; no other slot does"""
    n, m = {256: (2000, 8000), 1024: (4096, 2000)}[spb]
    rng = np.random.default_rng(seed + spb)
    clouds, planted = [], {}
    for b in range(2):
        a = _diag(rng, n, m)
        lo, hi, got, bpc = _slot_geometry(dtype, n, m, n, a)
        assert got == spb, (got, spb)
        blk = 1 + b
        hub = int(a[blk * spb + spb // 2])
        a[a == hub] = hub + 1
        a[blk * spb:(blk + 1) * spb] = hub
        planted[b] = (blk, hub)
        clouds.append(_cloud(rng, n, m, n, a, a))
    return Layout("block_hub_%d" % spb, n, m, clouds, planted=planted)


def covered_34(dtype, seed=4):
    """34 windows with (almost) one origin: every reference match in [r0, r0 + 64); matches spread over [r0 - WT/2, r0 + WT/2); the first slot of EVERY block
    matches the rows planted['hubs'], so those rows receive a live contribution from each of the 34 windows"""
    n, m, r0 = 8449, 17000, 8192
    wt = WT[np_dtype(dtype)]
    rng = np.random.default_rng(seed)
    ref = r0 + rng.integers(0, 64, n)
    a = r0 + rng.integers(-wt // 2, wt // 2, n)
    lo, hi, spb, bpc = _slot_geometry(dtype, n, m, n, ref)
    hubs = [r0, r0 + 37]
    first = np.arange(bpc) * spb
    a[first] = hubs[0]
    a[first[:-1] + 1] = hubs[1]
    b_slot = _rematch(rng, a, m, n)
    b_slot[first] = hubs[1]                                         # (the last block's only slot reaches both rows over the two launches)
    return Layout("covered_34", n, m, [_cloud(rng, n, m, n, ref, a, b_slot=b_slot)], planted={"hubs": hubs})


def blocks_257(dtype, seed=5):
    n, m = 65537, 131200
    rng = np.random.default_rng(seed)
    a = _diag(rng, n, m)
    return Layout("blocks_257", n, m, [_cloud(rng, n, m, n, a, a)])


def all_far(dtype, seed=6):
    """every window at row 0 (reference matches in [0, 64)), matches uniform over a cloud of m >> WT rows, and 500 slots of all blocks on ONE far row"""
    n, m, hub = 3000, 20000, 15001
    rng = np.random.default_rng(seed)
    clouds = []
    for b in range(2):
        ref = rng.integers(0, 64, n)
        a = rng.integers(0, m, n)
        a[a == hub] = hub - 1
        a[rng.permutation(n)[:500]] = hub
        clouds.append(_cloud(rng, n, m, n, ref, a))
    return Layout("all_far", n, m, clouds, planted={"hub": hub})


def small_target(dtype, n, m, seed=7):
    rng = np.random.default_rng(seed + n)
    clouds = []
    for b in range(2):
        a = rng.integers(0, m, n)
        clouds.append(_cloud(rng, n, m, n, a, a))
    return Layout("small_target_%d" % m, n, m, clouds)


def ragged(dtype, seed=8):
    """src_rows = [n, n - 1, spb, spb + 1, 1, 0] and a seventh cloud that is not alive"""
    n, m = 1000, 2000
    spb = window_slots(WT[np_dtype(dtype)], n, padded_targets(m))
    rng = np.random.default_rng(seed)
    clouds = []
    for nc in (n, n - 1, spb, spb + 1, 1, 0, n):
        a = _diag(rng, n, m, 200)
        a[::53] = rng.integers(0, m, len(range(0, n, 53)))
        a[nc:] = -1                                                 # (a cloud's pad queries have no match)
        clouds.append(_cloud(rng, n, m, nc, a, a))
    return Layout("ragged", n, m, clouds, alive=[1, 1, 1, 1, 1, 1, 0])


LAYOUTS = {
    "diagonal": diagonal, "edges": edges, "block_hub_256": lambda dt: block_hub(dt, 256), "block_hub_1024": lambda dt: block_hub(dt, 1024),
    "covered_34": covered_34, "blocks_257": blocks_257, "all_far": all_far, "small_target_70": lambda dt: small_target(dt, 300, 70),
    "small_target_1": lambda dt: small_target(dt, 1, 1), "ragged": ragged,
}
_BUILT = {}


def layout(name, dtype):
    """the layout (built once per dtype: the arrays are never written to)"""
    key = (name, np_dtype(dtype).name)
    if key not in _BUILT:
        _BUILT[key] = LAYOUTS[name](np_dtype(dtype))
    return _BUILT[key]


def check_conditions(lay, dtype):
    """The fixed conditions under which a layout is a test of the code it is meant for (asserted on the model alone, before any GPU result is read).
    -> a line of figures for the log"""
    dt = np_dtype(dtype)
    wt, name = WT[dt], lay.name
    G = [(lay.geometry(dt, b, "A"), lay.geometry(dt, b, "B")) for b in range(lay.N)]
    for c, (ga, gb) in zip(lay.clouds, G):
        n, m, nc, qo, tperm = c[:5]
        assert ga.spb <= SPB_MAX and ga.bpc == window_blocks(dt, n, lay.m_pad)
        assert np.array_equal(np.sort(qo), np.arange(n)) and np.array_equal(np.sort(tperm), np.arange(lay.m_pad)) and (tperm[:m] < m).all()
        assert (ga.lo == gb.lo).all(), "both launches add into one slab: the same origins"
        for k in (5, 6, 7):
            assert c[k].min() >= -1 and c[k].max() < m, "pad rows are never matched"
    ga = G[0][0]
    live = sum(int(g.live.sum()) for g, _ in G)
    far = sum(int(g.far.sum()) for g, _ in G)
    inw = sum(int(g.inwin.sum()) for g, _ in G)
    if name == "diagonal":
        assert lay.m_pad > wt and ga.bpc > 1
        assert inw >= 0.9 * live and far >= 10
        assert (lay.clouds[0][6] == -1).sum() == 1
    elif name == "edges":
        assert lay.m_pad > wt and lay.m == lay.m_pad
        for (b, where), slots in lay.planted.items():
            g = G[b][0]
            blk = {"first": 0, "interior": g.bpc // 2, "last": g.bpc - 1}[where]
            lo, hi = int(g.lo[blk]), int(g.hi[blk])
            if where == "first":
                assert lo == 0 and g.raw[blk] < 0 and "lo-1" not in slots
            if where == "last":
                assert lo == (lay.m_pad - wt) & ~15 and hi == lay.m_pad and "hi" not in slots
                assert g.raw[blk] > lay.m_pad - wt, "the clamp must act"
            if where == "interior":
                assert 0 < lo < (lay.m_pad - wt) & ~15 and sorted(slots) == sorted(("lo-1", "lo", "hi-1", "hi", "row0", "rowm-1"))
            want = {"lo-1": (lo - 1, False), "lo": (lo, True), "hi-1": (hi - 1, True), "hi": (hi, False),
                    "row0": (0, lo == 0), "rowm-1": (lay.m - 1, hi == lay.m_pad)}
            for kind, (s, row) in slots.items():
                assert g.blk[s] == blk and g.row[s] == row == want[kind][0] and bool(g.inwin[s]) == want[kind][1] and bool(g.far[s]) != want[kind][1], (where, kind)
    elif name.startswith("block_hub"):
        spb = int(name.rsplit("_", 1)[1])
        for b, (blk, hub) in lay.planted.items():
            g = G[b][0]
            assert g.spb == spb and g.indegree[hub] == spb and (g.row[g.blk == blk] == hub).all() and g.inwin[g.blk == blk].all()
        if spb == 4 * BLOCK:
            assert lay.n >= lay.m_pad
    elif name == "covered_34":
        ga, gb = G[0]
        assert ga.spb == BLOCK and ga.bpc == 34 and ga.lo.max() - ga.lo.min() <= 64
        assert ga.cover.max() == 34 > ROUND
        both = np.maximum(ga.live_cover, gb.live_cover)
        for hub in lay.planted["hubs"]:
            assert both[hub] >= 33 and ga.cover[hub] == 34, (hub, both[hub])
        last = ga.bpc - 1                                           # the windows past the 32nd of the list carry live contributions
        assert ga.inwin[ga.blk >= ROUND].any() and ga.inwin[ga.blk == last].all()
    elif name == "blocks_257":
        assert lay.N == 1 and ga.spb == BLOCK and ga.bpc >= 257 > MAXB
        assert ga.inwin[ga.blk == 256].any() and ga.live[ga.blk == 256].sum() == 1
    elif name == "all_far":
        assert lay.m_pad > 8 * wt and far >= 0.9 * live
        for g, _ in G:
            hub = lay.planted["hub"]
            assert (g.lo == 0).all() and g.indegree[hub] >= 500 and not g.inwin[g.row == hub].any() and len(np.unique(g.blk[g.row == hub])) == g.bpc
    elif name.startswith("small_target"):
        assert lay.m_pad <= wt
        for g, _ in G:
            assert g.bpc == (lay.n + g.spb - 1) // g.spb and (g.lo == 0).all() and (g.hi == lay.m_pad).all() and far == 0
    elif name == "ragged":
        spb = ga.spb
        rows = [int(c[2]) for c in lay.clouds]
        assert rows == [lay.n, lay.n - 1, spb, spb + 1, 1, 0, lay.n] and lay.alive.tolist() == [1, 1, 1, 1, 1, 1, 0]
        assert lay.n > spb + 1 and ga.bpc >= 2
        assert any(r % spb for r in rows if r) and any(r and r % spb == 0 and r < lay.n for r in rows) and 0 in rows
    else:
        raise KeyError(name)
    return "%s %s: spb %d, bpc %d, live %d, in window %d, far %d, max in-degree %d, max cover %d" % (
        name, dt.name, ga.spb, ga.bpc, live, inw, far, max(int(g.indegree.max()) for g, _ in G), max(int(g.cover.max()) for g, _ in G))


# ---------------------------------------------------------------- the values: a pool of reference points
P_SRC, P_TGT = 31, 37           # source / target values per cloud: every (source, target) pair is a reference point


def window_config(key):
    """the (mode, c, loss, differentiable, trim) tuples of point_math_ref._SUM_CFG"""
    return R.sum_config(key)


class Pool:
    """N poses and cotangents; per pose P_SRC source points (with weights) and P_TGT target rows (shared by the poses) such that EVERY pair is a
    well-conditioned reference point: the targets lie in a ball of radius 0.25, the transformed sources 0.5 .. 1.9 from its centre, so residuals are
    0.25 .. 2.15 (on both sides of the metric 1.0 and of the trim distance 2.0, below point_math_ref.residual_limit).  The float64 reference and its
    bound are evaluated once on the N x P_SRC x P_TGT pairs; it must pass check_case (no tie, weights inside the model's linear region) -- the seed
    is the first one whose reference does, decided on the reference alone."""

    def __init__(self, dtype, cfg, N, alive, unit_w=False, seeds=range(1, 9)):
        self.dt, self.cfg, self.N = np_dtype(dtype), cfg, N
        self.ar = R.Arith(self.dt, "device")
        assert R.residual_limit(cfg) >= 2.2
        err = None
        for seed in seeds:
            self._draw(seed, alive, unit_w)
            try:
                self.ref = R.reference(self.ar, cfg, self.inp, self.cot, allow_ties=False)
                R.check_case(self.ref, self.inp["p"].shape[0], [])
                self.seed = seed
                return
            except AssertionError as e:
                err = e
        raise AssertionError("no seed without a tie: %s" % err)

    def _draw(self, seed, alive, unit_w):
        dt, N = self.dt, self.N
        rng = np.random.default_rng(1000 * seed + N)
        f = lambda a: np.asarray(a).astype(dt).astype(np.float64)
        C, r = f(R.rotations(N, rng)), f(rng.uniform(-0.5, 0.5, (N, 3)))
        c0 = rng.uniform(-2, 2, 3)
        d = rng.normal(size=(P_TGT, 3))
        Y = f(c0 + 0.25 * d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0, 1, (P_TGT, 1)))
        nr = rng.normal(size=(P_TGT, 3))
        nr = f(nr / np.linalg.norm(nr, axis=1, keepdims=True))
        d = rng.normal(size=(N, P_SRC, 3))
        q = c0 + d / np.linalg.norm(d, axis=2, keepdims=True) * rng.uniform(0.5, 1.9, (N, P_SRC, 1))
        p = f(np.einsum("bji,bnj->bni", C, q - r[:, None, :]))            # C^T (q - r)
        w = f(np.ones((N, P_SRC)) if unit_w else rng.uniform(0.5, 1.0, (N, P_SRC)))
        Gs, gb = R.random_cotangents(N, dt, 11 + seed)
        self.C, self.r, self.Y, self.nrm, self.p, self.w, self.Gs, self.gb = C, r, Y, nr, p, w, Gs.numpy(), gb.numpy()
        self.alive = np.asarray(alive, dtype=np.float64)
        b, a, t = np.meshgrid(np.arange(N), np.arange(P_SRC), np.arange(P_TGT), indexing="ij")
        b, a, t = b.ravel(), a.ravel(), t.ravel()
        T = torch.tensor
        self.inp = dict(p=T(p[b, a]), y=T(Y[t]), nrm=T(nr[t]), C=T(C[b]), r=T(r[b]), w_init=T(w[b, a]), alive=T(self.alive[b]))
        self.cot = (Gs[torch.as_tensor(b)], gb[torch.as_tensor(b)])

    def pair(self, b, a, t):
        """index of pair (cloud, source value, target value) in the reference's arrays"""
        return (np.asarray(b) * P_SRC + np.asarray(a)) * P_TGT + np.asarray(t)

    def pose_rows(self):
        return np.concatenate((self.C.reshape(self.N, 9), self.r), 1)


def assign(lay, seed=0):
    """which pool value every query and every (original) target row holds: (N,n), (N,m) -- random, so that neighbouring slots differ"""
    rng = np.random.default_rng(77 + seed)
    return rng.integers(0, P_SRC, (lay.N, lay.n)), rng.integers(0, P_TGT, (lay.N, lay.m))


def slot_terms(lay, dtype, pool, a_src, a_tgt, which):
    """Per cloud and launch: the live slots' queries, sorted rows, original rows and reference indices.  -> list over clouds of dict(q, srow, orow, ref)"""
    out = []
    for b, c in enumerate(lay.clouds):
        g = lay.geometry(dtype, b, which)
        s = np.flatnonzero(g.live)
        q = c[3][s].astype(np.int64)
        srow = g.row[s]
        orow = c[4][srow].astype(np.int64)
        assert (orow < lay.m).all()
        out.append(dict(slot=s, q=q, srow=srow, orow=orow, ref=pool.pair(b, a_src[b, q], a_tgt[b, orow]), geom=g))
    return out


# ---------------------------------------------------------------- a numpy emulation of the pass (for the test of the comparator only)
def emulate(lay, dtype, cv, terms, fault=None):
    """The windowed pass on the host, in the dtype under test: terms = {which: [per cloud (live slots, cv) float64]} as slot_terms orders them; the
    contributions go to their block's slab or to the far rows by the model, the slabs are summed per window, then reduced as window_reduce_kernel
    does (passes of MAXB blocks, the list of the windows that reach a reduce block's rows, rounds of 32).  -> (N, m, cv) float64 in ORIGINAL row order.
    fault: None | ("window", cloud, blk) | "round" | "pass" | "edges" | "far" -- the planted faults the comparator must refuse"""
    dt = np_dtype(dtype)
    wt = WT[dt]
    out = np.zeros((lay.N, lay.m, cv))
    for b, c in enumerate(lay.clouds):
        m, m_pad, tperm = lay.m, lay.m_pad, c[4]
        ga = lay.geometry(dt, b, "A")
        slab = np.zeros((ga.bpc, wt * cv), dtype=dt)
        far = np.zeros(m_pad * cv, dtype=dt)
        for which in ("A", "B"):
            g = lay.geometry(dt, b, which)
            s = np.flatnonzero(g.live)
            t = terms[which][b].astype(dt)
            inw = g.inwin[s]
            if fault == "edges":                                    # lo and hi - 1 taken for far rows, and dropped
                edge = (g.row[s] == g.lo[g.blk[s]]) | (g.row[s] == g.hi[g.blk[s]] - 1)
                t = t[~edge]
                s, inw = s[~edge], inw[~edge]
            cols = np.arange(cv)[None, :]
            blk_s, rel = g.blk[s[inw]], (g.row[s[inw]] - g.lo[g.blk[s[inw]]])
            launch = np.zeros_like(slab)
            np.add.at(launch, (blk_s[:, None], rel[:, None] * cv + cols), t[inw])
            slab = slab + launch
            if fault != "far":
                np.add.at(far, g.row[s[~inw]][:, None] * cv + cols, t[~inw])
        gt = np.zeros(m * cv, dtype=dt)
        per = BLOCK * WR_U
        for e0 in range(0, m * cv, per):
            e = np.arange(e0, min(e0 + per, m * cv))
            rows = e // cv
            acc = far[e].copy()
            for b0 in range(0, ga.bpc, MAXB):
                if fault == "pass" and b0 > 0:
                    break
                blocks = np.arange(b0, min(b0 + MAXB, ga.bpc))
                relv = blocks[(ga.lo[blocks] <= rows[-1]) & (ga.lo[blocks] + wt > rows[0])]
                for k, blk in enumerate(relv):
                    if (fault == "round" and k >= ROUND) or fault == ("window", b, int(blk)):
                        continue
                    lo = int(ga.lo[blk])
                    msk = (rows >= lo) & (rows < lo + wt)
                    acc[msk] += slab[blk][e[msk] - lo * cv]
            gt[e] = acc
        out[b][tperm[:m]] = gt.reshape(m, cv).astype(np.float64)
    return out


def row_reference(lay, dtype, pool, cv, a_src, a_tgt):
    """gtgt's reference per ORIGINAL target row over both launches: (T, TB, indegree) each (N * m, ...).  The bound: the terms' bounds plus
    count * u * sum |term| with count = in-degree over both launches + the windows covering the row + 1 (the far accumulator): the additions the
    windowed form performs."""
    br, bB = pool.ref["bwd"]
    N, m = lay.N, lay.m
    keys, idx, cover = [], [], np.zeros((N, m))
    for which in ("A", "B"):
        for b, st in enumerate(slot_terms(lay, dtype, pool, a_src, a_tgt, which)):
            keys.append(b * m + st["orow"])
            idx.append(st["ref"])
            cover[b][lay.clouds[b][4][:m]] = st["geom"].cover[:m]
    keys, idx = np.concatenate(keys), np.concatenate(idx)
    S, A, Bb = (np.zeros((N * m, cv)) for _ in range(3))
    np.add.at(S, keys, br[idx, 3:3 + cv])
    np.add.at(A, keys, np.abs(br[idx, 3:3 + cv]))
    np.add.at(Bb, keys, bB[idx, 3:3 + cv])
    D = np.bincount(keys, minlength=N * m)
    count = D + cover.reshape(-1) + 1
    return S, Bb + count[:, None] * pool.ar.u * A, D


_POOLS = {}


def pool(dtype, key, N, alive=None, unit_w=False):
    """the Pool of configuration window_config(key) for N clouds (evaluated once and shared by the tests; never written to)"""
    alive = tuple(np.ones(N) if alive is None else np.asarray(alive, dtype=np.float64))
    k = (np_dtype(dtype).name, key, N, alive, unit_w)
    if k not in _POOLS:
        _POOLS[k] = Pool(dtype, window_config(key), N, alive, unit_w)
    return _POOLS[k]
