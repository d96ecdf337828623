"""numpy restatement of dicp_amd/csrc/dicp_fpfh_ball.h (whole-ball FPFH: fpfh_features_ball / compute_fpfh(whole_ball=True)), for the
CPU and GPU tests.  Written from the header's comment.

The near list of an OK row is every other OK live row inside the radius at a distance > 0, in ascending (cell key, row index) order of the
cloud's cell grid.  The ORDER comes from tests/iss_ball_ref.py (grid_order / full_index), the ARITHMETIC from the building blocks of
tests/fpfh_ref.py (pair_features, bin_theta, bin_unit), with int64 counts: fpfh_ref itself returns uint8 counts, which wrap past 255.
Before the pair arithmetic the slots outside the radius are removed from each row's list (the same double rule, r2 <= radius radius):
that keeps the order of the slots that stay, and with it every bit, and bounds the memory by the largest ball instead of the cloud.
"""
import numpy as np

import fpfh_ref as fr
import iss_ball_ref as ibr

BINS, CH = fr.BINS, fr.CH


def compress(points, idx, rows, radius):
    """idx (m, k) -> (m, k') with every slot outside the radius (or empty, or the row itself) removed and the others moved up in order"""
    m = idx.shape[0]
    P = np.asarray(points)[:, :3].astype(np.float64)
    j = np.asarray(idx).astype(np.int64)
    live = (j >= 0) & (j < rows) & (j != np.arange(m)[:, None])
    jc = np.where(live, j, 0)
    with np.errstate(all="ignore"):
        d = P[jc] - P[:, None, :]
        keep = live & (fr.dot(d, d) <= float(radius) * float(radius))
    width = max(int(keep.sum(axis=1).max()) if m else 0, 1)
    out = np.full((m, width), -1, dtype=np.int64)
    for i in range(m):
        sel = j[i][keep[i]]
        out[i, :sel.size] = sel
    return out


def fpfh_from_index(points, normals, idx, rows, radius):
    """fpfh_ref's arithmetic on an index of any width -> (out (m, 33) in the points' dtype, cnt (m, 33) int64)"""
    m, k = idx.shape
    P = np.asarray(points)[:, :3].astype(np.float64)
    Nn = np.asarray(normals).astype(np.float64)
    ok = fr.row_ok(P, Nn)
    ok[rows:] = False
    j = np.asarray(idx).astype(np.int64)
    live = (j >= 0) & (j < rows) & (j != np.arange(m)[:, None])
    jc = np.where(live, j, 0)
    f = fr.pair_features(P[:, None, :], Nn[:, None, :], P[jc], Nn[jc])
    with np.errstate(all="ignore"):
        r2 = f["r2"]
        near = live & ok[:, None] & ok[jc] & (r2 > 0.0) & (r2 <= float(radius) * float(radius))
        pair = near & f["frame"]
        ii = np.broadcast_to(np.arange(m)[:, None], (m, k))
        cnt = np.zeros((m, CH), dtype=np.int64)
        for b in (fr.bin_theta(f["cos"], f["sin"]), BINS + fr.bin_unit(f["alpha"]), 2 * BINS + fr.bin_unit(f["phi"])):
            np.add.at(cnt, (ii[pair], b[pair]), 1)
        c = pair.sum(axis=1)
        den = np.where(c > 0, c, 1).astype(np.float64)
        s = np.where((c > 0)[:, None], (100.0 * cnt.astype(np.float64)) / den[:, None], 0.0)
        acc = np.zeros((m, CH))
        for sl in range(k):
            wj = 1.0 / r2[:, sl]
            t = wj[:, None] * s[jc[:, sl]]
            acc = np.where(near[:, sl, None], acc + t, acc)
        out = np.zeros((m, CH))
        for g in range(3):
            S = np.zeros(m)
            for a in range(BINS):
                S = S + acc[:, g * BINS + a]
            fac = 100.0 / S
            u = np.where((S != 0.0)[:, None], acc[:, g * BINS:(g + 1) * BINS] * fac[:, None], 0.0)
            out[:, g * BINS:(g + 1) * BINS] = u + s[:, g * BINS:(g + 1) * BINS]
        return out.astype(np.asarray(points).dtype), cnt


def fpfh_ball_ref(points, normals, radius, rows=None, plan=None, row_order=False):
    """One cloud: points (m, >= 3), normals (m, 3) -> dict out (m, 33) in the points' dtype, cnt (m, 33) int64, order (the grid order).
    plan: as iss_ball_ref.grid_order.  row_order: a WRONG reference, the near list in row order"""
    points = np.asarray(points)
    m = points.shape[0]
    rows = m if rows is None else int(min(max(rows, 0), m))
    order = ibr.grid_order(points, rows, radius, plan)
    idx = compress(points, ibr.full_index(order, m, row_order), rows, radius)
    out, cnt = fpfh_from_index(points, normals, idx, rows, radius)
    return dict(out=out, cnt=cnt, order=order)


def fpfh_ball_ref_batch(points, normals, radius, rows=None, plans=None, **kw):
    """(N, m, c), (N, m, 3), rows a sequence or None -> dict of stacked out (N, m, 33), cnt (N, m, 33) int64"""
    outs = [fpfh_ball_ref(points[b], normals[b], radius, None if rows is None else int(rows[b]), plan=None if plans is None else plans[b], **kw)
            for b in range(points.shape[0])]
    return {key: np.stack([o[key] for o in outs]) for key in ("out", "cnt")}


def at_ref(full, at, rows):
    """the rows `at` (q,) names of one cloud's (m, ...) result -> (q, ...): zeros for an entry outside 0 <= at < rows"""
    at = np.asarray(at).astype(np.int64)
    live = (at >= 0) & (at < rows)
    out = np.zeros((at.size,) + full.shape[1:], dtype=full.dtype)
    out[live] = full[at[live]]
    return out
