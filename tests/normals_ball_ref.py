"""numpy restatement of dicp_amd/csrc/dicp_normals_ball.h (estimate_normals_ball: whole-ball normals with a gather backward), for the CPU and
GPU tests.  Written from the header's comment.

Everything is float64 on the exactly converted inputs; numpy rounds every operation on its own, as the header does with one statement per
product.  The live rows, the members and their order come from tests/iss_ball_ref.py, the mean and the covariance from tests/iss_ref.py
(both held to dicp_iss.h / dicp_iss_ball.h bit for bit); restated here are the Jacobi WITH eigenvectors, the sign, the curvature and the
gather.  `row_order` switches give WRONG references (members summed in row order) that the tests show the comparison to refuse.
"""
import numpy as np

import iss_ball_ref as ibr
import iss_ref as ir

REC = 13


def rotate_v(app, aqq, apq, arp, arq, V, p, q):
    """ir.rotate, statement for statement, with (c, s) also applied to the columns p, q of V (n, 3, 3)"""
    with np.errstate(all="ignore"):
        on = apq != 0.0
        diff = aqq - app
        two = 2.0 * apq
        zeta = diff / two
        zz = zeta * zeta
        h = 1.0 + zz
        den = np.abs(zeta) + np.sqrt(h)
        t = np.where(zeta < 0.0, -1.0, 1.0) / den
        tt = t * t
        g = 1.0 + tt
        c = 1.0 / np.sqrt(g)
        s = c * t
        u = t * apq
        cp, sq, sp, cq = c * arp, s * arq, s * arp, c * arq
        V = V.copy()
        for r in range(3):
            vp, vq = V[:, r, p].copy(), V[:, r, q].copy()
            cvp, svq, svp, cvq = c * vp, s * vq, s * vp, c * vq
            V[:, r, p] = np.where(on, cvp - svq, vp)
            V[:, r, q] = np.where(on, svp + cvq, vq)
        return (np.where(on, app - u, app), np.where(on, aqq + u, aqq), np.where(on, 0.0, apq), np.where(on, cp - sq, arp),
                np.where(on, sp + cq, arq), V)


def eigen(a, sweeps=ir.SWEEPS):
    """a: the six entries (xx, xy, xz, yy, yz, zz), each (n,) float64 -> lam (n, 3) ascending, v (n, 3, 3) with v[:, k] the eigenvector
    of lam[:, k]: the (diagonal value, index) pairs ordered ascending, ties to the lower index"""
    a = [np.array(x, dtype=np.float64) for x in a]
    n = a[0].shape[0]
    V = np.tile(np.eye(3), (n, 1, 1))
    for _ in range(sweeps):
        a[0], a[3], a[1], a[2], a[4], V = rotate_v(a[0], a[3], a[1], a[2], a[4], V, 0, 1)
        a[0], a[5], a[2], a[1], a[4], V = rotate_v(a[0], a[5], a[2], a[1], a[4], V, 0, 2)
        a[3], a[5], a[4], a[1], a[2], V = rotate_v(a[3], a[5], a[4], a[1], a[2], V, 1, 2)
    diag = np.stack((a[0], a[3], a[5]), axis=-1)
    order = np.argsort(diag, axis=1, kind="stable")
    lam = np.take_along_axis(diag, order, axis=1)
    v = np.stack([np.take_along_axis(V, order[:, None, k:k + 1].repeat(3, axis=1), axis=2)[:, :, 0] for k in range(3)], axis=1)
    return lam, v


def sign(v0, d):
    with np.errstate(all="ignore"):
        x, y, z = v0[:, 0] * d[:, 0], v0[:, 1] * d[:, 1], v0[:, 2] * d[:, 2]
        dot = (x + y) + z
    first = np.where(v0[:, 0] != 0, v0[:, 0], np.where(v0[:, 1] != 0, v0[:, 1], v0[:, 2]))
    return np.where(dot > 0, 1.0, np.where(dot < 0, -1.0, np.where(first < 0, -1.0, 1.0)))


def member_index(points, rows, radius, plan=None, row_order=False):
    """-> (P (m, 3) float64, ok (m,), mem (m, m - 1) bool, q, jc (m, m - 1): every row's OTHER live rows in grid order and which are members)"""
    points = np.asarray(points)
    order = ibr.grid_order(points, rows, radius, plan)
    idx = ibr.full_index(order, points.shape[0], row_order)
    P, ok, rws = ir._cloud(points, rows)
    mem, q, jc = ir.members(P, ok, idx, rws, radius)
    return P, ok, mem, q, jc, order


def forward_ref(points, radius, rows=None, viewpoint=None, min_neighbors=3, plan=None, row_order=False):
    """One cloud: points (m, >= 3) -> dict normals (m, 3), curv (m,), eig (m, 3) in the points' dtype, count (m,) int32, and the doubles
    lam, v (m, 3, 3: v[:, k] the k-th eigenvector), s (m,), n64 (m, 3), order (the grid order)"""
    points = np.asarray(points)
    dt = points.dtype
    P, ok, mem, q, _, order = member_index(points, rows, radius, plan, row_order)
    count = np.where(ok, 1 + mem.sum(axis=1), 0)
    lam, v = eigen(ir.covariance(mem, q, np.where(ok, count, 1)))
    vp = np.zeros(3) if viewpoint is None else np.asarray(viewpoint, dtype=dt).astype(np.float64)
    with np.errstate(all="ignore"):
        s = sign(v[:, 0], vp[None, :] - P)
        a = lam[:, 0] + lam[:, 1]
        t = a + lam[:, 2]
        curv = np.where(t > 0, lam[:, 0] / np.where(t > 0, t, 1.0), 0.0)
    on = ok & (count >= min_neighbors)
    n64 = np.where(on[:, None], s[:, None] * v[:, 0], 0.0)
    lam = np.where(ok[:, None], lam, 0.0)
    return dict(normals=n64.astype(dt), curv=np.where(on, curv, 0.0).astype(dt), eig=lam.astype(dt), count=count.astype(np.int32), lam=lam, v=v,
                s=np.where(on, s, 0.0), n64=n64, order=order)


def forward_ref_batch(points, radius, rows=None, viewpoint=None, plans=None, **kw):
    """(N, m, c) -> dict of stacked normals, curv, eig, count; viewpoint None, (3,) or (N, 3)"""
    vp = None if viewpoint is None else np.asarray(viewpoint)
    outs = [forward_ref(points[b], radius, None if rows is None else int(rows[b]), None if vp is None else (vp if vp.ndim == 1 else vp[b]),
                        plan=None if plans is None else plans[b], **kw) for b in range(points.shape[0])]
    return {key: np.stack([o[key] for o in outs]) for key in ("normals", "curv", "eig", "count")}


def term(R, y):
    """the three terms of nbl_term for records R (n, 13) and receiving coordinates y (n, 3), in double -> (n, 3)"""
    with np.errstate(all="ignore"):
        d = (y - R[:, 9:12]) - R[:, 6:9]
        G = R[:, :6]
        g = ((G[:, 0], G[:, 1], G[:, 2]), (G[:, 1], G[:, 3], G[:, 4]), (G[:, 2], G[:, 4], G[:, 5]))
        out = []
        for a in range(3):
            p0 = g[a][0] * d[:, 0]
            p1 = g[a][1] * d[:, 1]
            s1 = p0 + p1
            p2 = g[a][2] * d[:, 2]
            s2 = s1 + p2
            out.append(R[:, 12] * s2)
    return np.stack(out, axis=-1)


def gather_ref(points, records, radius, rows=None, plan=None, row_order=False):
    """One cloud: records (m, 13) float64 BY ORIGINAL ROW -> the gradient (m, 3) in the points' dtype: per row j the sum over its members
    in its own member order (j first) from +0 in double, members with f = 0 skipped, rounded once"""
    points = np.asarray(points)
    P, ok, mem, _, jc, _ = member_index(points, rows, radius, plan, row_order)
    R = np.asarray(records, dtype=np.float64)
    g = np.zeros((P.shape[0], 3))
    y = np.where(ok[:, None], P, 0.0)
    with np.errstate(all="ignore"):
        take = ok & (R[:, 12] != 0.0)
        g = np.where(take[:, None], g + term(R, y), g)
        for sl in range(mem.shape[1]):
            Ri = R[jc[:, sl]]
            take = mem[:, sl] & (Ri[:, 12] != 0.0)
            if take.any():
                g = np.where(take[:, None], g + term(Ri, y), g)
    return g.astype(points.dtype)


def records_by_row(slot_records, perm, m):
    """records (P, 13) in sorted-slot order and the grid's perm (P,) -> (m, 13) by original row (rows no slot names get zeros)"""
    out = np.zeros((m, REC))
    perm = np.asarray(perm)
    good = (perm >= 0) & (perm < m)
    out[perm[good]] = np.asarray(slot_records)[good]
    return out


# ------------------------------------------------------------------ the float64 torch composition that the gradient is held to
def composition(points64, radius, rows=None, viewpoint=None, min_neighbors=3, plan=None, points=None):
    """torch autograd on the CPU in float64: a CONSTANT membership mask from the reference, masked mean and covariance,
    torch.linalg.eigh, the reference's sign.  points64: a (m, 3) float64 torch tensor (finite everywhere; requires_grad as the caller
    likes); points: the cloud the membership, the live rows and the sign are taken from (default: points64's values).
    -> dict normals (m, 3), curv (m,) with zeros where the reference has them, C (m, 3, 3) the covariances"""
    import torch
    P = points64.detach().numpy() if points is None else np.asarray(points)
    m = P.shape[0]
    ref = forward_ref(P, radius, rows, viewpoint, min_neighbors, plan)
    _, ok, mem, _, jc, _ = member_index(P, rows, radius, plan)
    M = np.zeros((m, m))
    for i in range(m):
        M[i, jc[i][mem[i]]] = 1.0
        M[i, i] = 1.0 if ok[i] else 0.0
    on = ok & (ref["count"] >= min_neighbors)
    Mt, onb = torch.from_numpy(M), torch.from_numpy(on)
    n = Mt.sum(1).clamp(min=1.0)
    q = points64[None, :, :] - points64[:, None, :]                                   # q[i, j] = p_j - p_i
    mu = (Mt[:, :, None] * q).sum(1) / n[:, None]
    d = (q - mu[:, None, :]) * Mt[:, :, None]
    C = torch.einsum("ija,ijb->iab", d, d) / n[:, None, None]
    harmless = torch.diag(torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64))[None]   # (what eigh sees of the rows that are off)
    lam, vec = torch.linalg.eigh(torch.where(onb[:, None, None], C, harmless))
    v0 = vec[:, :, 0]
    flip = torch.sign((v0.detach() * torch.from_numpy(ref["v"][:, 0])).sum(1))        # eigh's sign is arbitrary: the reference's v_0
    nrm = v0 * (flip * torch.from_numpy(ref["s"]))[:, None]
    curv = lam[:, 0] / lam.sum(1)
    return dict(normals=torch.where(onb[:, None], nrm, torch.zeros_like(nrm)), curv=torch.where(onb, curv, torch.zeros_like(curv)), C=C)
