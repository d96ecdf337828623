"""The windowed backward of the ICP loop at operator level, on the GPU: dicp_accumulate_bwd_window (window_body), dicp_window_reduce and
dicp_permute_rows / dicp_permute_add_rows against the float64 reference of tests/point_math_ref.py, every value within the bound of that
module's first-order error model (safety factor 1, nothing tuned), on the match layouts of tests/icp_window_layouts.py: the numpy model there
proves -- before any GPU result is read -- that each layout reaches the branch it is meant for (a second pass of the reduce's MAXB-block loop, a
second round of its 32-window masks, row lists of a whole block, matches exactly at lo - 1 / lo / hi - 1 / hi, both clamps of the window origin,
m_pad <= WT, ragged row counts, NULL qorder / weights / alive / slab).  tests/test_icp_window_layouts.py holds the model to the sources and shows
that the comparator used here refuses a dropped window, round, pass, edge slot or far row.

Every case runs the sequence of one call of the loop: the first launch overwrites NaN-filled accumulators with the matches A, the second adds the
matches B under the same window origins, the slot-order gradients are un-permuted, and the slabs are reduced once with = into NaN and once with
+= into known values.

Largest |error| / bound per output family: DESIGN.md section 2 and profiles/r24_window_backward.txt.  With DICP_RECORD_RATIOS=<file> every test
appends its own figures to that file (the measurement; nothing here is tuned to it).
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_window_layouts as wl  # noqa: E402
import point_math_ref as R  # noqa: E402

from dicp_amd import _lib, _ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
DTYPES = [np.float32, np.float64]
ids = lambda d: np.dtype(d).name
SENTINEL = 777.0

# (layout, key of point_math_ref._SUM_CFG): 2 pt2pl/6 huber soft trim; 3 pt2pt/3 cauchy soft; 511 pt2pl/6 hard trim loss, hard trim; 512 pt2pt/6 hard
# huber, hard trim; 513 pt2pl/6 cauchy soft trim.  Each of pt2pl/6, pt2pt/3, pt2pt/6 meets diagonal, all_far and a block hub.
CASES = [("diagonal", 2), ("diagonal", 3), ("diagonal", 512), ("all_far", 513), ("all_far", 3), ("all_far", 512),
         ("block_hub_256", 511), ("block_hub_256", 3), ("block_hub_256", 512), ("block_hub_1024", 2), ("block_hub_1024", 3), ("block_hub_1024", 512),
         ("edges", 513), ("edges", 3), ("covered_34", 511), ("covered_34", 512), ("small_target_70", 513), ("small_target_70", 3),
         ("small_target_1", 2), ("small_target_1", 512), ("ragged", 2), ("ragged", 512)]
BIG = {np.dtype(np.float32): 2, np.dtype(np.float64): 512}         # blocks_257: one configuration per dtype


@pytest.fixture(autouse=True)
def _threads():
    before = torch.get_num_threads()
    torch.set_num_threads(4)            # (the reference's sensitivities are many small reverse passes: more threads only add overhead)
    yield
    torch.set_num_threads(before)


def _note(test, dtype, record):
    path = os.environ.get("DICP_RECORD_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(test=test, dtype=np.dtype(dtype).name, ratios=record)) + "\n")


def dev(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a if dt is None else np.asarray(a).astype(dt))).to(DEV)


def host(t):
    return t.cpu().numpy().astype(np.float64)


def run_case(lay, dtype, key, variant=None):
    """One layout under one configuration through the C entry points, held to the reference.  variant: None | "qorder_null" | "w_null" |
    "alive_null" | "slab_null".  -> {family: largest |error| / bound}"""
    dt = np.dtype(dtype)
    tdt, code = TDT[dt], _ops._DT[TDT[dt]]
    lib = _lib.load()
    st = _ops._stream()
    p = _ops._p
    print(wl.check_conditions(lay, dt))                             # the layout reaches its code: on the model alone
    cfg = wl.window_config(key)
    c, cv = cfg["c"], 6 if cfg["mode"] == "pt2pl" else 3
    N, n, m, m_pad = lay.N, lay.n, lay.m, lay.m_pad
    if variant == "alive_null":
        assert (lay.alive == 1).all()
    pool = wl.pool(dt, key, N, lay.alive, unit_w=variant == "w_null")
    ar, u = pool.ar, pool.ar.u
    a_src, a_tgt = wl.assign(lay)
    what = "%s %s %s%s" % (lay.name, dt.name, R.cfg_id(cfg), " " + variant if variant else "")
    bi = np.arange(N)[:, None]
    # ---- the inputs in the original orders, then the sorted copies the kernels read
    src, w0 = dev(pool.p[bi, a_src], dt), dev(pool.w[bi, a_src], dt)
    tgt = dev(np.concatenate((pool.Y[a_tgt], pool.nrm[a_tgt]), 2)[:, :, :c], dt)
    qorder, tperm = dev(lay.stack(3)), dev(lay.stack(4))
    spos_ref, spos = dev(lay.stack(5)), {"A": dev(lay.stack(6)), "B": dev(lay.stack(7))}
    rows = lay.src_rows
    src_rows = dev(rows) if (rows != n).any() else None
    alive = None if variant == "alive_null" else dev(lay.alive, dt)
    pose, gs, gb = dev(pool.pose_rows(), dt), dev(pool.Gs, dt), dev(pool.gb, dt)
    P = R.params_of(cfg, _lib.WeightParams)
    qo_arg = None if variant == "qorder_null" else qorder
    if variant == "qorder_null":
        assert (lay.stack(3) == np.arange(n)[None, :]).all()
    src_s = _ops._gather_rows_raw(src, qorder)
    w_s = None if variant == "w_null" else _ops._gather_rows_raw(w0.unsqueeze(-1), qorder).squeeze(-1).contiguous()
    tgt_s = _ops._gather_rows_raw(tgt, tperm)
    assert tuple(tgt_s.shape) == (N, m_pad, c)
    bpc, wt = lib.dicp_window_blocks(code, n, m_pad), lib.dicp_window_rows(code)
    assert bpc == lay.geometry(dt, 0, "A").bpc and wt == wl.WT[dt]
    nan = float("nan")
    full = lambda shape, v: torch.full(shape, v, dtype=tdt, device=DEV)
    gsrc_s = full((N, n, 3), nan)
    gw_s = None if variant == "w_null" else full((N, n), nan)
    with_slab = variant != "slab_null"
    slab = full((N, bpc, wt, cv), nan) if with_slab else None
    gfar = torch.zeros((N, m_pad, cv), dtype=tdt, device=DEV) if with_slab else None
    parts = {}
    for which, ow in (("A", 1), ("B", 0)):
        part = full((N, bpc, _lib.NBWD_PAD), nan if which == "A" else SENTINEL)
        _lib.check(lib.dicp_accumulate_bwd_window(code, ctypes.byref(P), p(src_s), p(tgt_s), c, p(spos[which]), p(spos_ref), p(qo_arg), p(pose), p(w_s), p(alive),
                                                  p(gs), p(gb), p(src_rows), N, n, m_pad, p(gsrc_s), p(slab), p(gfar), p(gw_s), p(part), ow, st),
                   "dicp_accumulate_bwd_window")
        parts[which] = part
        if which == "A":                                            # the pad slots of a ragged batch start at exactly zero
            torch.cuda.synchronize()
            g0, w0s = host(gsrc_s), host(gw_s) if gw_s is not None else np.zeros((N, n))
            dead = np.arange(n)[None, :] >= rows[:, None]
            assert (g0[dead] == 0).all() and (w0s[dead] == 0).all(), what + ": slots past src_rows must be 0 after the first launch"
            assert np.isfinite(g0).all() and np.isfinite(w0s).all()
    gsrc, gw = full((N, n, 3), nan), torch.zeros((N, n), dtype=tdt, device=DEV)
    _lib.check(lib.dicp_permute_rows(code, p(gsrc_s), p(qorder), N, n, n, n, 3, 3, p(gsrc), n, 3, st), "dicp_permute_rows")
    if gw_s is not None:
        _lib.check(lib.dicp_permute_add_rows(code, p(gw_s), p(qorder), N, n, n, n, 1, 1, p(gw), n, 1, st), "dicp_permute_add_rows")
    prefill = np.broadcast_to((0.5 + 0.125 * (np.arange(m * c) % 7)).reshape(1, m, c), (N, m, c))
    gt1, gt2 = full((N, m, c), nan), dev(prefill, dt)
    if with_slab:
        for g, ow in ((gt1, 1), (gt2, 0)):
            _lib.check(lib.dicp_window_reduce(code, p(slab), p(spos_ref), p(qo_arg), p(tperm), p(gfar), p(src_rows), N, n, m, m_pad, cv, p(g), c, ow, st),
                       "dicp_window_reduce")
    torch.cuda.synchronize()

    # ---- the reference: a slot's terms are its (source value, target value) pair's, per launch
    br, bB = pool.ref["bwd"]
    terms = {w: wl.slot_terms(lay, dt, pool, a_src, a_tgt, w) for w in "AB"}
    record = {}
    # gsrc, gw per point: term A + term B, the two bounds plus u |sum| for the one extra addition
    gsrc_h, gw_h = host(gsrc), host(gw)
    assert np.isfinite(gsrc_h).all() and np.isfinite(gw_h).all()
    cols = [0, 1, 2, 9]
    for b in range(N):
        A, B = terms["A"][b], terms["B"][b]
        assert np.array_equal(A["q"], B["q"])
        q = A["q"]
        ref = br[A["ref"]][:, cols] + br[B["ref"]][:, cols]
        bound = bB[A["ref"]][:, cols] + bB[B["ref"]][:, cols] + u * np.abs(ref)
        got = np.concatenate((gsrc_h[b, q], gw_h[b, q][:, None]), 1)
        if variant == "w_null":                                     # no weights, no gradient for them
            got[:, 3] = ref[:, 3]
        R.check_points(got, ref, bound, "%s cloud %d gsrc, gw" % (what, b), families={"gsrc": [0, 1, 2], "gw": [3]}, record=record)
        past = np.setdiff1d(np.arange(n), q)
        assert (gsrc_h[b, past] == 0).all() and (gw_h[b, past] == 0).all()
        if lay.alive[b] == 0:
            assert (gsrc_h[b] == 0).all(), what + ": a cloud that is not alive has zero source gradients"
    # the pose sums, per launch: the blocks' partial sums added in extended precision
    for w in "AB":
        ph = parts[w].cpu().numpy()
        assert np.isfinite(ph).all() and (ph[:, :, 12:] == 0).all(), what + ": the pad columns of bwd_partials are 0"
        cl = np.concatenate([np.full(len(t["ref"]), b) for b, t in enumerate(terms[w])])
        idx = np.concatenate([t["ref"] for t in terms[w]])
        Ps, PB, _ = R.sums_by(cl, N, br[idx, 10:22], bB[idx, 10:22], u)
        got = ph.astype(np.longdouble).sum(1).astype(np.float64)[:, :12]
        R.check_points(got, Ps, PB, "%s pose sums of launch %s" % (what, w), families={"pose": list(range(12))}, record=record)
        for b in np.flatnonzero(rows == 0):
            assert (ph[b] == 0).all(), what + ": a cloud of no rows has zero partial sums"
    if not with_slab:
        return record
    # gtgt per ORIGINAL target row: the sum over both launches; count = in-degree + covering windows + 1
    T, TB, D = wl.row_reference(lay, dt, pool, cv, a_src, a_tgt)
    fam = {"gtgt": [0, 1, 2]} if cv == 3 else {"gtgt": [0, 1, 2], "gnormal": [3, 4, 5]}
    far_h = host(gfar)
    assert np.isfinite(far_h).all() and (far_h[:, m:] == 0).all(), what + ": pad rows are never matched"
    g1, g2, pre = host(gt1).reshape(N * m, c), host(gt2).reshape(N * m, c), prefill.reshape(N * m, c)
    assert np.isfinite(g1[:, :cv]).all() and np.isfinite(g2).all()
    assert np.isnan(g1[:, cv:]).all() and (g2[:, cv:] == pre[:, cv:]).all(), what + ": columns cv .. c of gtgt are not the reduce's"
    assert (D > 0).any()
    assert (g1[D == 0, :cv] == 0).all() and (g2[D == 0] == pre[D == 0]).all(), what + ": a row nothing matches"
    R.check_points(g1[:, :cv], T, TB, what + " gtgt (=)", families=fam, record=record)
    ref2 = pre[:, :cv].astype(dt).astype(np.float64) + T
    R.check_points(g2[:, :cv], ref2, TB + u * np.abs(ref2), what + " gtgt (+=)", families=fam, record=record)
    for b in range(N):
        if lay.alive[b] == 0 or rows[b] == 0:
            assert (g1[b * m:(b + 1) * m, :cv] == 0).all(), what + ": a cloud that is not alive, or has no rows, has zero target gradients"
    return record


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name,key", CASES)
def test_layouts(name, key, dtype):
    """Every layout under the configurations rotated over them: gsrc and gw per point, gtgt (normals' columns included) per target row with the
    summation term of the additions the windowed form performs, the pose sums per launch; finite everywhere, exact zeros and untouched sentinels
    where nothing is added."""
    record = run_case(wl.layout(name, dtype), dtype, key)
    _note("window %s %s" % (name, R.cfg_id(wl.window_config(key))), dtype, record)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_blocks_257(dtype):
    """65537 slots against 131200 rows: 257 window blocks, the second pass of the reduce's loop over MAXB = 256 blocks (N = 1, one configuration)."""
    key = BIG[np.dtype(dtype)]
    record = run_case(wl.layout("blocks_257", dtype), dtype, key)
    _note("window blocks_257 %s" % R.cfg_id(wl.window_config(key)), dtype, record)


@pytest.mark.parametrize("variant", ["qorder_null", "w_null", "alive_null", "slab_null"])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_call_variants(dtype, variant):
    """The other ways the ABI lets a caller pass the same call, on the diagonal layout, held to the same reference: qorder == NULL (identity slot
    order), w_s == gw_s == NULL (unit weights), alive == NULL, slab == gts_far == NULL (gsrc, gw and the pose sums only)."""
    lay = wl.diagonal(np.dtype(dtype), identity=True) if variant == "qorder_null" else wl.layout("diagonal", dtype)
    record = run_case(lay, dtype, 2, variant)
    _note("window variant " + variant, dtype, record)
