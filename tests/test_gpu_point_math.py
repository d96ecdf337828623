"""The shipped per-point arithmetic at operator level, on the GPU: dicp_accumulate, dicp_accumulate_bwd and dicp_loss_weight{,_bwd} against the
float64 reference of tests/point_math_ref.py, every value within the bound of that module's first-order error model (safety factor 1; float32 with
the constants of the one-instruction forms of csrc/dicp_math.h).  tests/test_point_math_ref.py holds the g++ build of the same header to the same
model on a CPU, proves that the comparator refuses a perturbed reference, and checks on the reference alone that these inputs contain no tie.

Per-slot accuracy comes from batches of many clouds of ONE point: partials (N, 1, 32) then holds each point's 30 slots, bwd_partials its 12 pose
sums.  Sums over the points of a cloud are checked at the sizes around the 512-point block of dicp_accumulate_blocks.

Largest |error| / bound per output family: DESIGN.md section 2 and profiles/r10_point_math_bounds.txt.  With DICP_RECORD_RATIOS=<file> every test
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
import point_math_ref as R  # noqa: E402

from dicp_amd import _lib, _ops  # noqa: E402
from dicp_amd.loss import loss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
DTYPES = [np.float32, np.float64]
N_POINTS = R.GPU_POINTS


@pytest.fixture(autouse=True)
def _threads():
    before = torch.get_num_threads()
    torch.set_num_threads(4)            # (the reference's sensitivities are many small reverse passes: more threads only add overhead)
    yield
    torch.set_num_threads(before)


def _note(test, dtype, record, ties=()):
    path = os.environ.get("DICP_RECORD_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(test=test, dtype=np.dtype(dtype).name, ratios=record, ties=list(ties))) + "\n")


def dev(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a if dt is None else np.asarray(a).astype(dt))).to(DEV)


class GpuBackend:
    """Every point a cloud of its own (n = 1) with its own pose, through the library's C entry points.
    c_row: elements per target row (None: the configuration's); m: target rows per cloud, the matched one at a seeded position, every other NaN;
    idx: "given" | "null" (one row per point, m = 1) | "minus1" (-1: clamped to row 0, where the match then lies);
    w_init / alive: False passes NULL (the inputs must then hold ones)"""
    build = "device"

    def __init__(self):
        self.lib = _lib.load()

    def _layout(self, dtype, cfg, inp, c_row, m, idx):
        dt = np.dtype(dtype)
        N = inp["p"].shape[0]
        c = cfg["c"] if c_row is None else c_row
        rows = R.target_rows(inp, 6 if c >= 6 else 3, dt)
        j = np.random.default_rng(5).integers(0, m, N) if (idx == "given" and m > 1) else np.zeros(N, dtype=np.int64)
        tgt = np.full((N, m, c), np.nan, dtype=dt)
        tgt[np.arange(N), j, :rows.shape[1]] = rows
        ix = None if idx == "null" else dev((np.full(N, -1) if idx == "minus1" else j).astype(np.int32).reshape(N, 1))
        return N, c, j, dev(tgt), ix

    def _args(self, dtype, cfg, inp, w_init, alive):
        dt = np.dtype(dtype)
        N = inp["p"].shape[0]
        if not w_init:
            assert bool((inp["w_init"] == 1).all())
        if not alive:
            assert bool((inp["alive"] == 1).all())
        return (dev(inp["p"].numpy().reshape(N, 1, 3), dt), dev(R.pose_rows(inp, dt)), dev(inp["w_init"].numpy().reshape(N, 1), dt) if w_init else None,
                dev(inp["alive"].numpy(), dt) if alive else None, R.params_of(cfg, _lib.WeightParams))

    def forward(self, dtype, cfg, inp, c_row=None, m=1, idx="given", w_init=True, alive=True):
        dt = np.dtype(dtype)
        N, c, j, tgt, ix = self._layout(dtype, cfg, inp, c_row, m, idx)
        src, pose, w0, al, P = self._args(dtype, cfg, inp, w_init, alive)
        assert self.lib.dicp_accumulate_blocks(1) == 1
        part = torch.full((N, 1, _lib.NACC_PAD), float("nan"), dtype=TDT[dt], device=DEV)
        w = torch.full((N, 1), float("nan"), dtype=TDT[dt], device=DEV)
        _lib.check(self.lib.dicp_accumulate(_ops._DT[TDT[dt]], ctypes.byref(P), _ops._p(src), _ops._p(tgt), c, _ops._p(ix), _ops._p(pose), _ops._p(w0), _ops._p(al),
                                            None, N, 1, m, _ops._p(part), _ops._p(w), 1, _ops._stream()), "dicp_accumulate")
        torch.cuda.synchronize()
        part = part.cpu().numpy().astype(np.float64)
        assert (part[:, 0, R.NACC:] == 0).all(), "the pad slots of a partials row are written as 0"
        return np.concatenate((w.cpu().numpy().astype(np.float64), part[:, 0, :R.NACC]), 1)

    def backward(self, dtype, cfg, inp, cot, c_row=None, m=1, idx="given", w_init=True, alive=True):
        dt = np.dtype(dtype)
        N, c, j, tgt, ix = self._layout(dtype, cfg, inp, c_row, m, idx)
        src, pose, w0, al, P = self._args(dtype, cfg, inp, w_init, alive)
        gs, gb = dev(cot[0].numpy(), dt), dev(cot[1].numpy(), dt)
        gsrc, gtgt = torch.zeros_like(src), torch.zeros((N, m, c), dtype=TDT[dt], device=DEV)
        gw = torch.zeros((N, 1), dtype=TDT[dt], device=DEV) if w_init else None
        part = torch.full((N, 1, _lib.NBWD_PAD), float("nan"), dtype=TDT[dt], device=DEV)
        _lib.check(self.lib.dicp_accumulate_bwd(_ops._DT[TDT[dt]], ctypes.byref(P), _ops._p(src), _ops._p(tgt), c, _ops._p(ix), _ops._p(pose), _ops._p(w0), _ops._p(al),
                                                _ops._p(gs), _ops._p(gb), None, N, 1, m, _ops._p(gsrc), _ops._p(gtgt), _ops._p(gw), _ops._p(part), _ops._stream()),
                   "dicp_accumulate_bwd")
        torch.cuda.synchronize()
        gt = gtgt.cpu().numpy().astype(np.float64)
        row = gt[np.arange(N), j].copy()
        cv = 6 if cfg["mode"] == "pt2pl" else 3
        gt[np.arange(N), j, :cv] = 0
        assert (gt == 0).all(), "a gradient was written outside the matched row's %d columns" % cv
        gn = row[:, 3:6] if cv == 6 else np.zeros((N, 3))
        gwv = gw.cpu().numpy().astype(np.float64) if w_init else np.full((N, 1), np.nan)
        part = part.cpu().numpy().astype(np.float64)
        assert (part[:, 0, 12:] == 0).all()
        return np.concatenate((gsrc.cpu().numpy().astype(np.float64).reshape(N, 3), row[:, :3], gn, gwv, part[:, 0, :12]), 1)

    def loss_weight(self, dtype, name, diff, metric, tanh_k, err, gw):
        """through dicp_amd.loss.loss on a (1, n, r) tensor (the 3-D form: (N, n) weights)"""
        dt = np.dtype(dtype)
        e = dev(err.numpy()[None], dt).requires_grad_(True)
        w = loss(name=name, metric=metric, differentiable=diff, tanh_steepness=tanh_k).get_weight(e)
        assert tuple(w.shape) == (1, err.shape[0])
        if w.requires_grad:
            (w * dev(gw.numpy()[None], dt)).sum().backward()
        ge = e.grad if e.grad is not None else torch.zeros_like(e)
        return w.detach().cpu().numpy().astype(np.float64)[0], ge.cpu().numpy().astype(np.float64)[0]


@pytest.fixture(scope="module")
def gpu():
    return GpuBackend()


# ---------------------------------------------------------------- every point's w, 30 slots and gradients, over the whole grid and all edge sets
@pytest.mark.parametrize("cfg", R.grid(), ids=R.cfg_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_points_grid(gpu, dtype, cfg):
    """dicp_accumulate / dicp_accumulate_bwd on N clouds of one point: w_out against B(w), each of the 30 slots of partials (N,1,32) against its own
    bound, gsrc, gtgt (normals included), gw and the 12 pose sums of bwd_partials against the autograd reference, on random points (no tie) and
    on every edge set (zero residual with the hard Huber NaN, residual exactly the metric / the trim distance, saturated gates, w = 0, w around
    match_thresh, tiny and huge residuals, 2.5 km and 25 km from the origin, w_init of 0 / 1 / 1e-12 / 1e6, alive = 0)."""
    record, ties = {}, []
    R.run_config(gpu, dtype, cfg, N_POINTS, record, ties)
    _note("points_grid " + R.cfg_id(cfg), dtype, record, ties)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_gate_tail(gpu, dtype):
    """A soft gate between tanh argument -5 and saturation (the region the first-order check leaves out): 0 <= w <= w_ref + B(w), every slot finite."""
    for cfg in R.grid():
        if cfg["diff"] and (cfg["trim_on"] or cfg["loss"] == "trim"):
            R.run_gate_tail(gpu, dtype, cfg)


VARIANTS = {
    "idx_null": dict(idx="null"),                           # idx == NULL: one row per point
    "idx_minus1": dict(idx="minus1", m=3),                  # "no neighbour": row 0
    "padded_rows": dict(c_row="pad", m=64),                 # the sorted copies the sweep path feeds: 4 / 8 elements per row, m = m_pad
    "w_init_null": dict(w_init=False),
    "alive_null": dict(alive=False),
    "many_rows": dict(m=37),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_call_variants(gpu, dtype, variant):
    """The other ways the ABI lets a caller pass the same points: the results are held to the same reference and bounds."""
    kw = dict(VARIANTS[variant])
    record = {}
    cfgs = [c for c in R.grid() if c["ps"] == 0 and c["diff"] and c["trim_on"] and c["loss"] in ("huber", "cauchy")]
    assert len(cfgs) == 6
    for cfg in cfgs:
        kw_c = dict(kw)
        if variant == "padded_rows":
            kw_c["c_row"] = 8 if cfg["c"] == 6 else 4
            assert kw_c["m"] == gpu.lib.dicp_padded_targets(kw_c["m"])
        ar = R.Arith(dtype, "device")
        inp, cot = R.random_case(dtype, cfg, 1024)
        if kw.get("w_init") is False:
            inp["w_init"] = torch.ones_like(inp["w_init"])
        ref = R.reference(ar, cfg, inp, cot)
        R.check_case(ref, 1024, [])
        what = "%s %s %s" % (variant, np.dtype(dtype).name, R.cfg_id(cfg))
        got = gpu.forward(dtype, cfg, inp, **kw_c)
        R.check_points(got, ref["fwd"][0], ref["fwd"][1], what + " forward", families=R.FWD_FAMILIES, record=record)
        gotb = gpu.backward(dtype, cfg, inp, cot, **kw_c)
        if kw.get("w_init") is False:                       # no w_init, no gradient for it
            gotb[:, 9] = ref["bwd"][0][:, 9]
        R.check_points(gotb, ref["bwd"][0], ref["bwd"][1], what + " backward", families=R.BWD_FAMILIES, record=record)
    _note("call_variants " + variant, dtype, record)


# ---------------------------------------------------------------- sums over a cloud's points, around the 512-point block
@pytest.mark.parametrize("n", R.SUM_SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_block_sums(gpu, dtype, n):
    """Four clouds of n points, rows = [n, n - 1, 0, n] taking part (src_rows), alive = [1, 1, 1, 0], target rows of in-degree about 2: the partials
    summed in extended precision against the sum of the reference's terms, within the sum of the terms' bounds plus n u sum |term|; w_out, gsrc and
    gw per point; gtgt per target row with the summation term of its in-degree; rows past a cloud's own count carry weight 0 and w_out 0."""
    dt = np.dtype(dtype)
    K = R.sum_case(dtype, n)
    cfg, N, m = K["cfg"], K["N"], K["m"]
    ar = R.Arith(dtype, "device")
    ref = R.sum_reference(ar, K)
    lib = gpu.lib
    code = _ops._DT[TDT[dt]]
    P = R.params_of(cfg, _lib.WeightParams)
    src, tgt, idx, pose, w0, alive, rows = (dev(K[k]) for k in ("src", "tgt", "idx", "pose", "w_init", "alive", "rows"))
    nb = lib.dicp_accumulate_blocks(n)
    assert nb == (n + 511) // 512
    part = torch.full((N, nb, _lib.NACC_PAD), float("nan"), dtype=TDT[dt], device=DEV)
    w = torch.full((N, n), float("nan"), dtype=TDT[dt], device=DEV)
    _lib.check(lib.dicp_accumulate(code, ctypes.byref(P), _ops._p(src), _ops._p(tgt), cfg["c"], _ops._p(idx), _ops._p(pose), _ops._p(w0), _ops._p(alive),
                                   _ops._p(rows), N, n, m, _ops._p(part), _ops._p(w), n, _ops._stream()), "dicp_accumulate")
    gs, gb = dev(K["Gs"]), dev(K["gb"])
    gsrc, gtgt, gw = torch.zeros_like(src), torch.zeros_like(tgt), torch.zeros_like(w0)
    bpart = torch.full((N, nb, _lib.NBWD_PAD), float("nan"), dtype=TDT[dt], device=DEV)
    _lib.check(lib.dicp_accumulate_bwd(code, ctypes.byref(P), _ops._p(src), _ops._p(tgt), cfg["c"], _ops._p(idx), _ops._p(pose), _ops._p(w0), _ops._p(alive),
                                       _ops._p(gs), _ops._p(gb), _ops._p(rows), N, n, m, _ops._p(gsrc), _ops._p(gtgt), _ops._p(gw), _ops._p(bpart), _ops._stream()),
               "dicp_accumulate_bwd")
    torch.cuda.synchronize()
    cl, pt, row = K["cloud"], K["point"], K["row"]
    record = {}
    what = "sums n=%d %s %s" % (n, dt.name, R.cfg_id(cfg))
    # forward: per point w, per cloud the 30 slots
    wv = w.cpu().numpy().astype(np.float64)
    past = np.arange(n)[None, :] >= K["rows"][:, None]
    assert (wv[past] == 0).all(), "rows past a cloud's own count must report w_out 0"
    fr, fB = ref["fwd"]
    R.check_points(wv[cl, pt][:, None], fr[:, :1], fB[:, :1], what + " w_out", families={"w": [0]}, record=record)
    S, SB, _ = R.sums_by(cl, N, fr[:, 1:], fB[:, 1:], ar.u)
    got = part.cpu().numpy().astype(np.longdouble).sum(1).astype(np.float64)[:, :R.NACC]
    R.check_points(got, S, SB, what + " slot sums", families={"slots": list(range(30))}, record=record)
    assert (got[2] == 0).all() and got[3, R.ACC_SUMW] == 0, "an empty cloud and a cloud that is not alive carry no weight"
    # backward: per point gsrc and gw, per target row gtgt, per cloud the pose sums
    br, bB = ref["bwd"]
    g = np.concatenate((gsrc.cpu().numpy().astype(np.float64)[cl, pt], gw.cpu().numpy().astype(np.float64)[cl, pt][:, None]), 1)
    R.check_points(g, br[:, [0, 1, 2, 9]], bB[:, [0, 1, 2, 9]], what + " gsrc, gw", families={"gsrc": [0, 1, 2], "gw": [3]}, record=record)
    assert (gsrc.cpu().numpy()[past] == 0).all() and (gw.cpu().numpy()[past] == 0).all()
    cv = 6 if cfg["mode"] == "pt2pl" else 3
    T, TB, D = R.sums_by(cl * m + row, N * m, br[:, 3:3 + cv], bB[:, 3:3 + cv], ar.u)
    gt = gtgt.cpu().numpy().astype(np.float64).reshape(N * m, -1)
    assert D.max() >= 2, "some target rows must be matched more than once"
    assert (gt[D == 0] == 0).all() and (gt[:, cv:] == 0).all()
    R.check_points(gt[:, :cv], T, TB, what + " gtgt", families={"gtgt": [0, 1, 2]} if cv == 3 else {"gtgt": [0, 1, 2], "gnormal": [3, 4, 5]}, record=record)
    Ps, PB, _ = R.sums_by(cl, N, br[:, 10:22], bB[:, 10:22], ar.u)
    gotp = bpart.cpu().numpy().astype(np.longdouble).sum(1).astype(np.float64)[:, :12]
    R.check_points(gotp, Ps, PB, what + " pose sums", families={"pose": list(range(12))}, record=record)
    _note("block_sums n=%d" % n, dtype, record)


# ---------------------------------------------------------------- the stand-alone loss weight
@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_loss_weight(gpu, dtype, r):
    """dicp_loss_weight / dicp_loss_weight_bwd through dicp_amd.loss.loss: huber, cauchy and trim, differentiable and hard, both metric pairs, on random
    rows and on the edge rows (zero residual, exactly the metric, saturated, 1e-20 / 1e-30 / 1e20), each within its bound."""
    record, ties = {}, []
    R.run_loss(gpu, dtype, r, record, ties)
    _note("loss_weight r=%d" % r, dtype, record, ties)
