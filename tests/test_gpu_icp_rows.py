"""ICP.icp(..., source_rows=, target_rows=[, weight=]) -- the entry every operator that returns a padded batch with row counts feeds registration
through -- against the float64 oracle, cloud by cloud on the cloud's own rows (tests/icp_rows_ref.py: the inputs, the reference and why its inputs can
carry these bars; tests/test_icp_rows_ref.py shows that on the CPU).  `-m gpu`.

Bars: those of tests/test_gpu_parity.py.  float64: pose, deltas, pc 1e-10; weights 1e-9; costs rtol 1e-7; gradients rtol 1e-8 + 1e-9.  float32 against
the float64 reference, on the clouds clear of a hard decision: pose, deltas 1e-4; weights 2e-3; gradients 1e-3 x the gradient's scale; pc = C p + r
within what the pose bar allows, 1e-4 (1 + |p|_1).  Statistics: converged and iterations exactly, matched_ratio 1e-7.  On the pads: gradients and the
weights history exactly 0; nothing returned for a real row is non-finite."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_rows_ref as R  # noqa: E402

from dicp_amd import _lib  # noqa: E402
from dicp_amd.ICP import ICP  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

# how the search and the backward are forced (tests/test_gpu_ragged.py, tests/test_gpu_configs.py)
PATHS = {
    "auto": {},
    "valu": dict(knn_variant=_lib.KNN_VALU),
    "mfma": dict(knn_variant=_lib.KNN_MFMA),                                       # (float32 only)
    "sweep": dict(knn_variant=_lib.KNN_SWEEP, bwd_window=True, reuse_matches=True),
    "sweep-atomic": dict(knn_variant=_lib.KNN_SWEEP, bwd_window=False, reuse_matches=True),
    "sweep-cfg2": dict(knn_variant=_lib.KNN_SWEEP | (2 << 8), bwd_window=True),
    "sweep-cfg2-atomic": dict(knn_variant=_lib.KNN_SWEEP | (2 << 8), bwd_window=False),
    "sweep-no-reuse": dict(knn_variant=_lib.KNN_SWEEP, reuse_matches=False),
    "deterministic": dict(deterministic=True),
}
ALL = list(R.CASES)
F64 = [(p, c) for p in PATHS if p != "mfma" for c in ALL]


def npy(x):
    return x.detach().cpu().numpy()


def run(name, dtype, path="auto", rows_as="int32", batch_on="cuda"):
    """The library on the padded batch with row counts -> (out, leaves): leaves = the tensors whose .grad the loss sum(T gT) + sum over own rows (pc gpc) filled."""
    c, d = R.CASES[name], R.batch()
    cols = 6 if c.icp_type == "pt2pl" else 3
    put = lambda x: x.clone().to(dtype).to(batch_on).contiguous().requires_grad_(True)       # noqa: E731  (a leaf of its own: the batch is shared)
    src, tgt, T0 = put(d["source"]), put(d["target"][:, :, :cols]), put(d["T_init"])
    w = None if c.weight == "none" else put(R.weight_of(c))
    icp = ICP(icp_type=c.icp_type, differentiable=c.diff, max_iterations=c.K, tolerance=c.tol)
    icp.const_iter, icp.match_ratio_thresh = (c.mode == "const"), c.thresh
    for k, v in PATHS[path].items():
        setattr(icp, k, v)
    form = {"list": lambda v: list(v), "int32": lambda v: torch.tensor(v, dtype=torch.int32, device=DEV), "int64": lambda v: torch.tensor(v, dtype=torch.int64, device=DEV),
            "cpu": lambda v: torch.tensor(v, dtype=torch.int64)}[rows_as]
    out = icp.icp(src, tgt, T0, weight=w, trim_dist=c.trim, loss_fn=R.LOSSES[c.loss], dim=c.dim, source_rows=form(R.LS), target_rows=form(R.LT))
    gT, gpc = d["gT"].to(dtype).to(batch_on), d["gpc"].to(dtype).to(batch_on)
    loss = (out["T"] * gT).sum()
    for b in range(R.N):                                           # (a cloud's own rows only: what pc holds on a pad row is the pad's business)
        loss = loss + (out["pc"][b, :R.LS[b]] * gpc[b, :R.LS[b]]).sum()
    loss.backward()
    return out, dict(source=src, target=tgt, weight=w, T_init=T0)


def check(name, out, leaves, f64, tally=None):
    """Every output of the call against the per-cloud reference; -> the largest error of each kind, for the record."""
    c, ref = R.CASES[name], R.reference(name)
    rows = 3 if c.icp_type == "pt2pt" else 1
    held = np.ones(R.N, dtype=bool) if f64 else R.float32_held(name)
    if tally is not None:
        tally[0], tally[1] = tally[0] + int(held.sum()), tally[1] + int((~held).sum())
    K_run = max(int(r["iterations"]) for r in ref)
    assert out["deltas"].shape == (R.N, K_run, 6, 1) and out["costs"].shape == (R.N, K_run, 1) and out["weights"].shape == (R.N, K_run, R.N_PAD * rows, 1)
    assert out["pc"].shape == (R.N, R.N_PAD, 3) and out["T"].shape == (R.N, 4, 4)
    grads = {k: (None if v is None else npy(v.grad)) for k, v in leaves.items()}
    res = {k: npy(out[k]) for k in ("T", "pc", "deltas", "costs", "weights")}
    stats = {k: npy(v) for k, v in out["stats"].items()}
    worst = {}

    def close(tag, got, want, atol, rtol=0.0):
        want = np.asarray(want)
        worst[tag] = max(worst.get(tag, 0.0), float(np.max(np.abs(got - want) - rtol * np.abs(want), initial=0.0)))
        np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg="%s: %s of cloud %d" % (name, tag, b))

    gscale = {k: max([1.0] + [float(r["grad_" + k].abs().max()) for r in ref if r["grad_" + k] is not None]) for k in grads}
    for b, r in enumerate(ref):
        n, m, k = R.LS[b], R.LT[b], int(r["iterations"])
        # nothing returned for a real row is non-finite; the pads: weights history and gradients exactly 0
        for key, a in (("T", res["T"][b]), ("pc", res["pc"][b, :n]), ("deltas", res["deltas"][b]), ("costs", res["costs"][b]), ("weights", res["weights"][b, :, :n * rows]),
                       ("grad source", grads["source"][b, :n]), ("grad target", grads["target"][b, :m]), ("grad T_init", grads["T_init"][b]),
                       ("matched_ratio", stats["matched_ratio"][b]), ("iterations", stats["iterations"][b])):
            assert np.isfinite(a).all(), (name, b, key)
        assert (res["weights"][b, :, n * rows:] == 0).all(), (name, b, "weights history on the pads")
        assert (grads["source"][b, n:] == 0).all() and (grads["target"][b, m:] == 0).all(), (name, b, "gradient on the pads")
        if c.weight != "none":
            assert np.isfinite(grads["weight"][b, :n]).all() and (c.weight == "cloud" or (grads["weight"][b, n:] == 0).all()), (name, b, "weight gradient")
        if not held[b]:
            continue
        assert bool(stats["converged"][b]) == r["converged"] and float(stats["iterations"][b]) == r["iterations"], (name, b, stats["converged"][b], stats["iterations"][b], r["iterations"])
        close("matched_ratio", stats["matched_ratio"][b], r["matched_ratio"], 1e-7)
        close("T", res["T"][b], r["T"], 1e-10 if f64 else 1e-4)
        close("deltas", res["deltas"][b, :k], r["deltas"], 1e-10 if f64 else 1e-4)
        close("weights", res["weights"][b, :k, :n * rows], r["weights"], 1e-9 if f64 else 2e-3)
        if f64:
            close("costs", res["costs"][b, :k], r["costs"], 1e-10, rtol=1e-7)
            close("pc", res["pc"][b, :n], r["pc"], 1e-10)
        else:
            lever = 1.0 + np.abs(npy(R.batch()["source"][b, :n])).sum(axis=1, keepdims=True)
            worst["pc"] = max(worst.get("pc", 0.0), float(np.max(np.abs(res["pc"][b, :n] - npy(r["pc"])) / lever)))
            assert (np.abs(res["pc"][b, :n] - npy(r["pc"])) <= 1e-4 * lever).all(), (name, b, "pc")
        for key in ("source", "target", "weight", "T_init"):
            want = r["grad_" + key]
            if want is None:
                continue
            got = grads[key][b, :{"source": n, "target": m, "weight": n if c.weight == "point" else 1, "T_init": 4}[key]]
            if f64:
                close("grad " + key, got, want, 1e-9, rtol=1e-8)
            else:
                close("grad " + key, got, want, 1e-3 * gscale[key])
    print("%-46s %s" % (name, " ".join("%s %.1e" % kv for kv in worst.items())))
    return worst


@pytest.mark.parametrize("path,name", F64)
def test_float64_equals_the_per_cloud_oracle(path, name):
    out, leaves = run(name, torch.float64, path)
    check(name, out, leaves, True)


@pytest.mark.parametrize("path", ["auto", "valu", "mfma", "sweep", "sweep-atomic", "sweep-cfg2", "deterministic"])
def test_float32_meets_the_north_star_on_every_case(path):
    """float32 kernels against the float64 reference.  A cloud whose float64 run passes within 1e-4 of a hard decision (the argmin, a hard trim / Huber
    branch, the count threshold) may take the other side: left out, and the clouds held are at least 5x those (tests/test_gpu_parity.py's rule and cap)."""
    tally = [0, 0]
    for name in ALL:
        out, leaves = run(name, torch.float32, path)
        check(name, out, leaves, False, tally)
    assert tally[0] >= 5 * tally[1], tally


@pytest.mark.parametrize("rows_as,batch_on", [("list", "cuda"), ("int64", "cuda"), ("cpu", "cuda"), ("int32", "cpu"), ("list", "cpu")])
def test_every_form_of_the_row_counts_and_a_cpu_batch(rows_as, batch_on):
    """Row counts as a Python list, an int32 / int64 device tensor or a CPU tensor, the batch on the device or on the CPU: the same call -- the oracle's results in every form, and
    the statistics of the int32 device form bit for bit."""
    name = "pl-diff-3-huber-trim-tol-t0.3-point"
    out, leaves = run(name, torch.float64, "sweep", rows_as, batch_on)
    assert out["T"].device.type == batch_on and out["stats"]["iterations"].device.type == batch_on and leaves["source"].grad.device.type == batch_on
    check(name, out, leaves, True)
    base, _ = run(name, torch.float64, "sweep")
    for key in ("converged", "iterations", "matched_ratio"):
        assert torch.equal(out["stats"][key].cpu(), base["stats"][key].cpu()), key


def test_what_the_pad_rows_of_the_results_hold():
    """The docstring's word on the pads of what the call returns: `weights` 0 in every iteration; `pc` the pad row itself under the final pose -- NaN for
    a NaN row, and bit for bit the cloud's own pc where the pad is a copy of one of its rows."""
    name = "pl-diff-3-huber-trim-const-t0-none"
    out, _ = run(name, torch.float64, "sweep")
    d = R.batch()
    for b in range(R.N):
        n = R.LS[b]
        pad = out["pc"][b, n:].cpu()
        assert bool((out["weights"][b, :, n:] == 0).all())
        if R.SRC_PAD[b] == "nan":
            assert bool(torch.isnan(pad).all())
        elif R.SRC_PAD[b] == "copy":
            assert torch.equal(pad, out["pc"][b, torch.arange(R.N_PAD - n) % n].cpu())
        elif R.SRC_PAD[b] == "big":
            want = d["source"][b, n:] @ out["T"][b, :3, :3].cpu().T + out["T"][b, :3, 3].cpu()
            assert bool(((pad - want).abs() <= 1e-12 * want.abs()).all())
