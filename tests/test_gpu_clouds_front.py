"""The three forms of a cloud argument -- single clouds, a padded batch with row counts, a list -- give the same results, on the MI355X.

Per operator and dtype: three clouds of 1, 257 (one row past a 256-lane block) and 300 rows from a fixed seed, for the operators that allow
an empty cloud 0 rows in place of the 1.  Every forward output of the batch (row counts on the device and on the CPU) and of the list is
held bit for bit to the calls on each cloud alone, cut to the cloud's own rows, slots or voxels, and so are the same calls on CPU tensors;
container types, dtypes and devices are checked.  The padding of the batch is filled with rows that would be neighbours, be picked or
fill a voxel if a row count were ignored.  One backward per operator on the list form: gradients written once (knn / ball x-gradient, fps,
voxel) bit for bit against the single calls, gradients summed through float atomics within the bars of their own GPU test modules.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.ball import ball_query
from dicp_amd.fps import sample_farthest_points
from dicp_amd.knn import chamfer_distance, knn_points
from dicp_amd.normals import estimate_normals
from dicp_amd.voxel import voxel_downsample

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import walk_layouts as wl  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
K, RADIUS, VOXEL_SIZE = 4, 0.3, 0.25
ROW, SLOT, CLOUD, VOXEL = "row", "slot", "cloud", "voxel"
NORMALS_BAR = {torch.float32: 1e-3, torch.float64: 1e-9}   # tests/test_gpu_normals.py: |batch - single| / |single| per cloud

# name -> (the call on its cloud arguments and row counts, the kind and dtype of every output, two clouds, empty clouds allowed)
OPS = {
    "estimate_normals": (lambda p, rows=None: estimate_normals(p, k=K, rows=rows, return_curvature=True, return_neighbors=True),
                         ((ROW, None), (ROW, None), (ROW, torch.int64)), False, False),
    "voxel_downsample": (lambda p, rows=None: voxel_downsample(p, VOXEL_SIZE, rows=rows, return_counts=True, return_inverse=True),
                         ((VOXEL, None), (CLOUD, torch.int32), (VOXEL, torch.int32), (ROW, torch.int64)), False, False),
    "sample_farthest_points": (lambda p, rows=None: sample_farthest_points(p, K, rows=rows, return_rows=True, return_distances=True),
                               ((SLOT, None), (SLOT, torch.int64), (CLOUD, torch.int32), (SLOT, None)), False, True),
    "knn_points": (lambda x, y, x_rows=None, y_rows=None: knn_points(x, y, k=K, x_rows=x_rows, y_rows=y_rows),
                   ((ROW, None), (ROW, torch.int64)), True, True),
    "chamfer_distance": (lambda x, y, x_rows=None, y_rows=None: (chamfer_distance(x, y, x_rows=x_rows, y_rows=y_rows, reduction="none"),),
                         ((CLOUD, None),), True, True),
    "ball_query": (lambda x, y, x_rows=None, y_rows=None: ball_query(x, y, RADIUS, k=K, x_rows=x_rows, y_rows=y_rows, return_counts=True),
                   ((ROW, None), (ROW, torch.int64), (ROW, torch.int32)), True, True),
}


def _clouds(op, dtype):
    """-> (sizes per argument, clouds per argument (numpy, unit cube), zero-padded-in-name-only batches: the padding holds live-looking rows)"""
    two, empty_ok = OPS[op][2], OPS[op][3]
    first = 0 if empty_ok else 1
    sizes = [(first, 257, 300), (257, 300, first)][:2 if two else 1]
    dt = wl.np_dtype(dtype)
    rng = np.random.default_rng(20261018)
    clouds, batches = [], []
    for a, sz in enumerate(sizes):
        cl = [rng.uniform(0.0, 1.0, (n, 3)).astype(dt) for n in sz]
        pad = rng.uniform(0.0, 1.0, (3, max(sz), 3)).astype(dt)     # would be neighbours / fill voxels
        if op == "sample_farthest_points":
            pad += dt.type(5.0)                                      # would be picked: farther than any live row
        for b, c in enumerate(cl):
            pad[b, :sz[b]] = c
        clouds.append(cl)
        batches.append(pad)
    return sizes, clouds, batches


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _cut(kind, t, n, voxels):
    """an output of one cloud (batch row or single result) -> the part that is the cloud's own"""
    return t if kind == CLOUD else t[:{ROW: n, SLOT: min(K, n), VOXEL: voxels}[kind]]


def _per_cloud(op, outs, form, sizes, b):
    """the outputs of cloud b, cut, from a call in the given form"""
    kinds = OPS[op][1]
    if op == "chamfer_distance":                            # (N,) whatever the form; (1,) for single clouds
        return [outs[0][0 if form == "single" else b]]
    got = [o if form == "single" else o[b] for o in outs]
    voxels = int(got[1]) if op == "voxel_downsample" else None
    return [_cut(kind, t, sizes[0][b], voxels) for (kind, _), t in zip(kinds, got)]


def _check_types(op, outs, form, dtype, device, N):
    kinds = OPS[op][1]
    assert isinstance(outs, tuple) and len(outs) == len(kinds)
    for (kind, dt), o in zip(kinds, outs):
        if form == "list" and op != "chamfer_distance":
            assert isinstance(o, list) and len(o) == N
        else:
            assert isinstance(o, torch.Tensor)
            if form == "batch":
                assert o.shape[0] == N
        for t in (o if isinstance(o, list) else [o]):
            assert isinstance(t, torch.Tensor) and t.dtype == (dt or dtype) and t.device.type == device, (op, form, t.dtype, t.device)


def _forward_all_forms(op, dtype, device):
    """-> per-cloud cut outputs of the single calls; asserts the batch (rows on either device) and the list against them"""
    fn = OPS[op][0]
    sizes, clouds, batches = _clouds(op, dtype)
    T = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    names = ("x_rows", "y_rows") if OPS[op][2] else ("rows",)
    single = []
    for b in range(3):
        outs = fn(*[T(cl[b]) for cl in clouds])
        _check_types(op, outs, "single", dtype, device, 3)
        single.append(_per_cloud(op, outs, "single", sizes, b))
    calls = [("list", fn(*[[T(c) for c in cl] for cl in clouds]))]
    for rows_dev in ("cuda", "cpu"):
        rows = {nm: torch.tensor(sz, device=rows_dev) for nm, sz in zip(names, sizes)}
        calls.append(("batch", fn(*[T(p) for p in batches], **rows)))
    for form, outs in calls:
        _check_types(op, outs, form, dtype, device, 3)
        for b in range(3):
            got = _per_cloud(op, outs, form, sizes, b)
            assert len(got) == len(single[b])
            for i, (g, s) in enumerate(zip(got, single[b])):
                assert _bits(g, s), "%s %s: output %d of cloud %d differs from the call on the cloud alone" % (op, form, i, b)
    return single


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("op", sorted(OPS))
def test_forms_agree_bit_for_bit(op, dtype):
    dev = _forward_all_forms(op, dtype, "cuda")
    cpu = _forward_all_forms(op, dtype, "cpu")
    for b in range(3):
        for g, s in zip(cpu[b], dev[b]):
            assert _bits(g, s)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_output_and_lenient_rows(dtype):
    """estimate_normals with one output returns it bare; it and voxel_downsample take a row count with a single cloud"""
    _, (cl,), _ = _clouds("estimate_normals", dtype)
    p = torch.from_numpy(cl[2]).cuda()
    one = estimate_normals(p, k=K)
    lst = estimate_normals([p, p[:40]], k=K)
    assert isinstance(one, torch.Tensor) and isinstance(lst, list) and _bits(lst[0], one)
    cut = estimate_normals(p, k=K, rows=torch.tensor([[257]]))
    assert _bits(cut[:257], estimate_normals(p[:257], k=K)) and bool((cut[257:] == 0).all())
    cent, rows = voxel_downsample(p, VOXEL_SIZE, rows=[257])
    ref, ref_rows = voxel_downsample(p[:257], VOXEL_SIZE)
    assert _bits(cent, ref) and _bits(rows, ref_rows)


def _cotangents(shapes, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen, dtype=torch.float64).to(dtype).cuda() for s in shapes]


def _backward(op, args, cots_of):
    """op on leaf copies of args (tensors or lists of tensors) -> (outputs, the leaves' gradients in the same nesting); cots_of(outs) gives
    the (output, cotangent) pairs to run backward from"""
    leaves = [[t.clone().requires_grad_(True) for t in a] if isinstance(a, list) else a.clone().requires_grad_(True) for a in args]
    outs = OPS[op][0](*leaves)
    pairs = [(o, c) for o, c in cots_of(outs) if o.numel()]
    if pairs:
        torch.autograd.backward([o for o, _ in pairs], [c for _, c in pairs])
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)  # noqa: E731
    return outs, [[zero(t) for t in a] if isinstance(a, list) else zero(a) for a in leaves]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("op", ["estimate_normals", "voxel_downsample", "sample_farthest_points", "knn_points", "ball_query"])
def test_list_backward_against_single_calls(op, dtype):
    sizes, clouds, _ = _clouds(op, dtype)
    T = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    diff = {"estimate_normals": (0, 1), "voxel_downsample": (0,), "sample_farthest_points": (0, 3), "knn_points": (0,), "ball_query": (0,)}[op]
    diff = diff[:1] if op == "sample_farthest_points" else diff       # (the distances carry no gradient)
    plain = OPS[op][0](*[[T(c) for c in cl] for cl in clouds])       # the shapes of the list form's outputs
    cots = {i: _cotangents([plain[i][b].shape for b in range(3)], dtype, 100 + i) for i in diff}
    outs, grads = _backward(op, [[T(c) for c in cl] for cl in clouds], lambda o: [(o[i][b], cots[i][b]) for i in diff for b in range(3)])
    for b in range(3):
        souts, sgrads = _backward(op, [T(cl[b]) for cl in clouds], lambda o: [(_per_cloud(op, o, "single", sizes, b)[i], cots[i][b]) for i in diff])
        gx, sx = grads[0][b], sgrads[0]
        if op == "estimate_normals":
            ref = float(sx.double().norm())
            err = float((gx.double() - sx.double()).norm())
            print("estimate_normals cloud %d: |list - single| = %.3e of %.3e" % (b, err, ref))
            assert (err < NORMALS_BAR[dtype] * ref) if ref > 0 else err == 0
            continue
        assert _bits(gx, sx), "%s: the gradient of cloud %d differs from the call on the cloud alone" % (op, b)
        if len(clouds) == 2 and clouds[1][b].shape[0] == 0:
            assert bool((gx == 0).all()) and grads[1][b].numel() == 0
        elif len(clouds) == 2:                              # the y-gradient: float atomics, against the float64 terms of the kernel's lists
            idx = outs[1][b].cpu().numpy()
            g = cots[0][b].cpu().numpy()
            X, Y = clouds[0][b], clouds[1][b]
            Sx, Bx, Sy, By, D = wl.knn_grad_terms(X, Y, idx, g, dtype)
            if op == "ball_query":                          # tests/test_gpu_ball.py: (terms + 1) u sum |t|; knn_points: (D + 2) u sum |t|
                By = By * ((D + 1) / (D + 2))[:, None]
            gy = grads[1][b].cpu().numpy()
            assert np.all(gy[D == 0] == 0)
            r = wl.assert_within(gy, Sy, By, "%s cloud %d y-gradient" % (op, b))
            print("%s cloud %d: y-gradient worst error / bound %.3f, in-degree up to %d" % (op, b, r, int(D.max()) if D.size else 0))
