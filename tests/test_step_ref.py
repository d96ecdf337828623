"""tests/step_ref.py -- the float64 model the GPU tests hold dicp_step / dicp_step_bwd / dicp_loop_init to -- checked on the CPU:

  * against the g++ build of csrc/dicp_math.h (tests/hostcheck: hc_step_forward / hc_step_backward), with the model's own bounds;
  * against a second route (torch.linalg + torch.matrix_exp autograd in float64);
  * its comparators refuse wrong variants: a dropped last partial block, an unrounded delta, R for R^T, r + dr, the dim-2 system at slots 0:3,
    an adjoint without its G_A^T half;
  * the motion-bound property (motion_check) passes the formulas as written on an emulated run and refuses 0.999 for 1.0001, a dropped
    radius term, a dropped p0 term 2.5 km out, and e built with 1 ulp instead of 8.
"""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_ref as S  # noqa: E402
from point_math_ref import load_hostcheck  # noqa: E402

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
F32, F64 = np.float32, np.float64


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def io_of(T, dim, pose, **kw):
    io = dict(T=T, dim=dim, iter=0, const_iter=1, tolerance=0.0, pose_in=pose, cost_prev=None, alive=1.0, converged=0, iterations=0.0,
              matched_ratio=0.0, n_start=10.0, weights=False, w_copied=0, frame=None)
    io.update(kw)
    return io


def cases(T, dims=(2, 3), nblks=(1, 3, 17)):
    rng = np.random.RandomState(5)
    for dim in dims:
        for nblk in nblks:
            for ia, ang in enumerate(S.ANGLES):
                d = S.delta_star(rng, ang, (0.01, 1.0, 50.0)[ia % 3], dim)
                yield dim, nblk, d, S.make_partials(rng, nblk, T, dim, d, S.KAPPAS[T][ia % 3]), S.random_pose(rng, T)


def all_ok(res):
    return all(v[0] for v in res.values())


# ------------------------------------------------------------------ the model against the g++ build of the shared header
@needs_gxx
def test_model_holds_the_host_build_forward_and_backward():
    hc = load_hostcheck()
    rng = np.random.RandomState(11)
    worst = {}
    for dim, nblk, d, parts, pose in cases(F64):
        io = io_of(F64, dim, pose)
        ref = S.step_model(parts, io)
        acc = np.ascontiguousarray(ref["sums"][:30])
        C, r = np.ascontiguousarray(pose[:9]), np.ascontiguousarray(pose[9:])
        d6, Cn, rn, Areg = np.zeros(6), np.zeros(9), np.zeros(3), np.zeros(36)
        hc.hc_step_forward(ptr(acc), dim, ptr(C), ptr(r), ptr(d6), ptr(Cn), ptr(rn), ptr(Areg))
        got = {"cost": ref["cost"], "n_matched": ref["n_matched"], "areg": Areg, "delta": d6, "pose_out": np.concatenate([Cn, rn])}
        res = S.hold_forward(got, parts, io)
        assert all_ok(res), (dim, nblk, res)
        g_in, bp = rng.normal(size=12), rng.normal(size=(nblk, 16))
        g = S.sums4(bp[:, :12]) + g_in
        Gs, gb, gC, gr = np.zeros(36), np.zeros(6), np.zeros(9), np.zeros(3)
        hc.hc_step_backward(ptr(np.ascontiguousarray(g[:9])), ptr(np.ascontiguousarray(g[9:])), dim, ptr(C), ptr(d6), ptr(Areg), ptr(Gs), ptr(gb), ptr(gC), ptr(gr))
        resb = S.hold_backward({"gs": Gs, "gb": gb, "gpose": np.concatenate([gC, gr])}, g_in, bp, dim, pose, d6, Areg, F64)
        assert all_ok(resb), (dim, nblk, resb)
        for k, v in list(res.items()) + list(resb.items()):
            worst[k] = max(worst.get(k, 0.0), v[1])
    print("largest |error| / bound against the host build:", {k: "%.3g" % v for k, v in worst.items()})


@needs_gxx
def test_host_build_zero_pivot_and_all_zero_partials():
    hc = load_hostcheck()
    pose = S.random_pose(np.random.RandomState(2), F64)
    parts = S.ill_partials(None, "zeros", F64)
    ref = S.step_model(parts, io_of(F64, 3, pose))
    assert np.all(ref["delta"] == 0) and np.array_equal(ref["pose_out"], pose)
    d6, Cn, rn, Areg = np.ones(6), np.zeros(9), np.zeros(3), np.zeros(36)
    hc.hc_step_forward(ptr(np.zeros(30)), 3, ptr(np.ascontiguousarray(pose[:9])), ptr(np.ascontiguousarray(pose[9:])), ptr(d6), ptr(Cn), ptr(rn), ptr(Areg))
    assert np.all(d6 == 0) and np.array_equal(np.concatenate([Cn, rn]), pose)
    sing = np.zeros((6, 6))
    sing[:5, :5] = S.spd(np.random.RandomState(3), 5, 10.0)            # an exactly zero last pivot
    g = np.random.RandomState(4).normal(size=12)
    res = S.step_bwd_model(g, None, 3, pose, np.zeros(6), sing.ravel())
    assert np.all(res["gs"] == 0) and np.all(res["gb"] == 0)
    Gs, gb, gC, gr = np.ones(36), np.ones(6), np.zeros(9), np.zeros(3)
    hc.hc_step_backward(ptr(np.ascontiguousarray(g[:9])), ptr(np.ascontiguousarray(g[9:])), 3, ptr(np.ascontiguousarray(pose[:9])), ptr(np.zeros(6)),
                        ptr(np.ascontiguousarray(sing.ravel())), ptr(Gs), ptr(gb), ptr(gC), ptr(gr))
    assert all_ok(S.hold_backward({"gs": Gs, "gb": gb, "gpose": np.concatenate([gC, gr])}, g, None, 3, pose, np.zeros(6), sing.ravel(), F64))


# ------------------------------------------------------------------ the model against a second route
def test_model_agrees_with_a_second_route():
    """torch.linalg.solve + torch.matrix_exp forward, explicit inverse + matrix_exp autograd backward.  torch.matrix_exp is itself only good to
    ~4e-12 (tests/test_math_hostcheck.py): the rotation is compared at 1e-10, the rest at the conditioning of the systems (kappa <= 1e6)."""
    rng = np.random.RandomState(17)
    for dim, nblk, d, parts, pose in cases(F64, nblks=(3,)):
        io = io_of(F64, dim, pose)
        ref = S.step_model(parts, io)
        sl = S.slots(dim)
        D = len(sl)
        Ar = torch.tensor(ref["areg"].reshape(6, 6)[:D, :D])
        x = -torch.linalg.solve(Ar, torch.tensor(ref["sums"][S.ACC_B:S.ACC_B + 6][sl])).numpy()
        assert np.abs(x - ref["delta"][sl]).max() <= 2 * S.solve_bound(Ar.numpy(), x)
        ph = ref["delta"][:3]
        K = torch.tensor([[0, -ph[2], ph[1]], [ph[2], 0, -ph[0]], [-ph[1], ph[0], 0]])
        Cn = torch.matrix_exp(K).numpy().T @ pose[:9].reshape(3, 3)
        np.testing.assert_allclose(ref["pose_out"][:9].reshape(3, 3), Cn, rtol=0, atol=1e-10)
        np.testing.assert_array_equal(ref["pose_out"][9:], pose[9:] - ref["delta"][3:])
        g = rng.normal(size=12)
        a = S.step_bwd_model(g, None, dim, pose, ref["delta"], ref["areg"])
        b = S.step_bwd_model(g, None, dim, pose, ref["delta"], ref["areg"], route="second")
        for k in ("gs", "gb", "gpose"):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-8, atol=1e-9 * max(1.0, np.abs(a[k]).max()), err_msg=k)


# ------------------------------------------------------------------ the comparators refuse wrong variants
def wrong_outputs(parts, io, wrong):
    w = S.step_model(parts, io, wrong=wrong)
    return {"cost": w["cost"], "n_matched": w["n_matched"], "areg": w["areg"], "delta": w["delta_applied"], "pose_out": w["pose_out"]}


@pytest.mark.parametrize("T", [F32, F64])
def test_the_right_rule_passes_its_own_comparator(T):
    for dim, nblk, d, parts, pose in cases(T):
        io = io_of(T, dim, pose)
        assert all_ok(S.hold_forward(wrong_outputs(parts, io, None), parts, io))


@pytest.mark.parametrize("T", [F32, F64])
@pytest.mark.parametrize("wrong,dims,nblks,family", [("drop_last_block", (2, 3), (1, 3, 17), ("cost", "areg")), ("R_not_RT", (2, 3), (3,), ("pose_C",)),
                                                     ("r_plus", (2, 3), (3,), ("pose_r",)), ("dim2_slots_0_3", (2,), (3,), ("areg", "delta_off_slots"))])
def test_forward_comparator_refuses(T, wrong, dims, nblks, family):
    seen = 0
    for dim, nblk, d, parts, pose in cases(T, dims, nblks):
        if wrong == "R_not_RT" and np.abs(d[:3]).max() < 1e-3:
            continue                                   # (R = R^T to rounding at the smallest angles: nothing to refuse)
        io = io_of(T, dim, pose)
        res = S.hold_forward(wrong_outputs(parts, io, wrong), parts, io)
        assert any(not res[f][0] for f in family), (wrong, dim, nblk, res)
        seen += 1
    assert seen


def test_forward_comparator_refuses_an_unrounded_float32_delta():
    """the reference rounds delta to the cloud type BEFORE it moves the pose: a pose moved by the float64 step is off by up to half a float32
    ulp of delta -- which r' = r - delta[3:], held bit for bit, shows whenever the stored delta is not the applied one"""
    bad = seen = 0
    for dim, nblk, d, parts, pose in cases(F32, nblks=(3,)):
        io = io_of(F32, dim, pose)
        w = S.step_model(parts, io, wrong="unrounded_delta")
        got = {"cost": w["cost"], "n_matched": w["n_matched"], "areg": w["areg"], "delta": w["delta"], "pose_out": w["pose_out"]}     # (stores the rounded step, applies the exact one)
        res = S.hold_forward(got, parts, io)
        seen += 1
        bad += not all_ok(res)
    assert bad >= seen // 2, (bad, seen)              # (refused wherever the unrounded step rounds the pose differently: most clouds)


def test_backward_comparator_refuses_a_missing_transpose_half():
    rng = np.random.RandomState(23)
    for dim, nblk, d, parts, pose in cases(F64, nblks=(5,)):
        ref = S.step_model(parts, io_of(F64, dim, pose))
        g, bp = rng.normal(size=12), rng.normal(size=(nblk, 16))
        good = S.step_bwd_model(g, bp, dim, pose, ref["delta"], ref["areg"])
        assert all_ok(S.hold_backward({"gs": good["gs"], "gb": good["gb"], "gpose": good["gpose"]}, g, bp, dim, pose, ref["delta"], ref["areg"], F64))
        bad = S.step_bwd_model(g, bp, dim, pose, ref["delta"], ref["areg"], wrong="no_transpose_half")
        res = S.hold_backward({"gs": bad["gs"], "gb": bad["gb"], "gpose": bad["gpose"]}, g, bp, dim, pose, ref["delta"], ref["areg"], F64)
        assert not res["gs"][0], (dim, res)
        drop = S.step_bwd_model(g, bp[:-1], dim, pose, ref["delta"], ref["areg"])                 # ... and a dropped last block of the pose sums
        res = S.hold_backward({"gs": drop["gs"], "gb": drop["gb"], "gpose": drop["gpose"]}, g, bp, dim, pose, ref["delta"], ref["areg"], F64)
        assert not res["gr"][0]


def test_frame_pose_is_one_rounding_per_fused_step():
    rng = np.random.RandomState(31)
    for T in (F32, F64):
        pose = S.random_pose(rng, T, trans=300.0)
        assert np.array_equal(S.frame_pose(None, pose, T), pose)
        Ft = S.rT(np.concatenate([np.eye(3).ravel(), rng.normal(size=3) * 100]), T)
        out = S.frame_pose(Ft, pose, T)
        assert np.array_equal(out[:9], pose[:9]) and np.array_equal(out[9:], S.rT(pose[9:] + Ft[9:], T))
        Fr = S.rT(np.concatenate([S.rotation(rng).ravel(), rng.normal(size=3) * 100]), T)
        out = S.frame_pose(Fr, pose, T)
        exact = np.concatenate([(Fr[:9].reshape(3, 3) @ pose[:9].reshape(3, 3)).ravel(), Fr[:9].reshape(3, 3) @ pose[9:] + Fr[9:]])
        assert np.all(np.abs(out - exact) <= 3 * S.ulp(np.abs(exact) + 400.0, T))
    assert S.fma(1 + 2.0 ** -12, 1 + 2.0 ** -12, -1.0, F32) == float(F32(2.0 ** -11 + 2.0 ** -24))        # (the product's low bits survive)


# ------------------------------------------------------------------ the motion bound
def emulate(rng, T, offset, extent, frame_kind, n=500, step_scale=1.0, **model):
    """dicp_loop_init + 8 x dicp_step in numpy: the poses (rounded to T like the kernel's), the search poses, rmax and dcum of motion_model"""
    src = S.rT(rng.uniform(-0.5, 0.5, size=(n, 3)) * extent + offset * np.array([0.6, -0.64, 0.48]), T)
    centre = S.rT(src.mean(0) + rng.normal(size=3), T)
    if frame_kind == "none":
        frame = None
    else:
        Q = np.eye(3) if frame_kind == "translation" else S.rT(S.rotation(rng), T).reshape(3, 3)
        frame = S.rT(np.concatenate([Q.ravel(), -Q @ centre]), T)
    poses = [S.rT(np.concatenate([S.rotation(rng, 0.2).ravel(), rng.normal(size=3) + 0.05 * offset]), T)]
    for k in range(8):
        d = step_scale * S.delta_star(rng, 0.5 * (1e-6, 1e-3, 0.05, 0.3)[k % 4], 0.5 * (1e-6, 1e-3, 0.05, 0.3)[(k + k // 4) % 4], 3)
        poses.append(S.apply_delta(poses[-1], S.rT(d, T), T))
    poses = np.stack(poses)
    search = np.stack([S.frame_pose(frame, p, T) for p in poses])
    rmax = S.rmax_model(src, T)
    return src, poses, search, S.motion_model(poses, rmax, frame, T, **model)


MOTION_CASES = [(off, ext, fk) for off in (0.0, 300.0, 2500.0, 25000.0) for ext in (1.0, 20.0, 100.0) for fk in ("none", "translation", "rotated")]


@pytest.mark.parametrize("T", [F32, F64])
def test_motion_bound_as_written_holds_on_the_emulation(T):
    rng = np.random.RandomState(41)
    worst = [0.0, 0.0]
    for off, ext, fk in MOTION_CASES:
        src, poses, search, dcum = emulate(rng, T, off, ext, fk)
        w = S.motion_check(src, poses, search, dcum, T)
        worst = [max(a, b) for a, b in zip(worst, w)]
        assert w[0] <= 1.0 and w[1] <= 1.0, (off, ext, fk, w)
        assert np.all(np.diff(dcum[:, 0]) >= 0)
    print("largest lhs / rhs (world, search frame):", worst)
    assert worst[0] > 0.99                            # (the bound is tight: 0.02 % less fails, below)


@pytest.mark.parametrize("T", [F32, F64])
@pytest.mark.parametrize("name,model,which,only", [("0.999 for 1.0001", dict(factor=0.999), 0, None), ("no radius term", dict(radius_term=False), 0, None),
                                                   ("no p0 term 2.5 km out", dict(p0_term=False), 0, 2500.0), ("e from 1 ulp", dict(e_ulps=1.0), 1, None)])
def test_motion_property_refuses(T, name, model, which, only):
    rng = np.random.RandomState(43)
    refused = 0
    for off, ext, fk in MOTION_CASES:
        if only is not None and off != only:
            continue
        # (e only matters where the 0.01 % of slack in M does not cover the rounding of a point: float64 steps of 1e-13 .. 1e-8)
        src, poses, search, dcum = emulate(rng, T, off, ext, fk, step_scale=1e-7 if (which == 1 and T == F64) else 1.0, **model)
        refused += S.motion_check(src, poses, search, dcum, T)[which] > 1.0
    assert refused, name
    if only is not None:                              # (every cloud that far out must show it)
        assert refused == sum(1 for c in MOTION_CASES if c[0] == only)


# ------------------------------------------------------------------ lists, switch, skip verdicts: the rules at their edges
def test_guard_list_model_edges():
    T = F32
    spent = S.cert_spent(0.25, 1e-5, T)
    qu = np.array([np.nextafter(T(spent), T(np.inf)), spent, np.nextafter(T(spent), T(0)), -1.0, np.nan, 5.0], dtype=np.float64)
    ent, sc, upto = S.guard_list_model(3, qu, spent, 0, 6)
    assert ent == [3 * 6 + u for u in (1, 2, 3, 4)]
    assert S.guard_list_model(3, qu, spent, -1, 6)[0] == ent
    for st in (S.CERT_RECERTIFY, 1, 5, S.CERT_OFF_FOR_GOOD):
        assert S.guard_list_model(3, qu, spent, st, 6)[0] == [18 + u for u in range(6)]
        assert S.guard_list_model(3, qu, spent, st, 6, have=70, n=100)[1] == 0
    ent, sc, upto = S.guard_list_model(2, qu, spent, 0, 6, have=65, n=100)
    assert sc == 100 and upto == 100 and [e for e in ent if e < 0] == [-1 - (2 * 2 + 1), -1 - (2 * 2)]
    assert S.guard_list_model(2, qu, spent, 0, 6, have=64, n=100)[1:] == (None, 64)
    assert S.guard_list_model(2, qu, spent, 0, 6, have=0, n=100)[1:] == (None, None)
    assert S.guard_list_model(2, qu, spent, 0, 6, have=105, n=100)[1:] == (None, 100)


def test_cert_state_model_branches():
    O, R = S.CERT_OFF_FOR_GOOD, S.CERT_RECERTIFY
    rows = [  # units again, singles, state, units, back-off, sets, no-cert  -> next
        ((0, 0, 0, 0, 0, 0, 0), 0), ((9, 9, 3, 0, 0, 0, 0), 3),             # no certified iteration ran: untouched
        ((1, 0, 0, 10, 0, 0, 0), 0), ((5, 0, 0, 10, 0, 0, 0), -1), ((0, 60, 0, 10, 0, 0, 0), O), ((0, 60, 0, 10, 0, 1, 0), -1),
        ((5, 0, -1, 10, 0, 0, 0), 2), ((5, 0, -1, 10, 2, 0, 0), 4), ((5, 0, -1, 10, 16, 0, 0), 16), ((0, 60, -1, 10, 0, 1, 0), O), ((1, 0, -1, 10, 0, 0, 0), 0),
        ((0, 0, 3, 10, 4, 0, 0), 2), ((0, 0, 1, 10, 4, 0, 0), R), ((0, 0, O, 10, 0, 0, 0), O),
        ((0, 0, R, 10, 0, 0, 0), 0), ((0, 60, R, 10, 0, 0, 0), O), ((9, 0, R, 10, 0, 1, 0), -1), ((0, 0, R, 10, 0, 1, 0), 0),
        ((0, 0, 0, 10, 0, 1, 400), O), ((0, 0, 0, 10, 0, 1, 300), 0)]
    for (cu, cs, st, un, cb, se, nc), want in rows:
        cc, nxt = S.cert_state_model([cu, cs, st, un, cb, se, nc, 0], n=600)
        assert nxt == want, ((cu, cs, st, un, cb, se, nc), nxt, want)
        if un:
            assert cc[0] == cc[1] == cc[3] == cc[6] == 0 and cc[2] == want


def test_skip_model_verdicts():
    rng = np.random.RandomState(3)
    A = S.spd(rng, 6, 10.0)
    Gs, gb = rng.normal(size=(6, 6)), rng.normal(size=6)
    s = np.sqrt(np.diag(A))
    m = max((np.abs(Gs) * s[:, None] * s[None, :]).max(), (np.abs(gb) * s).max())
    eps = 2.0 ** -22
    assert S.skip_model(Gs, gb, A, np.zeros((0, 6)), 3, True, False, 16 * m / eps * 2, eps) == (2, 16 * m / eps * 2, 0)
    assert S.skip_model(Gs, gb, A, np.zeros((0, 6)), 3, True, False, 16 * m / eps / 2, eps) == (0, 16 * m / eps / 2, 1)
    assert S.skip_model(Gs, gb, A, np.zeros((0, 6)), 3, True, False, 0.0, eps) == (0, m, 1)                  # mref raised
    big = np.full((3, 6), 1e6)                                                                                # an earlier step that large keeps the sweep going
    assert S.skip_model(Gs, gb, A, big, 3, True, False, 16 * m / eps * 2, eps)[0] == 0
    assert S.skip_model(Gs, gb, A, np.zeros((0, 6)), 3, False, False, 1.0, eps) == (1, 1.0, 0)
    assert S.skip_model(Gs, gb, A, np.zeros((0, 6)), 3, True, True, 1.0, eps) == (2, 1.0, 0)
    Gn = Gs.copy()
    Gn[2, 3] = np.nan
    assert S.skip_model(Gn, gb, A, np.zeros((0, 6)), 3, True, False, 1e300, eps) == (0, 1e300, 1)
