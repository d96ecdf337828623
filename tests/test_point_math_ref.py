"""CPU side of the operator-level check of the per-point arithmetic (no GPU).

The g++ build of csrc/dicp_math.h (tests/hostcheck: correctly rounded sqrtf, '/', tanhf -- NOT the one-instruction forms the device ships) is held
to the float64 reference of tests/point_math_ref.py within that module's error model, with the constants of the correctly rounded forms, at safety
factor 1, over the whole configuration grid and every edge set, forward and backward, float32 and float64: this proves the model before any GPU
time is spent.  tests/test_gpu_point_math.py runs the same checks against the kernels with the device's constants.

Also here: the reference is pinned to the reference semantics (the oracle's loss_weight and skew; the real reference's loss in
tests/golden/loss_vectors_f32.npz); the comparator refuses a reference with one perturbed intermediate, a dropped or halved term, a NaN, and a tie
answered with a mixture; the model's list of operations is held to the sources; the inputs of the GPU tests contain no tie.
"""
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_math_ref as R  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "dicp_amd", "csrc")
DTYPES = [np.float32, np.float64]
dtype_id = lambda d: np.dtype(d).name


@pytest.fixture(scope="module")
def host():
    return R.HostBackend(R.load_hostcheck())


@pytest.fixture(autouse=True)
def _threads():
    before = torch.get_num_threads()
    torch.set_num_threads(4)
    yield
    torch.set_num_threads(before)


def _note(test, dtype, record, ties=()):
    import json
    path = os.environ.get("DICP_RECORD_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(test=test, dtype=np.dtype(dtype).name, ratios=record, ties=list(ties))) + "\n")


# ---------------------------------------------------------------- the host build within the model, whole grid, all edge sets
@pytest.mark.parametrize("cfg", R.grid(), ids=R.cfg_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_host_build_within_model(host, dtype, cfg):
    record, ties = {}, []
    R.run_config(host, dtype, cfg, 512, record, ties)
    _note("host points_grid " + R.cfg_id(cfg), dtype, record, ties)


def _has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return False


@pytest.fixture(scope="module")
def host_contracted():
    """the same header with a * b + c contracted into one rounding, as the device build does (-ffp-contract=on there): other roundings, same model"""
    import hostbuild
    return R.HostBackend(hostbuild.build("hostcheck.cpp", "hostcheck_fma", ("-mfma", "-ffp-contract=fast")))


@pytest.mark.skipif(not _has_fma(), reason="this CPU has no fused multiply-add")
@pytest.mark.parametrize("cfg", R.grid(), ids=R.cfg_id)
def test_contracted_float64_build_within_model(host_contracted, cfg):
    """In float64 the plain g++ build repeats the reference's own operations and agrees with it almost bit for bit, which says nothing about the bound.
    A build with fused multiply-adds rounds differently from the reference, as the device does: it must lie within the bound, which for that reason
    carries the reference's own float64 rounding as well (point_math_ref: THE REFERENCE'S OWN ERROR).  At the GPU tests' size, random points."""
    R.run_config(host_contracted, np.float64, cfg, R.GPU_POINTS, edges=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_host_gate_tail(host, dtype):
    for cfg in R.grid():
        if cfg["diff"] and (cfg["trim_on"] or cfg["loss"] == "trim"):
            R.run_gate_tail(host, dtype, cfg)


@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_host_loss_weight_within_model(host, dtype, r):
    record, ties = {}, []
    R.run_loss(host, dtype, r, record, ties)
    _note("host loss_weight r=%d" % r, dtype, record, ties)


# ---------------------------------------------------------------- the reference is the reference
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_chain_equals_the_reference_semantics(dtype):
    """The operation-by-operation chain (closed forms of J^T J, slot layout) against the tensor expressions of ICP.py:137-201 written with the oracle's
    loss_weight and skew: the same float64 values up to the rounding of two evaluation orders (1e-13 of the largest value of a point)."""
    ar = R.Arith(dtype, "host")
    for cfg in R.grid():
        inp, _ = R.random_case(dtype, cfg, 128)
        with torch.no_grad():
            a = R.Chain(ar, cfg, inp).forward_outputs().numpy()
        b = R.semantic_forward(cfg, inp, ar).numpy()
        assert (np.abs(a - b) <= 1e-13 * np.maximum(1.0, np.abs(b).max(1, keepdims=True))).all(), R.cfg_id(cfg)


def test_loss_reference_is_the_real_reference(golden):
    """tests/golden/loss_vectors_f32.npz (the reference's own loss on float32-rounded edge inputs): its float64 outputs pin LossChain, its float32 outputs
    (torch's CPU kernels, also 0.5-ulp operations and a tanh within 2 ulp) are held to the model like any other build."""
    g = golden("loss_vectors_f32")
    a64, a32 = R.Arith(np.float64, "host"), R.Arith(np.float32, "host")
    for name, metric in (("huber", 1.0), ("cauchy", 0.5), ("trim", 2.0)):
        for diff in (True, False):
            for tag in ("e1", "e3"):
                e = torch.tensor(g["%s_%s" % (name, tag)][0].astype(np.float64))
                key = "%s_%s_%s" % (name, "diff" if diff else "hard", tag)
                gw = torch.ones(e.shape[0], dtype=torch.float64)
                ch = R.LossChain(a64, name, diff, metric, 5.0, e, safe=False)
                w, ge = ch.forward_outputs().detach().numpy()[:, 0], ch.backward_outputs(gw).detach().numpy()
                w64 = g[key + "_f64"][0]
                np.testing.assert_allclose(w, w64, rtol=4e-16, atol=0, err_msg=key)
                if key + "_f64_grad" in g:
                    g64 = g[key + "_f64_grad"][0]
                    np.testing.assert_array_equal(np.isnan(ge), np.isnan(g64), err_msg=key)
                    if name == "huber" and not diff:
                        assert np.isnan(g64[:2]).all(), "the hard Huber slope at a zero residual is NaN in the reference"
                    # (float64's own rounding: 0.5 k (1 - th^2) from a th rounded at 2^-53 carries k 2^-53 absolutely, whatever is left of 1 - th^2)
                    np.testing.assert_allclose(ge, g64, rtol=1e-14, atol=5.0 * 2.0 ** -52, err_msg=key)
                # the float32 outputs of the reference against the float32 model
                c32 = R.LossChain(a32, name, diff, metric, 5.0, e)
                fo = c32.forward_outputs()
                ext = c32.extreme.numpy()
                ref = fo.detach().numpy().copy()
                if ext.any():
                    ref[ext] = R.LossChain(a32, name, diff, metric, 5.0, e, grads=False, ieee=True).forward_outputs().detach().numpy()[ext]
                tie = np.zeros(e.shape[0], dtype=bool)
                alts = []
                decs = c32.decision_bounds()
                for _, (_, _, t) in decs.items():
                    tie |= t.numpy()
                if tie.any():
                    alt = R.LossChain(a32, name, diff, metric, 5.0, e, flips={k: v[2] for k, v in decs.items()})
                    fa = alt.forward_outputs()
                    alts.append((fa.detach().numpy(), alt.bound(fa).numpy() if fa.requires_grad else np.full((e.shape[0], 1), a32.floor)))
                B = c32.bound(fo).numpy()
                B[ext & np.isfinite(ref[:, 0])] = np.inf        # (torch's norm does not square 1e20 or 1e-30 inside float32's range as the kernels' sum of squares does: at those rows only the class is held)
                R.check_points(g[key + "_f32"][0].astype(np.float64)[:, None], ref, B, "reference float32 " + key, tie, alts, extreme=ext)


# ---------------------------------------------------------------- the comparator refuses what is wrong
def _case(host, cfg_name, n=256):
    cfg = [c for c in R.grid() if R.cfg_id(c) == cfg_name][0]
    inp, cot = R.random_case(np.float32, cfg, n)
    ar = R.Arith(np.float32, "host")
    ref = R.reference(ar, cfg, inp, cot)
    R.check_case(ref, n, [])
    got = host.forward(np.float32, cfg, inp)
    R.check_points(got, ref["fwd"][0], ref["fwd"][1], "unperturbed")          # the true reference is accepted
    return cfg, inp, ar, ref, got


@pytest.mark.parametrize("node,cfg_name", [("lw", "pt2pt-c3-huber-diff-notrim-p0"), ("trim.th", "pt2pt-c3-none-diff-trim-p0"),
                                           ("d3", "pt2pt-c3-huber-diff-notrim-p0")])
def test_comparator_refuses_one_perturbed_intermediate(host, node, cfg_name):
    """lw, th or d3 of ONE point off by 16 u relative (8 ulp) in the reference: the true result is then off the bound of that point.  The point is chosen on
    the reference alone -- the one whose w moves most, in units of its bound -- and must move by more than 2 B(w): whatever the true result's own error
    (at most B), it then lies more than B from the perturbed reference."""
    cfg, inp, ar, ref, got = _case(host, cfg_name)
    w, Bw = ref["fwd"][0][:, 0], ref["fwd"][1][:, 0]
    rel = 16 * ar.u
    with torch.no_grad():
        moved = np.array([R.Chain(ar, cfg, R.take(inp, slice(i, i + 1)), perturb={node: (0, rel)}).forward_outputs().numpy()[0, 0] for i in range(len(w))])
    i = int(np.argmax(np.abs(moved - w) / Bw))
    assert abs(moved[i] - w[i]) > 2 * Bw[i], "no point of this configuration is sensitive enough to %s" % node
    with torch.no_grad():
        wrong = R.Chain(ar, cfg, inp, perturb={node: (i, rel)}).forward_outputs().numpy()
    assert (wrong[np.arange(len(w)) != i] == ref["fwd"][0][np.arange(len(w)) != i]).all()
    with pytest.raises(AssertionError, match="point %d " % i):
        R.check_points(got, wrong, ref["fwd"][1], "perturbed " + node)


def test_comparator_refuses_dropped_halved_nan_and_mixture(host):
    cfg, inp, ar, ref, got = _case(host, "pt2pl-c6-huber-diff-trim-p0")
    fr, fB = ref["fwd"]
    col = 1 + R.ACC_B                                                          # the first slot of b
    i = int(np.argmax(np.abs(fr[:, col]) / fB[:, col]))
    assert abs(fr[i, col]) > 4 * fB[i, col]
    for what, value in (("dropped", 0.0), ("halved", 0.5 * fr[i, col])):
        wrong = fr.copy()
        wrong[i, col] = value
        with pytest.raises(AssertionError, match="point %d " % i):
            R.check_points(got, wrong, fB, what)
    bad = got.copy()
    bad[7, 3] = np.nan
    with pytest.raises(AssertionError, match="point 7 "):
        R.check_points(bad, fr, fB, "NaN")
    nanref = fr.copy()
    nanref[7, 3] = np.nan
    R.check_points(bad, nanref, fB, "NaN where the reference is NaN")         # ... unless the reference is NaN at the same place
    with pytest.raises(AssertionError, match="point 7 "):
        R.check_points(got, nanref, fB, "a number where the reference is NaN")
    # a tie answered with a mixture: w from one side of the decision, the slots from the other
    cfgh = [c for c in R.grid() if R.cfg_id(c) == "pt2pt-c3-trim-hard-notrim-p0"][0]
    e_inp, _ = R.edge_sets(cfgh, np.float32)["at_metric"]
    eref = R.reference(ar, cfgh, e_inp, None, allow_ties=True)
    assert eref["tie"][:2].all() and len(eref["alts_fwd"]) >= 1, "residual exactly the metric is a placed tie of en < metric"
    one, other = eref["fwd"][0], eref["alts_fwd"][0][0]
    assert one[0, 0] != other[0, 0]
    egot = host.forward(np.float32, cfgh, e_inp)
    R.check_points(egot, eref["fwd"][0], eref["fwd"][1], "either side", eref["tie"], eref["alts_fwd"])
    mix = one.copy()
    mix[0, 0] = other[0, 0]
    with pytest.raises(AssertionError, match="matches neither side wholly"):
        R.check_points(mix, eref["fwd"][0], eref["fwd"][1], "mixture", eref["tie"], eref["alts_fwd"])


def test_extreme_points_gradients_are_held(host):
    """The gradients of the tiny / huge residuals (an intermediate outside float32's range) are compared like everything else: NaN in their place is
    refused, and so is a finite number where the documented edge is NaN."""
    for name, pinned_rows in (("pt2pl-c6-huber-diff-trim-p0", 0), ("pt2pt-c3-huber-diff-trim-p0", 2), ("pt2pt-c3-huber-hard-notrim-p1", 2)):
        cfg = [c for c in R.grid() if R.cfg_id(c) == name][0]

        class Wrong:
            build = "host"
            forward = staticmethod(host.forward)

            def __init__(self, value, rows):
                self.value, self.rows = value, rows

            def backward(self, dtype, cfg, inp, cot, **kw):
                g = host.backward(dtype, cfg, inp, cot)
                ext = R.Chain(R.Arith(dtype, "host"), cfg, inp).extreme.numpy()
                rows = np.flatnonzero(ext)
                assert len(rows) >= 4
                sel = rows if self.rows == "all" else rows[np.isnan(g[rows, 0])]
                g[sel] = self.value
                return g
        inp, cot, n, spans = R.config_case(np.float32, cfg, 64)
        ref = R.reference(R.Arith(np.float32, "host"), cfg, inp, cot, allow_ties=True)
        assert int(ref["pinned_nan"].sum()) == pinned_rows and int(ref["extreme"].sum()) >= 4, name
        R.run_config(host, np.float32, cfg, 64)
        with pytest.raises(AssertionError, match="tiny_huge"):
            R.run_config(Wrong(np.nan, "all"), np.float32, cfg, 64)
        if pinned_rows:
            with pytest.raises(AssertionError, match="tiny_huge"):
                R.run_config(Wrong(0.0, "nan"), np.float32, cfg, 64)


def test_threshold_decisions_next_to_a_tie_are_held():
    """w = match_thresh (1 +- 2^-18) is 32 ulp from the threshold in float32: outside the tie window where tw = lw = 1, so the decision itself is held;
    w = match_thresh exactly is the placed tie."""
    cfg = [c for c in R.grid() if R.cfg_id(c) == "pt2pt-c3-none-hard-notrim-p0"][0]
    for build in ("host", "device"):
        inp, _ = R.edge_sets(cfg, np.float32)["saturated"]
        ref = R.reference(R.Arith(np.float32, build), cfg, inp, None, allow_ties=True)
        assert not ref["tie"][3] and not ref["tie"][4] and ref["tie"][5]
        assert ref["fwd"][0][3, 1 + R.ACC_NMATCH] == 3 and ref["fwd"][0][4, 1 + R.ACC_NMATCH] == 0


def test_comparator_sensitivity_with_the_device_constants():
    """The same 16 u perturbations against the DEVICE's float32 bound, on the reference alone (no device here).  lw and th move w of the most sensitive point
    by more than 2 B(w): refused whatever the kernel's own error.  d3 does not reach 2 B: v_sqrt_f32 (1 ulp) and the three rounded squares under it
    give d3 itself 1.75 ulp = 3.5 u of legitimate error, m_div 1.5 ulp more on lw, so 16 u in d3 is only about 1.7 B(w).  It is more than B: a result
    whose own error is below 0.6 B is still refused, and the bound cannot be tighter without dropping a rounding the hardware makes."""
    ar = R.Arith(np.float32, "device")
    for node, cfg_name, need in (("lw", "pt2pt-c3-huber-diff-notrim-p0", 2.0), ("trim.th", "pt2pt-c3-none-diff-trim-p0", 2.0), ("d3", "pt2pt-c3-huber-diff-notrim-p0", 1.5)):
        cfg = [c for c in R.grid() if R.cfg_id(c) == cfg_name][0]
        inp, _ = R.random_case(np.float32, cfg, 256)
        ch = R.Chain(ar, cfg, inp)
        fo = ch.forward_outputs()
        w, Bw = fo.detach().numpy()[:, 0], ch.bound(fo).numpy()[:, 0]
        with torch.no_grad():
            moved = np.array([R.Chain(ar, cfg, R.take(inp, slice(i, i + 1)), perturb={node: (0, 16 * ar.u)}).forward_outputs().numpy()[0, 0] for i in range(256)])
        assert (np.abs(moved - w) / Bw).max() > need, (node, float((np.abs(moved - w) / Bw).max()))


# ---------------------------------------------------------------- the model's operations are the sources'
def _between(text, start, end):
    i = text.index(start)
    return text[i:text.index(end, i)]


def test_model_matches_the_sources():
    """A change of form must fail here, not silently make the constants of point_math_ref wrong."""
    math_h = open(os.path.join(CSRC, "dicp_math.h")).read()
    dev = _between(math_h, "#if defined(__HIP_DEVICE_COMPILE__)\nDICP_HD float  m_sqrt", "#else")
    assert "m_sqrt(float x)  { return %s; }" % R.DEVICE_FORMS["m_sqrt"] in dev
    assert "m_div(float a, float b) { return %s; }" % R.DEVICE_FORMS["m_div"] in dev
    assert "const float e = %s;" % R.DEVICE_FORMS["m_tanh"][0] in dev and "return %s;" % R.DEVICE_FORMS["m_tanh"][1] in dev
    assert abs(float(np.float32(2.8853900817779268)) - 2 / np.log(2)) <= 2.0 ** -23 * 2 / np.log(2) / 2      # fl(2 log2 e): the 0.5 ulp of the constant
    assert "1 ulp each" in math_h                                             # (the header's own statement of v_sqrt / v_rcp / v_exp)
    host = _between(math_h, "#else\nDICP_HD float  m_sqrt", "#endif")
    for form in ("return sqrtf(x);", "return a / b;", "return tanhf(x);"):
        assert form in host
    for form in ("double m_sqrt(double x) { return sqrt(x); }", "double m_div(double a, double b) { return a / b; }", "double m_tanh(double x) { return tanh(x); }"):
        assert form in math_h
    pw = _between(math_h, "DICP_HD void point_weights(", "// Forward: add this point's contribution")
    for op in ("s.d3 = m_sqrt(dot3(s.e3, s.e3));", "m_tanh(wp_val<T>(P.tanh_k) * (wp_val<T>(P.trim_dist) - s.d3) - T(3))", "T(0.5) * s.th + T(0.5)",
               "m_div(dl * dl, dl * dl + s.en * s.en)", "(s.en > dl) ? m_div(dl, s.en) : T(1)", "m_div(s.en, dl)", "m_div(T(1), T(1) + t * t)",
               "m_tanh(wp_val<T>(P.tanh_k) * (dl - s.en) - T(3))", "s.w = w0 * s.tw * s.lw;", "m_sqrt(s.w + T(1.0e-10))", "s.root - T(1.0e-5)", "s.u = s.ws * s.ws;"):
        assert op in pw, op
    pb = _between(math_h, "DICP_HD void point_backward(", "// ------------------------------------------------------------------ per-cloud step")
    for op in ("m_div(ubar * s.ws, s.root)", "(T(1) - s.lth * s.lth)", "(T(1) - s.th * s.th)", "m_div(-T(2) * s.en * s.lw * s.lw, dl * dl)"):
        assert op in pb, op
    # the stand-alone loss: m_sqrt, m_tanh and plain '/' (0.5 ulp in every build), in the kernels and in the host restatement alike
    soft = open(os.path.join(CSRC, "kernels_soft_svd.h")).read()
    hostcpp = open(R.HOSTCHECK_SRC).read()
    for text, start, end in ((soft, "void loss_eval(", "// ------------------------------------------------------- pose gradient"),
                             (hostcpp, "static void loss_eval_t(", 'extern "C"')):
        body = _between(text, start, end)
        assert "m_div" not in body
        for op in ("en = m_sqrt(s);", "(metric * metric) / (metric * metric + en * en)", "(en > metric) ? metric / en : T(1)", "en / metric", "T(1) / (T(1) + t * t)",
                   "m_tanh(kk * (metric - en) - T(3))", "-T(2) * en * wv * wv / (metric * metric)", "hard_huber_slope(en, metric)", "-T(0.5) * kk * (T(1) - th * th)",
                   "gw[i] * dw * e[k] / en"):
            assert op in body, op
    # nothing in the build relaxes the arithmetic: contraction only inside an expression, no fast-math
    from dicp_amd import _lib
    assert "-ffp-contract=on" in _lib.FLAGS and not [f for f in _lib.FLAGS if re.search(r"fast-math|unsafe|finite-math|approx", f)]
    assert ctypes_sizes_agree()


def ctypes_sizes_agree():
    import ctypes
    from dicp_amd import _lib
    return ctypes.sizeof(R.WeightParams) == ctypes.sizeof(_lib.WeightParams) and [f[0] for f in R.WeightParams._fields_] == [f[0] for f in _lib.WeightParams._fields_]


# ---------------------------------------------------------------- the GPU tests' inputs contain no tie (the seeds are chosen here, on the CPU)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_gpu_inputs_have_no_ties(dtype):
    """With the DEVICE's constants (the wider tie windows): the random points of every grid configuration at the GPU tests' size, the call variants' and
    the block sums' inputs; every edge set hits its edge.  Asserted on the reference alone."""
    ar = R.Arith(dtype, "device")
    for cfg in R.grid():
        inp, cot, n, spans = R.config_case(dtype, cfg, R.GPU_POINTS)
        R.check_case(R.reference(ar, cfg, inp, None, allow_ties=True), n, spans)
    for cfg in [c for c in R.grid() if c["ps"] == 0 and c["diff"] and c["trim_on"] and c["loss"] in ("huber", "cauchy")]:
        inp, _ = R.random_case(dtype, cfg, 1024)
        for unit in (False, True):
            if unit:
                inp["w_init"] = torch.ones_like(inp["w_init"])
            R.check_case(R.reference(ar, cfg, inp, None), 1024, [])
    for n in R.SUM_SIZES:
        R.sum_reference(ar, R.sum_case(dtype, n), backward=False)
