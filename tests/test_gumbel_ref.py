"""tests/gumbel_ref.py proved on a CPU: the reference is the oracle, the kernel-order emulation stays inside the model's bound (safety factor 1)
on every input set tests/test_gpu_gumbel.py uses, the comparator refuses five deliberately wrong emulations, and the restated hash has the
statistics of a uniform draw.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gumbel_ref as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
_SETS = {}


def designed(dtype, **kw):
    key = (np.dtype(dtype).name,) + tuple(sorted(kw.items()))
    if key not in _SETS:
        _SETS[key] = G.designed_sets(dtype, **kw)
    return _SETS[key]


def refused(res):
    return [k for k, v in res.items() if not v[0]]


def test_model_matches_the_sources():
    """the forms and constants the model describes are the ones in the sources"""
    src = open(os.path.join(ROOT, "dicp_amd", "csrc", "kernels_soft_svd.h")).read()
    assert "float  log_t(float v)  { return %s; }" % G.DEVICE_FORMS["log_t"] in src
    assert "float  exp_t(float v)  { return %s; }" % G.DEVICE_FORMS["exp_t"] in src
    assert G.DEVICE_FORMS["tile"] in src and G.GUM_TILE == 512
    common = open(os.path.join(ROOT, "dicp_amd", "csrc", "dicp_common.h")).read()
    assert re.search(r"BLOCK\s*=\s*%d\b" % G.BLOCK, common)
    math_h = open(os.path.join(ROOT, "dicp_amd", "csrc", "dicp_math.h")).read()
    assert "v_log_f32" in math_h and "v_exp_f32" in math_h and "v_rcp_f32" in math_h
    for const in ("0x7feb352du", "0x846ca68bu", "0x9E3779B9u", "0x85EBCA6Bu", "0xC2B2AE35u", "0x27D4EB2Fu"):
        assert src.count(const) >= 1


def test_reference_is_the_oracle():
    """float64: eps and 1 / tau round to themselves, so the restatement and oracle.dicp_oracle.nn_gumbel compute the same function; the two differ by
    the order of their float64 operations only (the model's own bound for a float64 pair of evaluations)"""
    for c, tau, eps in ((3, 0.5, 1e-10), (6, 0.05, 1e-20)):
        x, y, U, cot = G.random_set(2, 37, 61, c, np.float64, 7)
        ref = G.reference(x, y, U, eps, tau, np.float64)
        b = G.bounds(x, y, U, eps, tau, np.float64, ref=ref)
        ok, worst, at = G.compare(G.oracle_out(x, y, U, eps, tau), ref["out"], b["out"])
        assert ok, (worst, at)
        assert float(np.abs(G.oracle_out(x, y, U, eps, tau) - ref["out"]).max()) < 1e-13


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulation_inside_the_bound_designed(dtype):
    for name, (x, y, U, cot, eps, tau) in designed(dtype).items():
        res = G.hold(G.emulate(x, y, U, eps, tau, dtype, cot), x, y, U, eps, tau, dtype, cot)
        assert not refused(res), (name, res)
    for name, (x, y, U, cot, eps, tau) in designed(dtype, n=257, m=513, c=6).items():
        if name in ("near_j512", "equal_maxima", "noise_edges_eps1e-10"):
            res = G.hold(G.emulate(x, y, U, eps, tau, dtype, cot), x, y, U, eps, tau, dtype, cot)
            assert not refused(res), (name, res)


RANDOM_CASES = [(3, 300, 1100, 3, 0.5, 1e-10, 0.0), (3, 300, 1100, 6, 0.01, 1e-20, 2500.0), (3, 300, 1100, 3, 0.05, 1e-20, 100.0),
                (3, 1, 1100, 3, 0.1, 1e-20, 0.0), (3, 257, 2, 6, 0.1, 1e-10, 0.0), (3, 256, 1, 3, 0.01, 1e-20, 100.0), (3, 255, 513, 3, 0.01, 1e-10, 0.0),
                (3, 300, 511, 3, 0.5, 1e-20, 2500.0), (3, 300, 512, 6, 0.05, 1e-10, 0.0), (3, 300, 1025, 3, 0.1, 1e-20, 0.0)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulation_inside_the_bound_random(dtype):
    for k, (N, n, m, c, tau, eps, off) in enumerate(RANDOM_CASES):
        x, y, U, cot = G.random_set(N, n, m, c, dtype, 10 + k, off)
        res = G.hold(G.emulate(x, y, U, eps, tau, dtype, cot), x, y, U, eps, tau, dtype, cot)
        assert not refused(res), ((N, n, m, c, tau, eps, off), res)


def _faulty(dtype, name, fault, **kw):
    x, y, U, cot, eps, tau = designed(dtype)[name]
    return G.hold(G.emulate(x, y, U, eps, tau, dtype, cot, fault=fault, **kw), x, y, U, eps, tau, dtype, cot)


@pytest.mark.parametrize("dtype", DTYPES)
def test_refuses_a_missing_rescale_at_a_tile_start(dtype):
    for name in ("max_at_512", "near_j1024", "ascending"):
        assert "out" in refused(_faulty(dtype, name, "no_rescale_at_tile_start")), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_refuses_a_skipped_last_element_of_a_tile(dtype):
    for name in ("near_j511", "near_j1023"):
        assert set(refused(_faulty(dtype, name, "skip_tile_last"))) == {"out", "gx", "gy"}, name


@pytest.mark.parametrize("dtype", DTYPES)
def test_refuses_backward_noise_from_the_next_pair(dtype):
    """the forward is untouched: only the gradients leave the bound"""
    for name in ("near_j513", "noise_edges_eps1e-20"):
        res = _faulty(dtype, name, "bwd_noise_shift")
        assert "gy" in refused(res) and "out" not in refused(res), (name, res)


@pytest.mark.parametrize("dtype", DTYPES)
def test_refuses_a_key_without_the_cloud_term(dtype):
    """designed clouds whose neighbouring logits lie 0.07 apart, so the noise decides, with noise from the restated hash: with the cloud term dropped,
    cloud 0 still agrees and clouds 1, 2 do not"""
    x, y, _, cot, eps, tau = designed(dtype)["ascending"]
    N, n, m = x.shape[0], x.shape[1], y.shape[1]
    U = G.hash_uniform(5, N, n, m)
    good = G.hold(G.emulate(x, y, U, eps, tau, dtype, cot), x, y, U, eps, tau, dtype, cot)
    assert not refused(good), good
    wrong = G.emulate(x, y, G.hash_uniform(5, N, n, m, cloud_term=False), eps, tau, dtype, cot)
    assert set(refused(G.hold(wrong, x, y, U, eps, tau, dtype, cot))) == {"out", "gx", "gy"}
    first = G.hold({k: v[:1] for k, v in wrong.items()}, x[:1], y[:1], U[:1], eps, tau, dtype, cot[:1])
    assert not refused(first), first


def test_refuses_one_intermediate_off_by_16u():
    """float32, the two-target designed input: 1 / S of one query off by 16 u_T"""
    sets = designed(np.float32, m=2)
    x, y, U, cot, eps, tau = sets["near_j1"]
    res = G.hold(G.emulate(x, y, U, eps, tau, np.float32, cot), x, y, U, eps, tau, np.float32, cot)
    assert not refused(res), res
    for at in ((0, 0), (2, 299)):
        res = G.hold(G.emulate(x, y, U, eps, tau, np.float32, cot, fault="off_16u", at=at), x, y, U, eps, tau, np.float32, cot)
        assert "out" in refused(res) and res["out"][2][:2] == at, res


@pytest.mark.parametrize("seed", [0, 1, 0xFFFFFFFF])
def test_hash_statistics(seed):
    """fixed limits: mean within 4 sigma of 1/2 (sigma^2 = 1 / (12 count)), the lag-1 correlations along j, along i and across clouds within
    4 / sqrt(count), every value in [0, 1), and no more repeats within a row than the birthday expectation allows (m^2 / 2^25 per row of m draws
    from 2^24 values: 0.036 at m = 1100, so 240 over the 6600 rows; 4 sigma of that Poisson count on top)"""
    N, n, m = 6, 1100, 1100
    u = G.hash_uniform(seed, N, n, m)
    count = u.size
    assert u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u, u.astype(np.float32).astype(np.float64)) and np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))
    assert abs(u.mean() - 0.5) <= 4 * np.sqrt(1.0 / (12 * count))
    z = (u - 0.5) * np.sqrt(12.0)
    for a, b in ((z[:, :, 1:], z[:, :, :-1]), (z[:, 1:], z[:, :-1]), (z[1:], z[:-1])):
        assert abs(float((a * b).mean())) <= 4 / np.sqrt(a.size)
    rows = np.sort(u.reshape(N * n, m), axis=1)
    repeats = int((rows[:, 1:] == rows[:, :-1]).sum())
    expect = N * n * m * (m - 1) / 2.0 ** 25
    assert repeats <= expect + 4 * np.sqrt(expect), (repeats, expect)


def test_hash_key_chain_by_hand():
    """one draw, written out with Python integers"""
    def mix(v):
        v ^= v >> 16
        v = (v * 0x7feb352d) & 0xFFFFFFFF
        v ^= v >> 15
        v = (v * 0x846ca68b) & 0xFFFFFFFF
        return v ^ (v >> 16)
    seed, b, i, j = 0x7FFFFFFE, 2, 299, 1099
    key = mix(mix(seed ^ ((b * 0x9E3779B9) & 0xFFFFFFFF)) ^ ((i * 0x85EBCA6B) & 0xFFFFFFFF))
    want = (mix(key ^ ((j * 0xC2B2AE35 + 0x27D4EB2F) & 0xFFFFFFFF)) >> 8) / 2.0 ** 24
    assert G.hash_uniform(seed, 3, 300, 1100)[b, i, j] == want
