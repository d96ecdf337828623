"""The window model of tests/icp_window_layouts.py against the kernels' sources and the library's own host functions, the layouts against the
conditions that make them tests of the windowed backward's branches, and the comparator of tests/test_gpu_window_backward.py against planted
faults (no GPU: the model, the float64 reference and a numpy emulation of the pass)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_window_layouts as wl  # noqa: E402
import point_math_ref as R  # noqa: E402

from dicp_amd import _lib  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dicp_amd", "csrc")
DTYPES = [np.float32, np.float64]
ids = lambda d: np.dtype(d).name


@pytest.fixture(autouse=True)
def _threads():
    before = torch.get_num_threads()
    torch.set_num_threads(4)
    yield
    torch.set_num_threads(before)


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_window_constants_match_the_sources():
    common, bwd, host = _text("dicp_common.h"), _text("kernels_backward.h"), _text("dicp_kernels.hip")
    for name, value, text in (("BLOCK", wl.BLOCK, common), ("KNN_PAD", wl.KNN_PAD, common), ("MAXB", wl.MAXB, bwd), ("WR_U", wl.WR_U, bwd)):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m and int(m.group(1)) == value, name
    for ctype, dt in (("float", wl.F32), ("double", wl.F64)):
        m = re.search(r"template <> struct WindowRows<%s>\s*\{ static constexpr int v = (\d+); \};" % ctype, bwd)
        assert m and int(m.group(1)) == wl.WT[dt]
    assert (wl.WT[wl.F32], wl.WT[wl.F64]) == (1536, 768)
    assert "constexpr int SPB = 4 * BLOCK;" in bwd and wl.SPB_MAX == 4 * wl.BLOCK
    # the expressions the model repeats, as the kernels state them
    for line in (
            # window_slots
            "long s = (long)(WT - WT / 3) * n / (m_pad > 0 ? m_pad : 1);", "s = (s / BLOCK) * BLOCK;",
            "return (int)(s < BLOCK ? BLOCK : (s > 4 * BLOCK ? 4 * BLOCK : s));",
            # window_origin
            "if (m_pad <= WT || n <= 0) return 0;", "const int mid = min(blk * spb + spb / 2, n - 1);",
            "const int ctr = max(sp_ref_c[qo_c ? min(max(qo_c[mid], 0), n - 1) : mid], 0);", "return min(max(ctr - WT / 2, 0), m_pad - WT) & ~15;",
            # window_body: the cloud's own slots, slot -> query -> match, the window test
            "const int nc = rows_of(src_rows, cloud, n);", "const int s0 = blk * spb, s1 = min(nc, s0 + spb), s1_all = min(n, s0 + spb);",
            "pos[u] = qo_c ? min(max(qo_c[sq], 0), n - 1) : sq;",
            "const int lo = window_origin(spos_ref + (size_t)cloud * n, qo_c, blk, spb, nc, m_pad, WT);", "const int hi = min(lo + WT, m_pad);",
            "pos[u] = on[u] ? min(max(match_at(spos, cloud, pos[u]), 0), m_pad - 1) : 0;", "if (pos[u] >= lo && pos[u] < hi) {",
            # window_reduce_kernel: passes of MAXB blocks, the list of the windows that reach the block's rows, rounds of 32
            "const int e0 = rb * (BLOCK * WR_U);", "const int r_lo = e0 / CV, r_hi = min(e0 + BLOCK * WR_U - 1, m * cv - 1) / CV;",
            "for (int b0 = 0; b0 < bpc; b0 += MAXB) {", "const int nb = min(MAXB, bpc - b0);",
            "b0 + tid, spb, rows_of(src_rows, cloud, n), m_pad, WT);", "const bool rel = tid < nb && org <= r_hi && org + WT > r_lo;",
            "for (int bb = 0; bb < nrel; bb += 32) {", "const int nbb = min(32, nrel - bb);", "cover[u] |= (sr >= lo && sr < lo + WT) ? (1u << k) : 0u;"):
        assert line in bwd, line
    assert wl.ROUND == 32
    assert "int dicp_padded_targets(int m) { return m <= 0 ? 0 : ((m + KNN_PAD - 1) / KNN_PAD) * KNN_PAD; }" in host
    assert "const int spb = window_slots(dtype == DICP_F32 ? WindowRows<float>::v : WindowRows<double>::v, n, m_pad);" in host
    assert "return (n + spb - 1) / spb;" in host


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_model_against_the_host_functions(lib):
    assert (lib.dicp_window_rows(_lib.F32), lib.dicp_window_rows(_lib.F64)) == (wl.WT[wl.F32], wl.WT[wl.F64])
    ms = [0, 1, 63, 64, 65, 70, 128, 767, 768, 769, 1536, 1537, 2000, 5000, 5056, 8000, 17000, 20000, 131200, 1 << 20]
    ns = [0, 1, 255, 256, 257, 300, 1000, 2000, 4096, 5000, 8448, 8449, 65536, 65537, 1 << 20]
    for m in ms:
        m_pad = wl.padded_targets(m)
        assert lib.dicp_padded_targets(m) == m_pad
        for n in ns:
            for code, dt in ((_lib.F32, wl.F32), (_lib.F64, wl.F64)):
                assert lib.dicp_window_blocks(code, n, m_pad) == wl.window_blocks(dt, n, m_pad), (n, m, dt)
    # the sizes the layouts name
    for dt in (wl.F32, wl.F64):
        assert wl.window_blocks(dt, 8449, wl.padded_targets(17000)) == 34 and wl.window_blocks(dt, 65537, wl.padded_targets(131200)) == 257
        assert wl.window_slots(wl.WT[dt], 4096, wl.padded_targets(2000)) == 1024 and wl.window_slots(wl.WT[dt], 2000, wl.padded_targets(8000)) == 256


def test_model_on_a_hand_made_case():
    # float64: WT = 768.  n = 1000 slots against m = 2000 rows (m_pad 2048): spb = 512 * 1000 / 2048 = 250 -> 256, 4 blocks; matches 2 s by slot
    n, m = 1000, 2000
    sp = (2 * np.arange(n)).astype(np.int32)
    g = wl.geometry(np.float64, n, m, n, None, sp, sp)
    assert (g.spb, g.bpc) == (256, 4)
    # middle slots 128, 384, 640, 896 -> centres 256, 768, 1280, 1792 -> minus 384, clamped to [0, 2048 - 768], multiples of 16
    assert g.lo.tolist() == [0, 384, 896, 1280] and g.hi.tolist() == [768, 1152, 1664, 2048]
    assert g.far.sum() == 0 and g.cover[383] == 1 and g.cover[384] == 2 and g.cover[767] == 2 and g.cover[768] == 1 and g.cover[1999] == 1
    # a match at hi is far, at hi - 1 in window; at lo in window, at lo - 1 far
    for row, inw in ((1152, False), (1151, True), (384, True), (383, False)):
        s2 = sp.copy()
        s2[300] = row
        g2 = wl.geometry(np.float64, n, m, n, None, sp, s2)
        assert bool(g2.inwin[300]) == inw and bool(g2.far[300]) != inw and g2.indegree[row] == (2 if row % 2 == 0 else 1)
    # a ragged cloud of 300 slots: the middle slot of block 1 is its last own slot (299); slots past it are dead; the slot order is a permutation
    qo = np.arange(n)[::-1].astype(np.int32)
    qo = np.concatenate((qo[-300:], qo[:-300]))                     # own queries 299 .. 0 first
    g3 = wl.geometry(np.float64, n, m, 300, qo, sp, sp)
    assert g3.live.sum() == 300 and g3.lo[0] == max(2 * (299 - 128) - 384, 0) & ~15 and g3.lo[1] == max(2 * 0 - 384, 0) and g3.lo[3] == g3.lo[1]
    assert wl.geometry(np.float64, n, m, 0, qo, sp, sp).lo.tolist() == [0, 0, 0, 0]
    # m_pad <= WT: one origin, hi = m_pad
    g4 = wl.geometry(np.float32, 300, 70, 300, None, np.zeros(300, np.int32), np.full(300, -1, np.int32))
    assert g4.bpc == 1 and g4.lo.tolist() == [0] and g4.hi.tolist() == [128] and g4.indegree[0] == 300


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", sorted(wl.LAYOUTS))
def test_layouts_meet_their_conditions(name, dtype):
    print(wl.check_conditions(wl.layout(name, dtype), dtype))


# ---------------------------------------------------------------- the comparator refuses wrong sums
FAULTS = [("diagonal", "window"), ("covered_34", "round"), ("blocks_257", "pass"), ("edges", "edges"), ("all_far", "far")]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name,fault", FAULTS)
def test_comparator_refuses_wrong_sums(name, fault, dtype):
    """The numpy emulation of the pass (slab or far row by the model, sums per window in the dtype, the reduce in passes of MAXB blocks and rounds of 32
    windows), fed the reference's per-point terms, lies within the bound the GPU test uses -- and does not once one window's slab is left out of
    the reduce, the windows beyond the 32nd of a reduce block's list are, the blocks beyond the 256th are, the slots matched exactly to lo or
    hi - 1 are taken for far rows and dropped, or the far rows are dropped."""
    lay = wl.layout(name, dtype)
    wl.check_conditions(lay, dtype)
    key, cv = 2, 6
    P = wl.pool(dtype, key, lay.N, lay.alive)
    a_src, a_tgt = wl.assign(lay)
    br = P.ref["bwd"][0]
    terms = {w: [br[st["ref"], 3:3 + cv] for st in wl.slot_terms(lay, dtype, P, a_src, a_tgt, w)] for w in "AB"}
    T, TB, D = wl.row_reference(lay, dtype, P, cv, a_src, a_tgt)
    fam = {"gtgt": [0, 1, 2], "gnormal": [3, 4, 5]}
    record = {}
    good = wl.emulate(lay, dtype, cv, terms)
    R.check_points(good.reshape(-1, cv), T, TB, "emulation " + name, families=fam, record=record)
    print("%s %s: largest |error| / bound of the emulation %s" % (name, np.dtype(dtype).name, record))
    if fault == "window":                                           # a window in the middle of cloud 1 that holds contributions
        g = lay.geometry(dtype, 1, "A")
        blk = g.bpc // 2
        assert g.inwin[g.blk == blk].any()
        fault = ("window", 1, blk)
    bad = wl.emulate(lay, dtype, cv, terms, fault)
    with pytest.raises(R.OffBound):
        R.check_points(bad.reshape(-1, cv), T, TB, "emulation %s with fault %s" % (name, fault))
    nan = good.copy()
    nan[0, int(np.flatnonzero(D[:lay.m] == 0)[0]) if (D[:lay.m] == 0).any() else 0, 1] = np.nan      # (a row nothing matches, where there is one)
    with pytest.raises(R.OffBound):
        R.check_points(nan.reshape(-1, cv), T, TB, "emulation %s with a NaN" % name)
