"""Every refine path of the matrix-core search (`-m gpu`; csrc/knn_f16.hip), driven on purpose and pinned by its counters.

The cases of tests/f16_paths.py are EXACT clouds (every intermediate of score() is a float32 number), so both search forms -- all pairs
(dicp_knn, DICP_KNN_MFMA) and the sorted sweep (dicp_knn_sweep with the f16 image), the latter by index order and by SweepIndex.query_order -- must return
exactly the float64 oracle: argmin 0.5|x - y|^2, lowest index among exact ties.  No tolerance anywhere.  Beyond the indices, every search is held to
the model's prediction of what it leaves behind: the scale s, the far rows (meta words 0, 3, 8..) and the queries it ADDED to the two counters, AGAIN
(second filter pass) and SCAN (exact scan) -- which is what shows that a case took the branch it was built for (one, two, three or more candidate pieces;
rounds 2..4 of pass 2; the sweep's switch at F16_SCAN_MAX; no bound; far rows; the tie loop's lowest-ORIGINAL-index rule).  tests/test_f16_paths.py proves
the constructions and the model on the CPU, and that the comparator used here refuses a model with one of those rules mutated.

The one case whose counters are only bounded is the grey one (queries on a target at the origin: D0 + 0.5|x|^2 = 0, the margin's acceptance is decided by
the filter's own rounding): its indices are held exactly, each such query may have been counted once or not at all."""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib, _ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f16_paths as P      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7
CASES = P.cases()


def _meta(image, N, m_pad):
    """The meta words of an f16 image, as _ops.f16_counters reads them: s (word 0), nfar (3), AGAIN (6), SCAN (7), the far rows (8..)."""
    m_img = (int(m_pad) + 511) // 512 * 512
    w = image[N * m_img * 32:N * m_img * 32 + N * 320].view(torch.int32).view(N, 80).cpu().numpy()
    return dict(s=w[:, 0].copy().view(np.float32).astype(np.float64), nfar=w[:, 3].astype(np.int64), again=int(w[:, 6].sum()), scan=int(w[:, 7].sum()),
                far=[frozenset(w[c, 8:8 + min(int(w[c, 3]), 64)].tolist()) for c in range(N)])


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(case):
    y, x = _dev(case.y), _dev(case.x)
    pose, src_rows, tgt_rows = _dev(case.pose), _dev(case.src_rows), _dev(case.tgt_rows)
    N, n, m = case.N, case.n, case.m
    new = lambda: torch.full((N, n), SENTINEL, dtype=torch.int32, device=DEV)
    lines = []

    # ---- all pairs
    tgt4 = _ops.pack_target(y, None, tgt_rows)
    ref = _ops.knn(x, pose, tgt4, m, _lib.KNN_VALU, out=new(), src_rows=src_rows, tgt_rows=tgt_rows)
    img = _ops.f16_image(tgt4, m, tgt_rows)
    got = _ops.knn(x, pose, tgt4, m, _lib.KNN_MFMA, out=new(), src_rows=src_rows, tgt_rows=tgt_rows, image=img)
    meta = _meta(img, N, tgt4.shape[1])
    pred = P.predict(case, "brute")
    lines.append("all pairs        AGAIN %d SCAN %d | predicted %s" % (meta["again"], meta["scan"], P.describe(pred)))
    print(lines[-1])
    meta["idx"] = got.cpu().numpy()
    P.compare(meta, pred, "all pairs")
    assert (meta["idx"][~pred["valid"]] == SENTINEL).all(), "entries of idx past src_rows were written"
    assert torch.equal(got, ref), "all pairs: matrix-core and VALU indices differ"
    if "brute" in case.reach:
        assert case.reach["brute"](pred), "all pairs: the case does not reach its branch"

    # ---- the sweep, by index order and by its own query order
    sw = _ops.SweepIndex(y, tgt_rows=tgt_rows)
    tperm = sw.tperm.cpu().numpy()
    for label, qo in (("sweep, by index", None), ("sweep, ordered ", sw.query_order(x, pose, src_rows=src_rows))):
        idx0, spos0, idx1, spos1 = new(), new(), new(), new()
        sw.knn(x, pose, qo, out=idx0, cfg=2, spos=spos0, src_rows=src_rows, mfma=False)
        before = _meta(sw.make_image(), N, sw.tgs4.shape[1])
        sw.knn(x, pose, qo, out=idx1, cfg=2, spos=spos1, src_rows=src_rows, mfma=True)
        meta = _meta(sw.make_image(), N, sw.tgs4.shape[1])
        meta["again"] -= before["again"]
        meta["scan"] -= before["scan"]
        pred = P.predict(case, "sweep", tperm=tperm, qorder=None if qo is None else qo.cpu().numpy())
        lines.append("%s  AGAIN %d SCAN %d | predicted %s" % (label, meta["again"], meta["scan"], P.describe(pred)))
        print(lines[-1])
        meta["idx"] = idx1.cpu().numpy()
        # (the far rows of the sorted image are sorted positions)
        meta["far"] = [frozenset(int(tperm[c, r]) for r in meta["far"][c]) for c in range(N)]
        P.compare(meta, pred, label.strip())
        sp = spos1.cpu().numpy()
        v = pred["valid"]
        assert (meta["idx"][~v] == SENTINEL).all() and (sp[~v] == SENTINEL).all(), "entries past src_rows were written"
        for c in range(N):
            found = v[c] & (sp[c] >= 0)
            assert (tperm[c][sp[c][found]] == meta["idx"][c][found]).all(), "tperm[spos] != idx"
            assert (sp[c][v[c] & ~found] == -1).all() and (meta["idx"][c][v[c] & ~found] == 0).all()
            nq, mc = case.rows(c)
            odd = ~np.isfinite(P.scored_queries(case.x[c], None if case.pose is None else case.pose[c])).all(1)
            assert (found | odd | ~v[c]).all() or not P.scale_model(case.y[c, :mc])["finite"].any(), "a finite query without a match in a cloud with finite rows"
        assert torch.equal(idx0, idx1) and torch.equal(spos0, spos1), "%s: matrix-core and VALU sweep differ" % label.strip()
        if qo is None and "sweep" in case.reach:
            assert case.reach["sweep"](pred), "sweep: with the sort's own order of equal keys the case does not reach its branch"
    return lines


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_refine_path(case):
    print("\n%s\n  branch: %s" % (case.name, case.branch))
    _run(case)


@pytest.mark.parametrize("m", P.SIZES_M)
def test_sizes_all_clear(m):
    """The 16-row run, 32-row tile, 64-row sweep tile, 128-row chunk, 512-row stage, 128-query wave and 512-query block, each at -1 / 0 / +1."""
    for case in P.size_cases(m):
        _run(case)
