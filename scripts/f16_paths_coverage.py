"""Which refine paths of the matrix-core search tests/test_gpu_f16.py's cases can reach: the model of tests/f16_paths.py over cloud 0 of each case, on the CPU.
An ESTIMATE (those clouds are not exact, and the search frame is left out): a piece counts as a candidate when its best row is within 2E of the winner."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import f16_paths as P
import importlib.util
spec = importlib.util.spec_from_file_location("old", os.path.join(ROOT, "tests", "test_gpu_f16.py")); old = importlib.util.module_from_spec(spec); spec.loader.exec_module(old)
U = 2.0**-24
for name, src, tgt, src_rows, tgt_rows in old.CASES:
    c = 0
    n = src.shape[1] if src_rows is None else int(src_rows[c]); m = tgt.shape[1] if tgt_rows is None else int(tgt_rows[c])
    y = tgt[c, :m].numpy().astype(np.float32); x = src[c, :n].numpy().astype(np.float64)
    sm = P.scale_model(y)
    s = sm["s"]; img = sm["image"]; y64 = y.astype(np.float64)
    tp = P.stand_in_tperm(y); pos = np.empty(m, np.int64); pos[tp] = np.arange(m)
    pid_b = P.piece_ids(np.arange(m), "brute"); pid_s = P.piece_ids(pos, "sweep")
    uns_b = np.zeros(n, bool); uns_s = np.zeros(n, bool); unb = np.zeros(n, bool); farwin = 0; tie_rev = 0; ties2 = 0
    for a in range(0, n, 512):
        X = x[a:a+512]
        with np.errstate(invalid="ignore", over="ignore"):
            D = 0.5*((X[:, None, :] - y64[None])**2).sum(-1)
        D[:, ~sm["finite"]] = np.inf
        Di = np.where(img[None], D, np.inf); Db = Di.min(1)
        hx = 0.5*(X**2).sum(1); x1 = np.abs(X).sum(1)
        slack = 2.0**-9*(Db+hx); X2 = np.sqrt(2*hx); Y = X2+np.sqrt(2*(Db+slack))
        E = (32*U*(X2*Y+0.5*Y*Y) + U/s*(x1+1.7321*Y) + 3*2.0**-12/(s*s))*1.01
        ub = ~np.isfinite(Db) | (np.abs(X)*s > 60000).any(1) | ~(4*E <= slack)
        unb[a:a+512] = ub
        cand = Di - Db[:, None] <= 2*E[:, None]
        for pid, out in ((pid_b, uns_b), (pid_s, uns_s)):
            q, r = np.nonzero(cand); K = int(pid.max())+1
            out[a:a+512] = (np.bincount(np.unique(q*K+pid[r])//K, minlength=len(X)) >= 3) & ~ub
        best = D.min(1); farwin += int((best < Db).sum())
        tie = (D == best[:, None]); nt = tie.sum(1)
        for qq in np.nonzero(nt > 1)[0]:
            rows = np.nonzero(tie[qq])[0]; ties2 += 1
            tie_rev += int(rows[np.argmin(pos[rows])] != rows[0])
    wb = [int(uns_b[u:u+128].sum()) for u in range(0, n, 128)]
    xo = np.argsort(x[:, 0], kind="stable")
    ws = [int(uns_s[xo[u:u+128]].sum()) for u in range(0, n, 128)]
    print("%-36s s=%g nfar=%d cnt=%d | unbounded %d | brute unsure/wave max %d (waves>32: %d) | sweep unsure/unit max %d (units at 6: %d, at 7: %d, >32: %d) | far row wins %d | exact ties %d, sorted-first != lowest index %d" % (
        name, s, sm["nfar"], sm["cnt"], int(unb.sum()), max(wb), sum(w > 32 for w in wb), max(ws), sum(w == 6 for w in ws), sum(w == 7 for w in ws), sum(w > 32 for w in ws), farwin, ties2, tie_rev), flush=True)
