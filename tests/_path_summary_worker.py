"""Worker of test_gpu_path_summary.py::test_forced_paths_agree: the summaries along one tolerance path with K_max = 4097 (both
methods, both kernels) through the host entry, written to the .npz named on the command line.  The parent sets ABC_DIAG=1 and
ABC_SUMMARY_PATH."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from abcsmc_amd import _lib, abcutil, synthetic

ctx = _lib.default_context(0)
wl = synthetic.Workload(6, 3, 11)
X, Y = wl.rows(0, 6000)
X, Y = np.asarray(X), np.asarray(Y)
rows = np.arange(4) * 7
Ks = (1, 2, 7, 256, 257, 1000, 4097)
probs = (0.025, 0.5, 0.975, 0.1, 0.0, 1.0)
truth = Y[rows + 1]
out = dict(Y=Y, Ks=np.array(Ks), probs=np.array(probs), truth=truth)
for name, method, kernel in (("rej", "rejection", "epanechnikov"), ("ll0", "loclinear", "epanechnikov"),
                             ("ll1", "loclinear", "rectangular")):
    r = abcutil.particle_ranking_PLS_targets_path_summary(X, Y, X[rows], 0.5, Ks, probs=probs, truth=truth, method=method,
                                                          kernel=kernel, exclude=rows, ctx=ctx)
    out[name + "_quant"], out[name + "_cdf"] = r["quant"], r["cdf"]
    out["idx"] = r["idx"]
np.savez(sys.argv[1], **out)
