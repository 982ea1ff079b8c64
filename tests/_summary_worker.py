"""Worker of test_gpu_summary.py::test_forced_paths_agree: the summaries of fixed rankings (methods 0 and 1, both kernels) and
of a given weighted matrix, written to the .npz named on the command line.  The parent sets ABC_DIAG=1 and ABC_SUMMARY_PATH."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from abcsmc_amd import _lib, abcutil, synthetic

ctx = _lib.default_context(0)
wl = synthetic.Workload(6, 3, 11)
X, Y = wl.rows(0, 3000)
X, Y = np.asarray(X), np.asarray(Y)
rows = np.arange(5) * 7
probs = (0.025, 0.5, 0.975, 0.1, 0.0, 1.0)
out = {}
for name, method, kernel in (("rej", "rejection", "epanechnikov"), ("ll0", "loclinear", "epanechnikov"),
                             ("ll1", "loclinear", "rectangular")):
    r = abcutil.particle_ranking_PLS_targets_summary(X, Y, X[rows], 0.5, 2500, probs=probs, truth=Y[rows], method=method,
                                                     kernel=kernel, exclude=rows, ctx=ctx)
    out[name + "_quant"], out[name + "_cdf"] = r["quant"], r["cdf"]
rng = np.random.default_rng(5)
V = np.round(rng.normal(size=(4000, 2)), 1)
w = rng.uniform(0.0, 1.0, size=4000)
for name, ww in (("gen_eq", None), ("gen_w", w)):
    r = abcutil.weighted_summary(V, ww, probs=probs, truth=V[17], ctx=ctx)
    out[name + "_quant"], out[name + "_cdf"] = r["quant"], r["cdf"]
np.savez(sys.argv[1], **out)
