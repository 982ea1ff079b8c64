"""Worker of test_gpu_hpd.py::test_forced_global_path_gives_the_lds_bits: the highest-density intervals of fixed rankings at
K = 4096 (method 0; method 1 with both kernels) and of a given matrix with equal and unequal weights.  Run as a program it writes
them to the .npz named on the command line; the parent sets ABC_DIAG=1 and ABC_SUMMARY_PATH=global for it and calls compute()
itself for the LDS path's bits."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

MASS = (1e-6, 0.5, 0.95, 1 - 1e-9)
K = 4096


def generic_inputs():
    rng = np.random.default_rng(5)
    V = np.round(rng.normal(size=(K, 2)), 2)
    w = rng.uniform(0.0, 1.0, size=K)
    w[::97] = 0.0
    return V, w


def compute():
    from abcsmc_amd import _lib, abcutil, synthetic
    ctx = _lib.default_context(0)
    wl = synthetic.Workload(6, 3, 11)
    X, Y = wl.rows(0, 5000)
    X, Y = np.asarray(X), np.asarray(Y)
    rows = np.arange(3) * 7
    out = {}
    for name, method, kernel in (("rej", "rejection", "epanechnikov"), ("ll0", "loclinear", "epanechnikov"),
                                 ("ll1", "loclinear", "rectangular")):
        r = abcutil.particle_ranking_PLS_targets_hpd(X, Y, X[rows], 0.5, K, mass=MASS, method=method, kernel=kernel, exclude=rows,
                                                     ctx=ctx)
        for k in ("lo", "hi", "plo", "phi"):
            out[name + "_" + k] = r[k]
    V, w = generic_inputs()
    for name, ww in (("gen_eq", None), ("gen_w", w)):
        r = abcutil.weighted_hpd(V, ww, mass=MASS, ctx=ctx)
        for k in ("lo", "hi", "plo", "phi"):
            out[name + "_" + k] = r[k]
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **compute())
