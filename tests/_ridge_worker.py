"""Worker of test_gpu_ridge.py::test_table_and_direct_gather_agree: the ridge adjustment of a fixed set through the host entry,
written to the .npz named on the command line.  The parent sets ABC_DIAG=1 and ABC_ADJ_GATHER."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from abcsmc_amd import _lib, abcutil
from test_gpu_hcorr import hetero_data

ctx = _lib.default_context(0)
X, Y = hetero_data(1500, 5, 3, 41)
rows = np.arange(4) * 11
out = {}
for name, kernel in (("e", "epanechnikov"), ("r", "rectangular")):
    r = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[rows], 0.5, 300, exclude=rows, kernel=kernel, max_comp=3, rule=0,
                                                    ctx=ctx, ridge=(0.0, 1e-3, 1e-2, 1e-1, 1.0))
    for k in ("idx", "theta", "weight", "coef", "ridge_pick", "ridge_press"):
        out[name + "_" + k] = r[k]
np.savez(sys.argv[1], **out)
