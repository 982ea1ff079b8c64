"""Host-side wrappers of the posterior entropy of the batched ranking (abc_particle_ranking_pls_targets_entropy,
abc_weighted_entropy; include/abcsmc_hip.h), the product of an unweighted sample.  Built on abcutil's call helpers, and reachable as
abcutil.particle_ranking_PLS_targets_entropy and abcutil.knn_entropy as well: abcutil forwards the two names here.  They are kept
out of abcutil's own functions because those named particle_ranking_PLS_targets* are the family that works under row importance
weights, which this estimator refuses."""
import numpy as np

from . import _lib
from . import abcutil as U


def _entropy_arg(k, scale, lead, K, P):
    """Host arrays for the entropy of prod(lead) targets with K entries of P parameters and the abc_entropy pointing at them"""
    sc = _lib._host_doubles(scale, P, "scale")
    o = dict(H=np.empty(lead), knn=np.empty(lead + (K,)), zeros=np.empty(lead, dtype=np.uint64))
    d = _lib.Entropy(int(k), U._p(sc), U._p(o["H"]), U._p(o["knn"]), U._p(o["zeros"]))
    return d, o, (sc,)


def particle_ranking_PLS_targets_entropy(X_orig, Y_orig, targets, training_fraction, K, k=4, scale=None, method="rejection",
                                         kernel="rectangular", exclude=None, max_comp=0, rule=_lib.RULE_DEFAULT, ctx=None,
                                         transf=None, bounds=None, hcorr=False, ridge=None, row_weights=None):
    """particle_ranking_PLS_targets followed by the k-nearest-neighbour entropy of every target's posterior in all P parameters at
    once, computed on the device (abc_particle_ranking_pls_targets_entropy; the definition is in the header): the
    Kozachenko-Leonenko estimate over the target's K retained rows (method "rejection") or adjusted rows ("loclinear"; transf,
    bounds, hcorr and ridge as particle_ranking_PLS_targets_summary).  The lower, the more concentrated: the number the
    minimum-entropy criterion of Nunes & Balding (2010) compares (min_entropy_components).  k: the neighbour order, 1..8 (abctools
    uses 4).  scale: None, P positive values that the parameters are divided by before distances are taken, or "sd": the standard
    deviations of Y's columns, which makes H independent of the parameters' units.  The estimator is for an unweighted sample:
    "loclinear" needs kernel="rectangular" (the default here) and there may be no row importance weights, neither in the context
    nor as row_weights (handed on as it is); the library refuses the rest and says which
    it was.  Returns dict(H (B,): NaN when K <= k or a value is not finite, -inf when zeros > 0; knn (B, K): each
    entry's distance to its k-th nearest neighbour; zeros (B,): entries with k or more exact duplicates; idx (B, K), dist (B, K),
    ncomp)."""
    if isinstance(scale, str):
        if scale != "sd":
            raise ValueError("scale must be None, 'sd' or one value per parameter")
        scale = np.std(np.asarray(Y_orig, dtype=np.float64), axis=0, ddof=1)
    return U._targets_product("entropy", lambda lead, P: _entropy_arg(k, scale, lead, int(K), P), X_orig, Y_orig, targets,
                            training_fraction, K, method, kernel, exclude, max_comp, rule, ctx, transf, bounds, hcorr, ridge, row_weights)


def knn_entropy(values, k=4, scale=None, ctx=None):
    """The k-nearest-neighbour entropy of the rows of values (K, P) as one unweighted sample, on the device (abc_weighted_entropy;
    the definition is in the header); k and scale (None or P positive values) as particle_ranking_PLS_targets_entropy.  Returns
    dict(H, knn (K,), zeros)."""
    V = np.asarray(values, dtype=np.float64)
    K = V.shape[0]
    return U._weighted_product("entropy", lambda lead, P: _entropy_arg(k, scale, lead, K, P), V, None, ctx)
