"""Host-side wrappers of the highest-density intervals of the batched ranking (abc_particle_ranking_pls_targets_hpd,
abc_weighted_hpd; include/abcsmc_hip.h).  Built on abcutil's call helpers, and reachable as
abcutil.particle_ranking_PLS_targets_hpd and abcutil.weighted_hpd as well: abcutil forwards the two names here, as it does for
entropy.py."""
import numpy as np

from . import _lib
from . import abcutil as U


def _hpd_arg(mass, lead, P, outputs=("lo", "hi", "plo", "phi")):
    """Host arrays for the highest-density intervals of prod(lead) targets with P parameters and the abc_hpd pointing at them"""
    ms = np.ascontiguousarray(np.asarray(mass, dtype=np.float64).reshape(-1))
    o = {k: (np.empty(lead + (ms.size, P)) if k in outputs else None) for k in ("lo", "hi", "plo", "phi")}
    return _lib.Hpd(ms.ctypes.data, ms.size, U._p(o["lo"]), U._p(o["hi"]), U._p(o["plo"]), U._p(o["phi"])), o, (ms,)


def particle_ranking_PLS_targets_hpd(X_orig, Y_orig, targets, training_fraction, K, mass=(0.5, 0.95), method="rejection",
                                     kernel="epanechnikov", exclude=None, max_comp=0, rule=_lib.RULE_DEFAULT, ctx=None, transf=None,
                                     bounds=None, hcorr=False, ridge=None, row_weights=None, outputs=("lo", "hi", "plo", "phi")):
    """particle_ranking_PLS_targets followed by the highest-density interval of every target's posterior in every parameter: the
    shortest interval that holds each mass, computed on the device (abc_particle_ranking_pls_targets_hpd; the definition is in the
    header).  Values and weights are particle_ranking_PLS_targets_summary's, with the same method, kernel, transf, bounds, hcorr,
    ridge and row_weights.  mass: 1 to 16 values inside (0, 1).  Returns dict(lo, hi (B, nm, P): [b, m, j], the interval's ends;
    plo, phi (B, nm, P): their probabilities, so that (lo, hi) are the summary's quantiles at (plo, phi); mass, idx (B, K),
    dist (B, K), ncomp).  outputs: the members to compute, the others are None."""
    def make(lead, P):
        d, o, keep = _hpd_arg(mass, lead, P, outputs)
        o["mass"] = keep[0]
        return d, o, keep
    return U._targets_product("hpd", make, X_orig, Y_orig, targets, training_fraction, K, method, kernel, exclude, max_comp, rule, ctx,
                            transf, bounds, hcorr, ridge, row_weights)


def weighted_hpd(values, weights=None, mass=(0.95,), ctx=None, outputs=("lo", "hi", "plo", "phi")):
    """The highest-density intervals of every column of values (K, P) on the device (abc_weighted_hpd; the definition is in the
    header): equal weights when weights is None.  With equal weights and integer K * mass the interval is coda::HPDinterval's.
    Returns dict(lo, hi, plo, phi (nm, P))."""
    return U._weighted_product("hpd", lambda lead, P: _hpd_arg(mass, lead, P, outputs), values, weights, ctx)
