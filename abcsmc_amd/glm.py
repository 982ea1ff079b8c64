"""Host-side wrappers of the ABC-GLM posterior of the batched ranking (abc_glm_particle_ranking_pls_targets, abc_glm_weighted;
include/abcsmc_hip.h; Leuenberger & Wegmann 2010).  Built on abcutil's call helpers, and reachable as
abcutil.particle_ranking_PLS_targets_glm, abcutil.weighted_glm and abcutil.cross_validate_pls_glm as well: abcutil forwards the
three names here, as it does for hpd.py and entropy.py."""
import ctypes as C

import numpy as np

from . import _lib
from . import abcutil as U

OUTPUTS = tuple(k for k in _lib.GLM_OUTPUTS if k not in ("peaks", "c"))


def _glm_arg(G, cut, bw_scale, bw, lead, K, P, nA, outputs):
    """Host arrays for the GLM outputs of prod(lead) targets (C, c0 and sigma_s with room for nA components) and the abc_glm
    pointing at them"""
    unknown = set(outputs) - set(_lib.GLM_OUTPUTS)
    if unknown:
        raise ValueError("unknown outputs %s" % sorted(unknown))
    nA = min(int(nA), _lib.GLM_MAX)
    sh = _lib.glm_shapes(lead, K, P, nA, int(G))
    o = {k: (np.empty(sh[k], dtype=np.int32 if k == "status" else np.float64) if k in outputs else None) for k in _lib.GLM_OUTPUTS}
    if bw is not None:
        bw = np.ascontiguousarray(np.broadcast_to(np.asarray(bw, dtype=np.float64), tuple(lead) + (P,)))
    d = _lib.Glm(int(G), float(cut), float(bw_scale), U._p(bw), *[U._p(o[k]) for k in _lib.GLM_OUTPUTS])
    return d, o, (bw,)


def _levels(probs):
    """probs as a contiguous float64 vector of 1 to 64 levels strictly inside (0, 1), or None"""
    if probs is None:
        return None
    pr = np.ascontiguousarray(np.asarray(probs, dtype=np.float64).reshape(-1))
    if not (1 <= pr.size <= 64):
        raise ValueError("probs needs 1 to 64 levels")
    if not np.all((pr > 0.0) & (pr < 1.0)):
        raise ValueError("every level of probs must lie strictly inside (0, 1): the mixture's quantile at 0 or 1 is infinite")
    return pr


def _summary_arg(probs, truth, lead, P):
    """Host arrays for the exact quantiles and CDF of prod(lead) targets and the abc_summary pointing at them"""
    pr = _levels(probs)
    tr = None
    if truth is not None:
        tr = np.asarray(truth, dtype=np.float64)
        if tr.shape != tuple(lead) + (P,):
            raise ValueError("truth must have shape %s" % (tuple(lead) + (P,),))
        tr = np.ascontiguousarray(tr)
    o = dict(quant=None if pr is None else np.empty(tuple(lead) + (pr.size, P)), cdf=None if tr is None else np.empty(tuple(lead) + (P,)))
    sm = _lib.Summary(U._p(pr), 0 if pr is None else pr.size, U._p(tr), U._p(o["quant"]), U._p(o["cdf"]))
    return sm, o, (pr, tr)


def _unpack(o, lead, P, n):
    """C, c0 and sigma_s as the library packed them: at the model's n components"""
    B = int(np.prod(lead, dtype=np.int64))
    for k, tail in (("C", (n, P)), ("c0", (n,)), ("sigma_s", (n, n))):
        if o[k] is not None:
            m = int(np.prod(tail))
            o[k] = o[k].reshape(-1)[:B * m].reshape(tuple(lead) + tail).copy()
    return o


def particle_ranking_PLS_targets_glm(X_orig, Y_orig, targets, training_fraction, K, G=512, cut=3.0, bw=None, bw_scale=1.0,
                                     exclude=None, max_comp=0, rule=_lib.RULE_DEFAULT, ctx=None, row_weights=None, outputs=OUTPUTS,
                                     probs=None, truth=None):
    """particle_ranking_PLS_targets followed by the ABC-GLM posterior of every target on the device
    (abc_glm_particle_ranking_pls_targets; the definition is in the header): a general linear model of the PLS scores on the
    parameters fitted on the K retained rows, the retained sample as a mixture of Gaussian peaks of the marginal density's
    bandwidths (bw: given ones (B, P), else the bw.nrd0 rule times bw_scale), multiplied analytically by the likelihood of the
    observed scores.  Rows weigh their row_weights (1 without).  Returns dict(mean, var, mode, mode_dens, lo_x, step (B, P),
    dens (B, P, G) at x_g = fma(g, step, lo_x), ess, log_md (B,): the evidence, status (B,) int32, C (B, n, P), c0 (B, n),
    sigma_s (B, n, n), T (B, P, P), peaks (B, K, P) and c (B, K) when asked for, idx, dist (B, K), ncomp).  outputs: the members
    to compute, the others are None (with probs or truth all of them may be).  Parameter transforms, hcorr and ridge have no
    meaning here: the library refuses a context that holds one.
    probs (1 to 64 levels strictly inside (0, 1)) and truth (B, P): the exact quantiles quant (B, nq, P) of the marginal mixtures
    and their CDF at the truth, cdf (B, P) (abc_glm_particle_ranking_pls_targets_summary); with both None the call and its result
    are those without."""
    X, Y, T, N, M, P, B, K, ex = U._targets_args(X_orig, Y_orig, targets, training_fraction, K, exclude)
    summary = probs is not None or truth is not None
    if summary:                                            # (refused here before a context is asked for)
        sm, so, _keep2 = _summary_arg(probs, truth, (B,), P)
    ctx = U._ctx(ctx)
    A = max_comp if max_comp > 0 else min(M, P)
    d, o, _keep = _glm_arg(G, cut, bw_scale, bw, (B,), K, P, A, outputs)
    idx = np.empty((B, K), dtype=np.uint64)
    dist = np.empty((B, K))
    ncomp = C.c_int32(0)
    tail = (ctx.handle, U._p(X), U._p(Y), N, M, P, U._p(T), B, float(training_fraction), int(max_comp), int(rule), U._p(ex), K,
            U._p(idx), U._p(dist), C.addressof(ncomp))
    if not summary:
        call = lambda: ctx.check(_lib.lib().abc_glm_particle_ranking_pls_targets(C.byref(d), *tail))
    else:
        call = lambda: ctx.check(_lib.lib().abc_glm_particle_ranking_pls_targets_summary(C.byref(d), C.byref(sm), *tail))
        o.update(so)
    U._with_transf(ctx, None, None, P, row_weights=row_weights, call=call)
    _unpack(o, (B,), P, ncomp.value)
    o.update(idx=idx, dist=dist, ncomp=ncomp.value)
    return o


def weighted_glm(theta, stats, obs, weights=None, G=512, cut=3.0, bw=None, bw_scale=1.0, ctx=None, outputs=OUTPUTS, probs=None,
                 truth=None):
    """The ABC-GLM posterior of any retained sample with any statistics on the device (abc_glm_weighted): theta (K, P), stats
    (K, n), obs (n,), weights K values or None (equal).  Returns particle_ranking_PLS_targets_glm's outputs without the leading
    target axis.  probs and truth (P,): quant (nq, P) and cdf (P,) as there (abc_glm_weighted_summary)."""
    th, st = U._f(theta), U._f(stats)
    if th.ndim == 1:
        th = U._f(th.reshape(-1, 1))
    if st.ndim == 1:
        st = U._f(st.reshape(-1, 1))
    K, P = th.shape
    n = st.shape[1]
    ob = np.ascontiguousarray(np.asarray(obs, dtype=np.float64).reshape(-1))
    if st.shape[0] != K or ob.size != n:
        raise ValueError("shape mismatch")
    w = None if weights is None else np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
    if w is not None and w.size != K:
        raise ValueError("weights needs one entry per row")
    summary = probs is not None or truth is not None
    if summary:                                            # (refused here before a context is asked for)
        sm, so, _keep2 = _summary_arg(probs, truth, (), P)
    ctx = U._ctx(ctx)
    d, o, _keep = _glm_arg(G, cut, bw_scale, bw, (), K, P, n, outputs)
    if not summary:
        ctx.check(_lib.lib().abc_glm_weighted(C.byref(d), ctx.handle, U._p(th), U._p(st), K, P, n, U._p(ob), U._p(w)))
    else:
        ctx.check(_lib.lib().abc_glm_weighted_summary(C.byref(d), C.byref(sm), ctx.handle, U._p(th), U._p(st), K, P, n, U._p(ob), U._p(w)))
        o.update(so)
    for k in ("ess", "log_md", "status"):
        if o[k] is not None:
            o[k] = o[k][()]
    return o


def cross_validate_pls_glm(X_orig, Y_orig, n_targets, K, seed, training_fraction=0.5, max_comp=0, rule=_lib.RULE_DEFAULT, ctx=None,
                           statistic="mean", bw_scale=1.0, row_weights=None, posterior=None, probs=None, coverage=False):
    """Leave-one-out cross-validation of the ABC-GLM estimate, as abcutil.cross_validate_pls (cv4abc of the R package abc): the same
    rows for the same seed serve as pseudo-observed data, each ranked with itself excluded, and the posterior mean (statistic
    "mean") or mode ("mode") of its ABC-GLM posterior estimates its parameters.  Returns dict(rows, theta, post_<statistic>,
    pred_error (P,) as cross_validate_pls's, log_md, status, idx, ncomp).  posterior: the function that answers for
    particle_ranking_PLS_targets_glm (same arguments and result); None: the device.
    statistic "median": the exact median of every marginal (the level 0.5).  probs: levels strictly inside (0, 1), the result gains
    quant (n, nq, P).  coverage=True: the truth of a target is its own parameter row; the result gains truth_cdf (n, P), the
    posterior quantile of the truth in each marginal (ABCtoolbox's validation of this estimator, Wegmann et al. 2010), ci95 (P,), the
    share of the targets of status 0 with 0.025 <= truth_cdf <= 0.975, and coverage_ks (P,) (abcutil.coverage_ks).  Without
    probs, coverage and "median" the call handed to posterior is the one it was."""
    X, Y = U._f(X_orig), U._f(Y_orig)
    N = X.shape[0]
    n_targets = int(n_targets)
    if not (1 <= n_targets <= N):
        raise ValueError("n_targets must be in [1, N]")
    if statistic not in ("mean", "mode", "median"):
        raise ValueError("statistic must be 'mean', 'mode' or 'median'")
    pr = _levels(probs)
    rows = np.sort(np.random.default_rng(seed).choice(N, size=n_targets, replace=False)).astype(np.int64)
    theta = np.ascontiguousarray(Y[rows])
    call = particle_ranking_PLS_targets_glm if posterior is None else posterior
    kw = {} if row_weights is None else dict(row_weights=row_weights)
    median = statistic == "median"
    levels = pr
    if median:                                             # the level 0.5 behind the caller's own
        levels = np.array([0.5]) if pr is None else np.concatenate([pr, [0.5]])
        if levels.size > 64:
            raise ValueError("probs needs at most 63 levels beside the median's")
    if levels is not None:
        kw["probs"] = levels
    if coverage:
        kw["truth"] = theta
    r = call(X, Y, X[rows], training_fraction, K, bw_scale=bw_scale, exclude=rows, max_comp=max_comp, rule=rule, ctx=ctx,
             outputs=("log_md", "status") if median else (statistic, "log_md", "status"), **kw)
    pm = r["quant"][:, -1, :] if median else r[statistic]
    var = theta.var(axis=0, ddof=1) if n_targets > 1 else np.zeros(theta.shape[1])
    sse = ((pm - theta) ** 2).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(var > 0, sse / (n_targets * np.where(var > 0, var, 1.0)), np.nan)
    out = dict(rows=rows, theta=theta, pred_error=err, log_md=r["log_md"], status=r["status"], idx=r["idx"], ncomp=r["ncomp"])
    out["post_" + statistic] = pm
    if pr is not None:
        out["quant"] = r["quant"][:, :pr.size, :]
    if coverage:
        u = r["cdf"]
        ok = np.asarray(r["status"]) == 0
        out["truth_cdf"] = u
        with np.errstate(invalid="ignore"):
            inside = (u >= 0.025) & (u <= 0.975)
        out["ci95"] = inside[ok].mean(axis=0) if ok.any() else np.full(u.shape[1], np.nan)
        out["coverage_ks"] = U.coverage_ks(u)
    return out
