"""Host-side mirror of the reference's `namespace ABC` free functions (AbcUtil.h:78-172).

Same names, argument meaning and error behaviour as the reference (asserts / exits become
exceptions); every function is a thin call into the C ABI (include/abcsmc_hip.h), which runs the
HIP kernels.  Inputs are numpy arrays (host memory, as the reference's Eigen matrices); matrices
are converted to column-major float64, the reference's Mat2D layout.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Rng, lib, default_context


def _f(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ctx(ctx):
    return ctx if ctx is not None else default_context(0)


def rng(seed):
    """gsl_rng_alloc(gsl_rng_taus2) + gsl_rng_set (examples/include/examples.h:10,64)."""
    r = Rng()
    lib().abc_rng_set(C.byref(r), C.c_ulong(seed))
    return r


def rng_get(r):
    return lib().abc_rng_get(C.byref(r))


def particle_ranking_PLS(X_orig, Y_orig, target_values, training_fraction, K=None, max_comp=0,
                         rule=_lib.RULE_DEFAULT, details=False, ctx=None):
    """ABC::particle_ranking_PLS (AbcUtil.cpp:423-458).  Returns the ascending-distance particle
    indices (first K; K=None -> all N as the reference)."""
    ctx = _ctx(ctx)
    X, Y, obs = _f(X_orig), _f(Y_orig), _f(target_values)
    N, M = X.shape
    P = Y.shape[1]
    if Y.shape[0] != N or obs.size != M:
        raise ValueError("shape mismatch")
    if not (0 < training_fraction <= 1):
        raise ValueError("training_fraction must be in (0,1]")        # assert at AbcUtil.cpp:428
    K = N if K is None else int(K)
    A = max_comp if max_comp > 0 else min(M, P)
    idx = np.empty(K, dtype=np.uint64)
    dist = np.empty(K)
    ncomp = C.c_int32(0)
    R = np.empty((M, A), order="F")
    mean = np.empty(M)
    sd = np.empty(M)
    ctx.check(lib().abc_particle_ranking_pls(ctx.handle, _p(X), _p(Y), _p(obs), N, M, P,
                                             float(training_fraction), int(max_comp), int(rule), K,
                                             _p(idx), _p(dist), C.addressof(ncomp), _p(R), _p(mean), _p(sd)))
    if details:
        return dict(idx=idx, dist=dist, ncomp=ncomp.value, R=R, mean=mean, sd=sd)
    return idx


def _targets_args(X_orig, Y_orig, targets, training_fraction, K, exclude):
    """What the particle_ranking_PLS_targets family shares: column-major X, Y and targets (B, M), the sizes, K as an int and
    exclude as uint64 (B,) or None."""
    X, Y = _f(X_orig), _f(Y_orig)
    T = _f(np.atleast_2d(np.asarray(targets, dtype=np.float64)))
    N, M = X.shape
    P = Y.shape[1]
    B = T.shape[0]
    if Y.shape[0] != N or T.shape[1] != M:
        raise ValueError("shape mismatch")
    if not (0 < training_fraction <= 1):
        raise ValueError("training_fraction must be in (0,1]")
    K = int(K)
    ex = None
    if exclude is not None:
        ex = np.asarray(exclude, dtype=np.int64).astype(np.uint64)
        if ex.shape != (B,):
            raise ValueError("exclude needs one entry per target")
    return X, Y, T, N, M, P, B, K, ex


def _choice(what, value, table):
    if value not in table:
        raise ValueError("%s must be one of %s" % (what, sorted(table)))
    return table[value]


def _transf_kinds(transf, bounds, P):
    """(kind int32 (P,), lo (P,), hi (P,)) of a transf / bounds pair: transf a sequence of "none" / "log" / "logit" of length P,
    bounds (P, 2) read for the "logit" rows (None when there is none)"""
    b = None if bounds is None else np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
    kind, lo, hi = _lib.transf_arrays(transf, None if b is None else b[:, 0], None if b is None else b[:, 1])
    if kind.size != P or (b is not None and b.shape[0] != P):
        raise ValueError("transf needs one entry per parameter, bounds one row per parameter")
    if np.any((kind < 0) | (kind > 2)):
        raise ValueError("transf entries must be 'none', 'log' or 'logit'")
    return kind, lo, hi


def transform_params(Y, transf, bounds=None):
    """The forward parameter transforms of the local-linear adjustment in NumPy (the definition is in the header, "log and logit
    parameter transforms"): Y (..., P); "none": the value itself, bit for bit; "log": log(y) for finite y > 0, otherwise NaN (0
    too); "logit": log((y - lo) / (hi - y)) for lo < y < hi, otherwise NaN.  Works in Y's floating type (float64 by default)."""
    Y = np.asarray(Y)
    if Y.dtype.kind != "f":
        Y = Y.astype(np.float64)
    kind, lo, hi = _transf_kinds(transf, bounds, Y.shape[-1])
    T = Y.copy()
    ft = Y.dtype.type
    with np.errstate(all="ignore"):
        for j in range(kind.size):
            y = Y[..., j]
            if kind[j] == _lib.TRANSF_LOG:
                ok = (y > 0) & np.isfinite(y)
                T[..., j] = np.where(ok, np.log(np.where(ok, y, 1)), np.nan)
            elif kind[j] == _lib.TRANSF_LOGIT:
                l, h = ft(lo[j]), ft(hi[j])
                ok = (y > l) & (y < h)
                ys = np.where(ok, y, (l + h) / 2)
                T[..., j] = np.where(ok, np.log((ys - l) / (h - ys)), np.nan)
    return T


def untransform_params(T, transf, bounds=None):
    """The back direction of transform_params: NaN stays NaN; "log": exp(t); "logit": s = 1 / (1 + exp(-t)), y = (hi - lo) s + lo
    (one rounding, as fma) clamped to [lo, hi], so t = -inf gives lo and t = +inf gives hi; "none": the value itself."""
    T = np.asarray(T)
    if T.dtype.kind != "f":
        T = T.astype(np.float64)
    kind, lo, hi = _transf_kinds(transf, bounds, T.shape[-1])
    Y = T.copy()
    LD = np.longdouble
    ft = T.dtype.type
    with np.errstate(all="ignore"):
        for j in range(kind.size):
            t = T[..., j]
            if kind[j] == _lib.TRANSF_LOG:
                Y[..., j] = np.where(np.isnan(t), t, np.exp(t))
            elif kind[j] == _lib.TRANSF_LOGIT:
                l, h = ft(lo[j]), ft(hi[j])
                s = 1 / (1 + np.exp(-t))
                # fma(hi - lo, s, lo): the product of two float64 is exact in the 64-bit significand of x86's long double only up
                # to a second rounding, so the sum is made there and rounded once more; where long double is float64 this is the
                # plain expression
                y = ((h - l).astype(LD) * s.astype(LD) + LD(l)).astype(T.dtype) if T.dtype == np.float64 else (h - l) * s + l
                y = np.where(np.isposinf(t), h, np.where(np.isneginf(t), l, np.minimum(np.maximum(y, l), h)))
                Y[..., j] = np.where(np.isnan(t), t, y)
    return Y


def _ridge_list(ridge):
    """ridge= as the list of penalties: one number or a sequence"""
    return [float(v) for v in np.atleast_1d(np.asarray(ridge, dtype=np.float64)).reshape(-1)]


def _ridge_out(ctx, o, ridge, lead):
    """adds the ridge adjustment's record of the call just made to its result o: ridge_lambda (L,), ridge_pick lead + (P,),
    ridge_press lead + (L, P)"""
    pick, press = ctx.last_ridge()
    o["ridge_lambda"] = np.asarray(_ridge_list(ridge))
    o["ridge_pick"] = pick.reshape(lead + pick.shape[1:])
    o["ridge_press"] = press.reshape(lead + press.shape[1:])
    return o


def _with_transf(ctx, transf, bounds, P, call, hcorr=False, ridge=None, row_weights=None):
    """call() under the context's parameter transforms transf / bounds (None: whatever the context holds), with hcorr under the
    heteroscedastic variance correction (False: whatever the context holds), with ridge under the ridge adjustment with those
    penalties (None: whatever the context holds) and with row_weights under those row importance weights (None: whatever the
    context holds); all restored afterwards"""
    if row_weights is not None:
        with ctx.row_weights(row_weights):
            return _with_transf(ctx, transf, bounds, P, call, hcorr, ridge)
    if ridge is not None:
        with ctx.adjust_ridge(_ridge_list(ridge)):
            return _with_transf(ctx, transf, bounds, P, call, hcorr)
    if hcorr:
        with ctx.adjust_hcorr(True):
            return _with_transf(ctx, transf, bounds, P, call)
    if transf is None:
        if bounds is not None:
            raise ValueError("bounds without transf")
        return call()
    kind, lo, hi = _transf_kinds(transf, bounds, P)
    with ctx.param_transf(kind, lo, hi):
        return call()


def _tf_kw(transf, bounds, hcorr=False, ridge=None, row_weights=None):
    """transf / bounds / hcorr / ridge / row_weights as keywords for a wrapped call, only when they are given"""
    kw = {}
    if row_weights is not None:
        kw["row_weights"] = row_weights
    if hcorr:
        kw["hcorr"] = True
    if ridge is not None:
        kw["ridge"] = ridge
    if transf is not None:
        kw["transf"] = transf
    if bounds is not None:
        kw["bounds"] = bounds
    return kw


def particle_ranking_PLS_targets(X_orig, Y_orig, targets, training_fraction, K, exclude=None, max_comp=0,
                                 rule=_lib.RULE_DEFAULT, details=False, ctx=None, row_weights=None):
    """particle_ranking_PLS for B observed targets at once (abc_particle_ranking_pls_targets): ONE fit shared by all of
    them.  targets: (B, M); exclude: B row numbers (or None; -1 / 2**64 - 1 = none) never ranked for their target (the row
    still takes part in the fit).  Returns idx (B, K): row b = the first K of particle_ranking_PLS(X, Y, targets[b]).
    details=True: dict(idx, dist (B, K), post_mean (B, P): mean parameter row of each target's K rows, ncomp).
    row_weights: None or one importance weight per row of the table (N finite weights >= 0, at least one positive;
    abc_ctx_set_row_weights, the definition is in the header), set in the context around this call, here and in every
    particle_ranking_PLS_targets* function below.  A table whose rows are not draws from the prior needs them: the rows of an SMC
    generation from set 1 on come from the previous set's perturbation kernel, and their weight prior / proposal is what
    weight_predictive_prior returns for all N rows of the generation; it is accepted as is, any positive scale is fine:
        w = weight_predictive_prior(priors, theta, theta_prev, w_prev, dv_prev)  # theta: the N rows of this generation
        r = particle_ranking_PLS_targets(X, theta, targets, 0.5, K, details=True, row_weights=w)
        r["post_mean"]                                                           # sum w_e theta_e / sum w_e of the K rows
    idx and dist never depend on the weights.  post_mean becomes the weighted mean; under the adjustment a row weighs its kernel
    weight times its row weight everywhere (weight, the fit, hcorr, ridge, every product under "loclinear"), and under
    "rejection" the products are the weighted products of the retained rows.  A target whose retained rows all weigh 0 is not
    fitted: status bit 2 (value 4), NaN in coef, theta and the products, ess 0."""
    ctx = _ctx(ctx)
    X, Y, T, N, M, P, B, K, ex = _targets_args(X_orig, Y_orig, targets, training_fraction, K, exclude)
    idx = np.empty((B, K), dtype=np.uint64)
    dist = np.empty((B, K))
    pm = np.empty((B, P))
    ncomp = C.c_int32(0)
    _with_transf(ctx, None, None, P, row_weights=row_weights, call=lambda: ctx.check(lib().abc_particle_ranking_pls_targets(
        ctx.handle, _p(X), _p(Y), N, M, P, _p(T), B, float(training_fraction), int(max_comp), int(rule), _p(ex), K, _p(idx),
        _p(dist), _p(pm), C.addressof(ncomp))))
    if details:
        return dict(idx=idx, dist=dist, post_mean=pm, ncomp=ncomp.value)
    return idx


_KERNELS = {"epanechnikov": _lib.KERNEL_EPANECHNIKOV, "rectangular": _lib.KERNEL_RECTANGULAR}


def particle_ranking_PLS_targets_adjust(X_orig, Y_orig, targets, training_fraction, K, exclude=None, kernel="epanechnikov",
                                        max_comp=0, rule=_lib.RULE_DEFAULT, theta=True, ctx=None, transf=None, bounds=None, hcorr=False, ridge=None, row_weights=None):
    """particle_ranking_PLS_targets followed by the local-linear regression adjustment of every target's K rows on their PLS
    scores (abc_particle_ranking_pls_targets_adjust; Beaumont, Zhang & Balding 2002; the definition is in the header).  kernel:
    "epanechnikov" (default) or "rectangular".  Returns dict(idx (B, K), dist (B, K), theta (B, K, P): the adjusted rows, or None
    with theta=False, weight (B, K), coef (B, A + 1, P): [b, 0] = alpha, [b, 1 + k] = beta_k, post_mean = coef[:, 0]: the
    adjusted posterior means, rank (B,), status (B,): bit 0 a component skipped, bit 1 rectangular fallback, ncomp).
    transf / bounds: parameter transforms ("none" / "log" / "logit" per parameter, bounds (P, 2) for the "logit" rows; as
    transf and logit.bounds of R's abc), set in the context around this call: the regression runs on transform_params(Y), coef
    is on that scale, and theta holds the adjusted rows carried back, which stay inside the support.  post_mean is then
    untransform_params(coef[:, 0]): the fitted value at the observation carried back.  It is NOT the mean of the adjusted rows
    (the back-transform is not linear); particle_ranking_PLS_targets_joint's mean gives that.
    hcorr=True: the heteroscedastic variance correction (hcorr = TRUE of R's abc; abc_ctx_set_adjust_hcorr, the definition is in
    the header), set in the context around this call: theta holds the rows with their residuals rescaled by the fitted model of
    the residual variance, and the dict gains hcoef (B, A + 1, P): [b, 0] the log residual variance at the observation (NaN: the
    parameter was skipped, its rows are the plain adjustment's), [b, 1 + k] its slope g_k.  coef, and so alpha and post_mean,
    do not change.
    ridge: None, one penalty or an ascending sequence of at most 8 (abc_ctx_set_adjust_ridge, the definition is in the header;
    method = "ridge" of R's abc), set in the context around this call: coef, and so alpha, post_mean and theta, is per parameter
    the ridge fit of the penalty with the smallest exact leave-one-out PRESS, and the dict gains ridge_lambda (L,), ridge_pick
    (B, P): the chosen penalty's index, and ridge_press (B, L, P) (+inf: the fit interpolates).  rank and status do not change."""
    ctx = _ctx(ctx)
    kernel = _choice("kernel", kernel, _KERNELS)
    X, Y, T, N, M, P, B, K, ex = _targets_args(X_orig, Y_orig, targets, training_fraction, K, exclude)
    A = max_comp if max_comp > 0 else min(M, P)
    idx = np.empty((B, K), dtype=np.uint64)
    dist = np.empty((B, K))
    th = np.empty((B, K, P)) if theta else None
    w = np.empty((B, K))
    coef = np.empty((B, A + 1, P))
    rank = np.empty(B, dtype=np.int32)
    status = np.empty(B, dtype=np.int32)
    out = _lib.AdjustOut(_p(th), _p(w), _p(coef), _p(rank), _p(status))
    ncomp = C.c_int32(0)
    _with_transf(ctx, transf, bounds, P, hcorr=hcorr, ridge=ridge, row_weights=row_weights, call=lambda: ctx.check(lib().abc_particle_ranking_pls_targets_adjust(
        ctx.handle, _p(X), _p(Y), N, M, P, _p(T), B, float(training_fraction), int(max_comp), int(rule), _p(ex), K, kernel, _p(idx),
        _p(dist), C.byref(out), C.addressof(ncomp))))
    pm = coef[:, 0] if transf is None else untransform_params(coef[:, 0], transf, bounds)
    r = dict(idx=idx, dist=dist, theta=th, weight=w, coef=coef, post_mean=pm, rank=rank, status=status, ncomp=ncomp.value)
    if hcorr:
        r["hcoef"] = ctx.last_hcorr()
    if ridge is not None:
        _ridge_out(ctx, r, ridge, (B,))
    return r


def particle_ranking_PLS_targets_path(X_orig, Y_orig, targets, training_fraction, Ks, kernel="epanechnikov", exclude=None,
                                      max_comp=0, rule=_lib.RULE_DEFAULT, ctx=None, transf=None, bounds=None, hcorr=False, ridge=None, row_weights=None):
    """Tolerance path (abc_particle_ranking_pls_targets_path): particle_ranking_PLS_targets ONCE at K_max = Ks[-1], then the
    rejection estimate and the local-linear fit of particle_ranking_PLS_targets_adjust at every tolerance of the strictly ascending
    list Ks (at most 16): what cv4abc computes for tols = c(...), without ranking once per tolerance.  Tolerance t uses the first
    Ks[t] retained rows only, with the bandwidth h = dist[:, Ks[t] - 1].  Returns dict(post_mean (B, T, P): the mean parameter row,
    coef (B, T, A + 1, P), alpha (B, T, P) = coef[:, :, 0]: the adjusted posterior means (a view), rank (B, T), status (B, T), h (B, T),
    Ks, idx (B, K_max), dist (B, K_max), ncomp).  transf / bounds as particle_ranking_PLS_targets_adjust: coef and alpha are then on
    the transformed scale, post_mean (the rejection mean of the raw rows) and h do not change, and the dict gains alpha_back =
    untransform_params(alpha): the fitted value at the observation carried back, not the mean of the adjusted rows.  hcorr=True
    (as particle_ranking_PLS_targets_adjust): nothing above changes, and the dict gains hcoef (B, T, A + 1, P), the second fit at
    every tolerance.  ridge (as particle_ranking_PLS_targets_adjust): coef and alpha at slot (b, t) are the ridge fit of that call
    with K = Ks[t], and the dict gains ridge_lambda, ridge_pick (B, T, P) and ridge_press (B, T, L, P); post_mean, h, rank and
    status do not change."""
    ctx = _ctx(ctx)
    kernel = _choice("kernel", kernel, _KERNELS)
    ks = np.ascontiguousarray(np.asarray(Ks, dtype=np.int64).reshape(-1).astype(np.uint64))
    X, Y, T, N, M, P, B, K, ex = _targets_args(X_orig, Y_orig, targets, training_fraction, ks[-1] if ks.size else 0, exclude)
    nt = ks.size
    A = max_comp if max_comp > 0 else min(M, P)
    idx = np.empty((B, K), dtype=np.uint64)
    dist = np.empty((B, K))
    pm = np.empty((B, nt, P))
    coef = np.empty((B, nt, A + 1, P))
    rank = np.empty((B, nt), dtype=np.int32)
    status = np.empty((B, nt), dtype=np.int32)
    h = np.empty((B, nt))
    path = _lib.Path(_p(ks), nt, _p(pm), _p(coef), _p(rank), _p(status), _p(h))
    ncomp = C.c_int32(0)
    _with_transf(ctx, transf, bounds, P, hcorr=hcorr, ridge=ridge, row_weights=row_weights, call=lambda: ctx.check(lib().abc_particle_ranking_pls_targets_path(
        ctx.handle, _p(X), _p(Y), N, M, P, _p(T), B, float(training_fraction), int(max_comp), int(rule), _p(ex), kernel, _p(idx),
        _p(dist), C.byref(path), C.addressof(ncomp))))
    r = dict(post_mean=pm, coef=coef, alpha=coef[:, :, 0], rank=rank, status=status, h=h, Ks=ks.astype(np.int64), idx=idx,
             dist=dist, ncomp=ncomp.value)
    if transf is not None:
        r["alpha_back"] = untransform_params(coef[:, :, 0], transf, bounds)
    if hcorr:
        r["hcoef"] = ctx.last_hcorr().reshape(B, nt, A + 1, P)
    if ridge is not None:
        _ridge_out(ctx, r, ridge, (B, nt))
    return r


_METHODS = {"rejection": _lib.POSTERIOR_REJECTION, "loclinear": _lib.POSTERIOR_LOCLINEAR}


def particle_ranking_PLS_targets_path_summary(X_orig, Y_orig, targets, training_fraction, Ks, probs=(0.025, 0.5, 0.975), truth=None,
                                              method="rejection", kernel="epanechnikov", exclude=None, max_comp=0,
                                              rule=_lib.RULE_DEFAULT, ctx=None, transf=None, bounds=None, hcorr=False, ridge=None, row_weights=None):
    """particle_ranking_PLS_targets_path with the summaries of particle_ranking_PLS_targets_summary at every tolerance
    (abc_particle_ranking_pls_targets_path_summary; the definition is in the header): the ranking, the fit and, under "rejection",
    the sort of every (target, parameter) are made once for all of Ks.  Tolerance t's quantiles and CDF are those of the summary
    call with K = Ks[t] (bit for bit under "rejection").  Returns the path's dict plus quant (B, T, nq, P): [b, t, q, j], cdf
    (B, T, P) or None, and probs.  transf / bounds as particle_ranking_PLS_targets_path; under "loclinear" the quantiles and the
    CDF are those of the adjusted rows carried back.  hcorr=True: under "loclinear" the quantiles and the CDF are those of the
    variance-corrected rows, and the dict gains hcoef (B, T, A + 1, P); ignored under "rejection".  ridge: under "loclinear" the
    path's coef is the ridge fit and the dict gains ridge_lambda, ridge_pick (B, T, P) and ridge_press (B, T, L, P); ignored under
    "rejection"."""
    ctx = _ctx(ctx)
    method, kernel = _choice("method", method, _METHODS), _choice("kernel", kernel, _KERNELS)
    ks = np.ascontiguousarray(np.asarray(Ks, dtype=np.int64).reshape(-1).astype(np.uint64))
    X, Y, T, N, M, P, B, K, ex = _targets_args(X_orig, Y_orig, targets, training_fraction, ks[-1] if ks.size else 0, exclude)
    nt = ks.size
    A = max_comp if max_comp > 0 else min(M, P)
    idx = np.empty((B, K), dtype=np.uint64)
    dist = np.empty((B, K))
    pm = np.empty((B, nt, P))
    coef = np.empty((B, nt, A + 1, P))
    rank = np.empty((B, nt), dtype=np.int32)
    status = np.empty((B, nt), dtype=np.int32)
    h = np.empty((B, nt))
    path = _lib.Path(_p(ks), nt, _p(pm), _p(coef), _p(rank), _p(status), _p(h))
    sm, o, keep = _summary_arg(probs, None, (B, nt), P)     # quant (B, T, nq, P); truth is per target, the CDF per tolerance
    tr = None
    if truth is not None:
        tr = np.ascontiguousarray(np.asarray(truth, dtype=np.float64).reshape(B, P))
        o["cdf"] = np.empty((B, nt, P))
        sm.truth, sm.cdf = tr.ctypes.data, o["cdf"].ctypes.data
    ncomp = C.c_int32(0)
    _with_transf(ctx, transf, bounds, P, hcorr=hcorr, ridge=ridge, row_weights=row_weights, call=lambda: ctx.check(lib().abc_particle_ranking_pls_targets_path_summary(
        ctx.handle, _p(X), _p(Y), N, M, P, _p(T), B, float(training_fraction), int(max_comp), int(rule), _p(ex), method, kernel,
        _p(idx), _p(dist), C.byref(path), C.byref(sm), C.addressof(ncomp))))
    if transf is not None:
        o["alpha_back"] = untransform_params(coef[:, :, 0], transf, bounds)
    if hcorr and method == _lib.POSTERIOR_LOCLINEAR:
        o["hcoef"] = ctx.last_hcorr().reshape(B, nt, A + 1, P)
    if ridge is not None and method == _lib.POSTERIOR_LOCLINEAR:
        _ridge_out(ctx, o, ridge, (B, nt))
    o.update(post_mean=pm, coef=coef, alpha=coef[:, :, 0], rank=rank, status=status, h=h, Ks=ks.astype(np.int64), idx=idx, dist=dist,
             ncomp=ncomp.value, probs=keep[0])
    return o


def _targets_product(product, make, X_orig, Y_orig, targets, training_fraction, K, method, kernel, exclude, max_comp, rule, ctx,
                     transf=None, bounds=None, hcorr=False, ridge=None, row_weights=None):
    """The call of particle_ranking_PLS_targets_{summary,density,joint,draws}.  make(lead, P) -> (the product's struct, its outputs as a
    dict, what must stay alive during the call) for lead = (B,).  Returns the outputs with idx, dist and ncomp added.  transf /
    bounds: the parameter transforms of particle_ranking_PLS_targets_adjust around the call ("loclinear" only; "rejection" does
    not regress and ignores them).  The product itself works on the parameter's own scale, after the back-transform: a density
    grid or a smoothed draw may still pass a bound, as in R.  hcorr=True: the heteroscedastic variance correction of
    particle_ranking_PLS_targets_adjust around the call: under "loclinear" the product is of the corrected rows; "rejection"
    ignores it.  ridge: the ridge adjustment of particle_ranking_PLS_targets_adjust around the call: under "loclinear" the product
    is of the rows adjusted with the ridge fit and the outputs gain ridge_lambda, ridge_pick (B, P) and ridge_press (B, L, P);
    "rejection" ignores it."""
    ctx = _ctx(ctx)
    method, kernel = _choice("method", method, _METHODS), _choice("kernel", kernel, _KERNELS)
    X, Y, T, N, M, P, B, K, ex = _targets_args(X_orig, Y_orig, targets, training_fraction, K, exclude)
    d, o, _keep = make((B,), P)
    idx = np.empty((B, K), dtype=np.uint64)
    dist = np.empty((B, K))
    ncomp = C.c_int32(0)
    entry = getattr(lib(), "abc_particle_ranking_pls_targets_" + product)
    _with_transf(ctx, transf, bounds, P, hcorr=hcorr, ridge=ridge, row_weights=row_weights, call=lambda: ctx.check(entry(
        ctx.handle, _p(X), _p(Y), N, M, P, _p(T), B, float(training_fraction), int(max_comp), int(rule), _p(ex), K, method, kernel,
        _p(idx), _p(dist), None, C.byref(d), C.addressof(ncomp))))
    o.update(idx=idx, dist=dist, ncomp=ncomp.value)
    if ridge is not None and method == _lib.POSTERIOR_LOCLINEAR:
        _ridge_out(ctx, o, ridge, (B,))
    return o


def _weighted_product(product, make, values, weights, ctx):
    """The call of weighted_{summary,density,joint,draws}: values as (K, P) column-major, weights as K contiguous values or None, and
    make as _targets_product's with lead = ().  Returns the outputs."""
    ctx = _ctx(ctx)
    V = _f(values)
    if V.ndim == 1:
        V = _f(V.reshape(-1, 1))
    K, P = V.shape
    w = None if weights is None else np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
    if w is not None and w.size != K:
        raise ValueError("weights needs one entry per row")
    d, o, _keep = make((), P)
    ctx.check(getattr(lib(), "abc_weighted_" + product)(ctx.handle, _p(V), K, P, _p(w), C.byref(d)))
    return o


def _summary_arg(probs, truth, lead, P):
    """Host arrays for the summaries of prod(lead) targets with P parameters and the abc_summary pointing at them"""
    pr = np.ascontiguousarray(np.asarray(probs, dtype=np.float64).reshape(-1))
    tr = None if truth is None else np.ascontiguousarray(np.asarray(truth, dtype=np.float64).reshape(lead + (P,)))
    o = dict(quant=np.empty(lead + (np.atleast_1d(probs).size, P)), cdf=np.empty(lead + (P,)) if tr is not None else None)
    return _lib.Summary(pr.ctypes.data, pr.size, _p(tr), _p(o["quant"]), _p(o["cdf"])), o, (pr, tr)


def particle_ranking_PLS_targets_summary(X_orig, Y_orig, targets, training_fraction, K, probs=(0.025, 0.5, 0.975), truth=None,
                                         method="rejection", kernel="epanechnikov", exclude=None, max_comp=0,
                                         rule=_lib.RULE_DEFAULT, ctx=None, transf=None, bounds=None, hcorr=False, ridge=None, row_weights=None):
    """particle_ranking_PLS_targets followed by weighted posterior quantiles of every target's K retained rows and, with truth
    (B, P), the posterior CDF at the truth (abc_particle_ranking_pls_targets_summary; the definition is in the header).
    method "rejection": the rows' parameters, equal weights; "loclinear": the local-linear adjusted rows with the kernel's weights
    (as particle_ranking_PLS_targets_adjust).  Returns dict(quant (B, nq, P): [b, q, j], cdf (B, P) or None, probs, idx (B, K),
    dist (B, K), ncomp).  transf / bounds ("loclinear" only, here and in the density, joint and draws calls below): the parameter
    transforms of particle_ranking_PLS_targets_adjust; the values are then the adjusted rows carried back, and everything
    computed from them (quantiles, densities, covariances, bandwidths, the smoothing of smoothed draws) is on the parameter's own
    scale, so a density grid or a smoothed draw may still pass a bound, as in R."""
    def make(lead, P):
        s, o, keep = _summary_arg(probs, truth, lead, P)
        o["probs"] = keep[0]
        return s, o, keep
    return _targets_product("summary", make, X_orig, Y_orig, targets, training_fraction, K, method, kernel, exclude, max_comp, rule,
                            ctx, transf, bounds, hcorr, ridge, row_weights)


def weighted_summary(values, weights=None, probs=(0.025, 0.5, 0.975), truth=None, ctx=None):
    """Weighted quantiles (and the CDF at truth) of every column of values (K, P) on the device (abc_weighted_summary; the
    definition is in the header): equal weights when weights is None; with equal weights the quantiles are NumPy's "hazen".
    Returns dict(quant (nq, P), cdf (P,) or None)."""
    return _weighted_product("summary", lambda lead, P: _summary_arg(probs, truth, lead, P), values, weights, ctx)


def _density_arg(G, cut, bw_scale, bw, lead, P, dens=True):
    """Host arrays for the densities of prod(lead) targets with P parameters and the abc_density pointing at them"""
    G = int(G)
    lead = lead + (P,)
    b = None
    if bw is not None:
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(bw, dtype=np.float64), lead))
    o = dict(dens=np.empty(lead + (G,)) if dens else None, grid=np.empty(lead + (2,)), bw=np.empty(lead), mode=np.empty(lead),
             mode_dens=np.empty(lead))
    d = _lib.Density(G, float(cut), float(bw_scale), _p(b), _p(o["dens"]), _p(o["grid"]), _p(o["bw"]), _p(o["mode"]),
                     _p(o["mode_dens"]))
    return d, o, b


def _grid_points(grid, G):
    """x (..., G) from grid (..., 2) = lo_x, step: x_g = lo_x + g * step in float64, within one rounding of the device's
    fma(g, step, lo_x) (which is what mode holds)"""
    return grid[..., 0:1] + np.arange(G, dtype=np.float64) * grid[..., 1:2]


def particle_ranking_PLS_targets_density(X_orig, Y_orig, targets, training_fraction, K, G=512, cut=3.0, bw=None, bw_scale=1.0,
                                         method="rejection", kernel="epanechnikov", exclude=None, max_comp=0,
                                         rule=_lib.RULE_DEFAULT, dens=True, ctx=None, transf=None, bounds=None, hcorr=False, ridge=None, row_weights=None):
    """particle_ranking_PLS_targets followed by the weighted Gaussian kernel density of every (target, parameter) on a grid of G
    points and the mode taken from it (abc_particle_ranking_pls_targets_density; the definition is in the header: R's density()
    with bw.nrd0, cut and adjust = bw_scale).  method and kernel as particle_ranking_PLS_targets_summary; bw: given bandwidths
    (B, P) (or a scalar) in place of the rule.  Returns dict(dens (B, P, G) (None with dens=False), x (B, P, G): the grid points,
    grid (B, P, 2): lo_x and step, bw (B, P): the bandwidths used, mode (B, P), mode_dens (B, P), idx (B, K), dist (B, K),
    ncomp)."""
    o = _targets_product("density", lambda lead, P: _density_arg(G, cut, bw_scale, bw, lead, P, dens), X_orig, Y_orig, targets,
                         training_fraction, K, method, kernel, exclude, max_comp, rule, ctx, transf, bounds, hcorr, ridge, row_weights)
    o["x"] = _grid_points(o["grid"], int(G))
    return o


def weighted_density(values, weights=None, G=512, cut=3.0, bw=None, bw_scale=1.0, ctx=None):
    """The weighted Gaussian kernel density and mode of every column of values (K, P) on the device (abc_weighted_density; the
    definition is in the header); equal weights when weights is None.  Returns dict(dens (P, G), x (P, G), grid (P, 2), bw (P,),
    mode (P,), mode_dens (P,))."""
    o = _weighted_product("density", lambda lead, P: _density_arg(G, cut, bw_scale, bw, lead, P), values, weights, ctx)
    o["x"] = _grid_points(o["grid"], int(G))
    return o


def _joint_arg(G, cut, bw_scale, bw, pairs, lead, P, dens):
    """Host arrays for the joint outputs of prod(lead) targets with P parameters and the abc_joint pointing at them"""
    G = int(G)
    b = None
    if bw is not None:
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(bw, dtype=np.float64), lead + (P,)))
    pr, given = _lib._joint_pairs(pairs, P)
    n = pr.shape[0]
    e = lambda *shape: np.empty(lead + shape)
    o = dict(mean=e(P), cov=e(P, P), corr=e(P, P), dens=e(n, G, G) if dens else None, grid=e(P, 2), bw=e(P), mode=e(n, 2),
             mode_dens=e(n), pairs=pr)
    d = _lib.Joint(G, float(cut), float(bw_scale), _p(b), _p(given), n if given is not None else 0, _p(o["mean"]), _p(o["cov"]),
                   _p(o["corr"]), _p(o["dens"]), _p(o["grid"]), _p(o["bw"]), _p(o["mode"]), _p(o["mode_dens"]))
    return d, o, (b, given)


def particle_ranking_PLS_targets_joint(X_orig, Y_orig, targets, training_fraction, K, G=64, cut=3.0, bw=None, bw_scale=1.0, pairs=None,
                                       method="rejection", kernel="epanechnikov", exclude=None, max_comp=0, rule=_lib.RULE_DEFAULT,
                                       dens=True, ctx=None, transf=None, bounds=None, hcorr=False, ridge=None, row_weights=None):
    """particle_ranking_PLS_targets followed by the joint posterior of every target, what a pairs plot draws
    (abc_particle_ranking_pls_targets_joint; the definition is in the header): the weighted means, the covariance matrix
    (numpy.cov with aweights) and the Pearson correlations of the P parameters, and for every pair of parameters in pairs (rows
    (i, j), i != j; None: all i < j) the product-Gaussian kernel density (as MASS::kde2d, with the marginal densities' bandwidths) on a
    G x G grid and its mode.  method, kernel, bw, cut and bw_scale as particle_ranking_PLS_targets_density.  dens holds
    B * npairs * G * G doubles (3.9 GB for 1000 targets, 120 pairs, G = 64): choose pairs, G or dens=False accordingly.  Returns
    dict(mean (B, P), cov (B, P, P), corr (B, P, P), dens (B, npairs, G, G) (None with dens=False; [g, g']: g along parameter i),
    x (B, P, G): every parameter's grid points, grid (B, P, 2), bw (B, P), mode (B, npairs, 2), mode_dens (B, npairs), pairs
    (npairs, 2), idx (B, K), dist (B, K), ncomp)."""
    o = _targets_product("joint", lambda lead, P: _joint_arg(G, cut, bw_scale, bw, pairs, lead, P, dens), X_orig, Y_orig, targets,
                         training_fraction, K, method, kernel, exclude, max_comp, rule, ctx, transf, bounds, hcorr, ridge, row_weights)
    o["x"] = _grid_points(o["grid"], int(G))
    return o


def weighted_joint(values, weights=None, G=64, cut=3.0, bw=None, bw_scale=1.0, pairs=None, dens=True, ctx=None):
    """The joint posterior of the columns of values (K, P) on the device (abc_weighted_joint; the definition is in the header);
    equal weights when weights is None.  Returns dict(mean (P,), cov (P, P), corr (P, P), dens (npairs, G, G) or None, x (P, G),
    grid (P, 2), bw (P,), mode (npairs, 2), mode_dens (npairs,), pairs (npairs, 2))."""
    o = _weighted_product("joint", lambda lead, P: _joint_arg(G, cut, bw_scale, bw, pairs, lead, P, dens), values, weights, ctx)
    o["x"] = _grid_points(o["grid"], int(G))
    return o


def _draws_arg(S, smooth, seed, bw, bw_scale, stream, lead, P):
    """Host arrays for the draws of prod(lead) targets with P parameters and the abc_draws pointing at them"""
    S = int(S)
    b = None
    if smooth and bw is not None:
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(bw, dtype=np.float64), lead + (P,)))
    ids = _lib._draws_stream(stream, int(np.prod(lead, dtype=np.int64)))
    o = dict(draws=np.empty(lead + (S, P)), src=np.empty(lead + (S,), dtype=np.uint64), ess=np.empty(lead), bw=np.empty(lead + (P,)))
    d = _lib.Draws(S, int(bool(smooth)), float(bw_scale), _p(b), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(ids), _p(o["draws"]), _p(o["src"]),
                   _p(o["bw"]), _p(o["ess"]))
    return d, o, (b, ids)


def particle_ranking_PLS_targets_draws(X_orig, Y_orig, targets, training_fraction, K, S, smooth=False, seed=0, method="rejection",
                                       kernel="epanechnikov", bw=None, bw_scale=1.0, stream=None, exclude=None, max_comp=0,
                                       rule=_lib.RULE_DEFAULT, ctx=None, transf=None, bounds=None, hcorr=False, ridge=None, row_weights=None):
    """particle_ranking_PLS_targets followed by S posterior draws of every target, made on the device
    (abc_particle_ranking_pls_targets_draws; the definition is in the header): rows of the target's K retained rows resampled with
    their weights (method and kernel as particle_ranking_PLS_targets_summary), as they are (smooth=False, the weighted bootstrap)
    or with h_j z_j added to parameter j (smooth=True, the smoothed bootstrap: a sample of the kernel density estimate of
    particle_ranking_PLS_targets_density with the same bw and bw_scale).  seed keys the Philox stream of the draws (the context's
    generator is not used); stream: one id per target (None: target b takes b), so that a target split off into another call keeps
    its draws.  Nothing is clipped to prior bounds.  Returns dict(draws (B, S, P), src (B, S): the position in 0..K-1 of the row
    each draw came from (idx[b, src[b, s]] is its row of the set), ess (B,): the effective sample size W^2 / sum w^2, bw (B, P):
    the bandwidths used (NaN with smooth=False), idx (B, K), dist (B, K), ncomp)."""
    return _targets_product("draws", lambda lead, P: _draws_arg(S, smooth, seed, bw, bw_scale, stream, lead, P), X_orig, Y_orig,
                            targets, training_fraction, K, method, kernel, exclude, max_comp, rule, ctx, transf, bounds, hcorr, ridge, row_weights)


def weighted_draws(values, weights=None, S=1000, smooth=False, seed=0, bw=None, bw_scale=1.0, stream=None, ctx=None):
    """S draws of the rows of values (K, P) with the given weights on the device (abc_weighted_draws; the definition is in the
    header); equal weights when weights is None; smooth, seed, bw and bw_scale as particle_ranking_PLS_targets_draws; stream: the
    one stream id (None: 0).  Returns dict(draws (S, P), src (S,), ess, bw (P,))."""
    return _weighted_product("draws", lambda lead, P: _draws_arg(S, smooth, seed, bw, bw_scale, stream, lead, P), values, weights,
                             ctx)


# The products of an unweighted sample (entropy.py) answer under this module's names too.  They are forwarded, not defined here: the
# functions this module defines under the name particle_ranking_PLS_targets* are the family that works under row importance
# weights, every member of it, and the entropy is refused under them.
_UNWEIGHTED = ("particle_ranking_PLS_targets_entropy", "knn_entropy")
# The highest-density intervals (hpd.py) are forwarded the same way; they do work under row importance weights and any others.
_INTERVALS = ("particle_ranking_PLS_targets_hpd", "weighted_hpd")
# The ABC-GLM posterior (glm.py) likewise: an estimator of its own on the ranking's rows, under row importance weights too.
_GLM = ("particle_ranking_PLS_targets_glm", "weighted_glm", "cross_validate_pls_glm")


def __getattr__(name):
    if name in _UNWEIGHTED:
        from . import entropy
        return getattr(entropy, name)
    if name in _INTERVALS:
        from . import hpd
        return getattr(hpd, name)
    if name in _GLM:
        from . import glm
        return getattr(glm, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def hpd_levels(dens, step_x, step_y, probs=(0.5, 0.9, 0.95)):
    """Contour heights of highest-density regions of one gridded pair density (host only, pure NumPy).  dens: (G, G') values of f on
    a grid with cell area step_x * step_y.  The cells are sorted by descending f and their masses f * step_x * step_y accumulated;
    the level for probability alpha is the f of the first cell at which the cumulative mass reaches alpha times the grid's total
    mass.  Drawing the contour f = level encloses about alpha of the mass.  Returns an array shaped as probs."""
    f = np.sort(np.asarray(dens, dtype=np.float64).reshape(-1))[::-1]
    if f.size == 0 or not np.all(np.isfinite(f)):
        raise ValueError("dens must be a non-empty array of finite values")
    pr = np.asarray(probs, dtype=np.float64)
    if np.any(~(pr >= 0)) or np.any(pr > 1):
        raise ValueError("probs must lie in [0, 1]")
    mass = np.cumsum(f * (float(step_x) * float(step_y)))
    at = np.minimum(np.searchsorted(mass, pr.reshape(-1) * mass[-1], side="left"), f.size - 1)
    return f[at].reshape(pr.shape)


def cross_validate_pls(X_orig, Y_orig, n_targets, K, seed, training_fraction=0.5, max_comp=0, rule=_lib.RULE_DEFAULT,
                       ctx=None, method="rejection", kernel="epanechnikov", statistic="mean", coverage=False, transf=None,
                       bounds=None, hcorr=False, ridge=None, row_weights=None, entropy=False, entropy_k=4, entropy_scale="sd",
                       hpd=None):
    """Leave-one-out cross-validation of the PLS rejection step, as cv4abc of the R package abc: n_targets rows drawn
    without replacement (numpy Generator seeded with `seed`) serve as pseudo-observed data, each ranked against the set with
    itself excluded (the fit is shared: the row stays in it), and the posterior mean of its K nearest rows estimates its
    parameters.  Returns dict(rows, theta (true parameters, (n_targets, P)), post_mean, pred_error (P,): per parameter
    sum_b (post_mean_bj - theta_bj)^2 / (n_targets * Var_j(theta)), Var with n - 1 in the denominator as R's var; NaN where
    the true values do not vary).  method="loclinear": the estimate is instead the local-linear adjusted posterior mean alpha of
    particle_ranking_PLS_targets_adjust (kernel as there), the comparison cv4abc makes between "rejection" and "loclinear".
    statistic="median": the estimate (post_median instead of post_mean) and pred_error come from the posterior median (weighted
    for loclinear), cv4abc's default.  statistic="mode": they come from the mode of the weighted kernel density
    (particle_ranking_PLS_targets_density with its defaults; post_mode).  coverage=True adds truth_cdf (n_targets, P): each left-out row's true parameter's place in
    its own posterior (roughly uniform when calibrated), and ci95 (P,): the fraction of targets whose truth lies in
    [Q(0.025), Q(0.975)].  transf / bounds: the parameter transforms of particle_ranking_PLS_targets_adjust, handed to the
    "loclinear" calls (and only when given); the estimate under statistic="mean" is then its post_mean, the fitted value at the
    observation carried back.  hcorr=True: the heteroscedastic variance correction, handed on likewise and ignored under
    "rejection".  It rescales the adjusted rows about alpha and leaves alpha itself alone, so statistic="mean" under "loclinear"
    is unaffected; the median, the mode, truth_cdf and ci95 do change.  ridge: the penalties of the ridge adjustment, handed on
    likewise and ignored under "rejection"; alpha is then the ridge fit's, so every statistic under "loclinear" changes.
    row_weights: the row importance weights of particle_ranking_PLS_targets (one per row of the set), handed to every call, both
    methods: what a table that is not drawn from the prior needs.  entropy=True adds entropy (n_targets,): the k-nearest-neighbour
    entropy of each left-out row's posterior (particle_ranking_PLS_targets_entropy with k = entropy_k and scale = entropy_scale,
    same method, kernel and adjustment settings), and mean_entropy: their mean, what min_entropy_components compares.  The estimator
    takes entries of equal weight only: "loclinear" then needs kernel="rectangular", and the library refuses row_weights.
    hpd: None, or masses inside (0, 1); adds hpd (n_targets, nm, 2, P): the highest-density interval [lo, hi] of each left-out row's
    posterior for every mass (particle_ranking_PLS_targets_hpd, same method, kernel and adjustment settings), and hpd_coverage
    (nm, P): the share of the left-out rows whose true parameter lies in its interval, about the mass for a calibrated posterior."""
    X, Y = _f(X_orig), _f(Y_orig)
    N = X.shape[0]
    n_targets = int(n_targets)
    if not (1 <= n_targets <= N):
        raise ValueError("n_targets must be in [1, N]")
    if method not in ("rejection", "loclinear"):
        raise ValueError("method must be 'rejection' or 'loclinear'")
    if statistic not in ("mean", "median", "mode"):
        raise ValueError("statistic must be 'mean', 'median' or 'mode'")
    rows = np.sort(np.random.default_rng(seed).choice(N, size=n_targets, replace=False)).astype(np.int64)
    theta = np.ascontiguousarray(Y[rows])
    tkw = _tf_kw(transf, bounds, hcorr, ridge, row_weights)
    sm = None
    if statistic == "median" or coverage:
        sm = particle_ranking_PLS_targets_summary(X, Y, X[rows], training_fraction, K, probs=(0.5, 0.025, 0.975),
                                                  truth=theta if coverage else None, method=method, kernel=kernel, exclude=rows,
                                                  max_comp=max_comp, rule=rule, ctx=ctx, **tkw)
    if statistic == "median":
        r = sm
    elif statistic == "mode":
        r = particle_ranking_PLS_targets_density(X, Y, X[rows], training_fraction, K, method=method, kernel=kernel, exclude=rows,
                                                 max_comp=max_comp, rule=rule, dens=False, ctx=ctx, **tkw)
    elif method == "rejection":
        r = particle_ranking_PLS_targets(X, Y, X[rows], training_fraction, K, exclude=rows, max_comp=max_comp, rule=rule,
                                         details=True, ctx=ctx, **_tf_kw(None, None, row_weights=row_weights))
    else:
        r = particle_ranking_PLS_targets_adjust(X, Y, X[rows], training_fraction, K, exclude=rows, kernel=kernel,
                                                max_comp=max_comp, rule=rule, theta=False, ctx=ctx, **tkw)
    pm = sm["quant"][:, 0, :] if statistic == "median" else r["mode" if statistic == "mode" else "post_mean"]
    var = theta.var(axis=0, ddof=1) if n_targets > 1 else np.zeros(theta.shape[1])
    sse = ((pm - theta) ** 2).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(var > 0, sse / (n_targets * np.where(var > 0, var, 1.0)), np.nan)
    out = dict(rows=rows, theta=theta, pred_error=err, idx=r["idx"], ncomp=r["ncomp"])
    out["post_" + statistic] = pm
    if coverage:
        out["truth_cdf"] = sm["cdf"]
        out["ci95"] = ((sm["quant"][:, 1, :] <= theta) & (theta <= sm["quant"][:, 2, :])).mean(axis=0)
    if entropy:
        from .entropy import particle_ranking_PLS_targets_entropy
        en = particle_ranking_PLS_targets_entropy(X, Y, X[rows], training_fraction, K, k=entropy_k, scale=entropy_scale, method=method,
                                                  kernel=kernel, exclude=rows, max_comp=max_comp, rule=rule, ctx=ctx,
                                                  **tkw)
        out["entropy"] = en["H"]
        out["mean_entropy"] = float(np.mean(en["H"]))
    if hpd is not None:
        from .hpd import particle_ranking_PLS_targets_hpd
        hd = particle_ranking_PLS_targets_hpd(X, Y, X[rows], training_fraction, K, mass=hpd, method=method, kernel=kernel,
                                              exclude=rows, max_comp=max_comp, rule=rule, ctx=ctx, outputs=("lo", "hi"), **tkw)
        out["hpd"] = np.stack([hd["lo"], hd["hi"]], axis=2)
        out["hpd_coverage"] = ((hd["lo"] <= theta[:, None, :]) & (theta[:, None, :] <= hd["hi"])).mean(axis=0)
    return out


def min_entropy_components(X_orig, Y_orig, n_targets, K, seed, max_comps, entropy_k=4, entropy_scale="sd", **cv_kw):
    """The number of PLS components by the minimum-entropy criterion of Nunes & Balding (2010), with the components in the place
    of their summary statistics: cross_validate_pls(..., entropy=True) once per cap in max_comps (a sequence of caps, or an int c
    for 1..c; the same pseudo-observed rows every time, by seed), and the cap whose posteriors have the lowest mean entropy.
    Where the two existing rules judge how well the metrics predict the parameters, this one looks at the posterior the ranking
    produces.  cv_kw: further arguments of cross_validate_pls (training_fraction, rule, method, kernel, ...).  Returns
    dict(max_comp (C,): the caps; ncomp (C,): the count actually used under each; mean_entropy (C,); pred_error (C, P);
    best: the cap with the smallest mean entropy (NaN counts as largest; ties go to the smaller cap), best_ncomp: its count)."""
    caps = list(range(1, int(max_comps) + 1)) if np.ndim(max_comps) == 0 else [int(c) for c in max_comps]
    if not caps or min(caps) < 1:
        raise ValueError("max_comps must name at least one cap >= 1")
    for name in ("max_comp", "entropy"):
        if name in cv_kw:
            raise ValueError("%s is set by min_entropy_components" % name)
    cvs = [cross_validate_pls(X_orig, Y_orig, n_targets, K, seed, max_comp=c, entropy=True, entropy_k=entropy_k,
                              entropy_scale=entropy_scale, **cv_kw) for c in caps]
    me = np.array([cv["mean_entropy"] for cv in cvs])
    at = int(np.argmin(np.where(np.isnan(me), np.inf, me)))
    return dict(max_comp=np.array(caps), ncomp=np.array([cv["ncomp"] for cv in cvs]), mean_entropy=me,
                pred_error=np.stack([cv["pred_error"] for cv in cvs]), best=caps[at], best_ncomp=int(cvs[at]["ncomp"]))


def cross_validate_pls_path(X_orig, Y_orig, n_targets, Ks, seed, training_fraction=0.5, max_comp=0, rule=_lib.RULE_DEFAULT,
                            ctx=None, method="rejection", kernel="epanechnikov", statistic="mean", coverage=False, transf=None,
                            bounds=None, hcorr=False, ridge=None, row_weights=None):
    """cross_validate_pls at every tolerance of the strictly ascending list Ks from ONE call of
    particle_ranking_PLS_targets_path: cv4abc with tols = c(...).  The left-out rows are drawn from `seed` exactly as
    cross_validate_pls draws them.  method: "rejection" (the mean of the Ks[t] nearest rows) or "loclinear" (alpha of the fit at
    tolerance t).  Returns dict(rows, theta, Ks, post_mean (n_targets, T, P), pred_error (T, P) by cross_validate_pls's formula,
    best (P,): the index of the tolerance with the smallest error of each parameter (0 where every error is NaN), idx, ncomp).
    statistic="median" (cv4abc's default) or coverage=True take ONE call of particle_ranking_PLS_targets_path_summary instead:
    with "median" the estimate is post_median (n_targets, T, P) in place of post_mean, and pred_error and best come from it; with
    coverage=True the result gains truth_cdf (n_targets, T, P) and ci95 (T, P) as cross_validate_pls's at every tolerance,
    coverage_ks (T, P): the Kolmogorov distance of the finite truth_cdf values from the uniform (coverage_ks below), and
    best_calibrated (P,): the index of the tolerance with the smallest coverage_ks (0 where all are NaN).  transf / bounds as
    cross_validate_pls (handed on only when given); the "loclinear" mean estimate is then alpha_back of the path.  hcorr=True as
    cross_validate_pls: alpha and so statistic="mean" are unaffected; the median, truth_cdf, ci95 and coverage_ks do change.  ridge
    and row_weights as cross_validate_pls."""
    X, Y = _f(X_orig), _f(Y_orig)
    N = X.shape[0]
    n_targets = int(n_targets)
    if not (1 <= n_targets <= N):
        raise ValueError("n_targets must be in [1, N]")
    if method not in ("rejection", "loclinear"):
        raise ValueError("method must be 'rejection' or 'loclinear'")
    if statistic not in ("mean", "median"):
        raise ValueError("statistic must be 'mean' or 'median'")
    rows = np.sort(np.random.default_rng(seed).choice(N, size=n_targets, replace=False)).astype(np.int64)
    theta = np.ascontiguousarray(Y[rows])
    tkw = _tf_kw(transf, bounds, hcorr, ridge, row_weights)
    if statistic == "median" or coverage:
        r = particle_ranking_PLS_targets_path_summary(X, Y, X[rows], training_fraction, Ks, probs=(0.5, 0.025, 0.975),
                                                      truth=theta if coverage else None, method=method, kernel=kernel, exclude=rows,
                                                      max_comp=max_comp, rule=rule, ctx=ctx, **tkw)
    else:
        r = particle_ranking_PLS_targets_path(X, Y, X[rows], training_fraction, Ks, kernel=kernel, exclude=rows, max_comp=max_comp,
                                              rule=rule, ctx=ctx, **tkw)
    if statistic == "median":
        pm = np.ascontiguousarray(r["quant"][:, :, 0, :])
    else:
        pm = np.ascontiguousarray(r["post_mean"] if method == "rejection" else r.get("alpha_back", r["alpha"]))
    var = theta.var(axis=0, ddof=1) if n_targets > 1 else np.zeros(theta.shape[1])
    sse = ((pm - theta[:, None, :]) ** 2).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(var > 0, sse / (n_targets * np.where(var > 0, var, 1.0)), np.nan)
    best = np.argmin(np.where(np.isnan(err), np.inf, err), axis=0)
    out = dict(rows=rows, theta=theta, Ks=r["Ks"], pred_error=err, best=best, idx=r["idx"], ncomp=r["ncomp"])
    out["post_" + statistic] = pm
    if coverage:
        th = theta[:, None, :]
        out["truth_cdf"] = r["cdf"]
        out["ci95"] = ((r["quant"][:, :, 1, :] <= th) & (th <= r["quant"][:, :, 2, :])).mean(axis=0)
        out["coverage_ks"] = ks = coverage_ks(r["cdf"])
        out["best_calibrated"] = np.argmin(np.where(np.isnan(ks), np.inf, ks), axis=0)
    return out


def coverage_ks(truth_cdf):
    """The Kolmogorov distance sup_x |F_n(x) - x| between the empirical distribution of the finite values of truth_cdf along its
    first axis (n targets; values in [0, 1]) and the uniform distribution, per remaining index: the size of the coverage
    diagnostic's departure from calibration (no p-value).  With the m finite values sorted, u_(1) <= ... <= u_(m), it is
    max_i max(i / m - u_(i), u_(i) - (i - 1) / m).  NaN where no value is finite."""
    u = np.asarray(truth_cdf, dtype=np.float64)
    flat = u.reshape(u.shape[0], -1)
    out = np.full(flat.shape[1], np.nan)
    for c in range(flat.shape[1]):
        v = np.sort(flat[np.isfinite(flat[:, c]), c])
        m = v.size
        if m:
            i = np.arange(1, m + 1, dtype=np.float64)
            out[c] = max(np.max(i / m - v), np.max(v - (i - 1) / m))
    return out.reshape(u.shape[1:])


def _box_cox_table(X, what="X"):
    """A table of metrics as column-major float64 (n, M); a 1-D array is one column (the reference's Col)"""
    a = np.asarray(X, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    if a.ndim != 2 or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("%s must be a non-empty (n, M) table or a column" % what)
    return np.asfortranarray(a)


def _box_cox_shift(shift, X):
    """shift= as float64 (M,) or None; "auto": 1 - min_j for the columns whose minimum is <= 0, else 0 (minima taken here, on the host)"""
    M = X.shape[1]
    if isinstance(shift, str):
        if shift != "auto":
            raise ValueError("shift must be None, 'auto', a number or one number per column")
        mn = X.min(axis=0)
        if not np.isfinite(mn).all():
            raise ValueError("shift='auto' needs finite columns")
        return np.where(mn <= 0, 1.0 - mn, 0.0)
    sh = _lib._host_doubles(shift, M, "shift")
    if sh is not None and not np.isfinite(sh).all():
        raise ValueError("shift must be finite")
    return sh


def optimize_box_cox(X, lambda_min=-5, lambda_max=5, step=0.1, shift=None, skew=False, details=False, ctx=None):
    """ABC::optimize_box_cox (AbcUtil.cpp:89-109) for every column of X at once: the lambda of the reference's grid whose Box-Cox
    transform has the smallest |skewness| (the definition, the status bits and the one deviation are in the header).  X: (N, M), or
    a column (N,) as the reference takes it; shift: None, "auto", a number or one per column, added before the logarithm.  Returns
    lam (M,), or a float for a column; details=True: dict(lam, skew_best, pick, status, skew (M, L) if skew else None, grid,
    shift)."""
    Xf = _box_cox_table(X)
    sh = _box_cox_shift(shift, Xf)
    grid = _lib.box_cox_grid(lambda_min, lambda_max, step)
    r = _ctx(ctx).optimize_box_cox(Xf, grid, sh, skew=skew)
    if details:
        r.update(grid=grid, shift=sh)
        return r
    return float(r["lam"][0]) if np.ndim(X) == 1 else r["lam"]


def box_cox(X, lam, shift=None, ctx=None):
    """The Box-Cox transform y = ((x + shift)^lam - 1) / lam (lam == 0: log(x + shift)) of the columns of X (n, M), or of a
    column (n,): lam and shift a number or one per column (abc_box_cox).  Returns an array of X's shape."""
    Xf = _box_cox_table(X)
    if lam is None:
        raise ValueError("lam is required")
    la = _lib._host_doubles(lam, Xf.shape[1], "lam")
    if not np.isfinite(la).all():
        raise ValueError("lam must be finite")
    sh = _box_cox_shift(shift, Xf)
    out = _ctx(ctx).box_cox(Xf, la, sh)
    return out[:, 0] if np.ndim(X) == 1 else out


def box_cox_metrics(X, targets=None, lambda_min=-5, lambda_max=5, step=0.1, shift=None, ctx=None):
    """The metrics' pre-pass of a ranking: the search on the table X (N, M), then the transform of the table and of the targets
    (B, M) or (M,) with the table's lambda and shift.  Returns dict(lam, shift, pick, skew_best, status, X, targets): X and targets
    are what every later call must be given in place of the raw ones (targets None if none were given).  A column with status bit
    0 (an entry <= 0 after the shift) keeps lambda = 1: x - 1 + shift, an affine map."""
    Xf = _box_cox_table(X)
    T = None
    if targets is not None:
        T = np.asarray(targets, dtype=np.float64)
        if T.ndim not in (1, 2) or T.shape[-1] != Xf.shape[1]:
            raise ValueError("targets must be (B, M) or (M,)")
    sh = _box_cox_shift(shift, Xf)
    grid = _lib.box_cox_grid(lambda_min, lambda_max, step)
    ctx = _ctx(ctx)
    r = ctx.optimize_box_cox(Xf, grid, sh)
    out = dict(lam=r["lam"], shift=sh if sh is not None else np.zeros(Xf.shape[1]), pick=r["pick"], skew_best=r["skew_best"],
               status=r["status"], X=ctx.box_cox(Xf, r["lam"], sh), targets=None)
    if T is not None:
        out["targets"] = ctx.box_cox(np.asfortranarray(np.atleast_2d(T)), r["lam"], sh).reshape(T.shape)
    return out


def particle_ranking_simple(X_orig, Y_orig, target_values, K=None, details=False, ctx=None):
    """ABC::particle_ranking_simple (AbcUtil.cpp:408-421); Y_orig is unused, as in the reference."""
    ctx = _ctx(ctx)
    X, obs = _f(X_orig), _f(target_values)
    N, M = X.shape
    K = N if K is None else int(K)
    idx = np.empty(K, dtype=np.uint64)
    dist = np.empty(K)
    ctx.check(lib().abc_particle_ranking_simple(ctx.handle, _p(X), _p(obs), N, M, K, _p(idx), _p(dist)))
    if details:
        return dict(idx=idx, dist=dist)
    return idx


def calculate_doubled_variance(params, ctx=None):
    """ABC::calculate_doubled_variance (AbcUtil.cpp:528-537)."""
    ctx = _ctx(ctx)
    th = _f(params)
    K, P = th.shape
    dv = np.empty(P)
    ctx.check(lib().abc_calculate_doubled_variance(ctx.handle, _p(th), K, P, _p(dv)))
    return dv


def weight_predictive_prior(mpars, params, prev_params=None, prev_weights=None,
                            prev_doubled_variance=None, ctx=None):
    """ABC::weight_predictive_prior, both overloads (AbcUtil.cpp:539-586).  mpars: ctypes array of
    Prior (the POD form of the reference's vector<const Parameter*>)."""
    ctx = _ctx(ctx)
    th = _f(params)
    K, P = th.shape
    w = np.empty(K)
    if prev_params is None:
        ctx.check(lib().abc_weight_predictive_prior_uniform(ctx.handle, K, _p(w)))
        return w
    tp, wp, dvp = _f(prev_params), _f(prev_weights), _f(prev_doubled_variance)
    Kp = tp.shape[0]
    if tp.shape[1] != P or wp.size != Kp or dvp.size != P or len(mpars) != P:
        raise ValueError("shape mismatch")
    ctx.check(lib().abc_weight_predictive_prior(ctx.handle, C.addressof(mpars), _p(th), K, P, _p(tp), Kp,
                                                _p(wp), _p(dvp), _p(w)))
    return w


def setup_mvn_sampler(params, ctx=None):
    """ABC::setup_mvn_sampler (AbcUtil.cpp:462-488): P x P matrix, lower triangle = Cholesky factor."""
    ctx = _ctx(ctx)
    th = _f(params)
    K, P = th.shape
    L = np.empty((P, P), order="F")
    ctx.check(lib().abc_setup_mvn_sampler(ctx.handle, _p(th), K, P, _p(L)))
    return L


def gsl_rng_nonuniform_int(RNG, num_samples, weights, ctx=None):
    """ABC::gsl_rng_nonuniform_int (AbcUtil.cpp:111-120): advances RNG by num_samples outputs."""
    ctx = _ctx(ctx)
    w = _f(weights)
    idx = np.empty(int(num_samples), dtype=np.uint64)
    ctx.check(lib().abc_sample_posterior(ctx.handle, C.addressof(RNG), _p(w), w.size, int(num_samples), _p(idx)))
    return idx


def sample_posterior(RNG, num_samples, weights, posterior, ctx=None):
    """ABC::sample_posterior (AbcUtil.cpp:366-375)."""
    post = _f(posterior)
    return post[gsl_rng_nonuniform_int(RNG, num_samples, weights, ctx=ctx).astype(np.int64), :]


def _sample(fn, RNG, num_samples, weights, parameter_prior, pars, aux, want_seeds, ctx):
    ctx = _ctx(ctx)
    w, th, aux = _f(weights), _f(parameter_prior), _f(aux)
    K, P = th.shape
    n = int(num_samples)
    out = np.empty((n, P), order="F")
    parent = np.empty(n, dtype=np.uint64)
    seeds = np.empty(n, dtype=np.uint64) if want_seeds else None
    ctx.check(fn(ctx.handle, C.addressof(RNG), n, _p(w), _p(th), K, P, C.addressof(pars), _p(aux), _p(out),
                 _p(parent), _p(seeds)))
    return (out, parent, seeds) if want_seeds else (out, parent)


def sample_mvn_predictive_priors(RNG, num_samples, weights, parameter_prior, pars, L, seeds=False, ctx=None):
    """ABC::sample_mvn_predictive_priors (AbcUtil.cpp:391-404). Returns (noised_pars, parent_rows[, seeds])."""
    return _sample(lib().abc_sample_mvn_predictive_priors, RNG, num_samples, weights, parameter_prior, pars, L,
                   seeds, ctx)


def sample_predictive_priors(RNG, num_samples, weights, parameter_prior, pars, doubled_variance, seeds=False,
                             ctx=None):
    """ABC::sample_predictive_priors (AbcUtil.cpp:377-389). Returns (noised_pars, parent_rows[, seeds])."""
    return _sample(lib().abc_sample_predictive_priors, RNG, num_samples, weights, parameter_prior, pars,
                   doubled_variance, seeds, ctx)
