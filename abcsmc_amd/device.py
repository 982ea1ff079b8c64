"""Device-resident driver: one SMC generation turn-over with all inputs and outputs in HBM.

torch is used ONLY as plumbing here -- device allocations (torch tensors) and the current HIP
stream.  All arithmetic is done by libabcsmc_hip.so through `abc_generation_dev` (and the stage-level
`*_dev` entry points used by sharded.py).  Matrices are column-major: an (n, c) matrix is held as a
contiguous torch tensor of shape (c, n), i.e. one particle-major vector per column.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import GenerationCfg, GenerationIO, Rng, lib


def colmajor(a, device):
    """numpy (n, c) -> torch (c, n) contiguous float64 on device (column-major storage)."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return torch.from_numpy(np.ascontiguousarray(a.T)).to(device)


def to_numpy(t):
    """torch (c, n) column-major holder -> numpy (n, c)."""
    a = t.detach().cpu().numpy()
    return a.T if a.ndim == 2 else a


def priors_to_device(priors, device):
    raw = np.frombuffer(bytes(priors), dtype=np.uint8).copy()
    return torch.from_numpy(raw).to(device)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Generation:
    """Pre-allocated buffers + one call per generation (AbcSmc.cpp:634-664, 1041-1066, 490-518)."""

    def __init__(self, N, M, P, K, Kp, Nnext, train_frac=0.5, max_comp=0, rule=_lib.RULE_DEFAULT,
                 multivariate=True, device="cuda:0", ctx=None):
        self.device = torch.device(device)
        idx = self.device.index or 0
        self.ctx = ctx if ctx is not None else _lib.default_context(idx)
        self.cfg = GenerationCfg(N, M, P, K, Kp, Nnext, float(train_frac), int(max_comp), int(rule),
                                 int(bool(multivariate)), 0)
        f64, i64 = torch.float64, torch.int64
        d = self.device
        self.idx = torch.empty(K, dtype=i64, device=d)
        self.dist = torch.empty(K, dtype=f64, device=d)
        self.theta = torch.empty((P, K), dtype=f64, device=d)
        self.w = torch.empty(K, dtype=f64, device=d)
        self.dv = torch.empty(P, dtype=f64, device=d)
        self.L = torch.empty((P, P), dtype=f64, device=d)
        self.next = torch.empty((P, max(Nnext, 1)), dtype=f64, device=d)
        self.parent = torch.empty(max(Nnext, 1), dtype=i64, device=d)
        self.seeds = torch.empty(max(Nnext, 1), dtype=i64, device=d)
        self.ncomp = C.c_int32(0)
        self._io_key, self._io, self._args = None, None, None
        self._call = lib().abc_generation_dev

    def run(self, X, Y, obs, priors_dev, rng, theta_prev=None, w_prev=None, dv_prev=None):
        """X: (M, N), Y: (P, N), obs: (M,), all float64 on self.device; rng: _lib.Rng (advanced)."""
        cfg = self.cfg
        weighted = theta_prev is not None and cfg.Kp
        # (addresses AND shapes: torch's caching allocator hands the same address to a differently shaped tensor)
        key = (X.data_ptr(), Y.data_ptr(), obs.data_ptr(), priors_dev.data_ptr(),
               theta_prev.data_ptr() if weighted else 0, w_prev.data_ptr() if weighted else 0,
               dv_prev.data_ptr() if weighted else 0, X.shape, Y.shape, X.stride(), Y.stride(), obs.shape, priors_dev.shape,
               theta_prev.shape if weighted else None, theta_prev.stride() if weighted else None,
               w_prev.shape if weighted else None, dv_prev.shape if weighted else None)
        if key != self._io_key:           # (the argument block of the C call is rebuilt only when a buffer moved)
            assert X.shape == (cfg.M, cfg.N) and Y.shape == (cfg.P, cfg.N) and X.is_contiguous() and Y.is_contiguous()
            assert obs.numel() == cfg.M and obs.is_contiguous() and priors_dev.numel() >= 24 * cfg.P
            io = GenerationIO()
            io.X, io.Y, io.obs, io.priors = key[0], key[1], key[2], key[3]
            if weighted:
                assert theta_prev.shape == (cfg.P, cfg.Kp) and theta_prev.is_contiguous()
                assert w_prev.numel() == cfg.Kp and dv_prev.numel() == cfg.P and w_prev.is_contiguous() and dv_prev.is_contiguous()
                io.theta_prev, io.w_prev, io.dv_prev = key[4], key[5], key[6]
            io.idx, io.dist, io.theta = self.idx.data_ptr(), self.dist.data_ptr(), self.theta.data_ptr()
            io.w, io.dv, io.L = self.w.data_ptr(), self.dv.data_ptr(), self.L.data_ptr()
            io.next, io.parent, io.seeds = self.next.data_ptr(), self.parent.data_ptr(), self.seeds.data_ptr()
            self._io, self._io_key = io, key
            self._args = (self.ctx.handle, C.addressof(cfg), C.addressof(io), None, C.addressof(self.ncomp))
        self.ctx.set_stream(torch.cuda.current_stream(self.device).cuda_stream)      # (a no-op unless the stream changed)
        a = self._args
        self.ctx.check(self._call(a[0], a[1], a[2], C.addressof(rng), a[4]))
        if cfg.Nnext:
            self.ctx.warn_generation_giveups()
        return self


def _targets_holders(X, targets, Y, exclude, ctx, strict=False):
    """What the rank_targets family shares: the holders' layout asserts, the sizes, the leading dimensions (ldx, ldy, ldt; a
    single-column holder counts as dense), exclude as int64 on the device and the context on the current stream.  strict
    (rank_targets): X and targets have unit stride even with a single column, and Y may be None (P = 0)."""
    assert X.dim() == 2 and (X.stride(1) == 1 or (not strict and X.shape[1] == 1))
    assert targets.dim() == 2 and (targets.stride(1) == 1 or (not strict and targets.shape[1] == 1))
    assert strict or Y is not None
    M, N = X.shape
    B = targets.shape[1]
    P = Y.shape[0] if Y is not None else 0
    if Y is not None:
        assert Y.dim() == 2 and Y.shape[1] == N and (Y.stride(1) == 1 or P <= 1)
    assert targets.shape[0] == M
    dev = X.device
    ctx = ctx if ctx is not None else _lib.default_context(dev.index or 0)
    if exclude is not None:
        exclude = exclude.to(device=dev, dtype=torch.int64).contiguous()
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    ld = (X.stride(0) if M > 1 else N, Y.stride(0) if P > 1 else N, targets.stride(0) if M > 1 else B)
    return N, M, P, B, dev, ctx, exclude, ld


def _adjust_out(names, B, K, P, A, dev):
    """Device tensors for the named abc_adjust_out members, and the struct that points at them (the other members NULL)."""
    f64, i32 = torch.float64, torch.int32
    shapes = dict(theta=((B, K, P), f64), weight=((B, K), f64), coef=((B, A + 1, P), f64), rank=((B,), i32), status=((B,), i32))
    t = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in names}
    return t, _lib.AdjustOut(*(t[k].data_ptr() if k in t else None for k in shapes))


def rank_targets(X, model, A, targets, K, Y=None, exclude=None, post_mean=False, dist=True, ctx=None):
    """Batched ranking on the device (abc_rank_targets_dev).  X: (M, N) column-major holder (a column-slice view with a row
    stride >= N is fine: ldx = X.stride(0)); model: a finished model record (abc_pls_model_dev [+ abc_pls_wilcoxon_dev]) for
    (M, P, A); targets: (M, B) holder (ldt = targets.stride(0)); Y: (P, N) holder, needed for post_mean; exclude: int64 (B,)
    (-1: none).  Returns (idx (B, K) int64, dist (B, K) or None, post_mean (B, P) or None) as device tensors."""
    N, M, P, B, dev, ctx, exclude, (ldx, ldy, ldt) = _targets_holders(X, targets, Y, exclude, ctx, strict=True)
    idx = torch.empty((B, K), dtype=torch.int64, device=dev)
    d = torch.empty((B, K), dtype=torch.float64, device=dev) if dist else None
    pm = torch.empty((B, P), dtype=torch.float64, device=dev) if post_mean else None
    ctx.check(lib().abc_rank_targets_dev(ctx.handle, X.data_ptr(), ldx, _ptr(Y), ldy, N, M, P, model.data_ptr(), A,
                                         targets.data_ptr(), ldt, B, _ptr(exclude), K, idx.data_ptr(), _ptr(d), _ptr(pm)))
    return idx, d, pm


def rank_targets_adjust(X, model, A, targets, K, Y, exclude=None, kernel=_lib.KERNEL_EPANECHNIKOV, theta=True, weight=True,
                        dist=True, ctx=None):
    """rank_targets followed by the local-linear adjustment (abc_rank_targets_adjust_dev); Y: (P, N) holder (required).
    Returns dict(idx (B, K) int64, dist (B, K) or None, theta (B, K, P) or None, weight (B, K) or None, coef (B, A + 1, P),
    rank (B,) int32, status (B,) int32) as device tensors."""
    N, M, P, B, dev, ctx, exclude, (ldx, ldy, ldt) = _targets_holders(X, targets, Y, exclude, ctx)
    r = dict(idx=torch.empty((B, K), dtype=torch.int64, device=dev),
             dist=torch.empty((B, K), dtype=torch.float64, device=dev) if dist else None, theta=None, weight=None)
    members, out = _adjust_out(("theta",) * bool(theta) + ("weight",) * bool(weight) + ("coef", "rank", "status"), B, K, P, A, dev)
    r.update(members)
    ctx.check(lib().abc_rank_targets_adjust_dev(ctx.handle, X.data_ptr(), ldx, Y.data_ptr(), ldy, N, M, P, model.data_ptr(), A,
                                                targets.data_ptr(), ldt, B, _ptr(exclude), K, int(kernel), r["idx"].data_ptr(),
                                                _ptr(r["dist"]), C.byref(out)))
    return r


def param_transf(V, inverse=False, ctx=None):
    """The context's parameter transforms (Context.set_param_transf) over V, a (P, n) column-major holder (a view with a row
    stride >= n is fine): forward, or back with inverse=True (abc_param_transf_dev).  With nothing set it copies.  Returns a
    new contiguous (P, n) tensor."""
    assert V.dim() == 2 and (V.stride(1) == 1 or V.shape[1] == 1)
    P, n = V.shape
    dev = V.device
    ctx = ctx if ctx is not None else _lib.default_context(dev.index or 0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    out = torch.empty((P, n), dtype=torch.float64, device=dev)
    ctx.check(lib().abc_param_transf_dev(ctx.handle, V.data_ptr(), V.stride(0) if P > 1 else n, n, P, int(bool(inverse)),
                                         out.data_ptr(), n))
    return out


def adjust_hcorr(on=True, ctx=None, device=0):
    """Context manager: the heteroscedastic variance correction of the local-linear adjustment (Context.adjust_hcorr,
    abc_ctx_set_adjust_hcorr) on ctx, or on the default context of `device`, inside the block.  Every rank_targets_* call that
    regresses then makes its adjusted rows with the correction (rank_targets_adjust's theta, the products under method 1, the path
    summaries); their arguments and results are otherwise unchanged, and ctx.last_hcorr() returns the call's second fit."""
    ctx = ctx if ctx is not None else _lib.default_context(device)
    return ctx.adjust_hcorr(on)


def adjust_ridge(lambdas, ctx=None, device=0):
    """Context manager: the ridge adjustment with the penalty chosen by leave-one-out PRESS (Context.adjust_ridge,
    abc_ctx_set_adjust_ridge) on ctx, or on the default context of `device`, inside the block.  Every rank_targets_* call that
    regresses then returns, per parameter, the ridge fit of the penalty of `lambdas` with the smallest PRESS as coef, and makes its
    adjusted rows from it; their arguments and results are otherwise unchanged, and ctx.last_ridge() returns the call's picks and
    PRESS values."""
    ctx = ctx if ctx is not None else _lib.default_context(device)
    return ctx.adjust_ridge(lambdas)


def row_weights(w, ctx=None, device=0):
    """Context manager: row importance weights of the batched ranking (Context.row_weights, abc_ctx_set_row_weights; the definition
    is in the header) on ctx, or on the default context of `device`, inside the block.  w: one weight per row of the table, a
    tensor (a device tensor is copied on the device) or an array.  Every rank_targets_* call inside the block weighs entry e of a
    target by its kernel weight times w[idx[e]]; idx and dist do not change."""
    ctx = ctx if ctx is not None else _lib.default_context(device)
    return ctx.row_weights(w)


def _box_cox_holder(X, ctx):
    """What the two Box-Cox calls share: the (M, n) holder's layout assert, its sizes and leading dimension, the context on the
    current stream."""
    assert X.dim() == 2 and X.dtype == torch.float64 and (X.stride(1) == 1 or X.shape[1] == 1)
    M, n = X.shape
    dev = X.device
    ctx = ctx if ctx is not None else _lib.default_context(dev.index or 0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    return M, n, (X.stride(0) if M > 1 else n), dev, ctx


def optimize_box_cox(X, lambda_min=-5, lambda_max=5, step=0.1, shift=None, skew=False, ctx=None):
    """The Box-Cox skewness search over the metrics (abc_optimize_box_cox_dev; the definition is in the header).  X: (M, N)
    column-major holder (a view with a row stride >= N is fine); the grid is the reference's (_lib.box_cox_grid); shift: one
    value per metric added before the logarithm (a scalar, a sequence, a tensor, or None).  Returns dict(lam (M,), skew_best (M,),
    pick (M,) int32, status (M,) int32, skew (M, L) or None) as device tensors and grid (L,) as a host array.  Synchronises."""
    M, N, ldx, dev, ctx = _box_cox_holder(X, ctx)
    grid = _lib.box_cox_grid(lambda_min, lambda_max, step)
    sh = _lib._host_doubles(shift, M, "shift")
    f64, i32 = torch.float64, torch.int32
    r = dict(lam=torch.empty(M, dtype=f64, device=dev), skew_best=torch.empty(M, dtype=f64, device=dev),
             pick=torch.empty(M, dtype=i32, device=dev), status=torch.empty(M, dtype=i32, device=dev),
             skew=torch.empty((M, grid.size), dtype=f64, device=dev) if skew else None)
    out = _lib.BoxCoxOut(r["lam"].data_ptr(), r["skew_best"].data_ptr(), _ptr(r["skew"]), r["pick"].data_ptr(), r["status"].data_ptr())
    ctx.check(lib().abc_optimize_box_cox_dev(ctx.handle, X.data_ptr(), ldx, N, M, sh.ctypes.data if sh is not None else None,
                                             grid.ctypes.data, grid.size, C.byref(out)))
    r["grid"] = grid
    return r


def box_cox(X, lam, shift=None, out=None, ctx=None):
    """The Box-Cox transform (abc_box_cox_dev) of X, an (M, n) column-major holder: the table, or a block of targets held the same
    way.  lam: one exponent per metric (a sequence or a tensor, read on the host); shift as in optimize_box_cox; out: None for a
    new contiguous (M, n) tensor, or a holder of X's shape (X itself: in place).  Stream-ordered.  Returns out."""
    M, n, ldx, dev, ctx = _box_cox_holder(X, ctx)
    if lam is None:
        raise ValueError("lam is required")
    la = _lib._host_doubles(lam, M, "lam")
    sh = _lib._host_doubles(shift, M, "shift")
    if out is None:
        out = torch.empty((M, n), dtype=torch.float64, device=dev)
    assert out.shape == X.shape and out.dtype == torch.float64 and out.device == dev and (out.stride(1) == 1 or n == 1)
    ctx.check(lib().abc_box_cox_dev(ctx.handle, X.data_ptr(), ldx, n, M, la.ctypes.data, sh.ctypes.data if sh is not None else None,
                                    out.data_ptr(), out.stride(0) if M > 1 else n))
    return out


def _path_ks(Ks):
    """The tolerance list as a uint64 array (it stays in host memory) and its largest entry."""
    ks = np.ascontiguousarray(np.asarray(Ks, dtype=np.int64).reshape(-1).astype(np.uint64))
    return ks, (int(ks[-1]) if ks.size else 0)


def rank_targets_path(X, model, A, targets, Ks, Y, exclude=None, kernel=_lib.KERNEL_EPANECHNIKOV, post_mean=True, coef=True,
                      dist=True, ctx=None):
    """Tolerance path on the device (abc_rank_targets_path_dev): one ranking at K_max = Ks[-1], then the rejection mean and the
    local-linear fit of rank_targets_adjust at every tolerance of the strictly ascending list Ks (at most 16).  Returns
    dict(idx (B, K_max) int64, dist (B, K_max) or None, post_mean (B, T, P) or None, coef (B, T, A + 1, P) or None, rank (B, T)
    int32, status (B, T) int32, h (B, T): the bandwidths) as device tensors."""
    N, M, P, B, dev, ctx, exclude, (ldx, ldy, ldt) = _targets_holders(X, targets, Y, exclude, ctx)
    ks, K = _path_ks(Ks)
    T = ks.size
    f64, i32 = torch.float64, torch.int32
    r = dict(idx=torch.empty((B, K), dtype=torch.int64, device=dev),
             dist=torch.empty((B, K), dtype=f64, device=dev) if dist else None,
             post_mean=torch.empty((B, T, P), dtype=f64, device=dev) if post_mean else None,
             coef=torch.empty((B, T, A + 1, P), dtype=f64, device=dev) if coef else None,
             rank=torch.empty((B, T), dtype=i32, device=dev), status=torch.empty((B, T), dtype=i32, device=dev),
             h=torch.empty((B, T), dtype=f64, device=dev))
    path = _lib.Path(ks.ctypes.data, T, _ptr(r["post_mean"]), _ptr(r["coef"]), r["rank"].data_ptr(), r["status"].data_ptr(),
                     r["h"].data_ptr())
    ctx.check(lib().abc_rank_targets_path_dev(ctx.handle, X.data_ptr(), ldx, Y.data_ptr(), ldy, N, M, P, model.data_ptr(), A,
                                              targets.data_ptr(), ldt, B, _ptr(exclude), int(kernel), r["idx"].data_ptr(),
                                              _ptr(r["dist"]), C.byref(path)))
    return r


def rank_targets_path_summary(X, model, A, targets, Ks, Y, probs=(0.025, 0.5, 0.975), truth=None, method=_lib.POSTERIOR_REJECTION,
                              kernel=_lib.KERNEL_EPANECHNIKOV, exclude=None, quant=True, post_mean=True, coef=True, fit=True,
                              idx=True, dist=True, ctx=None):
    """rank_targets_path with the summaries of rank_targets_summary at every tolerance (abc_rank_targets_path_summary_dev): one
    ranking at K_max = Ks[-1] and, under rejection, one sort per (target, parameter) for all tolerances.  truth: (B, P) row-major
    device tensor or None.  quant=False leaves the quantiles out (truth is then needed); fit=False leaves rank, status and h out,
    idx=False the ranking.  Works on device tensors and copies nothing.  Returns rank_targets_path's dict (None for what was left
    out) plus quant (B, T, nq, P) or None and cdf (B, T, P) or None."""
    N, M, P, B, dev, ctx, exclude, (ldx, ldy, ldt) = _targets_holders(X, targets, Y, exclude, ctx)
    ks, K = _path_ks(Ks)
    T = ks.size
    f64, i32 = torch.float64, torch.int32
    pr = np.ascontiguousarray(np.asarray(probs, dtype=np.float64).reshape(-1))
    if truth is not None:
        truth = truth.to(device=dev, dtype=f64).contiguous()
        assert truth.shape == (B, P)
    r = dict(idx=torch.empty((B, K), dtype=torch.int64, device=dev) if idx else None,
             dist=torch.empty((B, K), dtype=f64, device=dev) if dist else None,
             post_mean=torch.empty((B, T, P), dtype=f64, device=dev) if post_mean else None,
             coef=torch.empty((B, T, A + 1, P), dtype=f64, device=dev) if coef else None,
             rank=torch.empty((B, T), dtype=i32, device=dev) if fit else None,
             status=torch.empty((B, T), dtype=i32, device=dev) if fit else None,
             h=torch.empty((B, T), dtype=f64, device=dev) if fit else None,
             quant=torch.empty((B, T, pr.size, P), dtype=f64, device=dev) if quant else None,
             cdf=torch.empty((B, T, P), dtype=f64, device=dev) if truth is not None else None)
    path = _lib.Path(ks.ctypes.data, T, _ptr(r["post_mean"]), _ptr(r["coef"]), _ptr(r["rank"]), _ptr(r["status"]), _ptr(r["h"]))
    sm = _lib.Summary(pr.ctypes.data, pr.size, _ptr(truth), _ptr(r["quant"]), _ptr(r["cdf"]))
    ctx.check(lib().abc_rank_targets_path_summary_dev(ctx.handle, X.data_ptr(), ldx, Y.data_ptr(), ldy, N, M, P, model.data_ptr(), A,
                                                      targets.data_ptr(), ldt, B, _ptr(exclude), int(method), int(kernel),
                                                      _ptr(r["idx"]), _ptr(r["dist"]), C.byref(path), C.byref(sm)))
    return r


def _rank_targets_product(product, make, X, model, A, targets, K, Y, method, kernel, exclude, dist, adjust, ctx):
    """The call of rank_targets_{summary,density,joint,draws}.  make(lead, P, dev) -> (the product's struct, its outputs as a dict, what
    must stay alive during the call) for lead = (B,).  Returns the outputs with idx, dist and the adjust members added."""
    N, M, P, B, dev, ctx, exclude, (ldx, ldy, ldt) = _targets_holders(X, targets, Y, exclude, ctx)
    d, r, _keep = make((B,), P, dev)
    r.update(idx=torch.empty((B, K), dtype=torch.int64, device=dev),
             dist=torch.empty((B, K), dtype=torch.float64, device=dev) if dist else None)
    members, adj = _adjust_out(adjust, B, K, P, A, dev)
    r.update(members)
    entry = getattr(lib(), "abc_rank_targets_%s_dev" % product)
    ctx.check(entry(ctx.handle, X.data_ptr(), ldx, Y.data_ptr(), ldy, N, M, P, model.data_ptr(), A, targets.data_ptr(), ldt, B,
                    _ptr(exclude), K, int(method), int(kernel), r["idx"].data_ptr(), _ptr(r["dist"]), C.byref(adj), C.byref(d)))
    return r


def _weighted_product(product, make, V, w, ctx):
    """The call of weighted_{summary,density,joint,draws}: the holder's layout assert, the context, the weights on the device, and make
    as _rank_targets_product's with lead = (); the context takes the current stream after make's work, just before the call."""
    assert V.dim() == 2 and (V.stride(1) == 1 or V.shape[1] == 1)
    P, K = V.shape
    dev = V.device
    ctx = ctx if ctx is not None else _lib.default_context(dev.index or 0)
    if w is not None:
        w = w.to(device=dev, dtype=torch.float64).contiguous()
        assert w.numel() == K
    d, r, _keep = make((), P, dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    entry = getattr(lib(), "abc_weighted_%s_dev" % product)
    ctx.check(entry(ctx.handle, V.data_ptr(), V.stride(0) if P > 1 else K, K, P, _ptr(w), C.byref(d)))
    return r


def _summary(probs, truth, lead, P, dev):
    """Device tensors for the summaries of prod(lead) targets with P parameters and the abc_summary pointing at them (truth:
    lead + (P,) values, P values in any shape when lead is empty, or None)"""
    f64 = torch.float64
    pr = np.ascontiguousarray(np.asarray(probs, dtype=np.float64).reshape(-1))
    if truth is not None:
        truth = truth.to(device=dev, dtype=f64).contiguous()
        assert truth.shape == lead + (P,) if lead else truth.numel() == P
    r = dict(quant=torch.empty(lead + (len(np.atleast_1d(probs)), P), dtype=f64, device=dev),
             cdf=torch.empty(lead + (P,), dtype=f64, device=dev) if truth is not None else None)
    return _lib.Summary(pr.ctypes.data, pr.size, _ptr(truth), _ptr(r["quant"]), _ptr(r["cdf"])), r, (pr, truth)


def rank_targets_summary(X, model, A, targets, K, Y, probs=(0.025, 0.5, 0.975), truth=None, method=_lib.POSTERIOR_REJECTION,
                         kernel=_lib.KERNEL_EPANECHNIKOV, exclude=None, dist=False, adjust=(), ctx=None):
    """rank_targets followed by weighted posterior quantiles and the posterior CDF at `truth` of every (target, parameter)
    (abc_rank_targets_summary_dev; method 0 rejection, 1 loclinear).  truth: (B, P) row-major device tensor or None.  adjust:
    names of abc_adjust_out members to return as well (method 1: "theta", "weight", "coef", "rank", "status").
    Returns dict(idx (B, K) int64, dist (B, K) or None, quant (B, nq, P), cdf (B, P) or None, and the adjust members)."""
    return _rank_targets_product("summary", lambda lead, P, dev: _summary(probs, truth, lead, P, dev), X, model, A, targets, K, Y,
                                 method, kernel, exclude, dist, adjust, ctx)


def weighted_summary(V, w=None, probs=(0.025, 0.5, 0.975), truth=None, ctx=None):
    """Weighted quantiles and CDF of P columns of K values (abc_weighted_summary_dev).  V: (P, K) holder of a K x P
    column-major matrix (row j = column j's values, unit stride); w: K weights or None (equal); truth: P values or None.
    Returns dict(quant (nq, P), cdf (P,) or None) as device tensors."""
    return _weighted_product("summary", lambda lead, P, dev: _summary(probs, truth, lead, P, dev), V, w, ctx)


def _density(G, cut, bw_scale, bw, lead, P, dev, dens, mode):
    """Device tensors for the densities of prod(lead) targets with P parameters and the abc_density pointing at them (bw: given
    bandwidths or None)"""
    f64 = torch.float64
    G = int(G)
    lead = lead + (P,)
    if bw is not None:
        bw = torch.as_tensor(bw, dtype=f64).to(dev).expand(lead).contiguous()
    r = dict(dens=torch.empty(lead + (G,), dtype=f64, device=dev) if dens else None,
             grid=torch.empty(lead + (2,), dtype=f64, device=dev), bw=torch.empty(lead, dtype=f64, device=dev),
             mode=torch.empty(lead, dtype=f64, device=dev) if mode else None,
             mode_dens=torch.empty(lead, dtype=f64, device=dev) if mode else None)
    d = _lib.Density(G, float(cut), float(bw_scale), _ptr(bw), _ptr(r["dens"]), _ptr(r["grid"]), _ptr(r["bw"]), _ptr(r["mode"]),
                     _ptr(r["mode_dens"]))
    return d, r, bw


def rank_targets_density(X, model, A, targets, K, Y, G=512, cut=3.0, bw=None, bw_scale=1.0, method=_lib.POSTERIOR_REJECTION,
                         kernel=_lib.KERNEL_EPANECHNIKOV, exclude=None, dist=False, adjust=(), dens=True, mode=True, ctx=None):
    """rank_targets followed by the weighted kernel density on G grid points and the mode of every (target, parameter)
    (abc_rank_targets_density_dev; method 0 rejection, 1 loclinear).  bw: given bandwidths (B, P) or None (the bw.nrd0 rule times
    bw_scale).  adjust: names of abc_adjust_out members to return as well (method 1).  Returns dict(idx (B, K) int64, dist (B, K)
    or None, dens (B, P, G) or None, grid (B, P, 2): lo_x and step (x_g = fma(g, step, lo_x)), bw (B, P): the bandwidths used,
    mode and mode_dens (B, P) or None, and the adjust members)."""
    return _rank_targets_product("density", lambda lead, P, dev: _density(G, cut, bw_scale, bw, lead, P, dev, dens, mode), X, model, A,
                                 targets, K, Y, method, kernel, exclude, dist, adjust, ctx)


def weighted_density(V, w=None, G=512, cut=3.0, bw=None, bw_scale=1.0, dens=True, mode=True, ctx=None):
    """The weighted kernel density and mode of P columns of K values (abc_weighted_density_dev).  V: (P, K) holder as
    weighted_summary's; w: K weights or None (equal); bw: P given bandwidths or None.  Returns dict(dens (P, G) or None,
    grid (P, 2), bw (P,), mode and mode_dens (P,) or None) as device tensors."""
    return _weighted_product("density", lambda lead, P, dev: _density(G, cut, bw_scale, bw, lead, P, dev, dens, mode), V, w, ctx)


def _joint(G, cut, bw_scale, bw, pairs, lead, P, dev, dens, mode):
    """Device tensors for the joint outputs of prod(lead) targets with P parameters and the abc_joint pointing at them; pairs: None
    or (npairs, 2).  Returns (struct, tensors, what must stay alive during the call)"""
    f64 = torch.float64
    G = int(G)
    if bw is not None:
        bw = torch.as_tensor(bw, dtype=f64).to(dev).expand(lead + (P,)).contiguous()
    pr, given = _lib._joint_pairs(pairs, P)
    n = pr.shape[0]
    e = lambda *shape: torch.empty(lead + shape, dtype=f64, device=dev)
    r = dict(mean=e(P), cov=e(P, P), corr=e(P, P), dens=e(n, G, G) if dens else None, grid=e(P, 2), bw=e(P),
             mode=e(n, 2) if mode else None, mode_dens=e(n) if mode else None, pairs=pr)
    d = _lib.Joint(G, float(cut), float(bw_scale), _ptr(bw), given.ctypes.data if given is not None else None,
                   n if given is not None else 0, _ptr(r["mean"]), _ptr(r["cov"]), _ptr(r["corr"]), _ptr(r["dens"]), _ptr(r["grid"]),
                   _ptr(r["bw"]), _ptr(r["mode"]), _ptr(r["mode_dens"]))
    return d, r, (bw, given)


def rank_targets_joint(X, model, A, targets, K, Y, G=64, cut=3.0, bw=None, bw_scale=1.0, pairs=None, method=_lib.POSTERIOR_REJECTION,
                       kernel=_lib.KERNEL_EPANECHNIKOV, exclude=None, dist=False, adjust=(), dens=True, mode=True, ctx=None):
    """rank_targets followed by the joint posterior of every target (abc_rank_targets_joint_dev; method 0 rejection, 1 loclinear):
    weighted means, covariance and correlation matrices of the P parameters, and for every pair in pairs ((npairs, 2) rows (i, j),
    i != j; None: all i < j) the product-Gaussian kernel density on a G x G grid with its mode.  bw: given bandwidths (B, P) or None
    (the marginal densities' rule times bw_scale).  dens holds B * npairs * G * G doubles: size the request accordingly.  Returns
    dict(idx (B, K) int64, dist (B, K) or None, mean (B, P), cov and corr (B, P, P), dens (B, npairs, G, G) or None ([g, g']: g on
    parameter i's grid), grid (B, P, 2): lo_x and step, bw (B, P), mode (B, npairs, 2) and mode_dens (B, npairs) or None, pairs: the
    (npairs, 2) int32 host array, and the adjust members)."""
    return _rank_targets_product("joint", lambda lead, P, dev: _joint(G, cut, bw_scale, bw, pairs, lead, P, dev, dens, mode), X, model,
                                 A, targets, K, Y, method, kernel, exclude, dist, adjust, ctx)


def weighted_joint(V, w=None, G=64, cut=3.0, bw=None, bw_scale=1.0, pairs=None, dens=True, mode=True, ctx=None):
    """The joint posterior of P columns of K values (abc_weighted_joint_dev).  V: (P, K) holder as weighted_summary's; w: K weights
    or None (equal); bw: P given bandwidths or None; pairs as rank_targets_joint.  Returns dict(mean (P,), cov and corr (P, P),
    dens (npairs, G, G) or None, grid (P, 2), bw (P,), mode (npairs, 2) and mode_dens (npairs,) or None, pairs) as device tensors
    (pairs: int32 host array)."""
    return _weighted_product("joint", lambda lead, P, dev: _joint(G, cut, bw_scale, bw, pairs, lead, P, dev, dens, mode), V, w, ctx)


def _draws(S, smooth, seed, bw, bw_scale, stream, lead, P, dev, draws, src):
    """Device tensors for the draws of prod(lead) targets with P parameters and the abc_draws pointing at them (bw: given
    bandwidths or None; stream: one id per target, host, or None)"""
    f64 = torch.float64
    S = int(S)
    if smooth and bw is not None:
        bw = torch.as_tensor(bw, dtype=f64).to(dev).expand(lead + (P,)).contiguous()
    else:
        bw = None
    ids = _lib._draws_stream(stream, int(np.prod(lead, dtype=np.int64)))
    r = dict(draws=torch.empty(lead + (S, P), dtype=f64, device=dev) if draws else None,
             src=torch.empty(lead + (S,), dtype=torch.int64, device=dev) if src else None,
             bw=torch.empty(lead + (P,), dtype=f64, device=dev), ess=torch.empty(lead, dtype=f64, device=dev))
    d = _lib.Draws(S, int(bool(smooth)), float(bw_scale), _ptr(bw), int(seed) & 0xFFFFFFFFFFFFFFFF,
                   ids.ctypes.data if ids is not None else None, _ptr(r["draws"]), _ptr(r["src"]), _ptr(r["bw"]), _ptr(r["ess"]))
    return d, r, (bw, ids)


def rank_targets_draws(X, model, A, targets, K, Y, S, smooth=False, seed=0, bw=None, bw_scale=1.0, stream=None,
                       method=_lib.POSTERIOR_REJECTION, kernel=_lib.KERNEL_EPANECHNIKOV, exclude=None, dist=False, adjust=(), draws=True,
                       src=True, ctx=None):
    """rank_targets followed by S posterior draws of every target (abc_rank_targets_draws_dev; method 0 rejection, 1 loclinear): the
    weighted bootstrap of the target's K retained rows, smoothed by the marginal densities' bandwidths with smooth=True (bw: given
    bandwidths (B, P) or None: the bw.nrd0 rule times bw_scale).  seed keys the draws' Philox stream; stream: one id per target
    (host values; None: target b takes b).  The adjusted rows are made in registers: nothing of size B K P is written unless
    "theta" is named in adjust.  Returns dict(idx (B, K) int64, dist (B, K) or None, draws (B, S, P) or None, src (B, S) int64
    or None, ess (B,), bw (B, P): NaN without smoothing, and the adjust members)."""
    return _rank_targets_product("draws", lambda lead, P, dev: _draws(S, smooth, seed, bw, bw_scale, stream, lead, P, dev, draws, src),
                                 X, model, A, targets, K, Y, method, kernel, exclude, dist, adjust, ctx)


def weighted_draws(V, w=None, S=1000, smooth=False, seed=0, bw=None, bw_scale=1.0, stream=None, draws=True, src=True, ctx=None):
    """S draws of the K rows of P columns with weights w (abc_weighted_draws_dev).  V: (P, K) holder as weighted_summary's; w: K
    weights or None (equal); the other arguments as rank_targets_draws (stream: the one id, None: 0).  Returns dict(draws (S, P) or
    None, src (S,) int64 or None, ess (0-d), bw (P,)) as device tensors."""
    return _weighted_product("draws", lambda lead, P, dev: _draws(S, smooth, seed, bw, bw_scale, stream, lead, P, dev, draws, src),
                             V, w, ctx)


def _entropy(k, scale, lead, K, P, dev, knn):
    """Device tensors for the entropy of prod(lead) targets with K entries of P parameters and the abc_entropy pointing at them
    (scale: P host values or None)"""
    sc = _lib._host_doubles(scale, P, "scale")
    r = dict(H=torch.empty(lead, dtype=torch.float64, device=dev),
             knn=torch.empty(lead + (K,), dtype=torch.float64, device=dev) if knn else None,
             zeros=torch.empty(lead, dtype=torch.int64, device=dev))
    d = _lib.Entropy(int(k), sc.ctypes.data if sc is not None else None, _ptr(r["H"]), _ptr(r["knn"]), _ptr(r["zeros"]))
    return d, r, (sc,)


def rank_targets_entropy(X, model, A, targets, K, Y, k=4, scale=None, method=_lib.POSTERIOR_REJECTION,
                         kernel=_lib.KERNEL_RECTANGULAR, exclude=None, dist=False, adjust=(), knn=True, ctx=None):
    """rank_targets followed by the k-nearest-neighbour entropy of every target's posterior in all P parameters at once
    (abc_rank_targets_entropy_dev; method 0 rejection, 1 loclinear; the definition is in the header).  k: 1..8; scale: P positive
    host values the parameters are divided by, or None.  The estimate is for entries of equal weight: method 1 needs the
    rectangular kernel (the default here), and the context may hold no row importance weights.  Returns dict(idx (B, K) int64,
    dist (B, K) or None, H (B,), knn (B, K) or None, zeros (B,) int64, and the adjust members)."""
    return _rank_targets_product("entropy", lambda lead, P, dev: _entropy(k, scale, lead, K, P, dev, knn), X, model, A, targets, K, Y,
                                 method, kernel, exclude, dist, adjust, ctx)


def weighted_entropy(V, w=None, k=4, scale=None, knn=True, ctx=None):
    """The k-nearest-neighbour entropy of the K rows of P columns as one unweighted sample (abc_weighted_entropy_dev).  V: (P, K)
    holder as weighted_summary's; w must be None (the library refuses weights); the other arguments as rank_targets_entropy.
    Returns dict(H (0-d), knn (K,) or None, zeros (0-d) int64) as device tensors."""
    return _weighted_product("entropy", lambda lead, P, dev: _entropy(k, scale, lead, V.shape[1], P, dev, knn), V, w, ctx)


def _hpd(mass, lead, P, dev, outputs):
    """Device tensors for the highest-density intervals of prod(lead) targets with P parameters and the abc_hpd pointing at them"""
    ms = np.ascontiguousarray(np.asarray(mass, dtype=np.float64).reshape(-1))
    r = {k: (torch.empty(lead + (ms.size, P), dtype=torch.float64, device=dev) if k in outputs else None)
         for k in ("lo", "hi", "plo", "phi")}
    return _lib.Hpd(ms.ctypes.data, ms.size, _ptr(r["lo"]), _ptr(r["hi"]), _ptr(r["plo"]), _ptr(r["phi"])), r, (ms,)


def rank_targets_hpd(X, model, A, targets, K, Y, mass=(0.5, 0.95), method=_lib.POSTERIOR_REJECTION, kernel=_lib.KERNEL_EPANECHNIKOV,
                     exclude=None, dist=False, adjust=(), outputs=("lo", "hi", "plo", "phi"), ctx=None):
    """rank_targets followed by the highest-density interval of every (target, parameter): the shortest interval that holds each
    mass (abc_rank_targets_hpd_dev; method 0 rejection, 1 loclinear; the definition is in the header).  mass: 1 to 16 host values
    inside (0, 1).  outputs: the members to compute, the others are None.  Returns dict(idx (B, K) int64, dist (B, K) or None, lo,
    hi, plo, phi (B, nm, P), and the adjust members); (lo, hi) are rank_targets_summary's quantiles at probs = (plo, phi)."""
    return _rank_targets_product("hpd", lambda lead, P, dev: _hpd(mass, lead, P, dev, outputs), X, model, A, targets, K, Y, method,
                                 kernel, exclude, dist, adjust, ctx)


def weighted_hpd(V, w=None, mass=(0.95,), outputs=("lo", "hi", "plo", "phi"), ctx=None):
    """The highest-density intervals of P columns of K values (abc_weighted_hpd_dev).  V: (P, K) holder as weighted_summary's; w: K
    weights or None (equal).  Returns dict(lo, hi, plo, phi (nm, P)) as device tensors."""
    return _weighted_product("hpd", lambda lead, P, dev: _hpd(mass, lead, P, dev, outputs), V, w, ctx)


def rank_targets_glm(X, model, A, targets, K, Y, G=512, cut=3.0, bw=None, bw_scale=1.0, exclude=None, dist=False,
                     outputs=("dens", "lo_x", "step", "mode", "mode_dens", "mean", "var", "ess", "log_md", "status"), ctx=None,
                     probs=None, truth=None):
    """rank_targets followed by the ABC-GLM posterior of every target (abc_glm_rank_targets_dev; the definition is in the header).
    bw: given bandwidths (B, P) or None (the marginal density's rule times bw_scale).  outputs: names among _lib.GLM_OUTPUTS.
    Works on device tensors; the one copy is the model's ncomp, read back after the call (a synchronisation).  Returns dict(idx (B, K)
    int64, dist (B, K) or None, ncomp, and the outputs asked
    for (None for the rest): dens (B, P, G), lo_x, step, mode, mode_dens, mean, var (B, P), ess, log_md (B,), status (B,) int32,
    C (B, n, P), c0 (B, n), sigma_s (B, n, n) at the model's n = ncomp, T (B, P, P), peaks (B, K, P), c (B, K)).
    probs (host: 1 to 64 levels strictly inside (0, 1)) and truth (a (B, P) device tensor): the exact quantiles quant (B, nq, P) of the
    marginal mixtures and their CDF at the truth, cdf (B, P) (abc_glm_rank_targets_summary_dev; outputs may then be empty); with
    both None the call and its result are those without."""
    N, M, P, B, dev, ctx, exclude, (ldx, ldy, ldt) = _targets_holders(X, targets, Y, exclude, ctx)
    unknown = set(outputs) - set(_lib.GLM_OUTPUTS)
    if unknown:
        raise ValueError("unknown outputs %s" % sorted(unknown))
    f64 = torch.float64
    nA = min(int(A), _lib.GLM_MAX)
    sh = _lib.glm_shapes((B,), K, P, nA, int(G))
    r = {k: (torch.empty(sh[k], dtype=torch.int32 if k == "status" else f64, device=dev) if k in outputs else None)
         for k in _lib.GLM_OUTPUTS}
    if bw is not None:
        bw = torch.as_tensor(bw, dtype=f64).to(dev).expand((B, P)).contiguous()
    d = _lib.Glm(int(G), float(cut), float(bw_scale), _ptr(bw), *[_ptr(r[k]) for k in _lib.GLM_OUTPUTS])
    r.update(idx=torch.empty((B, K), dtype=torch.int64, device=dev), dist=torch.empty((B, K), dtype=f64, device=dev) if dist else None)
    tail = (ctx.handle, X.data_ptr(), ldx, Y.data_ptr(), ldy, N, M, P, model.data_ptr(), A, targets.data_ptr(), ldt, B, _ptr(exclude), K,
            r["idx"].data_ptr(), _ptr(r["dist"]))
    if probs is None and truth is None:
        ctx.check(lib().abc_glm_rank_targets_dev(C.byref(d), *tail))
    else:
        from .glm import _levels
        pr = _levels(probs)
        if truth is not None:
            if tuple(truth.shape) != (B, P):
                raise ValueError("truth must have shape %s" % ((B, P),))
            truth = truth.to(device=dev, dtype=f64).contiguous()
        r["quant"] = torch.empty((B, pr.size, P), dtype=f64, device=dev) if pr is not None else None
        r["cdf"] = torch.empty((B, P), dtype=f64, device=dev) if truth is not None else None
        sm = _lib.Summary(pr.ctypes.data if pr is not None else None, 0 if pr is None else pr.size, _ptr(truth), _ptr(r["quant"]),
                          _ptr(r["cdf"]))
        ctx.check(lib().abc_glm_rank_targets_summary_dev(C.byref(d), C.byref(sm), *tail))
    n = min(max(int(model[0].item()), 0), int(A))
    for k, tail in (("C", (n, P)), ("c0", (n,)), ("sigma_s", (n, n))):      # packed at the model's n components
        if r[k] is not None:
            r[k] = r[k].reshape(-1)[:B * int(np.prod(tail))].reshape((B,) + tail)
    r["ncomp"] = n
    return r
