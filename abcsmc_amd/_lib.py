"""ctypes binding of libabcsmc_hip.so -- exactly the symbols include/abcsmc_hip.h declares."""
import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# ABCSMC_HIP_SO: developer override for A/B runs of diagnostic builds (scripts/); default = the in-tree build
SO_PATH = os.environ.get("ABCSMC_HIP_SO") or os.path.join(_HERE, "libabcsmc_hip.so")

PRIOR_GAUSS, PRIOR_UNIF_INT, PRIOR_UNIF_REAL = 0, 1, 2
RULE_MIN_PRESS, RULE_WILCOXON = 0, 1
# the drop-in's default everywhere (C++ facade ABC::component_rule, the shell's "pls_component_rule", these mirrors, bench.py): SURVEY A.2's
# best knowledge of upstream's optimal_num_components -- argmin PRESS reduced by the Wilcoxon signed-rank test
RULE_DEFAULT = RULE_WILCOXON
KDE_AUTO, KDE_FP64 = 0, 1
GRAM_AUTO, GRAM_FP64, GRAM_I8 = 0, 1, 2
KDE_RAN_NONE, KDE_RAN_FP64, KDE_RAN_SPLIT = 0, 1, 2
DT_F64, DT_I32, DT_I64 = 0, 1, 2
COMM_ID_BYTES = 128
COMM_NONE, COMM_RCCL, COMM_CALLBACKS = 0, 1, 2
NOISE_DEVICE, NOISE_REFERENCE_STREAM = 0, 1
WEIGHT_GAUSSIAN, WEIGHT_EPANECHNIKOV = 0, 1
ALIAS_DEVICE, ALIAS_HOST = 0, 1
KERNEL_EPANECHNIKOV, KERNEL_RECTANGULAR = 0, 1
ADJ_STATUS_SKIPPED, ADJ_STATUS_RECTANGULAR = 1, 2
POSTERIOR_REJECTION, POSTERIOR_LOCLINEAR = 0, 1
TRANSF_NONE, TRANSF_LOG, TRANSF_LOGIT = 0, 1, 2
TRANSF_KINDS = {"none": TRANSF_NONE, "log": TRANSF_LOG, "logit": TRANSF_LOGIT}
BOX_COX_MAXL = 512
BOX_COX_BAD, BOX_COX_CONSTANT, BOX_COX_SKIPPED = 1, 2, 4


class LibraryMissing(ImportError):
    pass


class AbcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("abcsmc_hip error %d: %s" % (code, msg))
        self.code = code


class AbcWarning(UserWarning):
    pass




class Prior(C.Structure):
    _fields_ = [("kind", C.c_int32), ("pad_", C.c_int32), ("a", C.c_double), ("b", C.c_double)]


class Rng(C.Structure):
    _fields_ = [("s1", C.c_uint32), ("s2", C.c_uint32), ("s3", C.c_uint32)]


class GenerationCfg(C.Structure):
    _fields_ = [("N", C.c_size_t), ("M", C.c_size_t), ("P", C.c_size_t),
                ("K", C.c_size_t), ("Kp", C.c_size_t), ("Nnext", C.c_size_t),
                ("train_frac", C.c_double),
                ("max_comp", C.c_int32), ("rule", C.c_int32), ("multivariate", C.c_int32),
                ("reserved", C.c_int32)]


class GenerationIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "X", "Y", "obs", "priors", "theta_prev", "w_prev", "dv_prev", "idx", "dist", "theta", "w",
        "dv", "L", "next", "parent", "seeds")]


class ShardedCfg(C.Structure):
    _fields_ = [("n_local", C.c_size_t), ("row0", C.c_size_t), ("N_total", C.c_size_t),
                ("M", C.c_size_t), ("P", C.c_size_t), ("K", C.c_size_t), ("Kp", C.c_size_t),
                ("nnext_local", C.c_size_t), ("next0", C.c_size_t), ("Nnext_total", C.c_size_t),
                ("train_frac", C.c_double),
                ("max_comp", C.c_int32), ("rule", C.c_int32), ("multivariate", C.c_int32), ("reserved", C.c_int32)]


class Path(C.Structure):
    """abc_path: Ks (host memory, T strictly ascending tolerances); every output pointer optional (None: not written)"""
    _fields_ = [("Ks", C.c_void_p), ("T", C.c_size_t), ("post_mean", C.c_void_p), ("coef", C.c_void_p), ("rank", C.c_void_p),
                ("status", C.c_void_p), ("h", C.c_void_p)]


class ParamTransf(C.Structure):
    """abc_param_transf_t: P kinds (host int32) and the logit bounds lo / hi (host doubles, None when no kind is logit)"""
    _fields_ = [("P", C.c_size_t), ("kind", C.c_void_p), ("lo", C.c_void_p), ("hi", C.c_void_p)]


def transf_arrays(kinds, lo=None, hi=None):
    """A parameter-transform setting as host arrays (kind int32 (P,), lo (P,), hi (P,)): kinds holds TRANSF_* values or the names
    "none" / "log" / "logit"; lo / hi are read for the logit entries (scalars broadcast) and are 0 elsewhere."""
    import numpy as np
    ks = [TRANSF_KINDS[k.lower()] if isinstance(k, str) and k.lower() in TRANSF_KINDS else k for k in kinds]
    if any(isinstance(k, str) for k in ks):
        raise ValueError("transf entries must be 'none', 'log' or 'logit'")
    kind = np.ascontiguousarray(np.asarray(ks, dtype=np.int64).reshape(-1).astype(np.int32))
    logit = kind == TRANSF_LOGIT
    if logit.any() and (lo is None or hi is None):
        raise ValueError("logit entries need bounds")
    out = []
    for b in (lo, hi):
        v = np.zeros(kind.size)
        if b is not None and logit.any():
            v[logit] = np.broadcast_to(np.asarray(b, dtype=np.float64), kind.shape)[logit]
        out.append(v)
    return kind, out[0], out[1]


class AdjustOut(C.Structure):
    """abc_adjust_out: every pointer optional (None: not written)"""
    _fields_ = [("theta", C.c_void_p), ("weight", C.c_void_p), ("coef", C.c_void_p), ("rank", C.c_void_p),
                ("status", C.c_void_p)]


class BoxCoxOut(C.Structure):
    """abc_box_cox_out: every pointer optional (None: not written) except lambda"""
    _fields_ = [("lam", C.c_void_p), ("best_skew", C.c_void_p), ("skew", C.c_void_p), ("pick", C.c_void_p), ("status", C.c_void_p)]


def box_cox_grid(lambda_min=-5.0, lambda_max=5.0, step=0.1):
    """The search grid of ABC::optimize_box_cox as float64 (L,) (abc_box_cox_grid): the reference's loop over its three float
    arguments, so the defaults give 100 values and never 0 exactly.  ValueError for what the library refuses."""
    import numpy as np
    g = np.empty(BOX_COX_MAXL)
    n = C.c_size_t(0)
    with np.errstate(over="ignore"):
        a, b, st = (float(np.float32(v)) for v in (lambda_min, lambda_max, step))
    if lib().abc_box_cox_grid(a, b, st, g.ctypes.data, g.size, C.byref(n)):
        raise ValueError("box_cox_grid(%r, %r, %r): bounds and step must be finite, step > 0, and the grid must have 1 to %d values"
                         % (lambda_min, lambda_max, step, BOX_COX_MAXL))
    return g[:n.value].copy()


def _host_doubles(a, n, what):
    """a as a C-contiguous float64 host array of n entries (a scalar is broadcast), or None"""
    import numpy as np
    if a is None:
        return None
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    v = np.asarray(a, dtype=np.float64)
    v = np.full(n, float(v)) if v.ndim == 0 else np.ascontiguousarray(v.reshape(-1))
    if v.size != n:
        raise ValueError("%s needs one entry per column" % what)
    return v


class Summary(C.Structure):
    """abc_summary: probs (host, nq levels), truth / quant / cdf optional (memory as the entry point's other arrays)"""
    _fields_ = [("probs", C.c_void_p), ("nq", C.c_size_t), ("truth", C.c_void_p), ("quant", C.c_void_p), ("cdf", C.c_void_p)]


class Density(C.Structure):
    """abc_density: G, cut, bw_scale, then bw (optional input) and the optional outputs dens / grid / bw_out / mode / mode_dens
    (memory as the entry point's other arrays)"""
    _fields_ = [("G", C.c_size_t), ("cut", C.c_double), ("bw_scale", C.c_double), ("bw", C.c_void_p), ("dens", C.c_void_p),
                ("grid", C.c_void_p), ("bw_out", C.c_void_p), ("mode", C.c_void_p), ("mode_dens", C.c_void_p)]


class Joint(C.Structure):
    """abc_joint: G, cut, bw_scale, bw (optional input), pairs (optional, HOST int32 npairs x 2) and npairs, then the optional
    outputs mean / cov / corr / dens / grid / bw_out / mode / mode_dens (memory as the entry point's other arrays)"""
    _fields_ = [("G", C.c_size_t), ("cut", C.c_double), ("bw_scale", C.c_double), ("bw", C.c_void_p), ("pairs", C.c_void_p),
                ("npairs", C.c_size_t), ("mean", C.c_void_p), ("cov", C.c_void_p), ("corr", C.c_void_p), ("dens", C.c_void_p),
                ("grid", C.c_void_p), ("bw_out", C.c_void_p), ("mode", C.c_void_p), ("mode_dens", C.c_void_p)]


class Draws(C.Structure):
    """abc_draws: S, smooth, bw_scale, bw (optional input), seed, stream (optional, HOST uint64, one id per target), then the
    optional outputs draws / src / bw_out / ess (memory as the entry point's other arrays)"""
    _fields_ = [("S", C.c_size_t), ("smooth", C.c_int), ("bw_scale", C.c_double), ("bw", C.c_void_p), ("seed", C.c_uint64),
                ("stream", C.c_void_p), ("draws", C.c_void_p), ("src", C.c_void_p), ("bw_out", C.c_void_p), ("ess", C.c_void_p)]


class Entropy(C.Structure):
    """abc_entropy: k (1..8), scale (optional, HOST float64, one value per parameter), then the optional outputs H / knn / zeros
    (memory as the entry point's other arrays)"""
    _fields_ = [("k", C.c_int), ("scale", C.c_void_p), ("H", C.c_void_p), ("knn", C.c_void_p), ("zeros", C.c_void_p)]


class Hpd(C.Structure):
    """abc_hpd: mass (host, nm masses inside (0, 1)), then the optional outputs lo / hi / plo / phi (memory as the entry point's
    other arrays)"""
    _fields_ = [("mass", C.c_void_p), ("nm", C.c_size_t), ("lo", C.c_void_p), ("hi", C.c_void_p), ("plo", C.c_void_p),
                ("phi", C.c_void_p)]


GLM_MAX = 32
GLM_OUTPUTS = ("dens", "lo_x", "step", "mode", "mode_dens", "mean", "var", "ess", "log_md", "C", "c0", "sigma_s", "T", "peaks", "c",
               "status")


class Glm(C.Structure):
    """abc_glm: G, cut, bw_scale, then bw (optional input) and the optional outputs in GLM_OUTPUTS' order (memory as the entry
    point's other arrays)"""
    _fields_ = ([("G", C.c_size_t), ("cut", C.c_double), ("bw_scale", C.c_double), ("bw", C.c_void_p)] +
                [(name, C.c_void_p) for name in GLM_OUTPUTS])


def glm_shapes(lead, K, P, n, G):
    """The shape of every output of an abc_glm for targets of shape lead (() for the generic entry) with n components"""
    lead = tuple(lead)
    return {"dens": lead + (P, G), "lo_x": lead + (P,), "step": lead + (P,), "mode": lead + (P,), "mode_dens": lead + (P,),
            "mean": lead + (P,), "var": lead + (P,), "ess": lead, "log_md": lead, "C": lead + (n, P), "c0": lead + (n,),
            "sigma_s": lead + (n, n), "T": lead + (P, P), "peaks": lead + (K, P), "c": lead + (K,), "status": lead}


def _draws_stream(stream, n):
    """The stream ids of an abc_draws as a C-contiguous uint64 host array of n entries, or None (target b takes id b)"""
    import numpy as np
    if stream is None:
        return None
    ids = np.ascontiguousarray(np.asarray(stream, dtype=np.uint64).reshape(-1))
    if ids.size != n:
        raise ValueError("stream needs one id per target")
    return ids


def _joint_pairs(pairs, P):
    """The pair list of an abc_joint as C-contiguous int32 (npairs, 2) host arrays: (all, given).  given is what the descriptor
    points at: the caller's rows (i, j), or None when pairs is None; all is then every i < j in the library's default order
    (0, 1), (0, 2), ..., and given otherwise."""
    import numpy as np
    if pairs is None:
        return np.array([(i, j) for i in range(P) for j in range(i + 1, P)], dtype=np.int32).reshape(-1, 2), None
    given = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    return given, given


ALL_REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
BROADCAST_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)


WX_REC_LEVELS = 6
WX_PATH_NONE, WX_PATH_CASCADE, WX_PATH_CASCADE_THEN_SORTED, WX_PATH_SORTED = -1, 0, 1, 2


class WxTestRecord(C.Structure):
    """abc_wx_test_record (include/abcsmc_hip.h)"""
    _fields_ = [("response", C.c_int32), ("candidate", C.c_int32), ("optimum", C.c_int32), ("n_levels", C.c_int32),
                ("verdict", C.c_int32), ("passed", C.c_int32), ("w_taken", C.c_int32), ("pad_", C.c_int32),
                ("nz", C.c_uint64), ("W", C.c_double),
                ("level_bins", C.c_int64 * WX_REC_LEVELS), ("level_lo2", C.c_int64 * WX_REC_LEVELS),
                ("level_hi2", C.c_int64 * WX_REC_LEVELS)]


class CommCallbacks(C.Structure):
    _fields_ = [("all_reduce_sum", ALL_REDUCE_FN), ("all_gather", ALL_GATHER_FN), ("broadcast", BROADCAST_FN),
                ("user", C.c_void_p)]


def make_priors(spec):
    arr = (Prior * len(spec))()
    for i, (k, a, b) in enumerate(spec):
        arr[i].kind, arr[i].a, arr[i].b = int(k), float(a), float(b)
    return arr


# symbol -> (restype, argtypes); MUST list every function declared in include/abcsmc_hip.h
_vp, _sz, _u64, _i, _d = C.c_void_p, C.c_size_t, C.c_uint64, C.c_int, C.c_double
SIGNATURES = {
    "abc_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "abc_ctx_destroy": (None, [_vp]),
    "abc_last_error": (C.c_char_p, [_vp]),
    "abc_ctx_set_stream": (_i, [_vp, _vp]),
    "abc_ctx_use_own_stream": (_i, [_vp]),
    "abc_ctx_set_kde_mode": (_i, [_vp, _i]),
    "abc_ctx_set_gram_mode": (_i, [_vp, _i]),
    "abc_kde_last_kernel": (_i, [_vp, _vp]),
    "abc_ctx_set_wx_record": (_i, [_vp, _i]),
    "abc_wx_last_record": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "abc_ctx_set_noise_mode": (_i, [_vp, _i]),
    "abc_ctx_set_weight_kernel": (_i, [_vp, _i]),
    "abc_perturb_giveups": (_i, [_vp, _vp, _i]),
    "abc_generation_giveups": (_i, [_vp, _vp]),
    "abc_generation_repeats": (_i, [_vp, _vp, _vp, _i]),
    "abc_ctx_set_alias_mode": (_i, [_vp, _i]),
    "abc_alias_stats": (_i, [_vp, _vp, _vp, _i]),
    "abc_select_stats": (_i, [_vp, _vp, _vp, _i]),
    "abc_ws_info": (_i, [_vp, _vp, _vp, _vp]),
    "abc_alias_table": (_i, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "abc_ctx_synchronize": (_i, [_vp]),
    "abc_version": (_i, []),
    "abc_timing_enable": (_i, [_vp, _i]),
    "abc_timing_read": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i]),
    "abc_timing_overhead": (_i, [_vp, _i, _vp]),
    "abc_rng_set": (None, [_vp, C.c_ulong]),
    "abc_rng_get": (C.c_uint32, [_vp]),
    "abc_rng_jump": (None, [_vp, _u64]),
    "abc_particle_ranking_pls": (_i, [_vp, _vp, _vp, _vp, _sz, _sz, _sz, _d, _i, _i, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "abc_particle_ranking_pls_targets": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _sz, _d, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp]),
    "abc_rank_targets_dev": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp]),
    "abc_targets_fallbacks": (_i, [_vp, _vp, _i]),
    "abc_ctx_set_param_transf": (_i, [_vp, _vp]),
    "abc_param_transf_dev": (_i, [_vp, _vp, _sz, _sz, _sz, _i, _vp, _sz]),
    "abc_param_transf": (_i, [_vp, _vp, _sz, _sz, _i, _vp]),
    "abc_param_transf_outside": (_i, [_vp, _vp, _i]),
    "abc_box_cox_grid": (_i, [C.c_float, C.c_float, C.c_float, _vp, _sz, _vp]),
    "abc_optimize_box_cox_dev": (_i, [_vp, _vp, _sz, _sz, _sz, _vp, _vp, _sz, _vp]),
    "abc_optimize_box_cox": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp]),
    "abc_box_cox_dev": (_i, [_vp, _vp, _sz, _sz, _sz, _vp, _vp, _vp, _sz]),
    "abc_box_cox": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "abc_ctx_set_adjust_hcorr": (_i, [_vp, _i]),
    "abc_adjust_last_hcorr": (_i, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "abc_adjust_hcorr_skipped": (_i, [_vp, _vp, _i]),
    "abc_ctx_set_adjust_ridge": (_i, [_vp, _vp, _sz]),
    "abc_adjust_last_ridge": (_i, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "abc_adjust_ridge_unscored": (_i, [_vp, _vp, _i]),
    "abc_ctx_set_row_weights": (_i, [_vp, _vp, _sz]),
    "abc_ctx_set_row_weights_dev": (_i, [_vp, _vp, _sz]),
    "abc_row_weights_info": (_i, [_vp, _vp, _vp, _vp]),
    "abc_rank_targets_adjust_dev": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _i, _vp, _vp,
                                         _vp]),
    "abc_particle_ranking_pls_targets_adjust": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _sz, _d, _i, _i, _vp, _sz, _i, _vp, _vp,
                                                     _vp, _vp]),
    "abc_rank_targets_path_dev": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _i, _vp, _vp, _vp]),
    "abc_particle_ranking_pls_targets_path": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _sz, _d, _i, _i, _vp, _i, _vp, _vp, _vp,
                                                   _vp]),
    "abc_rank_targets_path_summary_dev": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _i, _i, _vp, _vp,
                                               _vp, _vp]),
    "abc_particle_ranking_pls_targets_path_summary": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _sz, _d, _i, _i, _vp, _i, _i, _vp, _vp,
                                                           _vp, _vp, _vp]),
    "abc_particle_ranking_simple": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp]),
    "abc_calculate_doubled_variance": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "abc_weight_predictive_prior_uniform": (_i, [_vp, _sz, _vp]),
    "abc_weight_predictive_prior": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp]),
    "abc_setup_mvn_sampler": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "abc_sample_posterior": (_i, [_vp, _vp, _vp, _sz, _sz, _vp]),
    "abc_sample_mvn_predictive_priors": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp]),
    "abc_sample_predictive_priors": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp]),
    "abc_generation_dev": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "abc_stats_len": (_sz, [_sz, _sz]),
    "abc_stats_shift_dev": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _sz, _vp]),
    "abc_stats_accumulate_dev": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _sz, _u64, _u64, _vp]),
    "abc_model_len": (_sz, [_sz, _sz, _sz]),
    "abc_pls_model_dev": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _i, _vp]),
    "abc_pls_wilcoxon_dev": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _sz, _sz, _sz, _vp]),
    "abc_model_ncomp": (_i, [_vp, _vp, _sz, _sz, _sz, _vp]),
    "abc_simple_model_dev": (_i, [_vp, _vp, _vp, _sz, _sz, _vp]),
    "abc_project_distance_dev": (_i, [_vp, _vp, _sz, _sz, _sz, _sz, _sz, _vp, _i, _vp]),
    "abc_select_smallest_dev": (_i, [_vp, _vp, _sz, _sz, _u64, _vp, _vp]),
    "abc_select_begin_dev": (_i, [_vp, _u64, _vp, _vp]),
    "abc_select_hist_dev": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "abc_select_pick_dev": (_i, [_vp, _vp, _i, _vp, _u64]),
    "abc_select_count_dev": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "abc_select_compact_dev": (_i, [_vp, _vp, _sz, _vp, _u64, _u64, _u64, _vp, _vp]),
    "abc_sort_pairs_dev": (_i, [_vp, _vp, _vp, _sz]),
    "abc_merge_sorted_runs_dev": (_i, [_vp, _vp, _vp, _i, _sz, _vp, _vp]),
    "abc_gather_rows_dev": (_i, [_vp, _vp, _sz, _sz, _sz, _vp, _sz, _u64, _vp, _sz]),
    "abc_doubled_variance_dev": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "abc_weights_raw_dev": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp, _vp, _vp]),
    "abc_normalize_l2_dev": (_i, [_vp, _vp, _sz]),
    "abc_setup_mvn_sampler_dev": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "abc_resample_dev": (_i, [_vp, _vp, _vp, _sz, _u64, _sz, _vp]),
    "abc_perturb_dev": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _u64, _sz, _i, _vp, _vp, _vp, _u64]),
    "abc_comm_unique_id": (_i, [_vp]),
    "abc_comm_init_rank": (_i, [_vp, _i, _i, _vp]),
    "abc_comm_init_callbacks": (_i, [_vp, _i, _i, _vp]),
    "abc_comm_destroy": (_i, [_vp]),
    "abc_comm_info": (_i, [_vp, _vp, _vp, _vp]),
    "abc_ctx_create_multi": (_i, [_vp, _i, _vp]),
    "abc_generation_sharded_dev": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "abc_generation_multi": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    # ABC-GLM: the descriptor first, the context second
    "abc_glm_rank_targets_dev": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _vp]),
    "abc_glm_particle_ranking_pls_targets": (_i, [_vp, _vp, _vp, _vp, _sz, _sz, _sz, _vp, _sz, _d, _i, _i, _vp, _sz, _vp, _vp, _vp]),
    "abc_glm_weighted_dev": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, _sz, _sz, _sz, _vp, _vp]),
    "abc_glm_weighted": (_i, [_vp, _vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp]),
    # the same with the exact quantiles and CDF: glm, then the abc_summary, then the context
    "abc_glm_rank_targets_summary_dev": (_i, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp,
                                              _vp]),
    "abc_glm_particle_ranking_pls_targets_summary": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _vp, _sz, _d, _i, _i, _vp, _sz, _vp,
                                                          _vp, _vp]),
    "abc_glm_weighted_summary_dev": (_i, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _sz, _sz, _sz, _vp, _vp]),
    "abc_glm_weighted_summary": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp]),
}

# The posterior products (abc_summary, abc_density, abc_joint, abc_draws) share their four argument lists, each ending in the product's
# descriptor: a new product adds its name here.
_PRODUCT_ARGS = {
    "abc_rank_targets_%s_dev": [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _i, _i, _vp, _vp, _vp, _vp],
    "abc_particle_ranking_pls_targets_%s": [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _sz, _d, _i, _i, _vp, _sz, _i, _i, _vp, _vp, _vp, _vp,
                                            _vp],
    "abc_weighted_%s_dev": [_vp, _vp, _sz, _sz, _sz, _vp, _vp],
    "abc_weighted_%s": [_vp, _vp, _sz, _sz, _vp, _vp],
}
PRODUCTS = ("summary", "density", "joint", "draws")
# products of an unweighted sample: the same four argument lists; the entries refuse weights that are not all equal
UNWEIGHTED_PRODUCTS = ("entropy",)
# products of the summaries' sort that came after the four above: the same argument lists, any weights
INTERVAL_PRODUCTS = ("hpd",)
SIGNATURES.update((entry % product, (_i, args)) for product in PRODUCTS + UNWEIGHTED_PRODUCTS + INTERVAL_PRODUCTS
                  for entry, args in _PRODUCT_ARGS.items())

_LIB = None


def lib():
    """Load the HIP library; fail loudly when it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise LibraryMissing(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C abcsmc_amd/csrc` (there is no CPU fallback)" % SO_PATH)
        # One HIP runtime per process: PyTorch ships its own libamdhip64.so (same SONAME as /opt/rocm's).  Loaded after
        # PyTorch's, this library binds to that copy; loaded BEFORE it, it pulls in the system copy and PyTorch later adds its
        # own -- two runtimes, and the second to touch the device fails (abc_ctx_create then reports no usable GPU).  The
        # device / multi-GPU drivers of this package use torch for memory and streams anyway, so it goes first when present.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)   # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


class Context:
    """One abc_ctx per GPU (include/abcsmc_hip.h: abc_ctx_create)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        rc = lib().abc_ctx_create(int(device), C.byref(self._h))
        if rc:
            raise AbcError(rc, "abc_ctx_create(device=%d) failed: no usable GPU (HIP path is mandatory)" % device)
        self.device = device
        self._hcorr = False          # the variance correction as set through this object (adjust_hcorr restores it)
        self._ridge = ()             # the ridge penalties as set through this object (adjust_ridge restores them)
        self._row_weights = None     # the row weights as set through this object (row_weights restores them)

    @classmethod
    def from_handle(cls, handle, device):
        """a view of a context somebody else owns (MultiContext.context): not destroyed with this object"""
        self = cls.__new__(cls)
        self._h = C.c_void_p(handle)
        self.device = int(device)
        self._hcorr = False
        self._ridge = ()
        self._row_weights = None
        self._borrowed = True
        return self

    @property
    def handle(self):
        return self._h

    def check(self, rc):
        """non-zero status: AbcError (the ABI has no positive status)"""
        if rc:
            raise AbcError(rc, lib().abc_last_error(self._h).decode())

    def generation_repeats(self, reset=False):
        """(ranking repeats, generation repeats) since the context was created / the last reset: what the speculation on the
        component count has cost (abc_generation_repeats)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.check(lib().abc_generation_repeats(self._h, C.byref(a), C.byref(b), int(reset)))
        return a.value, b.value

    def select_stats(self, reset=False):
        """(bin selections, bin give-ups) since the context was created / the last reset: selections queued on the sampled-range
        bin path, and those of them the selection's own check repeated with the radix select (abc_select_stats)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.check(lib().abc_select_stats(self._h, C.byref(a), C.byref(b), int(reset)))
        return a.value, b.value

    def ws_info(self):
        """(reserved, asked, peak) of the scratch arena after the most recent call (abc_ws_info): the arena's bytes, the bound that
        call reserved before the rounding to 1 MiB, and the highest offset its allocations reached"""
        r, a, p = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self.check(lib().abc_ws_info(self._h, C.byref(r), C.byref(a), C.byref(p)))
        return r.value, a.value, p.value

    def generation_giveups(self):
        """proposals the most recent generation call gave up on (abc_generation_giveups); no synchronisation"""
        n = C.c_uint64(0)
        lib().abc_generation_giveups(self._h, C.byref(n))
        return n.value

    def warn_generation_giveups(self):
        """after abc_generation_dev: a Python warning when the perturbation gave up on proposals during that call (they are
        their valid parents / prior means; the reference would still be retrying, AbcUtil.cpp:132).  No synchronisation."""
        n = C.c_uint64(0)
        lib().abc_generation_giveups(self._h, C.byref(n))
        if n.value:
            import warnings
            self.last_warning = ("generation complete, but the perturbation gave up on %d proposal(s): they are their parents "
                                 "(MULTIVARIATE, after 16384 rejected attempts) or prior means (INDEPENDENT, after 1000); "
                                 "abc_perturb_giveups has the total" % n.value)
            warnings.warn(AbcWarning(self.last_warning), stacklevel=3)
        return n.value

    def set_stream(self, stream_ptr):
        if getattr(self, "_stream", -1) != stream_ptr:      # abc_ctx_set_stream synchronises: only on change
            self.check(lib().abc_ctx_set_stream(self._h, C.c_void_p(stream_ptr)))
            self._stream = stream_ptr

    def timing_enable(self, on=True):
        """False / 0: off; True / 1: every stage; 2: only the k_gram / k_kde kernel brackets"""
        self.check(lib().abc_timing_enable(self._h, int(on)))

    def timing_read(self, reset=True):
        """-> {stage: (device_ms, host_ms, launches)} accumulated since the last reset"""
        n = 32
        names = (C.c_char_p * n)()
        ms, hms, cnt = (C.c_double * n)(), (C.c_double * n)(), (C.c_longlong * n)()
        k = lib().abc_timing_read(self._h, names, ms, hms, cnt, n, int(reset))
        if k < 0:
            self.check(k)
        return {names[i].decode(): (ms[i], hms[i], cnt[i]) for i in range(k)}

    def timing_overhead(self, reps=50):
        """ms an event pair around one kernel reports beyond the kernel's execution (abc_timing_overhead)"""
        ov = C.c_double(0.0)
        self.check(lib().abc_timing_overhead(self._h, int(reps), C.byref(ov)))
        return ov.value

    def synchronize(self):
        self.check(lib().abc_ctx_synchronize(self._h))

    def kde_last_kernel(self):
        """KDE_RAN_FP64 / KDE_RAN_SPLIT: which kernel summed the pairs of the last weight call (abc_kde_last_kernel)"""
        w = C.c_int(0)
        self.check(lib().abc_kde_last_kernel(self._h, C.byref(w)))
        return w.value

    def set_wx_record(self, on):
        """switch the per-test record of the Wilcoxon reductions on this context on or off (abc_ctx_set_wx_record)"""
        self.check(lib().abc_ctx_set_wx_record(self._h, int(bool(on))))

    def wx_last_record(self):
        """(path, tests) of the last Wilcoxon reduction run with the record on (abc_wx_last_record): path one of WX_PATH_*, tests a
        list of dicts in plan order -- response, candidate, optimum, nz, levels [(bins, lo2, hi2), ...] (Python integers),
        n_levels, verdict, passed, W, w_taken"""
        n, path = C.c_size_t(0), C.c_int(0)
        self.check(lib().abc_wx_last_record(self._h, None, 0, C.byref(n), C.byref(path)))      # (the number of tests first)
        cap = n.value
        buf = (WxTestRecord * max(cap, 1))()
        if cap:
            self.check(lib().abc_wx_last_record(self._h, buf, cap, C.byref(n), C.byref(path)))
        out = []
        for r in buf[:n.value]:
            k = min(int(r.n_levels), WX_REC_LEVELS)
            out.append(dict(response=int(r.response), candidate=int(r.candidate), optimum=int(r.optimum), nz=int(r.nz),
                            levels=[(int(r.level_bins[i]), int(r.level_lo2[i]), int(r.level_hi2[i])) for i in range(k)],
                            n_levels=int(r.n_levels), verdict=int(r.verdict), passed=int(r.passed), W=float(r.W),
                            w_taken=int(r.w_taken)))
        return path.value, out

    def set_weight_kernel(self, kernel):
        """WEIGHT_GAUSSIAN (the reference's, default) or WEIGHT_EPANECHNIKOV (extension): abc_ctx_set_weight_kernel"""
        self.check(lib().abc_ctx_set_weight_kernel(self._h, int(kernel)))

    def set_noise_mode(self, mode):
        """NOISE_DEVICE (Philox stream on the device, default) or NOISE_REFERENCE_STREAM (the reference's sequential taus2
        consumption, host loop): abc_ctx_set_noise_mode"""
        self.check(lib().abc_ctx_set_noise_mode(self._h, int(mode)))

    def perturb_giveups(self, reset=False):
        """proposals the perturbation gave up on (abc_perturb_giveups)"""
        n = C.c_uint64(0)
        self.check(lib().abc_perturb_giveups(self._h, C.byref(n), int(reset)))
        return n.value

    def targets_fallbacks(self, reset=False):
        """targets the batched ranking recomputed by the exact single-target path (abc_targets_fallbacks)"""
        n = C.c_uint64(0)
        self.check(lib().abc_targets_fallbacks(self._h, C.byref(n), int(reset)))
        return n.value

    def set_param_transf(self, kinds=None, lo=None, hi=None):
        """The parameter transforms of the local-linear adjustment (abc_ctx_set_param_transf; the definition is in the header):
        kinds: one of "none" / "log" / "logit" (or TRANSF_*) per parameter, lo / hi: the logit entries' bounds.  None (or every
        kind "none") turns them off.  The setting is copied; it applies to every call of this context that regresses."""
        if kinds is None:
            self.check(lib().abc_ctx_set_param_transf(self._h, None))
            self._transf = None
            return
        kind, lo_a, hi_a = transf_arrays(kinds, lo, hi)
        tf = ParamTransf(kind.size, kind.ctypes.data, lo_a.ctypes.data, hi_a.ctypes.data)
        self.check(lib().abc_ctx_set_param_transf(self._h, C.byref(tf)))
        self._transf = (kind, lo_a, hi_a) if (kind != TRANSF_NONE).any() else None

    def param_transf(self, kinds=None, lo=None, hi=None):
        """Context manager: set_param_transf(kinds, lo, hi) inside the block, what was set before (through this object) after it."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            before = getattr(self, "_transf", None)
            self.set_param_transf(kinds, lo, hi)
            try:
                yield self
            finally:
                if before is None:
                    self.set_param_transf(None)
                else:
                    self.set_param_transf(*before)
        return scope()

    def param_transf_outside(self, reset=False):
        """entries the forward transforms found outside their domain (abc_param_transf_outside)"""
        n = C.c_uint64(0)
        self.check(lib().abc_param_transf_outside(self._h, C.byref(n), int(reset)))
        return n.value

    def optimize_box_cox(self, X, grid, shift=None, skew=False):
        """The Box-Cox skewness search over the columns of a host table (abc_optimize_box_cox; the definition is in the header):
        X float64 (N, M) Fortran-ordered, grid float64 (L,), shift float64 (M,) or None.  Returns dict(lam (M,), skew_best (M,),
        pick (M,) int32, status (M,) int32, skew (M, L) or None)."""
        import numpy as np
        N, M = X.shape
        r = dict(lam=np.empty(M), skew_best=np.empty(M), pick=np.empty(M, dtype=np.int32), status=np.empty(M, dtype=np.int32),
                 skew=np.empty((M, grid.size)) if skew else None)
        out = BoxCoxOut(*(r[k].ctypes.data if r[k] is not None else None for k in ("lam", "skew_best", "skew", "pick", "status")))
        self.check(lib().abc_optimize_box_cox(self._h, X.ctypes.data, N, M, shift.ctypes.data if shift is not None else None,
                                              grid.ctypes.data, grid.size, C.byref(out)))
        return r

    def box_cox(self, X, lam, shift=None):
        """The Box-Cox transform of a host table (abc_box_cox): X float64 (n, M) Fortran-ordered, lam float64 (M,), shift float64
        (M,) or None.  Returns a new (n, M) Fortran-ordered array."""
        import numpy as np
        n, M = X.shape
        out = np.empty((n, M), order="F")
        self.check(lib().abc_box_cox(self._h, X.ctypes.data, n, M, lam.ctypes.data, shift.ctypes.data if shift is not None else None,
                                     out.ctypes.data))
        return out

    def set_adjust_hcorr(self, on):
        """The heteroscedastic variance correction of the local-linear adjustment (abc_ctx_set_adjust_hcorr; the definition is
        in the header): on or off (the default).  It applies to every call of this context that regresses."""
        self.check(lib().abc_ctx_set_adjust_hcorr(self._h, int(on)))
        self._hcorr = bool(on)

    def adjust_hcorr(self, on=True):
        """Context manager: set_adjust_hcorr(on) inside the block, what was set before (through this object) after it."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            before = self._hcorr
            self.set_adjust_hcorr(on)
            try:
                yield self
            finally:
                self.set_adjust_hcorr(before)
        return scope()

    def last_hcorr(self):
        """hcoef of the last regressing call made under the variance correction (abc_adjust_last_hcorr): an array of shape
        (slots, A + 1, P), row 0 the log residual variance at the observation (NaN: the parameter was skipped), row 1 + k the
        slope g_k; (0, 0, 0) while there is nothing"""
        import numpy as np
        n, a1, P = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self.check(lib().abc_adjust_last_hcorr(self._h, None, 0, C.byref(n), C.byref(a1), C.byref(P)))
        out = np.empty((n.value, a1.value, P.value))
        if out.size:
            self.check(lib().abc_adjust_last_hcorr(self._h, out.ctypes.data, out.size, C.byref(n), C.byref(a1), C.byref(P)))
        return out

    def adjust_hcorr_skipped(self, reset=False):
        """(slot, parameter) pairs the variance correction skipped (abc_adjust_hcorr_skipped)"""
        n = C.c_uint64(0)
        self.check(lib().abc_adjust_hcorr_skipped(self._h, C.byref(n), int(reset)))
        return n.value

    def set_adjust_ridge(self, lambdas):
        """The ridge adjustment with the penalty chosen by leave-one-out PRESS (abc_ctx_set_adjust_ridge; the definition is in the
        header): a strictly ascending sequence of 1 to 8 finite penalties >= 0, or None / () for off (the default).  It applies
        to every call of this context that regresses."""
        import numpy as np
        lam = np.ascontiguousarray(np.asarray(() if lambdas is None else lambdas, dtype=np.float64).reshape(-1))
        self.check(lib().abc_ctx_set_adjust_ridge(self._h, lam.ctypes.data if lam.size else None, lam.size))
        self._ridge = tuple(lam.tolist())

    def adjust_ridge(self, lambdas):
        """Context manager: set_adjust_ridge(lambdas) inside the block, what was set before (through this object) after it."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            before = self._ridge
            self.set_adjust_ridge(lambdas)
            try:
                yield self
            finally:
                self.set_adjust_ridge(before)
        return scope()

    def last_ridge(self):
        """(pick (slots, P) int32, press (slots, L, P)) of the last regressing call made under the ridge adjustment
        (abc_adjust_last_ridge): the chosen penalty's index and the leave-one-out PRESS of every penalty (+inf: the fit
        interpolates); shapes (0, 0) and (0, 0, 0) while there is nothing"""
        import numpy as np
        n, L, P = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self.check(lib().abc_adjust_last_ridge(self._h, None, 0, None, 0, C.byref(n), C.byref(L), C.byref(P)))
        pick = np.empty((n.value, P.value), dtype=np.int32)
        press = np.empty((n.value, L.value, P.value))
        if pick.size:
            self.check(lib().abc_adjust_last_ridge(self._h, pick.ctypes.data, pick.size, press.ctypes.data, press.size, C.byref(n),
                                                   C.byref(L), C.byref(P)))
        return pick, press

    def adjust_ridge_unscored(self, reset=False):
        """(slot, parameter) pairs for which no penalty could be scored (abc_adjust_ridge_unscored)"""
        n = C.c_uint64(0)
        self.check(lib().abc_adjust_ridge_unscored(self._h, C.byref(n), int(reset)))
        return n.value

    def set_row_weights(self, w):
        """Row importance weights of the batched ranking (abc_ctx_set_row_weights / _dev; the definition is in the header): one
        finite weight >= 0 per row of the table, at least one positive, as a NumPy array / sequence (host) or a float64 torch tensor
        (a device tensor is read on the device); None for off (the default).  The context keeps its own copy.  It applies to every
        rank_targets_* / particle_ranking_PLS_targets* call of this context, whose N must equal the count."""
        import numpy as np
        if w is None:
            self.check(lib().abc_ctx_set_row_weights(self._h, None, 0))
            self._row_weights = None
            return
        if hasattr(w, "data_ptr"):                                   # a torch tensor
            import torch
            t = w.detach().reshape(-1).to(torch.float64).contiguous()
            if t.is_cuda:
                torch.cuda.synchronize(t.device)
                self.check(lib().abc_ctx_set_row_weights_dev(self._h, t.data_ptr(), t.numel()))
                self._row_weights = t.clone()
                return
            w = t.numpy()
        a = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1))
        if a.size == 0:
            raise ValueError("row weights: an empty array (None turns the setting off)")
        self.check(lib().abc_ctx_set_row_weights(self._h, a.ctypes.data, a.size))
        self._row_weights = a.copy()

    def row_weights(self, w):
        """Context manager: set_row_weights(w) inside the block, what was set before (through this object) after it."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            before = self._row_weights
            self.set_row_weights(w)
            try:
                yield self
            finally:
                self.set_row_weights(before)
        return scope()

    def row_weights_info(self):
        """(N, positive, ess) of the row weights that are set (abc_row_weights_info): their count (0: off), the number of positive
        ones and (sum w)^2 / sum w^2 of the whole table"""
        n, pos, ess = C.c_size_t(0), C.c_size_t(0), C.c_double(0.0)
        self.check(lib().abc_row_weights_info(self._h, C.byref(n), C.byref(pos), C.byref(ess)))
        return n.value, pos.value, ess.value

    def set_alias_mode(self, mode):
        """ALIAS_DEVICE (default: the resampling table built on the GPU by verified prefix scans) or ALIAS_HOST: abc_ctx_set_alias_mode"""
        self.check(lib().abc_ctx_set_alias_mode(self._h, int(mode)))

    def alias_stats(self, reset=False):
        """(device builds, host fallbacks) of the resampling table (abc_alias_stats)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.check(lib().abc_alias_stats(self._h, C.byref(a), C.byref(b), int(reset)))
        return a.value, b.value

    def alias_table(self, w):
        """(F, A, on_device): the Walker alias table of the weights w as the context builds it (abc_alias_table)"""
        import numpy as np
        w = np.ascontiguousarray(w, dtype=np.float64)
        F, A, on = np.empty(w.size), np.empty(w.size, dtype=np.uint64), C.c_int(0)
        self.check(lib().abc_alias_table(self._h, w.ctypes.data, w.size, F.ctypes.data, A.ctypes.data, C.byref(on)))
        return F, A, on.value

    def set_gram_mode(self, mode):
        """GRAM_AUTO (byte-limb statistics kernel for wide sets whose partitions hold >= 400 000 rows), GRAM_FP64, or GRAM_I8 (the
        byte-limb kernel from 200 000 rows: A/B runs, its own tests) -- abc_ctx_set_gram_mode"""
        self.check(lib().abc_ctx_set_gram_mode(self._h, int(mode)))

    def set_kde_mode(self, mode):
        """KDE_AUTO (split-operand matrix-pipe kernel where it applies) or KDE_FP64 (abc_ctx_set_kde_mode)"""
        self.check(lib().abc_ctx_set_kde_mode(self._h, int(mode)))

    # ---- communicator of the row-sharded generation (include/abcsmc_hip.h, "Multi-GPU") ----------------------
    def comm_init_rccl(self, world, rank, unique_id):
        """RCCL communicator from the 128-byte id rank 0 obtained with comm_unique_id() and handed to every rank"""
        buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self.check(lib().abc_comm_init_rank(self._h, int(world), int(rank), buf))

    def comm_init_callbacks(self, world, rank, all_reduce_sum, all_gather, broadcast):
        """collectives supplied by the caller: python callables (buf_ptr, count, dtype, stream) etc. -> 0 on success"""
        # A Python exception inside a ctypes callback is printed and turned into a return value of 0 -- which the C++ driver
        # reads as success and carries on with un-reduced statistics.  Every callback body is therefore guarded: an exception
        # (transport timeout, shape error) is logged, remembered (Context.comm_callback_error) and reported as a non-zero
        # status, so the collective -- and the generation -- fail with ABC_ERR_COMM.
        self.comm_callback_error = None

        def guarded(fn, what):
            def run(*a):
                try:
                    rc = fn(*a)
                    return int(rc) if rc is not None else 0
                except BaseException as e:       # noqa: BLE001 -- nothing may propagate into the C++ caller
                    import traceback
                    self.comm_callback_error = e
                    sys.stderr.write("abcsmc_amd: %s callback raised %s: %s\n" % (what, type(e).__name__, e))
                    traceback.print_exc()
                    return 1
            return run

        ar, ag, bc = guarded(all_reduce_sum, "all_reduce_sum"), guarded(all_gather, "all_gather"), guarded(broadcast, "broadcast")
        self._cb = CommCallbacks(ALL_REDUCE_FN(lambda u, b, n, dt, st: ar(b, n, dt, st)),
                                 ALL_GATHER_FN(lambda u, s, r, nb, st: ag(s, r, nb, st)),
                                 BROADCAST_FN(lambda u, b, nb, root, st: bc(b, nb, root, st)), None)
        self.check(lib().abc_comm_init_callbacks(self._h, int(world), int(rank), C.byref(self._cb)))

    def comm_info(self):
        k, w, r = C.c_int(0), C.c_int(1), C.c_int(0)
        self.check(lib().abc_comm_info(self._h, C.byref(k), C.byref(w), C.byref(r)))
        return k.value, w.value, r.value

    def comm_destroy(self):
        self.check(lib().abc_comm_destroy(self._h))

    def close(self):
        if self._h and not getattr(self, "_borrowed", False):
            lib().abc_ctx_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id():
    """128-byte RCCL id (abc_comm_unique_id); created on ONE rank and sent to the others"""
    buf = (C.c_char * COMM_ID_BYTES)()
    rc = lib().abc_comm_unique_id(buf)
    if rc:
        raise AbcError(rc, "abc_comm_unique_id failed (librccl.so.1 not loadable?)")
    return bytes(buf)


class MultiContext:
    """ndev contexts of ONE process joined by RCCL communicators (abc_ctx_create_multi)"""

    def __init__(self, devices):
        self.devices = [int(d) for d in devices]
        n = len(self.devices)
        self._arr = (C.c_void_p * n)()
        rc = lib().abc_ctx_create_multi((C.c_int * n)(*self.devices), n, self._arr)
        if rc:
            raise AbcError(rc, "abc_ctx_create_multi(%r) failed" % (self.devices,))

    def context(self, i):
        """the context of device i as a Context (a view: the MultiContext keeps the ownership); each is driven from its own
        host thread (abc_generation_sharded_dev is collective over the ndev contexts)"""
        return Context.from_handle(self._arr[i], self.devices[i])

    def generation(self, cfg, io, rng):
        """host-pointer generation over all devices (abc_generation_multi); -> ncomp"""
        nc = C.c_int32(0)
        rc = lib().abc_generation_multi(self._arr, len(self.devices), C.byref(cfg), C.byref(io), C.byref(rng), C.byref(nc))
        if rc:
            raise AbcError(rc, lib().abc_last_error(self._arr[0]).decode())
        return nc.value

    def close(self):
        for i in range(len(self.devices)):
            if self._arr[i]:
                lib().abc_ctx_destroy(self._arr[i])
                self._arr[i] = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_DEFAULT_CTX = {}


def default_context(device=0):
    if device not in _DEFAULT_CTX:
        _DEFAULT_CTX[device] = Context(device)
    return _DEFAULT_CTX[device]
