"""Which kernels the weight stage runs: a copy of the plan (abcsmc_amd/csrc/weights_plan.h: abc_weights_plan) and of the kernel
tables behind launch_weights_prev() and launch_weights_raw() in abcsmc_amd/csrc/weights.hip, so that a test can state the kernel
and branch it means to reach and check that it does.  tests/test_weights_dispatch.py holds this copy against the plan function
itself (tests/cxx/weights_plan_probe.cpp) and the tables of weights.hip; tests/test_gpu_weights_branches.py asserts through it
that its cases reach every instance.

Pair kernels (the `pair` of plan), as the tuple that names the template instance:
    ("split", V, WPS)       k_kde_split<V, WPS, ...>: V = chunks (1, 2), KS_FOLD + chunks (101, 102: the norm pieces in spare
                            K-slots) or KS_TOPN + chunks (201, 202: tiles in the order of the norm tops); WPS waves per SIMD
    ("split_lds", V, W)     k_kde_split_lds<V, W, ...>: three or four chunks, the previous tiles staged in LDS (3, 4, 103, 104, 203, 204)
    ("kde", PP)             k_kde<PP>, the fp64 kernel on PP padded columns
    ("epan", PP)            k_epan<PP>
    ("gen", epan)           k_kde_gen beyond 64 parameters; epan: its Epanechnikov branch
Behind a split kernel k_kde_fixups<PP> always follows (`fixup`): the far rows' pairs in fp64 or, where the split kernel declined
the call (`ran`), kde_body<PP> as its stand-in.

far() marks the rows the split kernel leaves to the fix-ups and ran() says which kernel summed the pairs, as
abc_kde_last_kernel reports it: the library does not hand out its far-row counters.
"""
import numpy as np

KS_FOLD, KS_TOPN = 100, 200
KS_BOUND, KS_NORM2 = 8.0, 400.0            # |scaled coordinate|, |scaled row|^2 of the split kernel's exact range
KS_LW_MIN, KS_LW_CAP = -100.0, 300.0       # -log2 w' of a non-zero previous weight
KS_MAX_FAR_J = 1024                        # far previous rows the column fix-up takes
W_COORD_BOUND = 2000.0                     # a scaled coordinate beyond it: exponents may leave int32, fp64 takes the call
KDE_LDS_W3 = 3                             # waves per SIMD of the three-chunk LDS kernels
TOPN_MIN_PAIRS = 4.0e9                     # ABC_KDE_TOPN_MIN_PAIRS' default
RAN_FP64, RAN_SPLIT = 1, 2                 # _lib.KDE_RAN_FP64, _lib.KDE_RAN_SPLIT
SQRT_LOG2E = np.sqrt(np.log2(np.e))


def padded_width(P):
    """PP: the next power of two from 2 on, beyond 64 the next multiple of 64"""
    PP = 2
    while PP < P:
        PP *= 2
    if P > 64:
        PP = (P + 63) // 64 * 64
    return PP


def chunks(P):
    return 1 if P <= 16 else 2 if P <= 32 else 3 if P <= 48 else 4


def kde_slices(kn, Kp, PP):
    """weights_plan.h: abc_kde_slices"""
    if kn == 0 or Kp == 0:
        return 1
    rows_per_slice = max(24576 // PP, 256)
    s = (Kp + rows_per_slice - 1) // rows_per_slice
    rb = (kn + 255) // 256
    if s * rb < 4096:
        s = (4096 + rb - 1) // rb
    s = min(s, max((64 << 20) // (8 * kn), 8))
    s = min(s, Kp // 64)
    s = max(s, 1)
    return min(s, 1024)


def plan(P, kn, Kp, kde_mode="auto", weight_kernel="gauss", topn_min_pairs=TOPN_MIN_PAIRS):
    """-> dict of what one stage-level call (abc_weights_raw_dev, abc_weight_predictive_prior: the previous set prepared inside
    the call, kn_max = kn) queues for P parameters, kn new rows and Kp previous ones:
        width    the padded width PP          chunks   16-parameter chunks (3: dealt out as four, three stored)
        split / fold / topn                   pair     the pair kernel (above)
        wrows    the k_wrows instance: (1,), (2,), (4, 3), (4,), or None (k_wscale)
        fixup    PP of k_kde_fixups<PP>, or None
        slices   column slices (the grid's y)  tiles   32-row tiles of the previous set
        lim_i    far new rows the fix-ups take: more, and the fp64 stand-in takes the call"""
    PP, NCH = padded_width(P), chunks(P)
    epan = weight_kernel == "epan"
    split = PP >= 8 and P <= 64 and kde_mode != "fp64" and not epan
    fold = split and P + 3 <= 16 * NCH
    topn = split and not fold and float(Kp * kn) >= topn_min_pairs
    rb = (kn + 255) // 256
    slices = kde_slices(kn, Kp, PP)
    if split:
        slices = min(slices, max(12288 // rb, 8))
    if epan:
        pair = ("gen", True) if PP > 64 else ("epan", PP)
    elif split:
        V = NCH + (KS_FOLD if fold else KS_TOPN if topn else 0)
        pair = ("split", V, 3 if NCH == 1 else 2) if NCH <= 2 else ("split_lds", V, KDE_LDS_W3 if NCH == 3 else 2)
    else:
        pair = ("gen", False) if PP > 64 else ("kde", PP)
    wrows = ((1,), (2,), (4, 3), (4,))[NCH - 1] if split else None
    return {"width": PP, "chunks": NCH, "split": split, "fold": fold, "topn": topn, "pair": pair, "wrows": wrows,
            "fixup": PP if split else None, "slices": slices, "tiles": (Kp + 31) // 32, "lim_i": kn // 16 + 32}


def scale(dv):
    """k_wprep: sqrt(log2 e) / sqrt(dv_p), 0 for a converged parameter"""
    dv = np.asarray(dv, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(dv != 0.0, SQRT_LOG2E / np.sqrt(np.where(dv != 0.0, dv, 1.0)), 0.0)


def centre(tp, dv):
    """k_wcentre: the first previous row plus the mean offset of the previous set from it, each offset clipped at +-16 units"""
    tp = np.asarray(tp, dtype=np.float64)
    sc = scale(dv)
    d = np.clip((tp - tp[0]) * sc, -16.0, 16.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sc != 0.0, tp[0] + d.mean(axis=0) / np.where(sc != 0.0, sc, 1.0), tp[0])


def far(th, tp, wp, dv):
    """-> (far_i, far_j, beyond): the rows of the new / the previous set that k_wrows takes out of the matrix work -- a scaled
    coordinate above KS_BOUND, a scaled squared norm above KS_NORM2, a non-zero previous weight with -log2 w' outside
    [KS_LW_MIN, KS_LW_CAP]; a previous row of weight 0 is never far (it takes no part anyway) --, and whether a coordinate of
    either set lies beyond W_COORD_BOUND (wc->far)"""
    th, tp, wp = (np.asarray(a, dtype=np.float64) for a in (th, tp, wp))
    sc, c = scale(dv), centre(tp, dv)
    a, b = (th - c) * sc, (tp - c) * sc
    out_a = ~(np.abs(a) <= KS_BOUND).all(axis=1) | ~((a * a).sum(axis=1) <= KS_NORM2)
    out_b = ~(np.abs(b) <= KS_BOUND).all(axis=1) | ~((b * b).sum(axis=1) <= KS_NORM2)
    with np.errstate(divide="ignore", invalid="ignore"):
        lw = -np.log2(wp)
    out_b = (out_b | ~((lw >= KS_LW_MIN) & (lw <= KS_LW_CAP))) & (wp != 0.0)
    beyond = bool((np.abs(a) > W_COORD_BOUND).any() or (np.abs(b) > W_COORD_BOUND).any())
    return out_a, out_b, beyond


def ran(pl, th, tp, wp, dv):
    """what abc_kde_last_kernel reports after the call that plan `pl` describes on these rows (th: the kn rows of the call)"""
    if not pl["split"]:
        return RAN_FP64
    fi, fj, beyond = far(th, tp, wp, dv)
    converged = bool((np.asarray(dv) == 0.0).any())
    on = not converged and not beyond and fi.sum() <= pl["lim_i"] and fj.sum() <= KS_MAX_FAR_J
    return RAN_SPLIT if on else RAN_FP64


def reachable(max_p=200):
    """-> the sets of pair kernels, k_wrows instances and fix-up widths the two launchers can reach"""
    pairs, wrows, fix = set(), set(), set()
    for P in range(1, max_p + 1):
        for mode in ("auto", "fp64"):
            for wk in ("gauss", "epan"):
                for minp in (TOPN_MIN_PAIRS, 0.0):
                    pl = plan(P, 300, 700, mode, wk, minp)
                    pairs.add(pl["pair"])
                    if pl["wrows"]:
                        wrows.add(pl["wrows"])
                    if pl["fixup"]:
                        fix.add(pl["fixup"])
    return pairs, wrows, fix
