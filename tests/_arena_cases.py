"""The catalogue of calls behind tests/test_gpu_arena.py and tests/test_arena_catalogue_cpu.py: one row per entry point of
include/abcsmc_hip.h that takes a context and can take memory from its scratch arena, at shapes where the hand-kept bound the entry
reserves (abc_ws_need, tg_need, the products' *_need, the host entries' staging) can be wrong by a factor.

CASES maps a name to a Case:
    entry      the C ABI function the row exercises (everything else its run calls goes through a second, preparing context)
    klass      "block": the row states arena blocks, the largest of which is at least 4 MiB and a quarter of what the entry reserves;
               "sharp": an entry whose reservation holds no generous term (SHARP_ENTRIES: the bound is the product's own plus a few
                        KiB, so the smallest under-count shows), blocks stated for the record;
               "stage": the generation, the reference-signature host functions and the stage entries, one case each at the shapes
                        tests/test_gpu_parity.py uses for them (STAGE_ENTRIES); their bound is abc_ws_need's sum, no block stated
    settings   what is set on the context around the call: hcorr, ridge (the penalties), transf, row_weights
    host()     the fixed inputs as NumPy arrays (synthetic.Workload or default_rng with fixed seeds), made once per process
    shapes     name -> shape of what host() returns, by the same arithmetic as blocks
    blocks     [(what, bytes, recipe)]: arena blocks of the call by arithmetic on the shapes, the one the shape is meant to stress
               first; recipe (or None) names the plan the bytes come from, so that the CPU test can make them again from the arrays
               host() builds (block_from_recipe)
    run(ctx, prep)   the call on ctx -> dict of NumPy outputs, every output member the entry has, and the path counters as
               "counter/..." entries.  Inputs that have to be on the device, and everything the call needs that another entry makes (the
               fitted model, a selection's state), are made once per process on prep, a context of their own.

The byte counts mirror the launchers' plans (tg_plan, sm_batch, aj_plan): a change of a plan shows up here as a failing (e) of the GPU
test, and the row is then given another shape, not another fraction."""
import contextlib
import ctypes as C
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from abcsmc_amd import _lib, synthetic  # noqa: E402

MIB = 1 << 20
RIDGE = (0.0, 1e-3, 1e-2, 0.1, 1.0, 10.0, 100.0, 1000.0)           # ABC_RIDGE_MAXL = 8 penalties
HPD_MASS = tuple((i + 1) / 17.0 for i in range(16))                # the most masses the header allows (16)
PATH_T = 16                                                        # ... and the most tolerances

# entries whose reservation is their own blocks plus a few KiB: nothing generous to hide an under-count in
SHARP_ENTRIES = {"abc_weighted_%s%s" % (p, s) for p in ("summary", "hpd", "density", "joint", "draws", "entropy") for s in ("_dev", "")} | {
    "abc_param_transf", "abc_param_transf_dev", "abc_optimize_box_cox_dev", "abc_optimize_box_cox", "abc_box_cox_dev", "abc_box_cox"}
# entries that run at the shapes tests/test_gpu_parity.py uses for them
STAGE_ENTRIES = {
    "abc_generation_dev", "abc_particle_ranking_pls", "abc_particle_ranking_simple", "abc_calculate_doubled_variance",
    "abc_weight_predictive_prior_uniform", "abc_weight_predictive_prior", "abc_setup_mvn_sampler", "abc_sample_posterior",
    "abc_sample_mvn_predictive_priors", "abc_sample_predictive_priors", "abc_alias_table", "abc_stats_shift_dev",
    "abc_stats_accumulate_dev", "abc_pls_model_dev", "abc_pls_wilcoxon_dev", "abc_simple_model_dev", "abc_project_distance_dev",
    "abc_select_smallest_dev", "abc_select_begin_dev", "abc_select_hist_dev", "abc_select_pick_dev", "abc_select_count_dev",
    "abc_select_compact_dev", "abc_sort_pairs_dev", "abc_merge_sorted_runs_dev", "abc_gather_rows_dev", "abc_doubled_variance_dev",
    "abc_weights_raw_dev", "abc_normalize_l2_dev", "abc_setup_mvn_sampler_dev", "abc_resample_dev", "abc_perturb_dev"}

# Functions of the header whose first parameter is a context and that no row names, each with its reason
EXEMPT = {
    "abc_ctx_destroy": "frees the context",
    "abc_last_error": "getter",
    "abc_ctx_set_stream": "setter",
    "abc_ctx_use_own_stream": "setter",
    "abc_ctx_synchronize": "waits for the stream, no arena",
    "abc_ctx_set_kde_mode": "setter",
    "abc_ctx_set_gram_mode": "setter",
    "abc_kde_last_kernel": "getter (a path counter of the rows)",
    "abc_ctx_set_wx_record": "setter",
    "abc_wx_last_record": "getter: reads the context's own record buffer",
    "abc_ctx_set_weight_kernel": "setter",
    "abc_ctx_set_noise_mode": "setter",
    "abc_ctx_set_alias_mode": "setter",
    "abc_alias_stats": "getter (a path counter of the rows)",
    "abc_perturb_giveups": "getter (a path counter of the rows)",
    "abc_generation_giveups": "getter",
    "abc_generation_repeats": "getter (a path counter of the rows)",
    "abc_select_stats": "getter (a path counter of the rows)",
    "abc_ws_info": "getter: the readout itself",
    "abc_timing_enable": "setter",
    "abc_timing_read": "getter",
    "abc_timing_overhead": "empty kernels between events, no arena",
    "abc_model_ncomp": "getter: one copy of the model header",
    "abc_targets_fallbacks": "getter (a path counter of the rows)",
    "abc_ctx_set_param_transf": "setter: a device allocation of the context's own",
    "abc_param_transf_outside": "getter",
    "abc_ctx_set_adjust_hcorr": "setter",
    "abc_adjust_last_hcorr": "getter: reads the context's own record buffer",
    "abc_adjust_hcorr_skipped": "getter",
    "abc_ctx_set_adjust_ridge": "setter",
    "abc_adjust_last_ridge": "getter: reads the context's own record buffer",
    "abc_adjust_ridge_unscored": "getter",
    "abc_ctx_set_row_weights": "setter: a device allocation of the context's own",
    "abc_ctx_set_row_weights_dev": "setter: a device allocation of the context's own",
    "abc_row_weights_info": "getter",
    "abc_comm_init_rank": "abc_comm_*: needs ranks",
    "abc_comm_init_callbacks": "abc_comm_*: needs ranks",
    "abc_comm_destroy": "abc_comm_*: needs ranks",
    "abc_comm_info": "abc_comm_*: getter",
    "abc_generation_sharded_dev": "sharded: needs ranks",
    "abc_generation_multi": "sharded: needs one context per device",
}


# ---- the launchers' plans, as arithmetic ---------------------------------------------------------------------------------------------
def cand_bytes(N, K, B, excl):
    """candidate segments, scattered copy and bin offsets of a chunk of targets (targets.hip: tg_plan, tg_chunk)"""
    S = 4096
    if N <= S:
        Cc = N
    else:
        f = (K + (1 if excl else 0)) / N
        qd = f * S + 4.0 * math.sqrt(S * f * (1.0 - f)) + 8.0
        q = S - 1 if qd >= S - 1 else int(qd)
        cap = ((q + 1.0) / S + 8.0 * math.sqrt(q + 1.0) / S) * N + 256.0
        Cc = N if cap >= N else int(cap)
        Cc = max(Cc, K)
    per = Cc * 24 + 2049 * 4
    return min(B, max(1, (512 * MIB) // per)) * per


def sort_bytes(B, K, P):
    """key and index buffers of one batch of targets on the summaries' global path (summary.hip: sm_batch); none up to K = 8192"""
    if K <= 8192:
        return 0
    return min(B, max(1, (256 * MIB) // (P * K * 24))) * P * K * 24


def moment_bytes(B, K, A, P, T=1):
    """moment blocks of one batch of targets, T sets on a path (adjust.hip: aj_plan, aj_batch)"""
    n = min(64, (K + 255) // 256)
    CH = (K + n - 1) // n
    part = ((K + CH - 1) // CH) * (1 + A) * (1 + A + P) * 8
    return min(B, max(1, (256 * MIB) // (T * part))) * T * part



def block_from_recipe(recipe, N, P, A, B):
    """the bytes of a block again, from the shapes of the arrays a row builds"""
    kind = recipe[0]
    if kind == "cand":
        return cand_bytes(N, recipe[1], B, True)
    if kind == "sort":
        return sort_bytes(B, recipe[1], P)
    if kind == "moment":
        return moment_bytes(B, recipe[1], A, P, recipe[2])
    if kind == "BKP":
        return B * recipe[1] * P * 8
    if kind == "BK":
        return recipe[2] * B * recipe[1] * 8
    if kind == "table":
        return N * (A + P) * 8
    raise ValueError(recipe)


def blk(what, recipe, N, P, A, B):
    return (what, block_from_recipe(recipe, N, P, A, B), recipe)


# ---- fixed inputs --------------------------------------------------------------------------------------------------------------------
FIT = dict(N=20000, M=8, P=16, A=8, seed=2024)                      # the one fit of the targets family's device rows
BIG = dict(N=120000, M=4, P=64, A=4, seed=77)                       # the path summary under row weights


def _fblk(what, recipe, B):
    """a block of a row on FIT"""
    return blk(what, recipe, FIT["N"], FIT["P"], FIT["A"], B)


@functools.lru_cache(maxsize=None)
def _table(N, M, P, seed):
    wl = synthetic.Workload(M, P, seed)
    X, Y = wl.rows(0, N)
    return wl, X, Y


def _target_rows(N, B):
    return (np.arange(B, dtype=np.int64) * 7 + 3) % N


@functools.lru_cache(maxsize=None)
def _fit_settings(N, M, P, seed):
    """row weights (some zero) and log / logit transforms the table's parameters are inside of"""
    _, _, Y = _table(N, M, P, seed)
    rw = np.random.default_rng(seed + 1).uniform(0.5, 1.5, N)
    rw[::97] = 0.0
    sd = Y.std(axis=0)
    kinds = ["logit" if j % 2 == 0 else ("log" if Y[:, j].min() > 0 else "none") for j in range(P)]
    return rw, (tuple(kinds), Y.min(axis=0) - sd, Y.max(axis=0) + sd)


def targets_host(fit, B):
    _, X, Y = _table(fit["N"], fit["M"], fit["P"], fit["seed"])
    rows = _target_rows(fit["N"], B)
    rw, tf = _fit_settings(fit["N"], fit["M"], fit["P"], fit["seed"])
    return dict(X=X, Y=Y, targets=np.ascontiguousarray(X[rows]), exclude=rows, truth=np.ascontiguousarray(Y[rows]), rw=rw, tf=tf)


def targets_shapes(fit, B):
    N, M, P = fit["N"], fit["M"], fit["P"]
    return dict(X=(N, M), Y=(N, P), targets=(B, M), exclude=(B,), truth=(B, P), rw=(N,))


def values_host(K, P, seed, weights=True):
    rng = np.random.default_rng(seed)
    V = np.asfortranarray(np.round(rng.normal(size=(K, P)) * (1.0 + np.arange(P)), 3))
    w = rng.uniform(0.0, 1.0, size=K)
    w[::53] = 0.0
    return dict(V=V, w=w if weights else None, truth=V[K // 3].copy())


def values_shapes(K, P, weights=True):
    s = dict(V=(K, P), truth=(P,))
    if weights:
        s["w"] = (K,)
    return s


# ---- what lives on the device, made once per process on the preparing context -------------------------------------------------------
_DEV = {}


def _dev(key, make):
    if key not in _DEV:
        _DEV[key] = make()
    return _DEV[key]


def _fit_dev(fit, prep):
    """the table and its fitted model on the device: the statistics pass and the fit run on prep"""
    def make():
        import torch
        from abcsmc_amd import device, sharded
        wl, X, Y = _table(fit["N"], fit["M"], fit["P"], fit["seed"])
        N, M, P, A = fit["N"], fit["M"], fit["P"], fit["A"]
        be = sharded.HipBackend("cuda:0", prep)
        dX, dY = device.colmajor(X, "cuda:0"), device.colmajor(Y, "cuda:0")
        stats = be.zeros(be.stats_len(M, P))
        be.stats_shift(dX, dY, stats)
        be.stats_accumulate(dX, dY, 0, N // 2, stats)
        model = be.zeros(be.model_len(M, P, A))
        be.pls_model(stats, device.colmajor(wl.observed(), "cuda:0"), M, P, A, _lib.RULE_MIN_PRESS, model)
        prep.synchronize()
        torch.cuda.synchronize()
        return dict(X=dX, Y=dY, stats=stats, model=model)
    return _dev(("fit", fit["N"], fit["M"], fit["P"], fit["seed"]), make)


def _targets_dev(fit, B, prep):
    def make():
        import torch
        from abcsmc_amd import device
        h = targets_host(fit, B)
        d = dict(_fit_dev(fit, prep))
        d.update(targets=device.colmajor(h["targets"], "cuda:0"), exclude=torch.from_numpy(h["exclude"]).to("cuda:0"),
                 truth=torch.from_numpy(h["truth"]).to("cuda:0"))
        return d
    return _dev(("targets", fit["N"], fit["seed"], B), make)


def _values_dev(K, P, seed, weights):
    def make():
        import torch
        from abcsmc_amd import device
        h = values_host(K, P, seed, weights)
        return dict(V=device.colmajor(h["V"], "cuda:0"), w=torch.from_numpy(h["w"]).to("cuda:0") if weights else None,
                    truth=torch.from_numpy(h["truth"]).to("cuda:0"))
    return _dev(("values", K, P, seed, weights), make)


# ---- outputs and counters ------------------------------------------------------------------------------------------------------------
def to_numpy(v):
    if v is None:
        return None
    if hasattr(v, "detach"):
        return v.detach().cpu().numpy()
    return np.asarray(v)


def _outputs(d, skip=()):
    return {k: to_numpy(v) for k, v in d.items() if v is not None and k not in skip}


def reset_counters(ctx):
    ctx.alias_stats(True)
    ctx.select_stats(True)
    ctx.targets_fallbacks(True)
    ctx.generation_repeats(True)
    ctx.perturb_giveups(True)


def read_counters(ctx, kde):
    c = {"counter/alias_stats": ctx.alias_stats(), "counter/select_stats": ctx.select_stats(),
         "counter/targets_fallbacks": ctx.targets_fallbacks(), "counter/generation_repeats": ctx.generation_repeats(),
         "counter/perturb_giveups": ctx.perturb_giveups()}
    if kde:
        c["counter/kde_last_kernel"] = ctx.kde_last_kernel()
    return {k: np.atleast_1d(np.asarray(v, dtype=np.int64)) for k, v in c.items()}


@contextlib.contextmanager
def applied(ctx, settings, host):
    """the row's settings on the context around the call, what was there before after it"""
    with contextlib.ExitStack() as st:
        if settings.get("hcorr"):
            st.enter_context(ctx.adjust_hcorr(True))
        if settings.get("ridge"):
            st.enter_context(ctx.adjust_ridge(list(settings["ridge"])))
        if settings.get("transf"):
            kinds, lo, hi = host["tf"]
            st.enter_context(ctx.param_transf(list(kinds), lo, hi))
        if settings.get("row_weights"):
            st.enter_context(ctx.row_weights(host["rw"]))
        yield


class Case:
    def __init__(self, name, entry, klass, host, shapes, call, blocks=(), settings=None, kde=False, A=None):
        self.name, self.entry, self.klass = name, entry, klass
        self.host, self.shapes, self.call = host, shapes, call
        self.blocks = [tuple(b) + (None,) * (3 - len(b)) for b in blocks]      # (a block without a recipe: fixed arithmetic)
        self.settings = dict(settings or {})
        self.kde = kde
        self.A = A                # components of the fit (block rows)

    @property
    def dominant(self):
        return max((b[1] for b in self.blocks), default=0)

    def run(self, ctx, prep):
        """the call on ctx (AbcError propagates) -> its outputs and path counters as NumPy arrays"""
        import torch
        h = self.host()
        reset_counters(ctx)
        with applied(ctx, self.settings, h):
            out = self.call(ctx, prep, h)
            ctx.synchronize()
            torch.cuda.synchronize()
        out = _outputs(out)
        out.update(read_counters(ctx, self.kde))
        return out


CASES = {}


def _add(name, entry, klass, host, shapes, call, blocks=(), settings=None, kde=False, A=None):
    assert name not in CASES, name
    CASES[name] = Case(name, entry, klass, host, shapes, call, blocks, settings, kde, A)


# ---- generic entries: abc_weighted_* in both forms ----------------------------------------------------------------------------------
def _generic(product, name, K, P, seed, dev_kw, host_kw, blocks_dev, blocks_host, weights=True):
    from_dev = dict(summary="weighted_summary", hpd="weighted_hpd", density="weighted_density", joint="weighted_joint",
                    draws="weighted_draws", entropy="weighted_entropy")[product]
    host = functools.partial(values_host, K, P, seed, weights)
    shapes = values_shapes(K, P, weights)

    def call_dev(ctx, prep, h, kw=dev_kw):
        from abcsmc_amd import device
        d = _values_dev(K, P, seed, weights)
        kw = {k: (d["truth"] if v == "truth" else v) for k, v in kw.items()}
        if product == "entropy":
            return getattr(device, from_dev)(d["V"], None, ctx=ctx, **kw)
        return getattr(device, from_dev)(d["V"], d["w"], ctx=ctx, **kw)

    def call_host(ctx, prep, h, kw=host_kw):
        from abcsmc_amd import abcutil
        kw = {k: (h["truth"] if v == "truth" else v) for k, v in kw.items()}
        if product == "entropy":
            return abcutil.knn_entropy(h["V"], ctx=ctx, **kw)
        return getattr(abcutil, from_dev)(h["V"], h["w"], ctx=ctx, **kw)

    if dev_kw is not None:
        _add("w%s_dev_%s" % (product, name), "abc_weighted_%s_dev" % product, "sharp", host, shapes, call_dev, blocks_dev)
    if host_kw is not None:
        _add("w%s_host_%s" % (product, name), "abc_weighted_%s" % product, "sharp", host, shapes, call_host, blocks_host)


PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)
for _K in (8192, 20000):        # the last LDS size; three sort chunks and two merge rounds
    _sb = [("sort buffers", sort_bytes(1, _K, 3))] if _K > 8192 else []
    _st = [("staged values", (_K * 3 + _K) * 8)]
    _generic("summary", "k%d" % _K, _K, 3, 101, dict(probs=PROBS, truth="truth"), dict(probs=PROBS, truth="truth"), _sb, _sb + _st)
    _generic("hpd", "k%d" % _K, _K, 3, 102, dict(mass=HPD_MASS), dict(mass=HPD_MASS), _sb, _sb + _st)
_dsb = [("sort buffers", sort_bytes(1, 9000, 5)), ("grid chunks' partial modes", 5 * 8 * 12)]
_generic("density", "dens", 9000, 5, 103, dict(G=4096, bw=0.25, dens=True, mode=True), dict(G=4096, bw=0.25),
         _dsb, _dsb + [("staged densities", 5 * 4096 * 8)])
_generic("density", "mode", 9000, 5, 103, dict(G=4096, bw=0.25, dens=False, mode=True), None, _dsb, None)
_generic("joint", "p17", 1000, 17, 104, dict(G=256, dens=False, mode=True), None,
         [("pair candidates", 136 * 16 * 12)], None)              # 136 pairs x 16 blocks of candidates
_generic("joint", "g129", 1000, 5, 105, dict(G=129, dens=True, mode=True), None, [("pair candidates", 10 * 9 * 12)], None)
_generic("joint", "g129p9", 1000, 9, 106, None, dict(G=129, dens=True), None,
         [("staged pair densities", 36 * 129 * 129 * 8)])         # B x pairs x G^2 doubles staged
_generic("draws", "smooth", 20000, 64, 107, dict(S=4096, smooth=True, seed=11), dict(S=4096, smooth=True, seed=11),
         [("sort buffers", sort_bytes(1, 20000, 64))],
         [("sort buffers", sort_bytes(1, 20000, 64)), ("staged values", (20000 * 64 + 20000) * 8)])
_generic("entropy", "p64", 3000, 64, 108, dict(k=4), dict(k=4), [("scaled values", 3000 * 64 * 8)],
         [("scaled values", 3000 * 64 * 8), ("staged values", 3000 * 64 * 8)], weights=False)


# ---- the targets family, device entries, on the one fit -----------------------------------------------------------------------------
ADJ_MEMBERS = ("theta", "weight", "coef", "rank", "status")


def _tg_dev(name, entry, B, call, blocks, settings=None, fit=FIT):
    def run(ctx, prep, h):
        return call(ctx, _targets_dev(fit, B, prep))
    _add(name, entry, "block", functools.partial(targets_host, fit, B), targets_shapes(fit, B), run, blocks, settings, A=fit["A"])


def _rank_plain(ctx, d):
    from abcsmc_amd import device
    idx, dist, pm = device.rank_targets(d["X"], d["model"], FIT["A"], d["targets"], 2000, Y=d["Y"], exclude=d["exclude"], post_mean=True,
                                        ctx=ctx)
    return dict(idx=idx, dist=dist, post_mean=pm)


_tg_dev("rank_plain", "abc_rank_targets_dev", 2000, _rank_plain, [_fblk("candidate segments", ("cand", 2000), 2000)])


def _adjust(dist, ctx, d):
    from abcsmc_amd import device                                   # coef, rank and status only: nothing of size B K P
    return device.rank_targets_adjust(d["X"], d["model"], FIT["A"], d["targets"], 4000, d["Y"], exclude=d["exclude"], theta=False,
                                      weight=False, dist=dist, ctx=ctx)


_ADJ_BLOCKS = [_fblk("moment blocks", ("moment", 4000, 1), 512), _fblk("candidate segments", ("cand", 4000), 512),
               _fblk("row-major table", ("table",), 512)]          # 4 B K >= N: the table is taken
for _n, _s in (("plain", None), ("hcorr", dict(hcorr=True)), ("ridge", dict(ridge=RIDGE)), ("transf", dict(transf=True)),
               ("row_weights", dict(row_weights=True))):
    _tg_dev("adjust_" + _n, "abc_rank_targets_adjust_dev", 512, functools.partial(_adjust, True), _ADJ_BLOCKS, _s)
_tg_dev("adjust_nodist", "abc_rank_targets_adjust_dev", 512, functools.partial(_adjust, False),
        _ADJ_BLOCKS + [_fblk("the arena's own dist", ("BK", 4000, 1), 512)])

PATH_KS = tuple(250 * (t + 1) for t in range(PATH_T))               # K_max = 4000


def _path(ctx, d):
    from abcsmc_amd import device
    return device.rank_targets_path(d["X"], d["model"], FIT["A"], d["targets"], PATH_KS, d["Y"], exclude=d["exclude"], ctx=ctx)


_PATH_BLOCKS = [_fblk("moment blocks of all tolerances", ("moment", 4000, PATH_T), 256), _fblk("candidate segments", ("cand", 4000), 256)]
for _n, _s in (("plain", None), ("hcorr", dict(hcorr=True)), ("ridge", dict(ridge=RIDGE)), ("transf", dict(transf=True)),
               ("row_weights", dict(row_weights=True))):
    _tg_dev("path_" + _n, "abc_rank_targets_path_dev", 256, _path, _PATH_BLOCKS, _s)

PROD_B, PROD_K = 40, 9000                                          # the global path of the summaries' sort, one batch


def _product(product, method, kw, ctx, d, K=PROD_K):
    from abcsmc_amd import device
    kw = {k: (d["truth"] if v == "truth" else v) for k, v in kw.items()}
    adjust = ("coef", "rank", "status") if method == 1 else ()
    return getattr(device, "rank_targets_" + product)(d["X"], d["model"], FIT["A"], d["targets"], K, d["Y"], method=method,
                                                      exclude=d["exclude"], dist=True, adjust=adjust, ctx=ctx, **kw)


_SORT = [_fblk("sort buffers", ("sort", PROD_K), PROD_B), _fblk("candidate segments", ("cand", PROD_K), PROD_B)]
PRODUCTS = {
    "summary": (dict(probs=PROBS, truth="truth"), _SORT),
    "hpd": (dict(mass=HPD_MASS), _SORT),
    "density": (dict(G=4096), _SORT),
    "joint": (dict(G=65), _SORT),                                    # all 120 pairs
    "draws": (dict(S=1000, smooth=True, seed=5), _SORT),
    "entropy": (dict(k=4), [_fblk("scaled values", ("BKP", PROD_K), PROD_B), _fblk("candidate segments", ("cand", PROD_K), PROD_B)]),
}
for _p, (_kw, _bl) in PRODUCTS.items():
    _e = "abc_rank_targets_%s_dev" % _p
    _kw1 = dict(_kw, kernel=_lib.KERNEL_RECTANGULAR) if _p == "entropy" else _kw
    _tg_dev("%s_m0" % _p, _e, PROD_B, functools.partial(_product, _p, 0, _kw), _bl)
    _tg_dev("%s_m1" % _p, _e, PROD_B, functools.partial(_product, _p, 1, _kw1), _bl)
    _tg_dev("%s_m1_transf" % _p, _e, PROD_B, functools.partial(_product, _p, 1, _kw1), _bl, dict(transf=True))
    if _p != "entropy":                                              # (the entropy is refused under row weights)
        _tg_dev("%s_m0_row_weights" % _p, _e, PROD_B, functools.partial(_product, _p, 0, _kw), _bl, dict(row_weights=True))
_tg_dev("summary_m1_hcorr", "abc_rank_targets_summary_dev", PROD_B, functools.partial(_product, "summary", 1, PRODUCTS["summary"][0]),
        _SORT, dict(hcorr=True))
_tg_dev("summary_m1_ridge", "abc_rank_targets_summary_dev", PROD_B, functools.partial(_product, "summary", 1, PRODUCTS["summary"][0]),
        _SORT, dict(ridge=RIDGE))

PS_KS = (100, 2000, 9000)


def _path_summary(method, Ks, fit, ctx, d):
    from abcsmc_amd import device
    return device.rank_targets_path_summary(d["X"], d["model"], fit["A"], d["targets"], Ks, d["Y"], probs=PROBS, truth=d["truth"],
                                            method=method, exclude=d["exclude"], ctx=ctx)


for _m in (0, 1):
    _tg_dev("path_summary_m%d" % _m, "abc_rank_targets_path_summary_dev", PROD_B, functools.partial(_path_summary, _m, PS_KS, FIT), _SORT)
_tg_dev("path_summary_m1_hcorr", "abc_rank_targets_path_summary_dev", PROD_B, functools.partial(_path_summary, 1, PS_KS, FIT), _SORT,
        dict(hcorr=True))
# sm_batch floors: the smaller tolerance sorts 2 targets a batch (246 MB), K_max 1 (154 MB); tg_need takes the maximum over the tolerances.
# (At P = 16 the same holds for Ks = (300000, 500000), but abc_ws_need's term for K = 500000 is then 0.8 GB and the sort buffers are
# 0.18 of the reservation; with 64 parameters the tolerances are smaller and the buffers more than half of it.)
BIG_KS = (80000, 100000)
assert sort_bytes(3, BIG_KS[0], BIG["P"]) > sort_bytes(3, BIG_KS[1], BIG["P"])
_tg_dev("path_summary_m0_row_weights_big", "abc_rank_targets_path_summary_dev", 3, functools.partial(_path_summary, 0, BIG_KS, BIG),
        [blk("sort buffers of the smaller tolerance", ("sort", BIG_KS[0]), BIG["N"], BIG["P"], BIG["A"], 3),
         blk("candidate segments", ("cand", BIG_KS[1]), BIG["N"], BIG["P"], BIG["A"], 3)], dict(row_weights=True), fit=BIG)


# ---- the targets family, host entries: every output member staged -------------------------------------------------------------------
HOST_K = 2000
HOST_B = 256          # the staged theta B K P x 8 = 65 MB (at B = 64 it is a quarter of the reservation or just below)


def _tg_host(name, entry, B, call, blocks, settings=None):
    _add(name, entry, "block", functools.partial(targets_host, FIT, B), targets_shapes(FIT, B), lambda ctx, prep, h: call(ctx, h), blocks,
         settings, A=FIT["A"])


def _host_plain(ctx, h):
    from abcsmc_amd import abcutil
    return abcutil.particle_ranking_PLS_targets(h["X"], h["Y"], h["targets"], 0.5, HOST_K, exclude=h["exclude"], max_comp=FIT["A"],
                                                rule=_lib.RULE_MIN_PRESS, details=True, ctx=ctx)


_tg_host("host_rank_plain", "abc_particle_ranking_pls_targets", 2000, _host_plain,
         [_fblk("candidate segments", ("cand", HOST_K), 2000), _fblk("staged idx and dist", ("BK", HOST_K, 2), 2000)])


def _host_adjust(ctx, h):
    from abcsmc_amd import abcutil
    return abcutil.particle_ranking_PLS_targets_adjust(h["X"], h["Y"], h["targets"], 0.5, HOST_K, exclude=h["exclude"], max_comp=FIT["A"],
                                                       rule=_lib.RULE_MIN_PRESS, ctx=ctx)


_HOST_THETA = [_fblk("staged theta", ("BKP", HOST_K), HOST_B), _fblk("candidate segments", ("cand", HOST_K), HOST_B)]
_tg_host("host_adjust", "abc_particle_ranking_pls_targets_adjust", HOST_B, _host_adjust, _HOST_THETA)
_tg_host("host_adjust_hcorr", "abc_particle_ranking_pls_targets_adjust", HOST_B, _host_adjust, _HOST_THETA, dict(hcorr=True))
_tg_host("host_adjust_ridge", "abc_particle_ranking_pls_targets_adjust", HOST_B, _host_adjust, _HOST_THETA, dict(ridge=RIDGE))


def _host_path(ctx, h):
    from abcsmc_amd import abcutil
    return abcutil.particle_ranking_PLS_targets_path(h["X"], h["Y"], h["targets"], 0.5, PATH_KS, exclude=h["exclude"], max_comp=FIT["A"],
                                                     rule=_lib.RULE_MIN_PRESS, ctx=ctx)


_tg_host("host_path", "abc_particle_ranking_pls_targets_path", 256, _host_path, _PATH_BLOCKS)


def _host_path_summary(method, ctx, h):
    from abcsmc_amd import abcutil
    return abcutil.particle_ranking_PLS_targets_path_summary(h["X"], h["Y"], h["targets"], 0.5, PS_KS, probs=PROBS, truth=h["truth"],
                                                             method=("rejection", "loclinear")[method], exclude=h["exclude"],
                                                             max_comp=FIT["A"], rule=_lib.RULE_MIN_PRESS, ctx=ctx)


for _m in (0, 1):
    _tg_host("host_path_summary_m%d" % _m, "abc_particle_ranking_pls_targets_path_summary", PROD_B,
             functools.partial(_host_path_summary, _m), _SORT)


def _host_product(product, method, ctx, h):
    """abc_particle_ranking_pls_targets_<product> with every member of the descriptor and, under method 1, of abc_adjust_out"""
    from abcsmc_amd import abcutil, entropy, hpd
    lib = _lib.lib()
    B, K, P, A = HOST_B, HOST_K, FIT["P"], FIT["A"]
    make = dict(summary=lambda: abcutil._summary_arg(PROBS, h["truth"], (B,), P),
                hpd=lambda: hpd._hpd_arg(HPD_MASS, (B,), P),
                density=lambda: abcutil._density_arg(512, 3.0, 1.0, None, (B,), P),
                joint=lambda: abcutil._joint_arg(33, 3.0, 1.0, None, ((0, 1), (2, 5), (3, 15)), (B,), P, True),
                draws=lambda: abcutil._draws_arg(500, True, 5, None, 1.0, None, (B,), P),
                entropy=lambda: entropy._entropy_arg(4, None, (B,), K, P))[product]
    d, o, _keep = make()
    X, Y, T, N, M, _, _, _, ex = abcutil._targets_args(h["X"], h["Y"], h["targets"], 0.5, K, h["exclude"])
    o.update(idx=np.empty((B, K), dtype=np.uint64), dist=np.empty((B, K)))
    adj = None
    if method == 1:
        o.update(theta=np.empty((B, K, P)), weight=np.empty((B, K)), coef=np.empty((B, A + 1, P)), rank=np.empty(B, dtype=np.int32),
                 status=np.empty(B, dtype=np.int32))
        adj = _lib.AdjustOut(*(o[k].ctypes.data for k in ADJ_MEMBERS))
    ncomp = C.c_int32(0)
    kernel = _lib.KERNEL_RECTANGULAR if product == "entropy" else _lib.KERNEL_EPANECHNIKOV
    p = abcutil._p
    ctx.check(getattr(lib, "abc_particle_ranking_pls_targets_" + product)(
        ctx.handle, p(X), p(Y), N, M, P, p(T), B, 0.5, A, _lib.RULE_MIN_PRESS, p(ex), K, method, kernel, p(o["idx"]), p(o["dist"]),
        C.byref(adj) if adj is not None else None, C.byref(d), C.addressof(ncomp)))
    o["ncomp"] = ncomp.value
    o.pop("probs", None)
    o.pop("pairs", None)
    return o


for _p in ("summary", "hpd", "density", "joint", "draws", "entropy"):
    _tg_host("host_%s_m1" % _p, "abc_particle_ranking_pls_targets_" + _p, HOST_B, functools.partial(_host_product, _p, 1), _HOST_THETA)
_tg_host("host_summary_m1_transf", "abc_particle_ranking_pls_targets_summary", HOST_B, functools.partial(_host_product, "summary", 1),
         _HOST_THETA, dict(transf=True))
_tg_host("host_summary_m1_row_weights", "abc_particle_ranking_pls_targets_summary", HOST_B, functools.partial(_host_product, "summary", 1),
         _HOST_THETA, dict(row_weights=True))


# ---- parameter transforms and Box-Cox ---------------------------------------------------------------------------------------------
TF_N, TF_P = 100000, 16


def _tf_host():
    rng = np.random.default_rng(31)
    V = np.asfortranarray(rng.uniform(0.01, 0.99, size=(TF_N, TF_P)))
    kinds = tuple(("none", "log", "logit")[j % 3] for j in range(TF_P))
    return dict(V=V, tf=(kinds, np.zeros(TF_P), np.ones(TF_P)))


def _tf_dev(inverse, ctx, prep, h):
    from abcsmc_amd import device
    d = _dev(("tf",), lambda: device.colmajor(h["V"], "cuda:0"))
    return dict(out=device.param_transf(d, inverse=inverse, ctx=ctx))


def _tf_hostcall(ctx, prep, h):
    out = np.empty((TF_N, TF_P), order="F")
    ctx.check(_lib.lib().abc_param_transf(ctx.handle, h["V"].ctypes.data, TF_N, TF_P, 0, out.ctypes.data))
    return dict(out=out)


_add("param_transf_dev", "abc_param_transf_dev", "sharp", _tf_host, dict(V=(TF_N, TF_P)), functools.partial(_tf_dev, False), [],
     dict(transf=True))
_add("param_transf_host", "abc_param_transf", "sharp", _tf_host, dict(V=(TF_N, TF_P)), _tf_hostcall,
     [("staged values", TF_N * TF_P * 8)], dict(transf=True))

BC_N, BC_M = 100000, 8


def _bc_host():
    rng = np.random.default_rng(41)
    X = np.asfortranarray(rng.lognormal(0.0, 0.7, size=(BC_N, BC_M)) * (1.0 + np.arange(BC_M)))
    return dict(X=X, lam=np.linspace(-1.0, 1.0, BC_M), shift=np.full(BC_M, 0.5))


_BC_L = 100                                                        # the reference's grid: 100 values
_BC_CHUNKS = [("chunk partial sums", BC_M * 3 * _BC_L * 8)]        # x the row chunks of the search (boxcox.hip: bc_chunks)


def _bc_search_dev(ctx, prep, h):
    from abcsmc_amd import device
    d = _dev(("bc",), lambda: device.colmajor(h["X"], "cuda:0"))
    r = device.optimize_box_cox(d, shift=h["shift"], skew=True, ctx=ctx)
    r.pop("grid")
    return r


def _bc_apply_dev(ctx, prep, h):
    from abcsmc_amd import device
    d = _dev(("bc",), lambda: device.colmajor(h["X"], "cuda:0"))
    return dict(out=device.box_cox(d, h["lam"], h["shift"], ctx=ctx))


_BC_SHAPES = dict(X=(BC_N, BC_M), lam=(BC_M,), shift=(BC_M,))
_add("box_cox_search_dev", "abc_optimize_box_cox_dev", "sharp", _bc_host, _BC_SHAPES, _bc_search_dev, _BC_CHUNKS)
_add("box_cox_search_host", "abc_optimize_box_cox", "sharp", _bc_host, _BC_SHAPES,
     lambda ctx, prep, h: ctx.optimize_box_cox(h["X"], _lib.box_cox_grid(), h["shift"], skew=True),
     _BC_CHUNKS + [("staged table", BC_N * BC_M * 8)])
_add("box_cox_apply_dev", "abc_box_cox_dev", "sharp", _bc_host, _BC_SHAPES, _bc_apply_dev, [])
_add("box_cox_apply_host", "abc_box_cox", "sharp", _bc_host, _BC_SHAPES,
     lambda ctx, prep, h: dict(out=ctx.box_cox(h["X"], h["lam"], h["shift"])), [("staged table", BC_N * BC_M * 8)])


# ---- generation, reference-signature host functions, stage entries: the shapes of tests/test_gpu_parity.py ------------------------
def _gen_host(N, M, P, Kp):
    wl, X, Y = _table(N, M, P, 12345)
    th, w, dv = wl.previous_set(Kp) if Kp else (None, None, None)
    return dict(X=X, Y=Y, obs=wl.observed(), theta_prev=th, w_prev=w, dv_prev=dv)


def _gen_shapes(N, M, P, Kp):
    s = dict(X=(N, M), Y=(N, P), obs=(M,))
    if Kp:
        s.update(theta_prev=(Kp, P), w_prev=(Kp,), dv_prev=(P,))
    return s


def _generation(N, M, P, K, Kp, Nn, A, multivariate, rule, ctx, prep, h):
    from abcsmc_amd import abcutil, device
    wl = _table(N, M, P, 12345)[0]
    dev = "cuda:0"
    key = ("gen", N, M, P, Kp)
    d = _dev(key, lambda: dict(X=device.colmajor(h["X"], dev), Y=device.colmajor(h["Y"], dev), obs=device.colmajor(h["obs"], dev),
                               priors=device.priors_to_device(_lib.make_priors(wl.prior_spec()), dev),
                               prev=tuple(device.colmajor(h[k], dev) for k in ("theta_prev", "w_prev", "dv_prev")) if Kp else ()))
    gen = device.Generation(N, M, P, K, Kp, Nn, 0.5, A, rule=rule, multivariate=multivariate, device=dev, ctx=ctx)
    r = abcutil.rng(67890)
    gen.run(d["X"], d["Y"], d["obs"], d["priors"], r, *d["prev"])
    out = dict(idx=gen.idx, dist=gen.dist, theta=gen.theta, w=gen.w, dv=gen.dv, next=gen.next, parent=gen.parent, seeds=gen.seeds,
               ncomp=gen.ncomp.value, rng=(r.s1, r.s2, r.s3))
    if multivariate:
        out["L"] = gen.L
    return out


for _n, _a in (("mvn", (20000, 32, 16, 2000, 2000, 20000, 8, True, 1)), ("independent", (20000, 32, 16, 2000, 2000, 20000, 8, False, 0)),
               ("first_set", (20000, 32, 16, 2000, 0, 20000, 8, True, 1)),
               ("k20000", (60000, 8, 6, 20000, 20000, 30000, 4, True, 1))):      # K >= 20000: the device alias build
    _add("generation_" + _n, "abc_generation_dev", "stage", functools.partial(_gen_host, _a[0], _a[1], _a[2], _a[4]),
         _gen_shapes(_a[0], _a[1], _a[2], _a[4]), functools.partial(_generation, *_a), kde=bool(_a[4]))

PAR = dict(N=20000, M=32, P=16, A=8, K=2000, Kp=2000, n=20000)


def _par_host():
    wl, X, Y = _table(PAR["N"], PAR["M"], PAR["P"], 12345)
    th, w, dv = wl.previous_set(PAR["Kp"])
    rng = np.random.default_rng(9)
    theta = np.asfortranarray(wl.mu_y + 0.45 * (Y[:PAR["K"]] - wl.mu_y))
    wk = rng.random(PAR["K"]) ** 3
    wk[3] = 0.0
    wbig = rng.random(30000) ** 3                                   # >= 20000 weights: the device alias build
    wbig[5] = 0.0
    dist = rng.chisquare(8, size=200000)
    return dict(X=X, Y=Y, obs=wl.observed(), theta_prev=th, w_prev=w, dv_prev=dv, theta=theta, w=wk, w_big=wbig, dist=dist)


_PAR_SHAPES = dict(X=(20000, 32), Y=(20000, 16), obs=(32,), theta_prev=(2000, 16), w_prev=(2000,), dv_prev=(16,), theta=(2000, 16),
                   w=(2000,), w_big=(30000,), dist=(200000,))


def _priors():
    return _lib.make_priors(_table(PAR["N"], PAR["M"], PAR["P"], 12345)[0].prior_spec())


def _stage(name, entry, call, kde=False):
    _add(name, entry, "stage", _par_host, _PAR_SHAPES, call, kde=kde)


def _ranking_pls(rule, ctx, prep, h):
    from abcsmc_amd import abcutil
    return abcutil.particle_ranking_PLS(h["X"], h["Y"], h["obs"], 0.5, K=PAR["K"], max_comp=PAR["A"], rule=rule, details=True, ctx=ctx)


_stage("ranking_pls_min_press", "abc_particle_ranking_pls", functools.partial(_ranking_pls, 0))
_stage("ranking_pls_wilcoxon", "abc_particle_ranking_pls", functools.partial(_ranking_pls, 1))


def _au(fn):
    """a function of abcutil by name, with the context as keyword"""
    def call(ctx, *a, **kw):
        from abcsmc_amd import abcutil
        return getattr(abcutil, fn)(*a, ctx=ctx, **kw)
    return call


_stage("ranking_simple", "abc_particle_ranking_simple",
       lambda ctx, prep, h: _au("particle_ranking_simple")(ctx, h["X"], None, h["obs"], K=PAR["K"], details=True))
_stage("doubled_variance_host", "abc_calculate_doubled_variance",
       lambda ctx, prep, h: dict(dv=_au("calculate_doubled_variance")(ctx, h["theta"])))
_stage("weight_uniform", "abc_weight_predictive_prior_uniform",
       lambda ctx, prep, h: dict(w=_au("weight_predictive_prior")(ctx, _priors(), h["theta"])))
_stage("weight_host", "abc_weight_predictive_prior",
       lambda ctx, prep, h: dict(w=_au("weight_predictive_prior")(ctx, _priors(), h["theta"], h["theta_prev"], h["w_prev"], h["dv_prev"])),
       kde=True)
_stage("mvn_host", "abc_setup_mvn_sampler", lambda ctx, prep, h: dict(L=_au("setup_mvn_sampler")(ctx, h["theta"])))


def _sample_posterior(key, ctx, prep, h):
    from abcsmc_amd import abcutil
    r = abcutil.rng(3)
    return dict(idx=abcutil.gsl_rng_nonuniform_int(r, PAR["n"], h[key], ctx=ctx), rng=(r.s1, r.s2, r.s3))


_stage("sample_posterior", "abc_sample_posterior", functools.partial(_sample_posterior, "w"))
_stage("sample_posterior_k30000", "abc_sample_posterior", functools.partial(_sample_posterior, "w_big"))


def _sample_priors(multivariate, ctx, prep, h):
    from abcsmc_amd import abcutil
    r = abcutil.rng(4)
    if multivariate:
        L = _dev(("par_L",), lambda: abcutil.setup_mvn_sampler(h["theta"], ctx=prep))
        out, parent, seeds = abcutil.sample_mvn_predictive_priors(r, PAR["n"], h["w"], h["theta"], _priors(), L, seeds=True, ctx=ctx)
    else:
        dv = 2.0 * h["theta"].var(axis=0, ddof=1)
        out, parent, seeds = abcutil.sample_predictive_priors(r, PAR["n"], h["w"], h["theta"], _priors(), dv, seeds=True, ctx=ctx)
    return dict(out=out, parent=parent, seeds=seeds, rng=(r.s1, r.s2, r.s3))


_stage("sample_mvn_priors", "abc_sample_mvn_predictive_priors", functools.partial(_sample_priors, True))
_stage("sample_priors", "abc_sample_predictive_priors", functools.partial(_sample_priors, False))


def _alias_table(ctx, prep, h):
    F, A, on = ctx.alias_table(h["w_big"])
    return dict(F=F, A=A, on_device=on)


_stage("alias_table_k30000", "abc_alias_table", _alias_table)


def _par_dev(prep):
    """the stage rows' inputs on the device, and what earlier stages make of them (on prep)"""
    def make():
        import torch
        from abcsmc_amd import device, sharded
        h = _par_host()
        N, M, P, A, K = PAR["N"], PAR["M"], PAR["P"], PAR["A"], PAR["K"]
        dev = "cuda:0"
        be = sharded.HipBackend(dev, prep)
        d = dict(X=device.colmajor(h["X"], dev), Y=device.colmajor(h["Y"], dev), obs=device.colmajor(h["obs"], dev),
                 priors=device.priors_to_device(_priors(), dev), theta=device.colmajor(h["theta"], dev),
                 theta_prev=device.colmajor(h["theta_prev"], dev), w_prev=device.colmajor(h["w_prev"], dev),
                 dv_prev=device.colmajor(h["dv_prev"], dev), w=device.colmajor(h["w"], dev), w_big=device.colmajor(h["w_big"], dev),
                 dist=device.colmajor(h["dist"], dev))
        d["shift"] = be.zeros(be.stats_len(M, P))
        be.stats_shift(d["X"], d["Y"], d["shift"])
        d["stats"] = d["shift"].clone()
        be.stats_accumulate(d["X"], d["Y"], 0, N // 2, d["stats"])
        d["model"] = be.zeros(be.model_len(M, P, A))
        be.pls_model(d["stats"], d["obs"], M, P, A, _lib.RULE_MIN_PRESS, d["model"])
        d["proj"] = be.empty(N)
        be.project_distance(d["X"], P, A, d["model"], d["proj"])
        d["idx"], d["seld"] = be.empty(K, torch.int64), be.empty(K)
        be.select_smallest(d["proj"], K, 0, d["idx"], d["seld"])
        d["L"] = be.empty((P, P))
        be.setup_mvn(d["theta"], d["L"])
        d["parent"] = be.empty(PAR["n"], torch.int64)
        be.resample(_rng(5), d["w"], 0, PAR["n"], d["parent"])
        # the distributed selection's state before every pass (its histograms "all-reduced" over the one shard), and after the last
        st, hist = be.zeros(8, torch.int64), be.zeros(2048, torch.int32)
        be.select_begin(K, st, hist)
        d["sel_states"], d["sel_hists"] = [], []
        for p in range(6):
            d["sel_states"].append(st.clone())
            be.select_hist(d["dist"], st, p, hist)
            d["sel_hists"].append(hist.clone())
            be.select_pick(st, p, hist, K)
        d["sel_final"] = st.clone()
        cnt = be.zeros(2, torch.int64)
        be.select_count(d["dist"], st, cnt)
        prep.synchronize()
        torch.cuda.synchronize()
        d["sel_counts"] = cnt.cpu().tolist()
        return d
    return _dev(("par",), make)


def _rng(seed):
    from abcsmc_amd import abcutil
    return abcutil.rng(seed)


def _be(ctx):
    from abcsmc_amd import sharded
    return sharded.HipBackend("cuda:0", ctx)


def _s_stats_shift(ctx, prep, h):
    d, be = _par_dev(prep), _be(ctx)
    out = be.zeros(be.stats_len(PAR["M"], PAR["P"]))
    be.stats_shift(d["X"], d["Y"], out)
    return dict(stats=out)


def _s_stats_accumulate(ctx, prep, h):
    d, be = _par_dev(prep), _be(ctx)
    out = d["shift"].clone()
    be.stats_accumulate(d["X"], d["Y"], 0, PAR["N"] // 2, out)
    return dict(stats=out)


def _s_pls_model(ctx, prep, h):
    d, be = _par_dev(prep), _be(ctx)
    out = be.zeros(be.model_len(PAR["M"], PAR["P"], PAR["A"]))
    be.pls_model(d["stats"], d["obs"], PAR["M"], PAR["P"], PAR["A"], _lib.RULE_MIN_PRESS, out)
    return dict(model=out)


def _s_wilcoxon(ctx, prep, h):
    d, be = _par_dev(prep), _be(ctx)
    N, M, P, A = PAR["N"], PAR["M"], PAR["P"], PAR["A"]
    out = d["model"].clone()
    ctx.check(_lib.lib().abc_pls_wilcoxon_dev(be._s(), d["X"].data_ptr(), d["Y"].data_ptr(), N, N, N, M, P, A, N // 2, out.data_ptr()))
    return dict(model=out)


def _s_simple_model(ctx, prep, h):
    d, be = _par_dev(prep), _be(ctx)
    out = be.zeros(be.model_len(PAR["M"], PAR["P"], 1))
    ctx.check(_lib.lib().abc_simple_model_dev(be._s(), d["stats"].data_ptr(), d["obs"].data_ptr(), PAR["M"], PAR["P"], out.data_ptr()))
    return dict(model=out)


def _s_project(ctx, prep, h):
    d, be = _par_dev(prep), _be(ctx)
    out = be.empty(PAR["N"])
    be.project_distance(d["X"], PAR["P"], PAR["A"], d["model"], out)
    return dict(dist=out)


def _s_select(key, K, ctx, prep, h):
    import torch
    d, be = _par_dev(prep), _be(ctx)
    idx, dist = be.empty(K, torch.int64), be.empty(K)
    be.select_smallest(d[key], K, 0, idx, dist)
    return dict(idx=idx, dist=dist)


def _s_select_begin(ctx, prep, h):
    import torch
    be = _be(ctx)
    st, hist = be.zeros(8, torch.int64), be.empty(2048, torch.int32)      # (begin writes the words of the state it uses)
    be.select_begin(PAR["K"], st, hist)
    return dict(state=st, hist=hist)


def _s_select_hist(ctx, prep, h):
    d, be = _par_dev(prep), _be(ctx)
    hist = d["sel_hists"][2].clone().zero_()
    be.select_hist(d["dist"], d["sel_states"][3], 3, hist)
    return dict(hist=hist)


def _s_select_pick(ctx, prep, h):
    d, be = _par_dev(prep), _be(ctx)
    st, hist = d["sel_states"][3].clone(), d["sel_hists"][3].clone()
    be.select_pick(st, 3, hist, PAR["K"])
    return dict(state=st, hist=hist)


def _s_select_count(ctx, prep, h):
    import torch
    d, be = _par_dev(prep), _be(ctx)
    cnt = be.zeros(2, torch.int64)
    be.select_count(d["dist"], d["sel_final"], cnt)
    return dict(counts=cnt)


def _s_select_compact(ctx, prep, h):
    import torch
    d, be = _par_dev(prep), _be(ctx)
    less, eq = d["sel_counts"]
    take = min(eq, PAR["K"] - less)
    idx, dist = be.empty(less + take, torch.int64), be.empty(less + take)
    be.select_compact(d["dist"], d["sel_final"], less, take, 1000, idx, dist)
    return dict(idx=idx, dist=dist)


def _s_sort_pairs(ctx, prep, h):
    import torch
    d, be = _par_dev(prep), _be(ctx)
    key = d["dist"].clone()
    idx = torch.arange(key.numel(), dtype=torch.int64, device=key.device)
    be.sort_pairs(key, idx)
    return dict(key=key, idx=idx)


def _s_merge(ctx, prep, h):
    import torch
    d, be = _par_dev(prep), _be(ctx)
    W, n = 4, 5000
    key, _ = torch.sort(d["dist"][:W * n].reshape(W, n), dim=1)
    key = key.reshape(-1).contiguous()
    idx = torch.arange(W * n, dtype=torch.int64, device=key.device)
    ok, oi = be.empty(W * n), be.empty(W * n, torch.int64)
    be.merge_runs(key, idx, W, n, ok, oi)
    return dict(key=ok, idx=oi)


def _s_gather(ctx, prep, h):
    d, be = _par_dev(prep), _be(ctx)
    out = be.zeros((PAR["P"], PAR["K"]))
    be.gather_rows(d["Y"], d["idx"], 0, out)
    return dict(theta=out)


def _s_dv(ctx, prep, h):
    d, be = _par_dev(prep), _be(ctx)
    out = be.empty(PAR["P"])
    be.doubled_variance(d["theta"], out)
    return dict(dv=out)


def _s_weights_raw(ctx, prep, h):
    d, be = _par_dev(prep), _be(ctx)
    out = be.empty(PAR["K"])
    be.weights_raw(d["priors"], d["theta"], 0, PAR["K"], d["theta_prev"], d["w_prev"], d["dv_prev"], out)
    return dict(w=out)


def _s_normalize(ctx, prep, h):
    d, be = _par_dev(prep), _be(ctx)
    out = d["w"].clone()
    be.normalize_l2(out)
    return dict(w=out)


def _s_mvn(ctx, prep, h):
    d, be = _par_dev(prep), _be(ctx)
    out = be.empty((PAR["P"], PAR["P"]))
    be.setup_mvn(d["theta"], out)
    return dict(L=out)


def _s_resample(key, ctx, prep, h):
    import torch
    d, be = _par_dev(prep), _be(ctx)
    out = be.empty(PAR["n"], torch.int64)
    be.resample(_rng(5), d[key], 7, PAR["n"], out)
    return dict(parent=out)


def _s_perturb(multivariate, ctx, prep, h):
    import torch
    d, be = _par_dev(prep), _be(ctx)
    n = PAR["n"]
    out, seeds = be.empty((PAR["P"], n)), be.empty(n, torch.int64)
    be.perturb(_rng(5), d["theta"], d["priors"], d["parent"], 0, n, multivariate, d["L"] if multivariate else d["dv_prev"], out, seeds, n)
    return dict(out=out, seeds=seeds)


_stage("stats_shift", "abc_stats_shift_dev", _s_stats_shift)
_stage("stats_accumulate", "abc_stats_accumulate_dev", _s_stats_accumulate)
_stage("pls_model", "abc_pls_model_dev", _s_pls_model)
_stage("pls_wilcoxon", "abc_pls_wilcoxon_dev", _s_wilcoxon)
_stage("simple_model", "abc_simple_model_dev", _s_simple_model)
_stage("project_distance", "abc_project_distance_dev", _s_project)
_stage("select_smallest", "abc_select_smallest_dev", functools.partial(_s_select, "proj", PAR["K"]))
_stage("select_smallest_bins", "abc_select_smallest_dev", functools.partial(_s_select, "dist", 20000))      # the sampled-range bins
_stage("select_begin", "abc_select_begin_dev", _s_select_begin)
_stage("select_hist", "abc_select_hist_dev", _s_select_hist)
_stage("select_pick", "abc_select_pick_dev", _s_select_pick)
_stage("select_count", "abc_select_count_dev", _s_select_count)
_stage("select_compact", "abc_select_compact_dev", _s_select_compact)
_stage("sort_pairs", "abc_sort_pairs_dev", _s_sort_pairs)
_stage("merge_sorted_runs", "abc_merge_sorted_runs_dev", _s_merge)
_stage("gather_rows", "abc_gather_rows_dev", _s_gather)
_stage("doubled_variance", "abc_doubled_variance_dev", _s_dv)
_stage("weights_raw", "abc_weights_raw_dev", _s_weights_raw, kde=True)
_stage("normalize_l2", "abc_normalize_l2_dev", _s_normalize)
_stage("mvn_sampler", "abc_setup_mvn_sampler_dev", _s_mvn)
_stage("resample", "abc_resample_dev", functools.partial(_s_resample, "w"))
_stage("resample_k30000", "abc_resample_dev", functools.partial(_s_resample, "w_big"))
_stage("perturb_mvn", "abc_perturb_dev", functools.partial(_s_perturb, True))
_stage("perturb_independent", "abc_perturb_dev", functools.partial(_s_perturb, False))
