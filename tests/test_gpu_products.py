"""The three posterior products (abc_summary, abc_density, abc_joint) through each of their four entry points (targets-host,
targets-dev, weighted-host, weighted-dev), straight through ctypes because the Python wrappers always pass every member: every
output member alone gives the bytes it has in the full request (what a shared stage / download / byte count gets wrong first), the
first call on a fresh context has reserved enough on its own, and every entry names itself when its descriptor is NULL.

Shapes of test_argument_errors in test_gpu_density.py: N = 800, M = 5, P = 3, A = 3, B = 4, K = 50; G = 16 grid points, all three
pairs for the joint, nq = 3 levels.  The values are continuous, so no output is NaN and np.array_equal compares bits."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, M, P, A, B, K, G, NQ = 800, 5, 3, 3, 4, 50, 16, 3
NPAIRS = P * (P - 1) // 2
PROBS = np.array([0.1, 0.5, 0.9])
INVALID = -1                             # ABC_ERR_INVALID; Context.check raises on every status but ABC_OK (0)
PRODUCTS = ("summary", "density", "joint")
ENTRIES = {"targets_host": "abc_particle_ranking_pls_targets_%s", "targets_dev": "abc_rank_targets_%s_dev",
           "weighted_host": "abc_weighted_%s", "weighted_dev": "abc_weighted_%s_dev"}
ARGUMENT = {"summary": "sum", "density": "den", "joint": "jt"}           # the descriptor's name in the header


def _shapes(product, lead):
    """the output members of a product's descriptor and their shapes for prod(lead) targets"""
    if product == "summary":
        return dict(quant=lead + (NQ, P), cdf=lead + (P,))
    marginal = dict(grid=lead + (P, 2), bw_out=lead + (P,))
    if product == "density":
        return dict(dens=lead + (P, G), **marginal, mode=lead + (P,), mode_dens=lead + (P,))
    return dict(mean=lead + (P,), cov=lead + (P, P), corr=lead + (P, P), dens=lead + (NPAIRS, G, G), **marginal,
                mode=lead + (NPAIRS, 2), mode_dens=lead + (NPAIRS,))


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


def _work(ctx):
    """the inputs of every call, in host and in device memory, and the model of the device entries"""
    import torch
    from abcsmc_amd import _lib, device, synthetic
    wl = synthetic.Workload(M, P, 4)
    X, Y = (np.asfortranarray(a) for a in wl.rows(0, N))
    rng = np.random.default_rng(5)
    h = dict(X=X, Y=Y, T=np.asfortranarray(X[:B]), V=np.asfortranarray(rng.normal(size=(K, P))), w=rng.uniform(0.1, 1.0, size=K),
             truth=rng.normal(size=(B, P)))
    d = {k: device.colmajor(v, DEV) for k, v in h.items() if k != "truth"}
    d["truth"] = torch.tensor(h["truth"], device=DEV)
    L = _lib.lib()
    stats = torch.empty(L.abc_stats_len(M, P), dtype=torch.float64, device=DEV)
    d["model"] = torch.empty(L.abc_model_len(M, P, A), dtype=torch.float64, device=DEV)
    obs = torch.zeros(M, dtype=torch.float64, device=DEV)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.check(L.abc_stats_shift_dev(ctx.handle, d["X"].data_ptr(), d["Y"].data_ptr(), N, N, N, M, P, stats.data_ptr()))
    ctx.check(L.abc_stats_accumulate_dev(ctx.handle, d["X"].data_ptr(), d["Y"].data_ptr(), N, N, N, M, P, 0, N // 2,
                                         stats.data_ptr()))
    ctx.check(L.abc_pls_model_dev(ctx.handle, stats.data_ptr(), obs.data_ptr(), M, P, A, 0, d["model"].data_ptr()))
    torch.cuda.synchronize()
    return dict(host=h, dev=d)


@pytest.fixture(scope="module")
def work(ctx):
    return _work(ctx)


def _call(work, ctx, product, entry, members):
    """One call of an entry of a product with exactly `members` of the descriptor's outputs non-NULL (None: a NULL descriptor).
    Every output starts as NaN.  -> (status, {member: numpy array})"""
    import torch
    from abcsmc_amd import _lib
    on_dev = entry.endswith("_dev")
    a = work["dev" if on_dev else "host"]
    p = (lambda t: t.data_ptr()) if on_dev else (lambda v: v.ctypes.data)
    lead = (B,) if entry.startswith("targets") else ()
    desc, out = None, {}
    if members is not None:
        for k in members:
            shape = _shapes(product, lead)[k]
            out[k] = torch.full(shape, np.nan, dtype=torch.float64, device=DEV) if on_dev else np.full(shape, np.nan)
        o = lambda k: p(out[k]) if k in out else None
        if product == "summary":                      # truth is an input: given when the CDF at it is asked for
            truth = a["truth"] if lead else a["truth"][0]
            desc = _lib.Summary(PROBS.ctypes.data, NQ, p(truth) if "cdf" in out else None, o("quant"), o("cdf"))
        elif product == "density":
            desc = _lib.Density(G, 3.0, 1.0, None, o("dens"), o("grid"), o("bw_out"), o("mode"), o("mode_dens"))
        else:
            desc = _lib.Joint(G, 3.0, 1.0, None, None, 0, o("mean"), o("cov"), o("corr"), o("dens"), o("grid"), o("bw_out"),
                              o("mode"), o("mode_dens"))
    ref = C.byref(desc) if desc is not None else None
    fn = getattr(_lib.lib(), ENTRIES[entry] % product)
    if entry == "targets_host":
        rc = fn(ctx.handle, p(a["X"]), p(a["Y"]), N, M, P, p(a["T"]), B, 0.5, A, 0, None, K, 0, 0, None, None, None, ref, None)
    elif entry == "targets_dev":
        rc = fn(ctx.handle, p(a["X"]), N, p(a["Y"]), N, N, M, P, p(a["model"]), A, p(a["T"]), B, B, None, K, 0, 0, None, None, None,
                ref)
    elif entry == "weighted_host":
        rc = fn(ctx.handle, p(a["V"]), K, P, p(a["w"]), ref)
    else:
        rc = fn(ctx.handle, p(a["V"]), K, K, P, p(a["w"]), ref)
    if on_dev:
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in out.items()}
    return rc, out


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("product", PRODUCTS)
def test_every_member_alone(work, ctx, product, entry):
    names = tuple(_shapes(product, ()))
    rc, full = _call(work, ctx, product, entry, names)
    ctx.check(rc)
    for k in names:
        assert np.isfinite(full[k]).all(), k
        rc, one = _call(work, ctx, product, entry, (k,))
        ctx.check(rc)
        assert np.array_equal(one[k], full[k]), k


@pytest.mark.parametrize("product", PRODUCTS)
def test_first_call_on_a_fresh_context(work, ctx, product):
    """each host entry's reservation is sufficient on its own: no earlier call has grown the workspace"""
    from abcsmc_amd import _lib
    names = tuple(_shapes(product, ()))
    for entry in ("targets_host", "weighted_host"):
        rc, warm = _call(work, ctx, product, entry, names)
        ctx.check(rc)
        fresh = _lib.Context(0)
        try:
            rc, first = _call(work, fresh, product, entry, names)
            fresh.check(rc)
        finally:
            fresh.close()
        for k in names:
            assert np.array_equal(first[k], warm[k]), (entry, k)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("product", PRODUCTS)
def test_each_entry_names_itself(work, ctx, product, entry):
    from abcsmc_amd import _lib
    rc, _ = _call(work, ctx, product, entry, None)
    assert rc == INVALID
    name = ENTRIES[entry] % product
    assert _lib.lib().abc_last_error(ctx.handle).decode() == "%s: null argument (%s is required)" % (name, ARGUMENT[product])
