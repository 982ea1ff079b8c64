"""The tolerance path's refits are the adjust call's fit chain (aj_fit_chain of adjust.hip), with every fit setting on at once: row
importance weights with zeros among them, log / logit parameter transforms, ridge with three penalties including 0 and the
variance correction.  Slot (b, t) of the path's hcoef, pick and press records, and of its coef, has the bits of
rank_targets_adjust with K = K_t under the same settings.

The settings live in the context the whole suite shares, so every call is made inside their context managers, which restore what
was there before."""
import numpy as np
import pytest

from test_gpu_adjust import _with_nc
from test_gpu_hcorr import _fit, _np, _same, hetero_data

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L3 = (0.0, 1e-1, 10.0)

# (N, M, P, A, comps, B, Ks).  The first: K = 1000 has 4 chunks of 250 rows and K = 257 on its own 2 of 129, so the refit's plan
# is not the path's.  The second: nc = A = 12 (set in the model header) and 80 parameters give 93 x 4 > 256 entry groups, the
# path's wide branch (k_adj_moments once per tolerance) and the second-stage kernel's branch past 256 groups.
SHAPES = [(3000, 6, 3, 3, 0, 5, (64, 257, 1000)), (1500, 16, 80, 12, 12, 3, (64, 300))]


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


_SETUPS = {}


def _setup(ctx, shape):
    """data, fit, targets, transforms and row weights of a shape, made once and shared (read only)"""
    if shape not in _SETUPS:
        N, M, P, A, comps, B, Ks = shape
        X, Y = hetero_data(N, M, P, 17 * N + P)
        lo, hi = Y.min(axis=0), Y.max(axis=0)
        Y = np.ascontiguousarray(0.1 + 0.8 * (Y - lo) / (hi - lo))      # every column in [0.1, 0.9]: inside every kind's domain
        F = _fit(ctx, X, Y, A)
        nc = comps if comps else F["ncomp"]
        model = _with_nc(F, nc) if comps else F["model"]
        kinds = [("logit", "none", "log")[j % 3] for j in range(P)]
        tf = (kinds, np.full(P, 0.05), np.full(P, 1.0))
        rng = np.random.default_rng(N + M)
        om = rng.uniform(0.1, 2.0, N)
        om[rng.uniform(size=N) < 0.05] = 0.0                             # positive with a few zeros
        assert 0 < (om == 0.0).sum() < N // 10
        _SETUPS[shape] = (F, model, nc, np.arange(B) * 11, tf, om)
    return _SETUPS[shape]


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=["chunks", "wide"])
def test_path_slots_are_the_adjust_call_with_every_setting_on(ctx, shape, kernel):
    import torch
    from abcsmc_amd import device
    N, M, P, A, comps, B, Ks = shape
    F, model, nc, rows, (kinds, lo, hi), om = _setup(ctx, shape)
    T, L = len(Ks), len(L3)
    Td, ex = device.colmajor(F["X"][rows], DEV), torch.tensor(rows)
    args = (F["Xd"], model, A, Td)
    ctx.adjust_hcorr_skipped(reset=True)
    ctx.adjust_ridge_unscored(reset=True)
    with ctx.row_weights(om), ctx.param_transf(kinds, lo, hi), ctx.adjust_ridge(L3), ctx.adjust_hcorr(True):
        g = _np(device.rank_targets_path(*args, Ks, F["Yd"], exclude=ex, kernel=kernel, ctx=ctx))
        hcoef = ctx.last_hcorr().reshape(B, T, A + 1, P)
        pick, press = ctx.last_ridge()
        pick, press = pick.reshape(B, T, P), press.reshape(B, T, L, P)
        # the zero weights leave every target enough rows at the smallest tolerance
        kept = (om[g["idx"][:, :Ks[0]].astype(np.int64)] > 0.0).sum(axis=1)
        assert kept.min() >= nc + 2, kept
        adj = []
        for K in Ks:
            a = _np(device.rank_targets_adjust(*args, K, F["Yd"], exclude=ex, kernel=kernel, theta=False, weight=False, ctx=ctx))
            a["hcoef"] = ctx.last_hcorr()
            a["pick"], a["press"] = ctx.last_ridge()
            adj.append(a)
    assert ctx.adjust_hcorr_skipped() == 0 and ctx.adjust_ridge_unscored() == 0      # not an equality of two empty records
    assert np.all(np.isfinite(hcoef)) and np.all(np.isfinite(g["coef"]))
    for t, K in enumerate(Ks):
        a = adj[t]
        assert a["hcoef"].shape == (B, A + 1, P) and a["pick"].shape == (B, P) and a["press"].shape == (B, L, P)
        assert _same(g["idx"][:, :K], a["idx"]) and _same(g["dist"][:, :K], a["dist"]), (kernel, K)
        for name, slot in (("hcoef", hcoef[:, t]), ("pick", pick[:, t]), ("press", press[:, t]), ("coef", g["coef"][:, t])):
            assert _same(slot, a[name]), (name, kernel, K, np.abs(slot - a[name]).max())
