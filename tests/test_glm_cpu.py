"""CPU: the NumPy reference of the ABC-GLM posterior (tests/_glm_ref.py, the header's definition) held to identities that do not
depend on it, the conditioning of the GPU test's inputs, and the accuracy of the estimator against rejection on the synthetic
linear-Gaussian workload (through the reference: no GPU)."""
import numpy as np
import pytest

import _density_ref as D
import _glm_cases as GC
import _glm_ref as R

LD = np.longdouble


def _lin_gauss(K, P, n, seed):
    rng = np.random.default_rng(seed)
    th = rng.normal(size=(K, P)) * rng.uniform(0.5, 2.0, size=P) + rng.normal(size=P)
    x = th @ (rng.normal(size=(P, n)) / np.sqrt(P)) + 0.5 * rng.normal(size=(K, n)) + rng.normal(size=n)
    return th, x, x[0] + 0.1


def _npdf(x, m, v):
    return np.exp(-(x - m) ** 2 / (2 * v)) / np.sqrt(2 * np.pi * v)


def test_hand_worked_three_rows():
    """P = n = 1, K = 3, equal weights, theta = (-1, 0, 1), x = (-1, 1/2, 1), o = 1/2, h = 1/2.  By hand: thbar = 0, xbar = 1/6,
    M_thth = 2/3, M_thx = 2/3, M_xx = 13/18, so C = 1, c0 = 1/6, R = 1/18, n_eff = 3 and Sigma_s = 3 R = 1/6.  Sigma_theta^-1 = 4,
    Q = 6 + 4 = 10, T = 1/10, u = 6 (1/2 - 1/6) = 2, v = (-2, 2, 6), t = (-1/5, 1/5, 3/5),
    log c = -((4, 0, 4) - (4, 4, 36) / 10) / 2 = (-9/5, 1/5, -1/5).  S = 1/6 + 1/4 = 5/12 and the residuals o - c0 - theta are
    (4/3, 1/3, -2/3)."""
    r = R.glm([[-1.0], [0.0], [1.0]], [[-1.0], [0.5], [1.0]], [0.5], bw=[0.5], G=5, cut=2.0)
    assert r["status"] == 0
    tol = dict(rtol=1e-13, atol=1e-15)
    assert np.allclose(r["C"], [[1.0]], **tol) and np.allclose(r["c0"], [1 / 6], **tol)
    assert np.allclose(r["sigma_s"], [[1 / 6]], **tol) and np.allclose(r["T"], [[0.1]], **tol)
    assert np.allclose(r["peaks"][:, 0], [-0.2, 0.2, 0.6], **tol)
    c = np.exp([-1.8, 0.2, -0.2])
    c /= c.sum()
    assert np.allclose(r["c"], c, **tol)
    mean = c @ np.array([-0.2, 0.2, 0.6])
    assert np.allclose(r["mean"], [mean], **tol)
    assert np.allclose(r["var"], [0.1 + c @ (np.array([-0.2, 0.2, 0.6]) - mean) ** 2], **tol)
    assert np.allclose(r["ess"], 1 / (c * c).sum(), **tol)
    lik = _npdf(np.array([4 / 3, 1 / 3, -2 / 3]), 0.0, 5 / 12)
    assert np.allclose(r["log_md"], np.log(lik.mean()), **tol)
    sd = np.sqrt(0.1)
    assert np.allclose(r["lo_x"], [-0.2 - 2 * sd], **tol) and np.allclose(r["step"], [(0.8 + 4 * sd) / 4], **tol)
    xg = r["lo_x"][0] + np.arange(5) * r["step"][0]
    f = sum(c[e] * _npdf(xg, t, 0.1) for e, t in enumerate((-0.2, 0.2, 0.6)))
    assert np.allclose(r["dens"][0], f, **tol)
    assert r["mode"][0] == xg[np.argmax(f)] and np.allclose(r["mode_dens"], [f.max()], **tol)


def paired_design(seed=3, half=24, P=2, n=2):
    """rows in +- pairs about 0 with the same statistics and the same weight, all on a grid of 1/8: M_thx = 0 exactly"""
    rng = np.random.default_rng(seed)
    th = rng.integers(-16, 17, size=(half, P)) / 8.0
    x = rng.integers(-16, 17, size=(half, n)) / 8.0
    w = rng.integers(1, 5, size=half).astype(np.float64)
    return np.concatenate([th, -th]), np.concatenate([x, x]), np.concatenate([w, w])


def test_uncorrelated_design_is_the_kernel_density():
    th, x, w = paired_design()
    o = np.array([0.25, -0.5])
    h = np.array([0.3, 0.45])
    r = R.glm(th, x, o, w, G=65, cut=3.0, bw=h)
    assert r["status"] == 0 and np.abs(r["C"]).max() < 1e-15
    assert np.allclose(r["c"], w / w.sum(), rtol=1e-13) and np.allclose(r["peaks"], th, rtol=1e-13, atol=1e-15)
    assert np.allclose(np.diag(r["T"]), h * h, rtol=1e-13)
    for j in range(2):
        kde = D.density(th[:, j], w, G=65, cut=3.0, bw=h[j])
        assert np.allclose([r["lo_x"][j], r["step"][j]], [kde["lo_x"], kde["step"]], rtol=1e-13)
        assert np.all(np.abs(r["dens"][j] - kde["dens"]) <= 1e-10 * kde["dens"] + 1e-290 * kde["dens"].max())
    # log_md = log N(o; xbar, Sigma_s): with C = 0, S = Sigma_s and every row has the same residual
    xbar = (w[:, None] * x).sum(axis=0) / w.sum()
    d = o - xbar
    Sg = r["sigma_s"]
    ref = -0.5 * (d @ np.linalg.solve(Sg, d)) - 0.5 * (2 * np.log(2 * np.pi) + np.log(np.linalg.det(Sg)))
    assert np.isclose(r["log_md"], ref, rtol=1e-12)


def test_shift_of_the_parameters():
    th, x, o = _lin_gauss(120, 3, 2, 5)
    w = np.random.default_rng(6).uniform(0.2, 1.0, size=120)
    shift = np.array([100.0, -7.5, 0.125])
    a = R.glm(th, x, o, w, G=33)
    b = R.glm(th + shift, x, o, w, G=33)
    assert a["status"] == 0 and b["status"] == 0
    for k in ("mean", "mode", "lo_x"):
        assert np.allclose(b[k], a[k] + shift, rtol=0, atol=1e-11), k
    assert np.allclose(b["peaks"], a["peaks"] + shift, rtol=0, atol=1e-11)
    for k in ("var", "ess", "log_md", "step", "T", "C", "sigma_s", "c"):
        assert np.allclose(b[k], a[k], rtol=1e-10, atol=0), k
    assert np.allclose(b["dens"], a["dens"], rtol=1e-8, atol=1e-300)


def test_density_integrates_to_one():
    th, x, o = _lin_gauss(200, 2, 3, 9)
    r = R.glm(th, x, o, G=2001, cut=9.0)
    for j in range(2):
        f = r["dens"][j]
        area = r["step"][j] * (f.sum() - 0.5 * (f[0] + f[-1]))
        assert abs(area - 1.0) < 1e-9, (j, area)


def _inverse(A):
    """Gauss-Jordan with partial pivoting in the matrix's own dtype"""
    n = A.shape[0]
    W = np.concatenate([np.array(A), np.eye(n, dtype=A.dtype)], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(W[k:, k])))
        W[[k, p]] = W[[p, k]]
        W[k] = W[k] / W[k, k]
        for i in range(n):
            if i != k:
                W[i] = W[i] - W[i, k] * W[k]
    return W[:, n:]


def long_double_chain(th, x, o, w, h):
    """Leuenberger & Wegmann's formulas as they stand, without the shift by thbar and with explicit inverses, in long double:
    T = (C' Sigma_s^-1 C + Sigma_theta^-1)^-1, v_e = C' Sigma_s^-1 (o - c0) + Sigma_theta^-1 theta_e, t_e = T v_e,
    c_e = w_e exp(-(theta_e' Sigma_theta^-1 theta_e - v_e' T v_e) / 2)"""
    th, x, o, w, h = (np.asarray(a, dtype=np.float64).astype(LD) for a in (th, x, o, w, h))
    K, P = th.shape
    n = x.shape[1]
    W = w.sum()
    neff = W * W / (w * w).sum()
    tb, xb = (w[:, None] * th).sum(0) / W, (w[:, None] * x).sum(0) / W
    tc, xc = th - tb, x - xb
    Mtt, Mtx, Mxx = (w[:, None] * tc).T @ tc / W, (w[:, None] * tc).T @ xc / W, (w[:, None] * xc).T @ xc / W
    C = (_inverse(Mtt) @ Mtx).T
    c0 = xb - C @ tb
    Sig = (Mxx - Mtx.T @ _inverse(Mtt) @ Mtx) * (neff / (neff - (P + 1)))
    Si = _inverse(Sig)
    Ti = np.diag(1 / (h * h))
    T = _inverse(C.T @ Si @ C + Ti)
    v = (C.T @ Si @ (o - c0))[None, :] + th @ Ti
    t = v @ T
    logc = np.log(w) - ((th @ Ti * th).sum(1) - (v @ T * v).sum(1)) / 2
    c = np.exp(logc - logc.max())
    c /= c.sum()
    mean = c @ t
    var = np.diag(T) + c @ (t - mean) ** 2
    S = Sig + C @ np.diag(h * h) @ C.T
    r = o - c0 - th @ C.T
    q = (r @ _inverse(S) * r).sum(1)
    Ls, _ = R.chol(S, LD(0))
    logn = np.log(w) - q / 2
    log_md = logn.max() + np.log(np.exp(logn - logn.max()).sum()) - (n * np.log(LD(8) * np.arctan(LD(1))) + 2 * np.log(np.diag(Ls)).sum()) / 2 - np.log(W)
    return dict(C=C, c0=c0, sigma_s=Sig, T=T, peaks=t, c=c, mean=mean, var=var, ess=1 / (c * c).sum(), log_md=log_md)


@pytest.mark.parametrize("K,P,n,seed", [(40, 1, 1, 1), (300, 4, 3, 2), (500, 16, 8, 3)])
def test_against_the_long_double_restatement(K, P, n, seed):
    """float64 against the unshifted long-double chain: relative to each output's largest magnitude, 1e-9 (the bar the device is
    held to against this reference), on inputs whose offsets are of the size of their spread"""
    th, x, o = _lin_gauss(K, P, n, seed)
    w = np.random.default_rng(seed).uniform(0.1, 1.0, size=K)
    r = R.glm(th, x, o, w, G=2)
    ref = long_double_chain(th, x, o, w, r["bw"])
    assert r["status"] == 0
    for k, v in ref.items():
        v = np.asarray(v, dtype=LD)
        err = np.abs(np.asarray(r[k]).astype(LD) - v).max() / np.abs(v).max()
        print(k, float(err))
        assert err < 1e-9, (k, float(err))
    full = R.glm(th, x, o, w, G=2, dtype=LD)
    for k in ref:
        assert np.abs(np.asarray(full[k]) - np.asarray(ref[k], dtype=LD)).max() <= 1e-12 * np.abs(np.asarray(ref[k], dtype=LD)).max(), k


def test_status_bits_of_the_reference():
    th, x, o = _lin_gauss(30, 3, 2, 11)
    dup = th.copy()
    dup[:, 2] = dup[:, 0]
    assert R.glm(dup, x, o, G=2)["status"] == 1
    assert R.glm(th[:4], x[:4], o, G=2)["status"] == 2             # K = P + 1
    bad = th.copy()
    bad[5, 1] = np.nan
    r = R.glm(bad, x, o, G=2)
    assert r["status"] == 4 and np.all(np.isnan(r["mean"])) and np.isnan(r["log_md"])
    w = np.ones(30)
    w[5] = 0.0
    assert R.glm(bad, x, o, w, G=2)["status"] == 0                 # (an uncounted row is not looked at)
    with np.errstate(all="ignore"):
        assert R.glm(th, x, o, np.zeros(30), G=2)["status"] == 2   # (no counted row: n_eff is NaN)


def test_facade_compiles():
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ("#include \"abcsmc_amd/cxx/AbcUtilHip.hpp\"\n"
           "void f() {\n"
           "  ABC::Mat2D X(9, 2), Y(9, 3), T(2, 2);\n"
           "  std::vector<ABC::TargetGlm> r = ABC::particle_ranking_PLS_targets_glm(X, Y, T, 0.5f, 6);\n"
           "  std::vector<ABC::TargetGlm> s = ABC::particle_ranking_PLS_targets_glm(X, Y, T, 0.5f, 6, 64, 2.0, 1.5);\n"
           "  ABC::TargetGlm g = ABC::weighted_glm(Y, X, ABC::Row(2)), h = ABC::weighted_glm(Y, X, ABC::Row(2), std::vector<double>(9, 1.0), 33);\n"
           "  double v = r[0].mean[0] + s[0].dens(1, 2) + g.log_md + h.var[2] + h.status; (void)v;\n"
           "}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", root, "-x", "c++", "-"], input=src, text=True,
                       capture_output=True, cwd=root)
    assert p.returncode == 0, p.stderr


@pytest.mark.parametrize("row", GC.CASES, ids=[c[0] for c in GC.CASES])
def test_gpu_cases_are_well_conditioned(oracle, row):
    """the condition numbers of M_thth and Sigma_s of every target of every GPU case, from the CPU oracle's fit at the case's
    number of components, stay below 1e4; every target is fitted (status 0)"""
    c = GC.case(row)
    X, Y, T, ex, om, bw = GC.inputs(c)
    fit = oracle.particle_ranking_pls(X, Y, T[0], 0.5, max_comp=c["nc"])
    idx, S, O = GC.rank(X, fit["mean"], fit["sd"], fit["R"], c["nc"], T, c["K"], ex)
    worst = 0.0
    for b in range(c["B"]):
        th, xs = Y[idx[b]], S[idx[b]]
        w = np.ones(c["K"]) if om is None else om[idx[b]]
        r = R.glm(th, xs, O[b], w, G=2, bw=None if bw is None else bw[b])
        assert r["status"] == 0, b
        keep = w > 0
        Mtt = np.cov(th[keep].T, aweights=w[keep]).reshape(c["P"], c["P"])
        worst = max(worst, np.linalg.cond(Mtt), np.linalg.cond(r["sigma_s"]))
    print(c["name"], "worst condition number %.1f" % worst)
    assert worst < 1e4


def numpy_posterior(oracle):
    """particle_ranking_PLS_targets_glm's answer from the CPU oracle's fit, a NumPy ranking and the reference"""
    def call(X, Y, T, training_fraction, K, bw_scale=1.0, exclude=None, max_comp=0, rule=0, ctx=None, outputs=()):
        fit = oracle.particle_ranking_pls(X, Y, T[0], training_fraction, max_comp=max_comp, rule=rule)
        nc = fit["ncomp"]
        idx, S, O = GC.rank(X, fit["mean"], fit["sd"], fit["R"], nc, T, K, exclude)
        rs = [R.glm(Y[idx[b]], S[idx[b]], O[b], G=2, bw_scale=bw_scale) for b in range(T.shape[0])]
        out = {k: np.array([r[k] for r in rs]) for k in ("mean", "log_md", "status")}
        out.update(idx=idx, ncomp=nc)
        return out
    return call


def test_cross_validation_is_not_worse_than_rejection(oracle):
    """synthetic's linear-Gaussian workload, 60 left-out rows, K = 200 of 4000: the prediction error of the ABC-GLM posterior mean
    does not exceed that of the rejection mean of the same retained rows, in any parameter (DESIGN.md records both)"""
    from abcsmc_amd import glm, synthetic
    X, Y = synthetic.Workload(8, 4).rows(0, 4000)
    cv = glm.cross_validate_pls_glm(X, Y, 60, 200, seed=7, posterior=numpy_posterior(oracle))
    assert np.all(cv["status"] == 0)
    rej = np.array([Y[cv["idx"][b]].mean(axis=0) for b in range(60)])
    var = cv["theta"].var(axis=0, ddof=1)
    err_rej = ((rej - cv["theta"]) ** 2).sum(axis=0) / (60 * var)
    print("ncomp", cv["ncomp"], "pred_error glm", cv["pred_error"], "rejection", err_rej)
    assert np.all(cv["pred_error"] <= err_rej)
