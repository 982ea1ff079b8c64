"""Every model-fit kernel (pls.hip: k_pls_fit<NW, GMEM, NB>, k_pls_fit16<NW, NB>, and the internal branches of tests/_pls_dispatch.py)
against the long-double model of tests/_pls_ref.py, on statistics records built on the host.

Per case: the model buffer is prefilled with NaN and followed by a guard of 8 doubles; abc_pls_model_dev runs twice.
  * every entry is written and nothing else: no NaN in the record, the guard and the statistics record untouched, the two runs
    bit-identical;
  * exact fields: the header, mean (bit-exact to the fp64 replica), sd (1 ulp), zobs, oscore (the m-ascending fma chain with the
    device's own R), per (first strict argmin of the device's PRESS column), ncomp;
  * identities of the device's own W, P, R, Q in long double: |w| = 1, W'W = I, P'R = I, R'XX R diagonal with tt on it,
    q_a = XY_0'r_a / tt_a, and the Rayleigh check (w_a is a dominant direction of XY_a XY_a', XY deflated with the device's own
    p, q, tt): valid where the eigenvector is not unique, it catches non-convergence at an exact tie;
  * R, W, P, Q column by column against the reference fit within its gap-derived bound (_pls_ref.column_bounds), on the
    components the reference calls well conditioned;
  * H and PRESS within their entry-wise bounds of the reference evaluated on the device's own R and Q; per equal to the
    reference's argmin except where that is ambiguous, and then within the bound of the minimum.
"""
import numpy as np
import pytest

import _pls_ref as PR
from _pls_dispatch import fit_plan, reachable

LD = np.longdouble
U = PR.U

# (M, P, A, kind, N, ntrain); kind: see _records.  N None: max(4 M, 300) rows, half of them training rows
CASES = [
    # every instantiation on the synthetic workload
    (7, 5, 4, "wl", None, None), (8, 1, 4, "wl", None, None),                         # <1,F,1>
    (12, 20, 4, "wl", None, None),                                                    # <1,F,2>
    (16, 40, 4, "wl", None, None), (10, 65, 4, "wl", None, None),                     # <1,F,0>, square4 and generic
    (20, 1, 4, "wl", None, None), (63, 15, 63, "wl", None, None),                     # <4,F,1>, A = M
    (48, 31, 48, "wl", None, None),                                                   # <4,F,2>, A = M
    (40, 40, 8, "wl", None, None), (17, 65, 4, "wl", None, None),                     # <4,F,0>
    (65, 1, 8, "wl", None, None), (200, 15, 32, "wl", None, None),                    # <8,F,1>
    (200, 20, 10, "wl", None, None),                                                  # <8,F,2>
    (65, 33, 8, "wl", None, None), (65, 65, 8, "wl", None, None),                     # <8,F,0>
    (600, 16, 8, "wl", 2400, None), (100, 1, 100, "wl", None, None),                  # <8,T,1>
    (63, 63, 32, "wl", None, None), (1, 100, 1, "wl", None, None),                    # <8,T,0>
    # k_pls_fit16, folded and not, X'X in LDS / registers / global memory
    (17, 2, 4, "wl", None, None), (32, 16, 8, "wl", None, None), (64, 16, 8, "wl", None, None),
    (37, 20, 20, "wl", None, None), (64, 20, 8, "wl", None, None), (65, 30, 8, "wl", None, None),
    (128, 16, 8, "wl", None, None), (129, 2, 8, "wl", None, None), (40, 16, 40, "wl", None, None),
    (50, 12, 1, "wl", None, None),                                                    # A = 1
    # planted relative gaps, an exact tie
    (20, 8, 4, "gap1e-2", 128, 64), (12, 8, 4, "gap1e-4", 128, 64), (70, 16, 4, "gap1e-4", 256, 128),
    (40, 32, 6, "gap1e-6", 128, 64), (16, 16, 3, "gap1e-6", 64, 32),
    (20, 2, 2, "tie", 128, 64), (10, 4, 3, "tie", 128, 64), (40, 40, 4, "tie", 128, 64),
    # awkward data
    (32, 16, 8, "zerovar", None, None), (65, 33, 8, "zerovar", None, None),
    (17, 5, 4, "constresp", None, None), (10, 20, 4, "constresp", None, None),
    (20, 3, 4, "allconst", None, None), (8, 1, 3, "allconst", None, None), (20, 1, 4, "allconst", None, None),
    (10, 65, 2, "allconst", None, None), (70, 8, 3, "allconst", None, None), (20, 4, 3, "constX", None, None),
    (40, 20, 4, "allconst", None, None), (70, 20, 4, "allconst", None, None),       # zero components on fit16 NB = 2
    (100, 1, 100, "allconst", None, None), (200, 40, 4, "allconst", None, None),    # ... k_pls_fit's eight-thread q
    (30, 6, 5, "wl", 300, 300), (65, 40, 6, "wl", 400, 400),                          # empty validation partition
    (24, 6, 4, "wl", 300, 299), (24, 6, 4, "wl", 300, 2),                             # n1 = 1, n0 = 2
    (32, 16, 8, "pilot", 4000, 2000), (12, 3, 3, "pilot", 1000, 500),              # the record's shift 1e3 sd off centre
    (40, 10, 8, "scaled", None, None), (14, 40, 5, "scaled", None, None),
]


def _id(c):
    return "%s-M%d-P%d-A%d%s" % (c[3], c[0], c[1], c[2], "" if c[5] is None else "-tr%d" % c[5])


def _hadamard(n):
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


def _records(M, P, kind, N, seed):
    """rows X (N x M), Y (N x P), the observed metrics of a case and the statistics record's shift (None: the mean of the first
    256 rows, as abc_stats_shift_dev takes it)"""
    from abcsmc_amd import synthetic
    rng = np.random.default_rng(seed)
    if kind.startswith("gap"):
        # both partitions centred with orthonormal columns (equal norms over the set: z-scoring scales uniformly) and
        # Y = X B, B'B = V diag(s^2) V' with V a normalised Hadamard matrix (equal column norms): XY'XY has the planted spectrum
        g = float(kind[3:])
        half = N // 2
        parts = []
        for _ in range(2):
            Z = rng.normal(size=(half, M))
            Z -= Z.mean(0)
            parts.append(np.linalg.qr(Z)[0] * np.sqrt(half))
        X = np.concatenate(parts, 0)
        s = np.concatenate([[1.0, np.sqrt(1 - g)], np.linspace(0.7, 0.1, P - 2)])
        Um = np.linalg.qr(rng.normal(size=(M, P)))[0]
        V = _hadamard(P) / np.sqrt(P)
        Y = X @ (Um * s) @ V.T
        return X, Y, rng.normal(size=M), None
    if kind == "tie":
        # exactly orthogonal +-1 columns in both partitions, responses equal to metrics: XY'XY = c I exactly
        Hd = _hadamard(N // 2)[:, 1:M + 1]
        X = np.concatenate([Hd, Hd[::-1]], 0)
        Y = X[:, :P].copy()
        return X, Y, rng.normal(size=M), None
    wl = synthetic.Workload(M, P, seed)
    X, Y = wl.rows(0, N)
    X, Y = np.array(X), np.array(Y)
    obs = np.array(wl.observed())
    if kind == "zerovar":
        X[:, 2] = 0.5
    elif kind == "constresp":
        Y[:, 1] = 0.75
    elif kind == "allconst":
        Y[:] = -1.5
    elif kind == "constX":
        X[:] = 0.25
    elif kind == "pilot":
        # an unrepresentative pilot: the record is kept about a shift 1001 sd off centre, so that zstats_body's centred
        # cross-products G - d S' - S d' + n d d' cancel by about 1e6
        Z = np.concatenate([X, Y], 1)
        return X, Y, obs, Z.mean(0) + 1001.0 * Z.std(0, ddof=1)
    elif kind == "scaled":
        X *= 10.0 ** np.linspace(-6, 6, M)
        Y *= 10.0 ** np.linspace(6, -6, P)
        obs *= 10.0 ** np.linspace(-6, 6, M)
    return X, Y, obs, None


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _run_model(gpu_ctx, stats, obs, M, P, A, simple=False):
    import torch
    from abcsmc_amd import _lib
    lib = _lib.lib()
    dev = "cuda:0"
    ds = torch.from_numpy(stats.copy()).to(dev)
    do = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float64)).to(dev)
    L = lib.abc_model_len(M, P, 0 if simple else A)
    assert PR.model_layout(M, P, 0 if simple else A)["len"] == L and PR.stats_layout(M, P)["len"] == lib.abc_stats_len(M, P), \
        "tests/_pls_ref.py's record layouts differ from the library's"
    out = []
    for _ in range(2):
        m = torch.full((L + 8,), float("nan"), dtype=torch.float64, device=dev)
        if simple:
            gpu_ctx.check(lib.abc_simple_model_dev(gpu_ctx.handle, ds.data_ptr(), do.data_ptr(), M, P, m.data_ptr()))
        else:
            gpu_ctx.check(lib.abc_pls_model_dev(gpu_ctx.handle, ds.data_ptr(), do.data_ptr(), M, P, A, 0, m.data_ptr()))
        torch.cuda.synchronize()
        out.append(m.cpu().numpy())
    assert np.array_equal(_bits(ds.cpu().numpy()), _bits(stats)), "the statistics record changed"
    assert np.array_equal(_bits(out[0]), _bits(out[1])), "two runs of the same record differ"
    guard = out[0][L:]
    assert np.isnan(guard).all() and np.array_equal(_bits(guard), _bits(np.full(8, np.nan))), "the guard was written"
    return out[0][:L], L


# worst error / bound ratios per (family, field) and flagged counts: filled by the cases, written out by _report
REPORT = {"ratio": {}, "components": 0, "ill": {"exhausted": 0, "gap": 0, "bound": 0}, "ambiguous": 0, "responses": 0,
          "zero": 0, "sign_free": 0}
_FIELDS = (("columns", ("R", "W", "Pl", "Q")), ("identities", ("|w|", "W'W", "P'R", "R'XXR", "P identity", "Q identity")),
           ("Rayleigh", ("rayleigh",)), ("H", ("H",)), ("PRESS", ("PRESS",)))


@pytest.fixture(scope="module", autouse=True)
def _report(request):
    """after the module's cases: the worst error / bound ratio per kernel family and field, and the flagged counts, on the
    terminal (a report, not a test)"""
    yield
    if not REPORT["ratio"]:
        return
    fams = sorted({k[0] for k in REPORT["ratio"]}, key=str)
    lines = ["pls-model worst error / bound    " + "".join("%12s" % name for name, _ in _FIELDS)]
    for fam in fams:
        vals = [max([REPORT["ratio"].get((fam, f), 0.0) for f in fields]) for _, fields in _FIELDS]
        lines.append("pls-model %-22s" % (fam,) + "".join("%12.3g" % v for v in vals))
    ill = REPORT["ill"]
    lines.append("pls-model flagged: %d of %d non-zero components ill-conditioned (%d exhausted, %d at a gap below %.0e, %d by "
                 "their bound), %d of %d argmins ambiguous; %d zero components; %d components compared up to sign"
                 % (sum(ill.values()), REPORT["components"], ill["exhausted"], ill["gap"], PR.GAP_MIN, ill["bound"],
                    REPORT["ambiguous"], REPORT["responses"], REPORT["zero"], REPORT["sign_free"]))
    cap = request.config.pluginmanager.getplugin("capturemanager")
    with cap.global_and_fixture_disabled():
        print("\n" + "\n".join(lines))


def _ratio(fam, field, err, bound):
    if bound > 0:
        k = (fam, field)
        REPORT["ratio"][k] = max(REPORT["ratio"].get(k, 0.0), float(err / bound))


def _check_exact_fields(m, stats, obs, M, P, A):
    g = PR.unpack_model(m, M, P, A)
    n0, n1 = stats[0], stats[1]
    mean64, sd64 = PR.moments_f64(stats, M, P)
    assert np.array_equal(_bits(g["mean"]), _bits(mean64)), "mean not bit-exact"
    assert np.all(np.abs(g["sd"] - sd64) <= np.spacing(sd64)), "sd beyond 1 ulp"
    sd, mean = g["sd"][:M], g["mean"][:M]
    with np.errstate(divide="ignore", invalid="ignore"):
        zobs = np.where(sd == 0.0, 0.0, (obs - mean) / sd)
    assert np.array_equal(_bits(g["zobs"]), _bits(zobs)), "zobs not bit-exact"
    return g, n0, n1


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_pls_model_against_long_double_reference(gpu_ctx, case):
    M, P, A, kind, N, ntrain = case
    N = N or max(4 * M, 300)
    ntrain = N // 2 if ntrain is None else ntrain
    X, Y, obs, shift = _records(M, P, kind, N, seed=7000 + 37 * M + P)
    stats = PR.stats_record(X, Y, ntrain, shift)
    if kind == "pilot":
        Z = np.concatenate([X, Y], 1)
        assert np.all(np.abs(shift - Z.mean(0)) >= 1e3 * Z.std(0, ddof=1)), "the shift is not 1e3 sd off centre"
    m, L = _run_model(gpu_ctx, stats, obs, M, P, A)
    assert not np.isnan(m).any(), "NaN in the model record (%d entries)" % int(np.isnan(m).sum())
    g, n0, n1 = _check_exact_fields(m, stats, obs, M, P, A)
    plan = fit_plan(M, P, A)
    fam = plan["kernel"]
    # ---- header, per, ncomp, oscore ------------------------------------------------------------------------------------------
    press_dev = g["press"]
    per_dev = np.array([1 + min(range(A), key=lambda a: (press_dev[a, j], a)) for j in range(P)])
    # (the first strict argmin: min over (value, index))
    assert np.array_equal(g["per"], per_dev.astype(float)), (g["per"], per_dev)
    ncomp = max(1, int(per_dev.max()))
    assert np.array_equal(g["hdr"], [ncomp, A, n0 + n1, 0.0]), g["hdr"]
    for k in range(A):
        assert g["oscore"][k] == PR.fma_dot(g["zobs"], g["R"][:, k]), ("oscore", k)
    # ---- the reference ------------------------------------------------------------------------------------------------------
    ref = PR.reference(stats, M, P, A)
    z, f = ref["z"], ref["fit"]
    XX, XY0, eXX, eXY = z["XX"][0], z["XY"][0], z["eXX"][0], z["eXY"][0]
    CE = 4 * (M + P) + 64
    dl = ref["delta_in"]
    W, Rr, Pl, Q = (g[k].astype(LD) for k in ("W", "R", "Pl", "Q"))
    # zero components: exactly zero columns and H rows
    for a in np.nonzero(f["zero"])[0]:
        for key in ("W", "R", "Pl", "Q"):
            assert (g[key][:, a] == 0).all(), ("zero component", key, a)
        assert (g["H"][a] == 0).all() and (g["H"][:, a] == 0).all(), ("zero component H", a)
        if a > 0:              # (the first one's PRESS, YY, is held by the PRESS bound below)
            assert np.array_equal(_bits(press_dev[a]), _bits(press_dev[a - 1])), ("zero component PRESS", a)
    REPORT["zero"] += int(f["zero"].sum())
    # ---- identities of the device's own W, P, R, Q; the Rayleigh check ---------------------------------------------------------
    XYd = np.array(XY0, dtype=LD)
    n0XY = np.sqrt(np.sum(XYd * XYd))
    live = []
    for a in range(A):
        if f["zero"][a]:
            break
        na = np.sqrt(np.sum(XYd * XYd))
        rho = float(n0XY / na) if na > 0 else np.inf
        if not np.isfinite(rho) or 1.0 / rho < PR.EXHAUSTED:
            break                                              # exhausted: rounding-level directions from here on
        live.append(a)
        w, r, p, q = W[:, a], Rr[:, a], Pl[:, a], Q[:, a]
        xr = XX @ r
        tt = r @ xr
        assert abs(np.sqrt(w @ w) - 1) <= 4 * (M + 8) * U, ("|w|", a)
        _ratio(fam, "|w|", abs(np.sqrt(w @ w) - 1), 4 * (M + 8) * U)
        # Rayleigh: |XY_a' w|^2 >= l_max(XY_a' XY_a) (1 - tol)
        if P > 1:
            lmax = LD(np.linalg.eigvalsh((XYd.T @ XYd).astype(np.float64))[-1])
            val = np.sum((XYd.T @ w) ** 2)
            tol = 1e-12 + 4 * (CE * U + dl) * rho * rho
            assert val >= lmax * (1 - tol), ("Rayleigh", a, float(1 - val / lmax), tol)
            _ratio(fam, "rayleigh", max(float(1 - val / lmax), 0.0), tol)
        # P = XX R / tt: X'X r = tt p
        axr = np.abs(XX) @ np.abs(r)
        err = np.sqrt(np.sum((xr - tt * p) ** 2))
        bnd = 2 * CE * U * rho * np.sqrt(np.sum(axr ** 2)) + 2 * np.sqrt(np.sum((eXX @ np.abs(r)) ** 2))
        assert err <= bnd, ("XX r = tt p", a, float(err), float(bnd))
        _ratio(fam, "P identity", err, bnd)
        # q_a = XY_0' r_a / tt_a
        qx = (XY0.T @ r) / tt
        err = np.sqrt(np.sum((q - qx) ** 2))
        bnd = ((CE * U * (a + 1) * rho * np.sqrt(np.sum((np.abs(XY0).T @ np.abs(r)) ** 2))
                + np.sqrt(np.sum((eXY.T @ np.abs(r)) ** 2))) / abs(tt) + (2 * CE * U + 4 * dl) * rho * np.sqrt(np.sum(qx ** 2)))
        assert err <= bnd, ("q identity", a, float(err), float(bnd))
        _ratio(fam, "Q identity", err, bnd)
        XYd = XYd - tt * np.outer(p, q)
    if live:
        k = len(live)
        rho_max = float(n0XY / np.sqrt(np.sum(XYd * XYd))) if np.sum(XYd * XYd) > 0 else 1.0 / PR.EXHAUSTED
        rho_max = min(max(rho_max, 1.0), 1.0 / PR.EXHAUSTED)
        Wl, Rl, Pll = W[:, :k], Rr[:, :k], Pl[:, :k]
        # (the device's z-scored X'X carries the input error, asymmetrically: (G - d_a S_b) - d_b S_a is rounded differently from
        # (G - d_b S_a) - d_a S_b; the identities hold for that matrix, so they hold for the exact one to the input error too)
        tolI = (CE * U + 2 * dl) * rho_max * (1 + f["proj"][:k].max()) * k
        e = np.abs(Wl.T @ Wl - np.eye(k)).max()
        assert e <= tolI, ("W'W = I", float(e), tolI)
        _ratio(fam, "W'W", e, tolI)
        e = np.abs(Pll.T @ Rl - np.eye(k)).max() if k else 0
        bnd = tolI * np.abs(np.outer(np.sqrt(np.sum(Pll ** 2, 0)), np.sqrt(np.sum(Rl ** 2, 0)))).max()
        assert e <= max(bnd, tolI), ("P'R = I", float(e), float(bnd))
        _ratio(fam, "P'R", e, max(bnd, tolI))
        T = Rl.T @ XX @ Rl
        tts = np.sqrt(np.abs(np.diag(T)))
        off = np.abs(T - np.diag(np.diag(T))) / np.outer(tts, tts)
        bnd = tolI + 2 * float(np.max(np.abs(Rl).T @ eXX @ np.abs(Rl) / np.outer(tts, tts)))
        assert off.max() <= bnd, ("R'XX R diagonal", float(off.max()), bnd)
        _ratio(fam, "R'XXR", off.max(), bnd)
    # ---- R, W, P, Q against the reference fit --------------------------------------------------------------------------------
    REPORT["components"] += int((~f["zero"]).sum())
    ill = np.nonzero(ref["ill"])[0]
    if len(ill):                         # (the first ill-conditioned component's reason; every later one follows it)
        a0 = ill[0]
        exhausted = not np.isfinite(f["rho"][a0]) or 1.0 / f["rho"][a0] < PR.EXHAUSTED
        REPORT["ill"]["exhausted" if exhausted else "gap" if P > 1 and f["gap"][a0] < PR.GAP_MIN else "bound"] += len(ill)
    for a in range(A):
        if ref["ill"][a] or f["zero"][a]:
            continue
        # the sign convention (largest |entry| of the eigenvector positive) decides the sign where that entry is unique by a
        # margin the device's error cannot cross; elsewhere (e.g. eigenvectors with entries of equal magnitude) the columns are
        # compared up to one common sign
        fixed = P == 1 or f["qmargin"][a] > 1e-8 + 8 * ref["e"][a]
        sgn = 1 if fixed else (1 if g["W"][:, a].astype(LD) @ f["W"][:, a] > 0 else -1)
        REPORT["sign_free"] += int(not fixed)
        for key, rk in (("R", "R"), ("W", "W"), ("Pl", "Pl"), ("Q", "Q")):
            rf = f[rk][:, a]
            err = np.sqrt(np.sum((sgn * g[key][:, a].astype(LD) - rf) ** 2))
            bnd = ref["e"][a] * np.sqrt(np.sum(rf * rf)) + 4 * U * np.sqrt(np.sum(rf * rf))
            assert err <= bnd, ("column", key, a, float(err / np.sqrt(np.sum(rf * rf))), ref["e"][a], f["gap"][a], fixed)
            _ratio(fam, key, err, bnd)
    # ---- H, PRESS, per ---------------------------------------------------------------------------------------------------------
    pr = PR.press(z, g["R"], g["Q"])
    errH = np.abs(g["H"].astype(LD) - pr["H"])
    bH = pr["H_err"] + 2 * U * np.abs(pr["H"])
    assert np.all(errH <= bH), ("H", float(np.max(errH - bH)))
    _ratio(fam, "H", float(np.max(errH / np.where(bH > 0, bH, 1))), 1.0)
    errP = np.abs(press_dev.astype(LD) - pr["press"])
    assert np.all(errP <= pr["bound"]), ("PRESS", float(np.max(errP - pr["bound"])))
    _ratio(fam, "PRESS", float(np.max(errP / np.where(pr["bound"] > 0, pr["bound"], 1))), 1.0)
    REPORT["responses"] += P
    REPORT["ambiguous"] += int(pr["ambiguous"].sum())
    for j in range(P):
        if not pr["ambiguous"][j]:
            assert per_dev[j] == pr["per"][j], ("per", j, per_dev[j], pr["per"][j])
        else:
            lo = np.min(pr["press"][:, j])
            assert pr["press"][per_dev[j] - 1, j] - lo <= 2 * pr["bound"][:, j].max(), ("ambiguous per", j)


@pytest.mark.gpu
@pytest.mark.parametrize("M,P,kind", [(7, 5, "wl"), (40, 3, "zerovar"), (129, 20, "scaled"), (10, 2, "constX")])
def test_simple_model_fields(gpu_ctx, M, P, kind):
    """abc_simple_model_dev: header [0, 0, n, 0], mean / sd / zobs as the PLS record's, nothing written past zobs"""
    X, Y, obs, shift = _records(M, P, kind, 300, seed=11 * M + P)
    stats = PR.stats_record(X, Y, 150, shift)
    m, L = _run_model(gpu_ctx, stats, obs, M, P, 0, simple=True)
    o = PR.model_layout(M, P, 0)
    assert not np.isnan(m[:o["zobs"] + M]).any()
    assert np.isnan(m[o["zobs"] + M:]).all(), "the simple model wrote past its z-scores"
    g, n0, n1 = _check_exact_fields(m, stats, obs, M, P, 0)
    assert np.array_equal(g["hdr"], [0.0, 0.0, n0 + n1, 0.0]), g["hdr"]


def test_cases_reach_every_instantiation_and_branch():
    """through the mirror of launch_pls_model: the cases above reach all 15 instantiations and every internal branch"""
    plans = [fit_plan(M, P, A) for M, P, A, _, _, _ in CASES]
    assert {p["kernel"] for p in plans} == reachable()
    for fam in ("fit", "fit16"):
        got = lambda key: {p[key] for p in plans if p["kernel"][0] == fam}
        assert got("xx") == {"lds", "reg", "global"}, (fam, got("xx"))
        assert got("press") == {"gemm", "entry"}, fam
    assert {p["eig"] for p in plans if p["kernel"][0] == "fit"} == {None, "square1", "square2", "square4", "generic"}
    assert {(p["kernel"], p["fold_z"]) for p in plans if p["kernel"][0] == "fit16"} >= {
        (("fit16", 4, 1), True), (("fit16", 4, 1), False), (("fit16", 4, 2), True), (("fit16", 4, 2), False)}
    assert {p["q8"] for p in plans if p["kernel"][0] == "fit" and p["kernel"][1] > 1} == {True, False}
    # the generic eigen-step in both modes (LDS and global memory), P == 1 on one, four and eight waves
    assert {p["kernel"][2] for p in plans if p["eig"] == "generic"} == {False, True}
    assert {p["kernel"][1] for p in plans if p["eig"] is None} == {1, 4, 8}
    # every kind of awkward data reaches both kernel families
    for kind in ("allconst", "constresp", "zerovar", "tie", "scaled", "pilot"):
        assert {fit_plan(M, P, A)["kernel"][0] for M, P, A, k, _, _ in CASES if k == kind} == {"fit", "fit16"}, kind
    # zero components (an exactly-zero X'Y) on every latency-tuned kernel, every eigen-step and P == 1, and on both ways of
    # computing q in k_pls_fit
    zplans = [fit_plan(M, P, A) for M, P, A, k, _, _ in CASES if k in ("allconst", "constX")]
    assert {p["kernel"] for p in zplans} >= {("fit16", 4, 1), ("fit16", 4, 2), ("fit16", 8, 1), ("fit16", 8, 2)}
    assert {p["eig"] for p in zplans} == {None, "generic", "square1", "square2", "square4"}
    assert {p["q8"] for p in zplans if p["kernel"][0] == "fit"} == {True, False}
