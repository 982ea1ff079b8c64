"""A long-double model of the PLS fit from a statistics record (abcsmc_amd/csrc/pls.hip: zstats_body, k_pls_fit, k_pls_fit16),
for the tests: tests/test_pls_ref_cpu.py checks it without a GPU, tests/test_gpu_pls_model.py holds every fit kernel against it.

Everything runs in NumPy longdouble (x87 extended: a 64-bit mantissa, unit roundoff 5.4e-20), against fp64 kernels (unit
roundoff U = 2^-53 = 1.1e-16): the reference's own rounding is three orders below every bound it is used with.

What it computes from a host copy of the record (layouts: abc_internal.h, stats_layout / model_layout):
  * moments_f64: mean and sd in zstats_body's exact fp64 operation order (the library is built with -ffp-contract=off, so
    mean matches bit for bit; sd to 1 ulp, for the square root);
  * zstats: the moments and both partitions' z-scored cross-products (X'X, X'Y) and YYte by zstats_body's formulas, in long
    double, with an entry-wise bound of how far the kernels' fp64 evaluation of the same formulas may lie from them;
  * fit: the kernel-PLS2 loop with the device's conventions (P == 1: w = XY; otherwise w = XY q with q the dominant eigenvector
    of XY'XY, its largest |component| positive, ties to the lowest index; r orthogonalised against the earlier components;
    tt = r'XXr, p = XXr / tt, q = XY'r / tt; XY deflated), each component's relative eigen-gap and deflated size, an error
    bound per component and the ill-conditioned flags;
  * press: H, c, PRESS, per and ncomp from the validation partition for given R and Q, with an entry-wise bound of the
    device's statistics-form evaluation and the ambiguous argmins.

A component whose w = XY q is exactly zero (an exactly-zero cross-product matrix: a constant response with P == 1, every
response or every metric constant) is a ZERO component: w, r, p, q and its H row are 0, its PRESS is the previous count's
(YY for the first), and every later component is zero as well (declared deviations).
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53                 # unit roundoff of the fp64 kernels

# ---- thresholds of the ill-conditioned flags ------------------------------------------------------------------------------
GAP_MIN = 1e-9                 # relative eigen-gap (l1 - l2) / l1 below which the dominant direction is not determined in fp64
EXHAUSTED = 1e-9               # |XY_a| / |XY_0| below which the deflated cross-products are rounding noise (A near M)
BOUND_MAX = 1e-6               # a component whose column bound exceeds this is not compared column by column


def stats_layout(M, P):
    C16 = (M + P + 15) // 16 * 16
    o = {"C16": C16, "n": 0, "shift": 2}
    o["sum"] = [2 + C16, 2 + 2 * C16]
    o["G"] = [2 + 3 * C16, 2 + 3 * C16 + C16 * C16]
    o["len"] = o["G"][1] + C16 * C16
    return o


def model_layout(M, P, A):
    o = {"hdr": 0, "mean": 4}
    o["sd"] = o["mean"] + M + P
    o["zobs"] = o["sd"] + M + P
    o["oscore"] = o["zobs"] + M
    o["R"] = o["oscore"] + A
    o["Q"] = o["R"] + M * A
    o["W"] = o["Q"] + P * A
    o["P"] = o["W"] + M * A
    o["H"] = o["P"] + M * A
    o["press"] = o["H"] + A * A
    o["per"] = o["press"] + A * P
    o["len"] = o["per"] + P
    return o


def unpack_model(m, M, P, A):
    """views of a host model record: R, W, Pl (M x A), Q (P x A), H (A x A), press (A x P), column-major as the device writes"""
    o = model_layout(M, P, A)
    mat = lambda key, r, c: m[o[key]:o[key] + r * c].reshape(c, r).T
    return {"hdr": m[0:4], "mean": m[o["mean"]:o["mean"] + M + P], "sd": m[o["sd"]:o["sd"] + M + P],
            "zobs": m[o["zobs"]:o["zobs"] + M], "oscore": m[o["oscore"]:o["oscore"] + A], "R": mat("R", M, A),
            "Q": mat("Q", P, A), "W": mat("W", M, A), "Pl": mat("P", M, A), "H": mat("H", A, A),
            "press": mat("press", A, P), "per": m[o["per"]:o["per"] + P]}


def stats_record(X, Y, ntrain, shift=None):
    """a statistics record of rows X (N x M), Y (N x P), the first ntrain of them training rows, as abc_stats_shift_dev +
    abc_stats_accumulate_dev leave it (shift: the mean of the first min(N, 256) rows unless given), in fp64 (the record is the
    input of the fit: any finite values do)"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    N, M = X.shape
    P = Y.shape[1]
    L = stats_layout(M, P)
    s = np.zeros(L["len"])
    Zr = np.concatenate([X, Y], 1)
    if shift is None:
        shift = Zr[:min(N, 256)].mean(0) if N else np.zeros(M + P)
    s[L["shift"]:L["shift"] + M + P] = shift
    Z = Zr - np.asarray(shift, dtype=np.float64)
    for part, sl in enumerate((slice(0, ntrain), slice(ntrain, N))):
        z = Z[sl]
        s[part] = z.shape[0]
        s[L["sum"][part]:L["sum"][part] + M + P] = z.sum(0)
        G = np.zeros((L["C16"], L["C16"]))
        G[:M + P, :M + P] = z.T @ z
        s[L["G"][part]:L["G"][part] + L["C16"] ** 2] = G.T.reshape(-1)
    return s


def _parts(stats, M, P):
    L = stats_layout(M, P)
    C, C16 = M + P, L["C16"]
    s = np.asarray(stats, dtype=np.float64)
    S = [s[L["sum"][p]:L["sum"][p] + C] for p in range(2)]
    G = [s[L["G"][p]:L["G"][p] + C16 * C16].reshape(C16, C16).T[:C, :C] for p in range(2)]
    return s[0], s[1], s[L["shift"]:L["shift"] + C], S, G


def moments_f64(stats, M, P):
    """(mean, sd) of the M + P columns in zstats_body's fp64 operation order"""
    n0, n1, shift, S, G = _parts(stats, M, P)
    n = n0 + n1
    s = S[0] + S[1]
    d = s / n if n > 0 else np.zeros_like(s)
    g = np.diag(G[0]) + np.diag(G[1])
    ss = g - (n * d) * d
    ss = np.where(ss < 0.0, 0.0, ss)
    sd = np.sqrt(ss / (n - 1.0)) if n >= 2 else np.zeros_like(s)
    return shift + d, sd


def zstats(stats, M, P):
    """zstats_body in long double: d (mean - shift), sd, XX[part], XY[part] (the z-scored cross-products), YY (YYte), and
    entry-wise bounds of how far the kernels' fp64 values may lie from them: eXX[part], eXY[part], eYY.  The bound of an entry
    is U (6 t + propagated d errors) / (sd_a sd_b) + U (k_a + k_b + 2) |z|: t the sum of the absolute terms of the centred
    cross-product (four terms, at most six roundings), d's error U D (a sum of two and a division), k the relative error of a
    deviation (its centred sum of squares cancels by (g + n d^2) / ss)"""
    n0, n1, shift, S, G = _parts(stats, M, P)
    n = LD(n0) + LD(n1)
    SL = [S[p].astype(LD) for p in range(2)]
    GL = [G[p].astype(LD) for p in range(2)]
    s = SL[0] + SL[1]
    d = s / n if n > 0 else np.zeros(M + P, dtype=LD)
    ss = np.diag(GL[0]) + np.diag(GL[1]) - n * d * d
    ss = np.where(ss < 0, LD(0), ss)
    sd = np.sqrt(ss / (n - 1)) if n >= 2 else np.zeros(M + P, dtype=LD)
    # relative bounds: d (a sum of two and a division), sd (the centred sum of squares cancels by (g + n d^2) / ss)
    Dd = (np.abs(SL[0]) + np.abs(SL[1])) / max(n, LD(1)) + np.abs(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        ksd = np.where(ss > 0, (np.diag(np.abs(GL[0]) + np.abs(GL[1])) + 2 * n * d * d + 2 * n * Dd * np.abs(d)) / ss + 2, 0)
    out = {"n0": float(n0), "n1": float(n1), "d": d, "sd": sd, "XX": [], "XY": [], "eXX": [], "eXY": []}
    den = np.outer(sd, sd)
    pos = den > 0
    for part, npart in ((0, LD(n0)), (1, LD(n1))):
        cross = GL[part] - np.outer(d, SL[part]) - np.outer(SL[part], d) + npart * np.outer(d, d)
        Z = np.where(pos, cross / np.where(pos, den, 1), LD(0))
        term = (6 * (np.abs(GL[part]) + np.abs(np.outer(d, SL[part])) + np.abs(np.outer(SL[part], d)) + npart * np.abs(np.outer(d, d)))
                + np.outer(Dd, np.abs(SL[part]) + npart * np.abs(d)) + np.outer(np.abs(SL[part]) + npart * np.abs(d), Dd))
        E = np.where(pos, U * (term / np.where(pos, den, 1) + (ksd[:, None] + ksd[None, :] + 2) * np.abs(Z)), LD(0))
        out["XX"].append(Z[:M, :M])
        out["XY"].append(Z[:M, M:])
        out["eXX"].append(E[:M, :M])
        out["eXY"].append(E[:M, M:])
        if part == 1:
            out["YY"] = np.diag(Z)[M:].copy()
            out["eYY"] = np.diag(E)[M:].copy()
    return out


def dominant_eigvec(S):
    """(q, l1, gap, residual) of a symmetric PSD long-double matrix: float64 eigh, then corrections in long double along the
    other eigenvectors until |S q - l q| <= 1e-17 |S|; q has unit norm, its largest |component| positive (ties: lowest index);
    gap = (l1 - l2) / l1"""
    n = S.shape[0]
    lam, V = np.linalg.eigh(S.astype(np.float64))
    q = V[:, -1].astype(LD)
    VL = V.astype(LD)
    nrmS = max(np.max(np.abs(S)), LD(1e-300))
    res = LD(0)
    for _ in range(30):
        q /= np.sqrt(q @ q)
        mu = q @ (S @ q)
        r = S @ q - mu * q
        res = np.sqrt(r @ r)
        if res <= 1e-17 * nrmS:
            break
        corr = np.zeros(n, dtype=LD)
        for i in range(n - 1):
            den = mu - LD(lam[i])
            if abs(den) > 1e-13 * nrmS:
                corr += VL[:, i] * ((VL[:, i] @ r) / den)
        q = q + corr
    q /= np.sqrt(q @ q)
    big = int(np.argmax(np.abs(q)))
    if q[big] < 0:
        q = -q
    l1 = q @ (S @ q)
    l2 = LD(lam[-2]) if n > 1 else LD(0)
    gap = max(float((l1 - l2) / l1), 0.0) if l1 > 0 else 0.0
    return q, l1, gap, float(res / nrmS)


def fit(XY0, XX, A):
    """the kernel-PLS2 loop in long double on z-scored cross-products (XY0: M x P, XX: M x M) -> dict of W, R, Pl, Q, tt,
    per component: gap, rho = |XY_0| / |XY_a| (Frobenius), zero (a zero component), qmargin (the eigenvector's largest |entry|
    over its second largest, 1 - ...), and proj (sum_j |p_j'w_a| |r_j| / |r_a|)"""
    XY = np.array(XY0, dtype=LD)
    XX = np.asarray(XX, dtype=LD)
    M, P = XY.shape
    W, R, Pl = (np.zeros((M, A), dtype=LD) for _ in range(3))
    Q = np.zeros((P, A), dtype=LD)
    tt_all = np.zeros(A, dtype=LD)
    n0 = np.sqrt(np.sum(XY * XY))
    info = {"gap": np.ones(A), "rho": np.full(A, np.inf), "zero": np.zeros(A, bool), "qmargin": np.ones(A), "proj": np.zeros(A)}
    zero = False
    for a in range(A):
        na = np.sqrt(np.sum(XY * XY))
        info["rho"][a] = float(n0 / na) if na > 0 else np.inf
        if not zero:
            if P == 1:
                w = XY[:, 0].copy()
            else:
                q, _, info["gap"][a], _ = dominant_eigvec(XY.T @ XY)
                aq = np.sort(np.abs(q))[::-1]
                info["qmargin"][a] = float(1 - aq[1] / aq[0])
                w = XY @ q
            zero = not np.any(w != 0)
        if zero:
            info["zero"][a:] = True
            info["gap"][a:] = 0.0
            break
        w /= np.sqrt(w @ w)
        pw = np.array([Pl[:, j] @ w for j in range(a)], dtype=LD)
        r = w.copy()
        for j in range(a):
            r -= pw[j] * R[:, j]
        if a:
            info["proj"][a] = float(np.sum(np.abs(pw) * np.sqrt(np.sum(R[:, :a] ** 2, 0))) / np.sqrt(r @ r))
        xr = XX @ r
        tt = r @ xr
        p, qa = xr / tt, (XY.T @ r) / tt
        XY -= tt * np.outer(p, qa)
        W[:, a], R[:, a], Pl[:, a], Q[:, a], tt_all[a] = w, r, p, qa, tt
    return {"W": W, "R": R, "Pl": Pl, "Q": Q, "tt": tt_all, **info}


def column_bounds(f, M, P, delta_in):
    """relative error bound of each component's columns (R, W, Pl, Q) of an fp64 fit against this one, and the ill-conditioned
    flags.  First-order perturbation of a dominant eigenvector: a relative error d of XY_a (2 d of S_a = XY_a'XY_a) moves it by
    at most 2 d / gap.  XY_a carries the error of the inputs (delta_in, relative to |XY_0|) and of every earlier component
    (e_k, propagated through its deflation), so relative to its own size rho_a (delta_in + sum_{k<a} e_k); the
    orthogonalisation of r adds proj_a sum_{k<a} e_k.  The rounding of the kernels' own chains (dot products of length M and P
    forming S_a, w and the deflation, relative to |XY_0|; the eigen-squaring, closed by a power step with S) is C_E U rho_a /
    gap_a with C_E = 4 (M + P) + 64: a worst-case first-order count of the longest chains, with room for the squaring.
      e_a = 2 rho_a (delta_in + sum_{k<a} e_k) / gap_a + proj_a sum_{k<a} e_k + C_E U rho_a / gap_a
    (P == 1: gap_a = 1, no eigenproblem.)  A component is ill-conditioned if gap_a < GAP_MIN, 1 / rho_a < EXHAUSTED, or
    e_a > BOUND_MAX; every later one is then ill-conditioned too."""
    A = len(f["gap"])
    CE = 4 * (M + P) + 64
    e = np.zeros(A)
    ill = np.zeros(A, bool)
    acc = 0.0
    for a in range(A):
        if f["zero"][a]:
            ill[a:] = False
            e[a:] = 0.0
            break
        g = 1.0 if P == 1 else f["gap"][a]
        rho = f["rho"][a]
        if g < GAP_MIN or not np.isfinite(rho) or 1.0 / rho < EXHAUSTED:
            ill[a:] = True
            e[a:] = np.inf
            break
        e[a] = 2 * rho * (delta_in + acc) / g + f["proj"][a] * acc + CE * U * rho / g
        if e[a] > BOUND_MAX:
            ill[a:] = True
            e[a:] = np.inf
            break
        acc += e[a]
    return e, ill


def press(z, R, Q):
    """H, c, PRESS (A x P), its entry-wise bound, per (first strict argmin + 1), the ambiguous argmins, ncomp, for rotations R
    and regression loadings Q (fp64 values, e.g. the device's own) on the validation statistics z (zstats).
    The device evaluates c = XYte'R and H = R'(XXte R) as fp64 chains of length M (pls_gemm or one thread per entry): their
    errors are at most gamma_{M+2} |R|'|XYte| and gamma_{2M+4} |R|'|XXte||R|, plus the propagated z-score errors.  PRESS_j(a) =
    YY_j - 2 sum_{k<a} q_jk c_jk + sum_{k,l<a} q_jk q_jl H_kl is then accumulated in A steps of at most four operations each:
    gamma_{4A+8} on the sum of the absolute terms, plus the propagated errors of c, H and YY.  (gamma_k = k U, first order.)
    A response's argmin is ambiguous where another count lies within twice the bound of the minimum (a bound of 0: every term
    is exactly 0, the device's values too, and its strict argmin takes the first count)."""
    RL, QL = np.asarray(R, dtype=LD), np.asarray(Q, dtype=LD)
    M, A = RL.shape
    P = QL.shape[0]
    XXte, XYte, YY = z["XX"][1], z["XY"][1], z["YY"]
    H = RL.T @ (XXte @ RL)
    c = XYte.T @ RL                                  # P x A
    aR = np.abs(RL)
    Hab = aR.T @ (np.abs(XXte) @ aR)
    H_err = (2 * M + 4) * U * Hab + aR.T @ (z["eXX"][1] @ aR)
    c_err = (M + 2) * U * (np.abs(XYte).T @ aR) + z["eXY"][1].T @ aR
    pr = np.zeros((A, P), dtype=LD)
    bound = np.zeros((A, P))
    for j in range(P):
        q = QL[j]
        aq = np.abs(q)
        for a in range(A):
            qa, ca, Ha = q[:a + 1], c[j, :a + 1], H[:a + 1, :a + 1]
            pr[a, j] = YY[j] - 2 * (qa @ ca) + qa @ (Ha @ qa)
            s_abs = abs(YY[j]) + 2 * (aq[:a + 1] @ np.abs(ca)) + aq[:a + 1] @ (np.abs(Ha) @ aq[:a + 1])
            prop = 2 * (aq[:a + 1] @ c_err[j, :a + 1]) + aq[:a + 1] @ (H_err[:a + 1, :a + 1] @ aq[:a + 1]) + z["eYY"][j]
            bound[a, j] = float((4 * A + 8) * U * s_abs + prop)
    per = np.zeros(P, dtype=int)
    amb = np.zeros(P, bool)
    for j in range(P):
        best = 0
        for a in range(1, A):
            if pr[a, j] < pr[best, j]:
                best = a
        per[j] = best + 1
        tol = 2 * bound[:, j].max()
        amb[j] = tol > 0 and any(a != best and pr[a, j] - pr[best, j] <= tol for a in range(A))   # (bound 0: exact values)
    ncomp = max(1, int(per.max())) if P else 1
    return {"H": H, "c": c, "press": pr, "bound": bound, "H_err": H_err, "per": per, "ambiguous": amb, "ncomp": ncomp}


def reference(stats, M, P, A):
    """the whole long-double model of a record: z (zstats), fit (fit on the training statistics), e / ill (column_bounds),
    delta_in (relative error of the kernels' z-scored training cross-products), pr (press on the reference's own R, Q)"""
    z = zstats(stats, M, P)
    nXY = np.sqrt(np.sum(z["XY"][0] ** 2))
    nXX = np.sqrt(np.sum(z["XX"][0] ** 2))
    d_xy = float(np.sqrt(np.sum(z["eXY"][0] ** 2)) / nXY) if nXY > 0 else 0.0
    d_xx = float(np.sqrt(np.sum(z["eXX"][0] ** 2)) / nXX) if nXX > 0 else 0.0
    delta_in = max(d_xy, d_xx, U)
    f = fit(z["XY"][0], z["XX"][0], A)
    e, ill = column_bounds(f, M, P, delta_in)
    pr = press(z, f["R"].astype(np.float64), f["Q"].astype(np.float64))
    return {"z": z, "fit": f, "e": e, "ill": ill, "delta_in": delta_in, "press": pr}


def fma_dot(a, b):
    """index-ascending fp64 fma chain, evaluated exactly (the kernels' observed-score chains)"""
    from fractions import Fraction
    s = 0.0
    for x, y in zip(a, b):
        s = float(Fraction(float(x)) * Fraction(float(y)) + Fraction(s))
    return s
