"""NumPy model of the device noise stream (resample.hip: philox, normal4, mv_noise, indep_noise, k_perturb*) and of the
proposals built from it, written from the stream's specification in DESIGN.md (§2, declared deviations, "noise stream"):

    key      k0 = s1 ^ 0x5bd1e995,  k1 = s2 ^ (s3 * 0x9E3779B1 mod 2^32)   (the abc_rng state the call was entered with)
    counter  (lo32(gi), hi32(gi), attempt, w),  gi = i0 + i
             multivariate: w = qd, columns 4 qd .. 4 qd + 3 of L;  independent: w = 0x80000000 | p, first deviate only
    block    Philox4x32-10 -> two Box-Muller pairs (x, y) and (z, w): radius from the first word of a pair, angle from the second

The integer part is exact (uint64 arithmetic).  The deviates follow normal4 with its f32 steps emulated in numpy float32 and
log2 / sqrt / cos / sin taken in float64: the device evaluates those on the f32 transcendental hardware, whose error is not
reproducible on the host, so every deviate carries a bound `zbound` (see `normal4_ref`).  A wrong key, counter word, column,
row group or slice offset moves a deviate by O(1), far outside that bound."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
MVN_MAX_TRIES = 1 << 14
INDEP_MAX_TRIES = 1000
GAUSS, UNIF_INT, UNIF_REAL = 0, 1, 2          # abc_prior kinds (include/abcsmc_hip.h)

# zbound = ZB_MULT x (first-order propagation of one unit error in each hardware step, `_pair`).  The measured worst
# |z_dev - z_ref| / unit over the cases of tests/test_gpu_proposals.py is recorded there; ZB_MULT keeps >= 8x headroom over it.
ZB_MULT = 16.0

_NEG2LN2 = np.float32(-1.3862943611198906)
_HALF = np.float32(0.5)
_TWO32 = np.float32(32.0)


def philox_key(s1, s2, s3):
    """(k0, k1) of the stream from an abc_rng state"""
    s1, s2, s3 = int(s1) & 0xFFFFFFFF, int(s2) & 0xFFFFFFFF, int(s3) & 0xFFFFFFFF
    return s1 ^ 0x5BD1E995, s2 ^ ((s3 * 0x9E3779B1) & 0xFFFFFFFF)


def philox4x32_10(ctr, k0, k1):
    """ctr: (4, ...) array of 32-bit words (any integer dtype) -> (4, ...) uint64 array of the output words"""
    c = [np.asarray(w, dtype=np.uint64) & M32 for w in ctr]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c)


def _ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return np.spacing(np.maximum(x, np.float32(np.finfo(np.float32).tiny))).astype(np.float64)


def _pair(ru, ra):
    """one Box-Muller pair: (z_cos, z_sin, unit) with unit the first-order error of the hardware steps"""
    s = ru.astype(np.float64).astype(np.float32) + _HALF                      # (float)ru + 0.5f: two f32 roundings
    l32 = np.log2(s.astype(np.float64)).astype(np.float32)                    # v_log_f32, correctly rounded here
    lg = l32 - _TWO32                                                         # - 32.0f
    t = np.maximum(_NEG2LN2 * lg, np.float32(0.0)).astype(np.float64)        # fmax(NEG2LN2 * lg, 0)
    rad = np.sqrt(t)
    ang = (ra >> np.uint64(8)).astype(np.float64) * 2.0 ** -24              # revolutions, exact
    c, sn = np.cos(2.0 * np.pi * ang), np.sin(2.0 * np.pi * ang)
    # one ulp of the logarithm's output, carried through the f32 product (plus its rounding) and the square root, where the
    # derivative grows without bound as t -> 0 (the top of the range): bounded by the square roots of the interval's ends
    e_t = 1.3862943611198906 * _ulp32(l32) + _ulp32(t)
    e_rad = np.maximum(np.sqrt(t + e_t) - rad, rad - np.sqrt(np.maximum(t - e_t, 0.0))) + rad * 2.0 ** -24
    unit = e_rad + rad * 2.0 ** -22                                           # + the sine / cosine and the final product
    return rad * c, rad * sn, unit


def normal4_ref(words):
    """words: (4, ...) Philox output words -> (z_ref, zbound), both (4, ...): the four deviates normal4 makes of them"""
    w = np.asarray(words, dtype=np.uint64)
    z0, z1, u0 = _pair(w[0], w[1])
    z2, z3, u1 = _pair(w[2], w[3])
    z = np.stack([z0, z1, z2, z3])
    return z, ZB_MULT * np.stack([u0, u0, u1, u1])


def c_round(x):
    """C round(): half away from zero, exactly"""
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0.0)


def _gauss_units(a, b, v):
    """(c, e): the reference's Gaussian likelihood is c exp(-u^2 / 2) with c = 1 / (sqrt(2 pi) |b|) in double, as d_valid
    computes it; e = exp(-u^2 / 2) in units of 2^-1074 (the smallest subnormal), in long double (no underflow)"""
    u = (np.asarray(v, dtype=np.longdouble) - np.longdouble(a)) / np.longdouble(abs(b))
    c = 1.0 / (np.sqrt(2.0 * np.pi) * abs(b))
    return np.longdouble(c), np.exp(-u * u / 2) * np.longdouble(2.0) ** 1074


def recast_valid(prior, v, tol):
    """(recast value, valid, ambiguous) of candidates v (float64 array) with error bounds tol, for one prior (kind, a, b):
    d_recast + d_valid.  Ambiguous: the device's candidate may fall on the other side of a support or rounding edge"""
    kind, a, b = int(prior[0]), float(prior[1]), float(prior[2])
    if kind == GAUSS:
        # near |u| ~ 38.6 the double exp returns a subnormal, quantised at 2^-1074, and the product c exp rounds to zero below
        # half of that: valid iff c rint(e) > 1/2.  The edge is known to within one unit of the exponential's subnormal result
        # (the device's exp may round the other way): ambiguous when one unit either side changes the verdict
        c, e = _gauss_units(a, b, v)
        half = np.longdouble(0.5)
        ok = c * np.rint(e) > half
        amb = (c * np.floor(e * (1 - 1e-6)) > half) != (c * np.ceil(e * (1 + 1e-6)) > half)
        return v, ok, amb
    if kind == UNIF_INT:
        r = c_round(v)
        amb = np.abs(np.abs(v - np.trunc(v)) - 0.5) <= tol
        return r, (a <= r) & (r <= b), amb
    return v, (a <= v) & (v <= b), (np.abs(v - a) <= tol) | (np.abs(v - b) <= tol)


def prior_mean(prior):
    kind, a, b = int(prior[0]), float(prior[1]), float(prior[2])
    return a if kind == GAUSS else (b + a) / 2.0


def _ulp64(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)))


def _counters(gi, attempt, w):
    gi = np.asarray(gi, dtype=np.uint64)
    return (gi & M32, gi >> np.uint64(32), np.full(gi.shape, attempt, dtype=np.uint64),
            np.full(gi.shape, w, dtype=np.uint64))


def mv_noise_ref(key, gi, attempt, L):
    """(L z, tol of L z, z, zbound) for rows gi at one attempt; L: (P, P), its lower triangle is used"""
    k0, k1 = key
    P = L.shape[0]
    nq = (P + 3) // 4
    zs, zb = [], []
    for qd in range(nq):
        z, b = normal4_ref(philox4x32_10(_counters(gi, attempt, qd), k0, k1))
        zs.append(z)
        zb.append(b)
    z = np.concatenate(zs)[:P]          # (P, n)
    zb = np.concatenate(zb)[:P]
    Lt = np.tril(np.asarray(L, dtype=np.float64))
    x = (Lt.astype(np.longdouble) @ z.astype(np.longdouble)).astype(np.float64)
    aL = np.abs(Lt)
    tol = aL @ zb + P * 2.0 ** -52 * (aL @ np.abs(z))          # hardware deviates + the fma chain's roundings
    return x, tol, z, zb


def indep_noise_ref(key, gi, attempt, p, sigma):
    k0, k1 = key
    z, b = normal4_ref(philox4x32_10(_counters(gi, attempt, 0x80000000 | p), k0, k1))
    return sigma * z[0], abs(sigma) * b[0] + _ulp64(sigma * z[0]), z[0], b[0]


def proposals_ref(key, theta, parent, priors, L_or_dv, multivariate, i0, n, max_attempts=None):
    """What abc_perturb_dev returns for rows i0 .. i0 + n - 1, given the parents of those rows.

    key: (k0, k1) (philox_key); theta: (K, P); parent: (n,) row indices; priors: P (kind, a, b); L_or_dv: (P, P) factor
    (multivariate) or (P,) doubled variances.  Returns dict: x (n, P) proposals, tol (n, P) bound on |x_dev - x| for the
    accepted candidate (0 on integer coordinates and kept parents / prior means), attempt (n,) the accepting attempt (-1: the
    row gave up; independent noise: the largest over the coordinates), ambiguous (n,) bool, giveups (count as the device
    counts them: one per row multivariate, one per coordinate independent)."""
    theta = np.asarray(theta, dtype=np.float64)
    parent = np.asarray(parent, dtype=np.int64)[:n]
    P = theta.shape[1]
    mu = theta[parent]                                   # (n, P)
    gi = np.uint64(i0) + np.arange(n, dtype=np.uint64)
    x = np.zeros((n, P))
    tol = np.zeros((n, P))
    att = np.full(n, -1, dtype=np.int64)
    amb = np.zeros(n, dtype=bool)
    giveups = 0
    if multivariate:
        tries = MVN_MAX_TRIES if max_attempts is None else max_attempts
        pend = np.arange(n)
        for attempt in range(tries):
            if pend.size == 0:
                break
            nz, ntol, _, _ = mv_noise_ref(key, gi[pend], attempt, L_or_dv)
            ok = np.ones(pend.size, dtype=bool)
            cand = np.empty((pend.size, P))
            ctol = np.empty((pend.size, P))
            for a in range(P):
                v = nz[a] + mu[pend, a]
                t = ntol[a] + 4.0 * _ulp64(v)
                r, good, am = recast_valid(priors[a], v, t)
                cand[:, a] = r
                ctol[:, a] = np.where(int(priors[a][0]) == UNIF_INT, 0.0, t)
                ok &= good
                amb[pend] |= am
            x[pend[ok]] = cand[ok]
            tol[pend[ok]] = ctol[ok]
            att[pend[ok]] = attempt
            pend = pend[~ok]
        x[pend] = mu[pend]                               # give up: keep the parent
        giveups = int(pend.size)
    else:
        tries = INDEP_MAX_TRIES if max_attempts is None else max_attempts
        dv = np.asarray(L_or_dv, dtype=np.float64)
        att[:] = 0
        for p in range(P):
            sigma = np.sqrt(dv[p])
            isint = int(priors[p][0]) == UNIF_INT
            pend = np.arange(n)
            for attempt in range(tries):
                if pend.size == 0:
                    break
                nz, ntol, _, _ = indep_noise_ref(key, gi[pend], attempt, p, sigma)
                v = nz + mu[pend, p]
                t = ntol + 4.0 * _ulp64(v)
                r, good, am = recast_valid(priors[p], v, t)
                amb[pend] |= am
                x[pend[good], p] = r[good]
                tol[pend[good], p] = 0.0 if isint else t[good]
                att[pend[good]] = np.maximum(att[pend[good]], attempt)
                pend = pend[~good]
            x[pend, p] = prior_mean(priors[p])           # give up: the prior mean
            att[pend] = -1
            giveups += int(pend.size)
    return dict(x=x, tol=tol, attempt=att, ambiguous=amb, giveups=giveups)
