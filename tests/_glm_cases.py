"""Inputs and shapes shared by tests/test_glm_cpu.py and tests/test_gpu_glm.py.

The tables come from a linear-Gaussian model with fixed seeds: theta ~ N(mu, diag(s^2)) with s in [0.5, 2], metrics
X = theta Bx + 0.6 E with Bx ~ N(0, 1 / P), so that the parameters are nearly uncorrelated and the metrics' residuals about the
parameters are white: the condition numbers of M_thth and Sigma_s on the retained rows stay far below 1e4
(test_glm_cpu.test_gpu_cases_are_well_conditioned measures them with the CPU oracle's fit).

CASES: the shapes of the GPU test.  K in {P + 2, 63, 64, 65, 1025}, P in {1, 2, 16, 17, 32}, ncomp in {1, 8, 32}, B in {1, 3, 20},
G in {2, 257}; mode is what the case adds: "equal" weights, "weights" (row weights with zeros and one of 1e-300), "bw" (given
bandwidths), "exclude".  nc is the number of components the device entry is held to (the model's header is set to it); M >= nc."""
import numpy as np

import _loclinear_ref as LL


def table(N, M, P, seed):
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.5, 2.0, size=P)
    mu = rng.normal(size=P)
    Y = mu + s * rng.normal(size=(N, P))
    Bx = rng.normal(size=(P, M)) / np.sqrt(P)
    X = (Y - mu) @ Bx + 0.6 * rng.normal(size=(N, M)) + rng.normal(size=M)
    return np.asfortranarray(X), np.asfortranarray(Y)


#            name          N     M   P   nc  K     B   G    mode
CASES = [("p1_kmin",      600,   4,  1,  1,  3,    1,  2,   "equal"),
         ("p2_k63",       1500,  5,  2,  1,  63,   3,  257, "weights"),
         ("p16_k64",      1500,  12, 16, 8,  64,   20, 2,   "bw"),
         ("p17_k65",      1500,  12, 17, 8,  65,   3,  257, "exclude"),
         ("p32_k1025",    3000,  40, 32, 32, 1025, 3,  2,   "equal"),
         ("p2_kmin",      600,   4,  2,  1,  4,    3,  2,   "equal"),
         ("p2_k1025",     4000,  5,  2,  1,  1025, 1,  257, "weights")]
FIELDS = ("name", "N", "M", "P", "nc", "K", "B", "G", "mode")


def case(row):
    return dict(zip(FIELDS, row))


def inputs(c):
    """X, Y, targets (B, M), exclude (B,) or None, row weights (N,) or None, bw (B, P) or None of a case"""
    X, Y = table(c["N"], c["M"], c["P"], 1000 + c["K"] + c["P"])
    rows = (np.arange(c["B"]) * 37 + 5) % c["N"]
    targets = np.ascontiguousarray(X[rows]) + (0.0 if c["mode"] == "exclude" else 0.05)
    exclude = rows.astype(np.int64) if c["mode"] == "exclude" else None
    om = None
    if c["mode"] == "weights":
        om = np.random.default_rng(c["K"]).uniform(0.1, 1.0, size=c["N"])
        om[::7] = 0.0
        om[3::11] = 1e-300
    bw = None
    if c["mode"] == "bw":
        bw = np.random.default_rng(c["P"]).uniform(0.2, 0.6, size=(c["B"], c["P"]))
    return X, Y, targets, exclude, om, bw


def rank(X, mean, sd, R, nc, targets, K, exclude=None):
    """The ranking in NumPy from a fit's R, mean and sd: (idx (B, K) int64, S (N, nc) the rows' scores, O (B, nc) the targets')"""
    S = LL.scores(X, mean, sd, R, nc)
    O = LL.scores(targets, mean, sd, R, nc)
    idx = np.empty((O.shape[0], K), dtype=np.int64)
    for b in range(O.shape[0]):
        d = np.sqrt(((S - O[b]) ** 2).sum(axis=1))
        if exclude is not None and exclude[b] >= 0:
            d[exclude[b]] = np.inf
        idx[b] = np.argsort(d, kind="stable")[:K]
    return idx, S, O
