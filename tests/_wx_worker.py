"""The cases of tests/test_gpu_wilcoxon.py and the child process that runs them under the library's diagnostic switches
(ABC_WX_NOBOUNDS, ABC_WX_BC_CAP_KB: read once per process, so each setting needs a process of its own).

    python tests/_wx_worker.py OUTDIR CASE [CASE ...]

runs each case's reduction with the per-test record on and once more with it off, and writes OUTDIR/CASE.pkl (the model record
before and after, the record, the path).  The parent regenerates the data from the case's seed and computes the references.
"""
import os
import pickle
import sys

import numpy as np

# name -> (N, M, P, A, kind, seed, noise); half of the rows are validation rows
# the sorted path: validation rows either side of 256 and 512 (k_wx_ranksum's blocks), tie groups of three (one straddles every
# block edge: 3 x 85 = 255), a response constant on the validation rows, every KC of k_wx_scores (A = 2, 4, 8, 9, 20) and the wide
# kernel (A = 33, 40), one / two / twelve responses
CASES_SORTED = {
    "s255": (510, 6, 2, 2, "triples", 1, 1.5),
    "s256": (512, 6, 1, 4, "plain", 2, 1.5),
    "s257": (514, 10, 2, 9, "triples", 3, 1.5),
    "s511": (1022, 36, 1, 33, "plain", 44, 1.5),
    "s512": (1024, 44, 2, 40, "triples", 5, 1.5),
    "s513": (1026, 12, 12, 9, "const", 6, 1.5),
    "s771": (1542, 24, 2, 20, "skew", 7, 1.5),
    "s1000": (2000, 12, 3, 8, "grid", 8, 1.5),
    "s3000": (6000, 10, 12, 2, "pairs", 9, 1.5),
    "s513z": (1026, 10, 3, 6, "zeros", 10, 1.5),
}
# the cascade: 16 384 validation rows and just above (an odd count: the last row goes through k_wx_scores<KC>)
# c8_copies is the tie-heavy kind that sends bins of the exact step to k_wx_ranks_big, guaranteed by its data once a test gets to
# the exact step (every test does in the forced runs): 50 distinct validation rows make at most 50 distinct keys per test, each
# 327 or 328 times; the exact step has at most nbcap = 10 bins at 16 391 rows, so some bin holds two distinct keys or more, its
# keys are not all one value (k_wx_ranks ranks such a bin in place), and equal keys share a linear sub-bin -- 327 keys, above
# WX_WALK = 48, which is what hands the bin over (as a bin above WX_CAP_S = 4096 keys would).  test_cascade_small asserts those
# properties of the data.  c16_skew (tie groups of up to a few hundred keys among single ones) gets there as well, not by necessity.
CASES_CASCADE = {
    "c8_plain": (32782, 12, 8, 8, "plain", 11, 1.5),
    "c8_pairs": (32768, 12, 6, 8, "pairs", 12, 1.5),
    "c8_copies": (32782, 12, 6, 8, "copies50", 13, 1.5),
    "c8_grid": (32770, 12, 6, 8, "grid", 14, 1.5),
    "c16_plain": (32782, 20, 4, 16, "plain", 15, 1.5),
    "c16_skew": (32770, 20, 3, 16, "skew", 16, 1.5),
    "c32_plain": (32782, 36, 3, 32, "plain", 17, 1.5),
    "c32_pairs": (32768, 36, 2, 32, "pairs", 18, 1.5),
    "c8_const": (32782, 12, 6, 8, "const", 19, 1.5),
    "c8_zeros": (32778, 12, 6, 8, "zeros", 20, 1.5),
    # the validation scores from k_project_mfma<2> with the loadings in front of the observed scores in LDS (from 249 metrics on;
    # an even first validation row, so launch_project_scores takes them: tests/_project_dispatch.py, scores_plan)
    "c32_loadings": (32768, 249, 2, 17, "plain", 33, 1.5),
}
# many open tests (every test kept open: ABC_WX_NOBOUNDS), so that a fine level has enough groups of tests for two and four rows
# per thread at 65 537 validation rows (tests/_wx_dispatch.py)
CASES_MANY = {
    "a8_r2": (131074, 12, 16, 8, "plain", 21, 0.3),
    "a8_r4": (131074, 12, 32, 8, "plain", 22, 0.3),
    "a16_r2": (131074, 20, 8, 16, "plain", 23, 0.3),
}
# two distinct validation rows: tie groups of 16 385 and 16 386 keys outgrow a bin of the exact step (WX_CAP = 16 384) once a test
# gets there (forced), and the reduction repeats itself on the sorted path
# ... and one distinct validation row (16 391 copies): every test has ONE key, so all its differences have one sign and every level's
# interval of 2 W must be the point +- m (m + 1), whatever the bins
CASES_OUTGROW = {"c8_two_rows": (65542, 12, 3, 8, "copies2", 31, 1.5), "c8_one_row": (32782, 12, 6, 8, "copies1", 32, 1.5)}
# level 0 with two rows per thread: 191 x 2048 + 1 validation rows, one group of tests
CASES_LARGE = {"l8": (782338, 10, 2, 8, "plain", 41, 1.5), "l16": (782338, 18, 2, 16, "plain", 42, 1.5)}
CASES = dict(CASES_SORTED, **CASES_CASCADE, **CASES_MANY, **CASES_OUTGROW, **CASES_LARGE)


def make_data(name):
    """-> (X, Y, obs, A): a latent-factor set (A factors, loadings falling off by 0.8 per factor, columns rescaled), the kind's
    ties and constants put into the validation half"""
    N, M, P, A, kind, seed, noise = CASES[name]
    rng = np.random.default_rng(seed)
    r = min(A, 12)
    Lf = rng.normal(size=(N, r))
    Ax, Ay = rng.normal(size=(r, M)), rng.normal(size=(r, P)) * (0.8 ** np.arange(r))[:, None]
    X = Lf @ Ax + 0.3 * rng.normal(size=(N, M))
    Y = Lf @ Ay
    Y = Y + noise * Y.std(0) * rng.normal(size=(N, P))
    nt0 = N // 2
    nv = N - nt0
    if kind == "zeros":
        # Zero differences: integer metrics whose columns add up to exactly zero over the training rows and over the validation rows
        # (one row of each takes minus the others' sum) have a column mean of exactly zero however it is summed, so a validation
        # row of zeros has z-scores, scores and predictions of exactly zero: |e_a*| = |e_a'| for every test.  Forty such rows.
        X = np.round(2.0 * X)
        X[nt0:nt0 + 40] = 0.0
        X[0] -= X[:nt0].sum(0)
        X[nt0 + 100] -= X[nt0:].sum(0)
        assert not X[:nt0].sum(0).any() and not X[nt0:].sum(0).any()
        Y[nt0 + 40:nt0 + 50] = Y[nt0 + 30:nt0 + 40]
        return np.asfortranarray(X), np.asfortranarray(Y), X[0].copy(), A
    X = X * 10.0 ** rng.uniform(-1, 1, size=M) + rng.uniform(-3, 3, size=M)
    Y = Y * 10.0 ** rng.uniform(-1, 1, size=P) + rng.uniform(-3, 3, size=P)
    if kind == "grid":                                   # every value on a grid of a quarter of its column's deviation
        X = np.round(X / (0.25 * X.std(0))) * (0.25 * X.std(0))
        Y = np.round(Y / (0.25 * Y.std(0))) * (0.25 * Y.std(0))
    elif kind == "pairs":                                # every validation row twice
        src = nt0 + (np.arange(nv) // 2) * 2
        X[nt0:], Y[nt0:] = X[src], Y[src]
    elif kind == "triples":
        src = nt0 + (np.arange(nv) // 3) * 3
        X[nt0:], Y[nt0:] = X[src], Y[src]
    elif kind.startswith("copies"):                      # c distinct validation rows
        c = int(kind[6:])
        src = nt0 + (np.arange(nv) % c)
        X[nt0:], Y[nt0:] = X[src], Y[src]
    elif kind == "skew":                                 # tie groups of every size from one row to a few hundred
        src = nt0 + np.minimum((rng.random(nv) ** 3 * nv).astype(np.int64), nv - 1)
        X[nt0:], Y[nt0:] = X[src], Y[src]
    elif kind == "const":
        Y[nt0:, 0] = Y[nt0, 0]                           # a response constant on the validation rows
        if P > 1:
            Y[:, 1] = Y[:, 1].mean() + 1e-9 * rng.normal(size=N)       # ... and one that nothing predicts
    elif kind not in ("plain", "zeros"):
        raise ValueError(kind)
    return np.asfortranarray(X), np.asfortranarray(Y), X[0].copy(), A


def main(argv):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    import _wx_record
    from abcsmc_amd import _lib
    outdir, names = argv[1], argv[2:]
    ctx = _lib.default_context(0)
    for name in names:
        X, Y, obs, A = make_data(name)
        run = _wx_record.run_reduction(ctx, X, Y, obs, A, 0.5, record=True, both=True)
        tmp = os.path.join(outdir, name + ".tmp")
        with open(tmp, "wb") as fh:
            pickle.dump(run, fh)
        os.replace(tmp, os.path.join(outdir, name + ".pkl"))
        print("WX_WORKER", name, "path", run["path"], "tests", len(run["rec"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
