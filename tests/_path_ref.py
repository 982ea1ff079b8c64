"""NumPy reference of the tolerance path (include/abcsmc_hip.h, abc_rank_targets_path_dev): the adjustment's definition applied
to the first K_t rows of one ranking at K_max, for every tolerance K_t of an ascending list.  Rows e >= K_t are never read for
tolerance t."""
import numpy as np

import _loclinear_ref as R

LD = np.longdouble


def path(dist, S_rows, o, theta_rows, Ks, kernel=0, A=None):
    """one target: dist (K_max,), S_rows (K_max, nc), o (nc,), theta_rows (K_max, P) in ranking order; Ks strictly ascending with
    Ks[-1] == K_max.  Returns dict(post_mean (T, P), coef (T, A + 1, P), rank (T,), status (T,), h (T,)); post_mean in
    np.longdouble (the exact mean to that precision), the rest as R.loclinear gives them."""
    dist = np.asarray(dist, dtype=np.float64)
    S_rows = np.asarray(S_rows, dtype=np.float64)
    theta_rows = np.asarray(theta_rows, dtype=np.float64)
    Ks = [int(k) for k in Ks]
    assert Ks[0] >= 1 and all(a < b for a, b in zip(Ks, Ks[1:])) and Ks[-1] == dist.size
    pm, coef, rank, status, h = [], [], [], [], []
    for K in Ks:
        r = R.loclinear(dist[:K], S_rows[:K], o, theta_rows[:K], kernel=kernel, A=A)
        pm.append(theta_rows[:K].astype(LD).sum(axis=0) / LD(K))
        coef.append(r["coef"])
        rank.append(r["rank"])
        status.append(r["status"])
        h.append(dist[K - 1])
    return dict(post_mean=np.array(pm), coef=np.array(coef), rank=np.array(rank, dtype=np.int32),
                status=np.array(status, dtype=np.int32), h=np.array(h))
