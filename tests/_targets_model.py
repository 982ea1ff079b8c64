"""The batched-targets selection (abcsmc_amd/csrc/targets.hip, launch_rank_targets) twice over, numpy only:

  * a copy of the HOST decisions -- tg_kc, tg_rpt, tg_plan, tg_chunk, the target groups of a chunk, tg_sample_row and which kernel
    scores the rows -- so that a test can state the branch it means to reach and check that it does (launch_plan);
  * an exact model of ONE target's selection on the device (select_model): the order-preserving keys, the sorted sample, the threshold
    key, the candidate set, the bins and the three conditions under which the device gives the target to the exact single-target
    path.  All of it is integer work on the keys of the reference distances, which come from a promised operation order, so the
    model predicts per target whether ctx.targets_fallbacks() rises.

tests/test_targets_model_cpu.py holds the copy to the text of targets.hip and pins it on both sides of every threshold;
tests/test_gpu_targets_branches.py asserts through it what each case reaches.

Reference distances (independent of the device): z = (x - mean) / sd with true division, 0 where sd == 0; scores are the
m-ascending fma chains against R (targets: _pls_ref.fma_dot; rows: the oracle's projection, in the GPU tests); d2 the k-ascending
fma chain of (s_k - o_k)^2 over k < ncomp; sqrt.  With one metric and one component every fma has one non-zero term, so plain
numpy is exact (m1_distances) and thousands of targets are cheap.

Not reachable through the public entry, and so asserted nowhere:
  * `bc < 1` in tg_chunk (one target's buffers beyond 512 MiB) needs C >= 22.4e6 rows' worth of candidates: a set of that size is
    not a test shape;
  * `p.C < K` in tg_plan: cap >= f N + 256 > K whenever the plan is sampled (q + 1 > f S), so the clamp never binds;
  * a threshold key below the key of +0 (t2 = -1) needs a NaN with the sign bit set among the sample's distances; the device's
    NaNs from finite or NaN inputs carry no sign bit."""
import numpy as np

TG_S = 4096                     # sampled rows
TG_NB = 2048                    # linear bins per target
TG_CAP = 1024                   # keys one work-group sorts
TG_CSTRIDE = 32                 # words between two targets' candidate counters
TG_CHUNK_BYTES = 512 << 20      # candidate buffers of one chunk of targets
ROW_BLOCKS = 4096               # the clamp of the grid-stride kernels k_tg_row_scores and k_tg_dist_one (256 rows per work-group)
KERNELS = ("k_tg_scores", "k_tg_row_scores", "k_tg_sample", "k_tg_threshold", "k_tg_cand", "k_tg_bins", "k_tg_sort",
           "k_tg_dist_one", "k_tg_drop", "k_tg_post_mean")
KCS = (1, 2, 4, 8, 16, 32, 0)   # the instances of k_tg_cand (0: more than 32 components, read as needed)

U64 = np.uint64
PAD = (1 << 64) - 1             # the key of an excluded or absent sample row
SIGN = 1 << 63
KEY_ZERO = SIGN                 # key of +0.0
KEY_INF = SIGN | 0x7FF0000000000000
ROW_SCORES = ("row_scores",)    # k_tg_row_scores, where launch_project_distance_scores declines


# ---- the host decisions ----------------------------------------------------------------------------------------------------------
def tg_kc(A):
    """the padded component count k_tg_cand holds in registers; 0: more than 32, read from the scores as they are needed"""
    if A > 32:
        return 0
    kc = 1
    while kc < A:
        kc *= 2
    return kc


def tg_kco(A):
    return tg_kc(A) or A


def tg_rpt(kc):
    """rows per thread of the candidate pass: as many as 32 score registers hold, at most four"""
    return 1 if (kc == 0 or kc >= 32) else min(32 // kc, 4)


def tg_plan(N, K, any_excl):
    """-> (ns, q, C): sampled rows, rank of the threshold among them, candidate capacity per target (doubles, truncation)"""
    ns = N if N < TG_S else TG_S
    Kx = K + (1 if any_excl else 0)
    if ns == N:
        return ns, K - 1, N
    f = float(Kx) / float(N)
    qd = f * TG_S + 4.0 * float(np.sqrt(np.float64(TG_S * f * (1.0 - f)))) + 8.0
    q = TG_S - 1 if qd >= float(TG_S - 1) else int(qd)
    frac = (q + 1.0) / TG_S + 8.0 * float(np.sqrt(np.float64(q + 1.0))) / TG_S
    cap = frac * float(N) + 256.0
    C = N if cap >= float(N) else int(cap)
    if C < K:
        C = K
    return ns, q, C


def tg_chunk(C, B):
    """targets per chunk"""
    per = C * 24 + (TG_NB + 1) * 4
    bc = TG_CHUNK_BYTES // per
    if bc < 1:
        bc = 1
    return min(bc, B)


def tg_groups(N, kc, nb):
    """the target groups of a chunk of nb targets -> dict(rb, groups, tgs, last): row blocks of the candidate pass, groups
    (blockIdx.y), targets per group, targets of the last group (last < tgs: ragged, b1 clipped)"""
    rows = 256 * tg_rpt(kc)
    rb = (N + rows - 1) // rows
    groups = 1 if rb >= 2048 else (2048 + rb - 1) // rb
    if groups > nb:
        groups = nb
    tgs = (nb + groups - 1) // groups
    groups = (nb + tgs - 1) // tgs
    return {"rb": rb, "groups": groups, "tgs": tgs, "last": nb - (groups - 1) * tgs}


def tg_sample_row(j, n, ns):
    if ns == n:
        return j
    stride = n // ns
    return j * stride + stride // 2


def sample_rows(n, ns):
    """tg_sample_row(j, n, ns) for every j < ns"""
    j = np.arange(ns, dtype=np.int64)
    if ns == n:
        return j
    stride = n // ns
    return j * stride + stride // 2


def scoring_kernel(N, ldx, x_aligned, M, A):
    """the kernel that scores the rows: launch_project_distance_scores' (row_test = 0, the scores' leading dimension N; dist and S
    come from the arena, on 16-byte boundaries) or ROW_SCORES where it declines"""
    from _project_dispatch import NOT_A_SHAPE, fused_plan
    k = fused_plan(N, ldx, x_aligned, M, A, 0, N)
    return ROW_SCORES if k == NOT_A_SHAPE else k


def launch_plan(N, M, A, B, K, any_excl, ldx=None, x_aligned=True):
    """everything launch_rank_targets decides on the host for one call"""
    ldx = N if ldx is None else ldx
    kc = tg_kc(A)
    ns, q, C = tg_plan(N, K, any_excl)
    bc = tg_chunk(C, B)
    chunks = []
    for c0 in range(0, B, bc):
        nb = min(B - c0, bc)
        chunks.append(dict(tg_groups(N, kc, nb), c0=c0, nb=nb))
    blocks = min((N + 255) // 256, ROW_BLOCKS)
    scoring = scoring_kernel(N, ldx, x_aligned, M, A)
    return {"kc": kc, "kco": kc or A, "rpt": tg_rpt(kc), "plan": "exact" if ns == N else "sampled", "ns": ns, "q": q, "C": C,
            "bc": bc, "chunks": chunks, "nchunks": len(chunks), "scoring": scoring,
            "groups": sorted({c["groups"] for c in chunks}), "ragged": any(c["last"] < c["tgs"] for c in chunks),
            # a thread of k_tg_row_scores (if it runs) and of k_tg_dist_one (if a target gives up) takes a second trip
            "second_trip": N > blocks * 256}


# ---- keys --------------------------------------------------------------------------------------------------------------------------
def key_of(d):
    """the order-preserving uint64 key of a double (tg_key), elementwise"""
    b = np.ascontiguousarray(d, dtype=np.float64).view(U64)
    return np.where(b >> U64(63), ~b, b | U64(SIGN))


def dist_of(k):
    """tg_dist: the double of a key"""
    k = np.ascontiguousarray(k, dtype=U64)
    b = np.where(k >> U64(63), k & U64(SIGN - 1), ~k)
    return b.view(np.float64)


def canonical(d):
    """the distances with every NaN the positive quiet one, which is what the device's arithmetic makes of a NaN input"""
    d = np.array(d, dtype=np.float64)
    d[np.isnan(d)] = np.float64(np.nan)
    b = d.view(U64)
    b[np.isnan(d)] = U64(0x7FF8000000000000)
    return d


def t2_of(tkey):
    """k_tg_threshold's conservative bound of the squared distance at the threshold key"""
    tkey = int(tkey)
    if tkey >= KEY_INF:
        return np.float64(np.inf)
    if tkey < KEY_ZERO:
        return np.float64(-1.0)
    td = dist_of(np.array([tkey], dtype=U64))[0]
    with np.errstate(over="ignore", under="ignore"):
        u = np.nextafter(td, np.inf)
        return np.nextafter(np.nextafter(u * u, np.inf), np.inf)


def prefilter(d2, t2):
    """k_tg_cand's first test on the squared distance: at or below the bound, or NaN"""
    d2 = np.asarray(d2, dtype=np.float64)
    return (d2 <= t2) | np.isnan(d2)


# ---- one target's selection --------------------------------------------------------------------------------------------------------
def select_detail(d, K, excl=None, any_excl=None):
    """the device's selection of the K smallest of the N distances d, the row excl left out (None: none; any_excl: some target of
    the call excludes a row, which is what the plan looks at -- default: this one does) -> dict(verdict, c, C, maxbin, tkey, lo0,
    lo, shift, hist, offs, bstar, need, cand, keys)"""
    keys = key_of(canonical(d))
    N = keys.size
    any_excl = (excl is not None) if any_excl is None else any_excl
    assert excl is None or any_excl
    ns, q, C = tg_plan(N, K, any_excl)
    rows = sample_rows(N, ns)
    sk = np.full(TG_S, PAD, dtype=U64)
    sk[:ns] = keys[rows]
    if excl is not None:
        sk[:ns][rows == excl] = U64(PAD)
    sk.sort()
    tkey, lo0 = int(sk[q]), int(sk[0])
    cand = keys <= U64(tkey)
    if excl is not None:
        cand[excl] = False
    cand = np.flatnonzero(cand)
    c = int(cand.size)
    out = {"c": c, "C": C, "maxbin": 0, "tkey": tkey, "lo0": lo0, "cand": cand, "keys": keys, "ns": ns, "q": q}
    if c > C:
        return dict(out, verdict="overflow")
    if c < K:
        return dict(out, verdict="short")
    span = tkey - lo0
    room = lo0 - KEY_ZERO if lo0 > KEY_ZERO else 0
    lo = lo0 - min(span, room)
    shift = 0
    while shift < 63 and ((tkey - lo) >> shift) >= TG_NB - 1:
        shift += 1
    ck = keys[cand]
    bins = np.where(ck <= U64(lo), U64(0), (ck - U64(lo)) >> U64(shift)).astype(np.int64)
    hist = np.bincount(bins, minlength=TG_NB + 1)
    assert hist.size == TG_NB + 1 and hist[TG_NB] == 0, "a key at or below the threshold beyond the last bin"
    offs = np.concatenate(([0], np.cumsum(hist)[:-1]))
    live = offs < K
    maxbin = int(hist[live].max())
    bstar = int(np.flatnonzero((offs < K) & (K <= offs + hist))[0])
    out.update(lo=lo, shift=shift, hist=hist, offs=offs, bins=bins, bstar=bstar, need=K - int(offs[bstar]), maxbin=maxbin)
    return dict(out, verdict="bin" if maxbin > TG_CAP else "ok")


def select_model(d, K, excl=None, any_excl=None):
    """-> (verdict, c, C, largest bin at or before the K-th key): "ok", or why the device gives the target to the exact path --
    "overflow" (c > C), "short" (c < K), "bin" (a bin above TG_CAP at or before the K-th key)"""
    s = select_detail(d, K, excl, any_excl)
    return s["verdict"], s["c"], s["C"], s["maxbin"]


def reference_order(d, excl=None):
    """rows ascending by (distance, row), the excluded row removed; NaN behind +inf"""
    order = np.argsort(key_of(canonical(d)), kind="stable")
    return order if excl is None else order[order != excl]


# ---- reference distances -----------------------------------------------------------------------------------------------------------
def tg_ncomp(header, A):
    """clamp(int(model[0]), 0, A), the conversion truncating"""
    nc = int(header)
    return 0 if nc < 0 else min(nc, A)


def zscore(x, mean, sd):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sd == 0, 0.0, (np.asarray(x, dtype=np.float64) - mean) / sd)


def target_scores(t, mean, sd, R, ncomp):
    """the observed scores of one target: m-ascending fma chains, each fma evaluated exactly"""
    from _pls_ref import fma_dot
    z = zscore(t, mean, sd)
    return np.array([fma_dot(z, R[:, k]) for k in range(ncomp)], dtype=np.float64)


def m1_scores(x, mean, sd, r):
    """one metric, one component: fma(z, r, 0) = the rounded product (a -0 product becomes +0)"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return zscore(x, mean, sd) * r + 0.0


def m1_distances(x, mean, sd, r, t, ncomp=1):
    """the N distances of the rows x to the target value t under one metric and one component"""
    x = np.asarray(x, dtype=np.float64)
    if ncomp == 0:
        return np.zeros(x.size)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        d = m1_scores(x, mean, sd, r) - m1_scores(np.float64(t), mean, sd, r)
        return np.sqrt(d * d + 0.0)


# ---- constructed inputs (one metric, one component, in z units: x = mean + sd z) -----------------------------------------------
def m1_record(seed):
    """-> (mean, sd, r) of a one-metric, one-component record, on no round scale"""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-3, 3)
    return np.float64(scale * rng.normal()), np.float64(scale * rng.uniform(0.5, 2.0)), np.float64(rng.choice([-1.0, 1.0]) *
                                                                                                  rng.uniform(0.5, 2.0))


def m1_x(z, mean, sd):
    """metric values whose z-scores are (about) z"""
    return mean + sd * np.asarray(z, dtype=np.float64)


def ordinary_rows(N, seed):
    return np.random.default_rng(seed).normal(size=N)


def split_rows(N, seed, far):
    """sampled plan, for a target at 0.  far="sample": the sampled rows lie 100 units farther than the others, so the threshold lets
    every other row through (c > C: "overflow").  far="others": the other rows lie 100 units farther, so only sampled rows pass, q + 1
    of them (c < K once K > q + 1: "short")."""
    ns, _, _ = tg_plan(N, 1, False)
    assert ns < N and far in ("sample", "others")
    z = np.random.default_rng(seed).uniform(0.5, 1.5, size=N)
    s = np.zeros(N, dtype=bool)
    s[sample_rows(N, ns)] = True
    z[s if far == "sample" else ~s] += 100.0
    return z


def tied_rows(N, ties, seed, at=0.25):
    """`ties` identical rows (every second one from row 1 on), the rest ordinary: a target at `at` has them as its nearest"""
    z = 3.0 + np.abs(np.random.default_rng(seed).normal(size=N))
    z[1:2 * ties:2] = at
    return z
