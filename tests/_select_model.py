"""The selection of the K smallest distances (abcsmc_amd/csrc/select.hip, launch_select_smallest) twice over, numpy only:

  * a copy of the HOST decisions -- which path launch_select_smallest takes from (n, K, force_radix), inside the radix path K == n
    (k_init_pairs) against the six-pass select, which sort sort_pairs_u64 runs, and the grid clamps (the 512 histogram blocks, the
    CP_CHUNK blocks and 256-wide slabs of k_scan_u32, the ST_CHUNK blocks and `per` of k_sort_scan) -- so that a test can state the
    branch it means to reach and check that it does;
  * an exact model of ONE bin selection on the order-preserving keys (bin_model): the 4096 sample rows, q in the doubles of
    k_bs_sample (the library is built with -ffp-contract=off -fno-fast-math, plain Python doubles give the same value), hi (the top
    24 bits of the q-th sample key, 40 ones below), lo, shift, the bin of every key, the counts, b*, need and the verdict: "ok",
    "overflow" (a bin at or below b* holds more than BS_CAP keys) or "short" (fewer than K keys at or below hi).  The verdict says
    whether Context.select_stats() counts a give-up for a call of abc_select_smallest_dev.

tests/test_select_model_cpu.py holds the copy to the text of select.hip and pins it on both sides of every threshold;
tests/test_gpu_select_branches.py asserts through it what each case reaches.  The constructed inputs of both live here (CASES).

Contract: the reference order is the stable argsort of the keys, which is ascending (distance, row).  It covers non-negative,
non-NaN doubles, +0, subnormals, 1e308 and +inf included.  -0 and NaN are outside it and asserted nowhere.

Not reachable through the public entry, and so asserted nowhere:
  * the clamp q = BS_S - 1 in k_bs_sample: the bin path needs 2 K <= n, so f <= 1/2 and qd <= 2048 + 128 + 8 = 2184;
  * `shift < 63` in k_bs_sample: nbins - 1 >= 4095, so the loop ends at shift <= 53 for any 64-bit span;
  * a bin index at or beyond nbins - 1: a counted key is at most hi and (hi - lo) >> shift < nbins - 1;
  * K <= 2^20 failing while 2 K <= n holds needs n > 2^21 (reached: the radix case K = 2^20 + 1), K > 2^32 of the counters never."""
import math

import numpy as np

BS_NB = 4096
BS_NB_BIG = 16384
BS_S = 4096
BS_CAP = 1024
SC_N = 4096
SC_MAX_N = 1 << 18
CP_CHUNK = 2048
ST_CHUNK = 2048
HIST_BLOCKS = 512               # the clamp of k_bs_hist, k_sel_hist and k_sel_hist_fused (256 keys per work-group and round)
BIG_K = 1 << 18                 # beyond it the bin path takes BS_NB_BIG bins
MAX_BIN_K = 1 << 20             # beyond it the radix path
IDX_LIMIT = 1 << 48             # idx_base + n may not exceed it (k_sort_chunks keeps an element's position in the top 16 bits)

U64 = np.uint64
SIGN = 1 << 63
ONES40 = (1 << 40) - 1
KEY_ONE = SIGN | 0x3FF0000000000000      # key of 1.0


# ---- keys ------------------------------------------------------------------------------------------------------------------------
def keys_of(d):
    """key_of of select.hip: the IEEE bit pattern as an order-preserving uint64"""
    b = np.ascontiguousarray(d, dtype=np.float64).view(U64)
    return np.where(b >> U64(63) != 0, ~b, b | U64(SIGN))


def dists_of(k):
    """dist_of of select.hip"""
    k = np.ascontiguousarray(k, dtype=U64)
    b = np.where(k >> U64(63) != 0, k & U64(SIGN - 1), ~k)
    return b.view(np.float64)


def reference_order(d):
    """ascending (distance, row): the stable argsort of the keys"""
    return np.argsort(keys_of(d), kind="stable")


# ---- the host decisions ----------------------------------------------------------------------------------------------------------
def select_path(n, K, force_radix=False):
    """launch_select_smallest: "bins/4096", "bins/16384" or "radix" """
    bins = (not force_radix) and n >= 4 * BS_S and 2 * K <= n and K <= MAX_BIN_K
    if not bins:
        return "radix"
    return "bins/4096" if K <= BIG_K else "bins/16384"


def radix_plan(n, K):
    """select_by_radix: every key kept (k_init_pairs) or the six histogram passes, count, scan and write"""
    return "init_pairs" if K == n else "six_pass"


def sort_plan(n):
    """sort_pairs_u64 on the whole key: "none", "chunk" (one k_sort_chunks), "chunks+merge" or "lsd" (eight radix passes)"""
    if n <= 1:
        return "none"
    if n <= SC_MAX_N:
        return "chunk" if (n + SC_N - 1) // SC_N == 1 else "chunks+merge"
    return "lsd"


def merge_rounds(n):
    """rounds of eight chunks a thread of k_merge_chunks searches"""
    return ((n + SC_N - 1) // SC_N + 7) // 8


def hist_blocks(n):
    return min((n + 255) // 256, HIST_BLOCKS)


def cp_blocks(n):
    return (n + CP_CHUNK - 1) // CP_CHUNK


def scan_slabs(m):
    """256-wide slabs k_scan_u32 walks over m counters"""
    return (m + 255) // 256


def st_blocks(n):
    return (n + ST_CHUNK - 1) // ST_CHUNK


def st_per(nb):
    """block counts one thread of k_sort_scan adds"""
    return (nb + 255) // 256


def launch_plan(n, K, force_radix=False):
    """what one call of abc_select_smallest_dev reaches, by the host's arithmetic alone"""
    path = select_path(n, K, force_radix)
    plan = {"path": path, "hist_blocks": hist_blocks(n), "hist_clamped": (n + 255) // 256 > HIST_BLOCKS}
    if path == "radix":
        plan.update(radix=radix_plan(n, K), sort=sort_plan(K), cp_blocks=cp_blocks(n), scan_slabs=scan_slabs(cp_blocks(n)))
        if plan["sort"] == "lsd":
            plan.update(st_blocks=st_blocks(K), st_per=st_per(st_blocks(K)))
        if plan["sort"] == "chunks+merge":
            plan.update(merge_rounds=merge_rounds(K))
    else:
        plan.update(nbins=BS_NB if path == "bins/4096" else BS_NB_BIG)
    return plan


# ---- one bin selection -----------------------------------------------------------------------------------------------------------
def sample_rows(n):
    """the rows k_bs_sample reads: (t + 1024 j) stride + stride / 2 over t < 1024, j < 4, i.e. every i < 4096"""
    stride = n // BS_S
    return np.arange(BS_S, dtype=np.int64) * stride + stride // 2


def sample_q(n, K):
    """rank (0-based) of the upper key among the samples, in the doubles of k_bs_sample"""
    f = float(K) / float(n)
    qd = f * BS_S + 4.0 * math.sqrt(BS_S * f * (1.0 - f)) + 8.0
    return BS_S - 1 if qd >= float(BS_S - 1) else int(qd)


def bin_model(d, K, nbins=None):
    """-> dict: q, lo, hi, shift, bins (per key; -1: above hi, not counted), counts, offs, tot, bstar, need (None when tot < K),
    crowded (bins at or below b* beyond BS_CAP), verdict"""
    k = keys_of(d)
    n = k.size
    if nbins is None:
        nbins = BS_NB if K <= BIG_K else BS_NB_BIG
    sk = np.sort(k[sample_rows(n)])
    q = sample_q(n, K)
    lo = int(sk[0])
    hi = (int(sk[q]) & ~ONES40) | ONES40
    span = hi - lo
    shift = 0
    while shift < 63 and (span >> shift) >= nbins - 1:
        shift += 1
    counted = k <= U64(hi)
    rel = np.where(k <= U64(lo), U64(0), k - U64(lo)) >> U64(shift)
    bins = np.where(counted, rel, U64(0)).astype(np.int64)
    assert bins.max() < nbins - 1 or not counted.any()
    bins[~counted] = -1
    counts = np.bincount(bins[counted], minlength=nbins).astype(np.int64)
    offs = np.concatenate(([0], np.cumsum(counts)))
    tot = int(offs[-1])
    out = {"q": q, "lo": lo, "hi": hi, "shift": shift, "nbins": nbins, "bins": bins, "counts": counts, "offs": offs, "tot": tot,
           "bstar": None, "need": None, "crowded": []}
    over = (offs[:-1] < K) & (counts > BS_CAP)
    out["crowded"] = np.nonzero(over)[0].tolist()
    if tot >= K:
        bstar = int(np.nonzero((offs[:-1] < K) & (K <= offs[1:]))[0][0])
        out["bstar"], out["need"] = bstar, K - int(offs[bstar])
    out["verdict"] = "overflow" if over.any() else ("short" if tot < K else "ok")
    return out


def expected_stats(path, verdict):
    """what one call adds to (bin selections, bin give-ups)"""
    if path == "radix":
        return (0, 0)
    return (1, 0) if verdict == "ok" else (1, 1)


# ---- constructed inputs ----------------------------------------------------------------------------------------------------------
# The key-exact cases live in the binade of 1.0: a key is KEY_ONE + o with an offset o < 2^40, so every key shares its top 24 bits,
# hi = KEY_ONE + 2^40 - 1 whatever q is, and with lo = KEY_ONE the span 2^40 - 1 gives shift = 29 under 4096 bins: the bin of a key
# is o >> 29 (2048 bins in use), the key hi itself is offset 2^40 - 1 of bin 2047 and hi + 1 is 1.0 + 2^-12.
FLAT_SHIFT = 29
FLAT_W = 1 << FLAT_SHIFT
FLAT_BINS = 1 << (40 - FLAT_SHIFT)


def flat(offsets):
    """offsets from the key of 1.0 (any sign) -> distances"""
    return dists_of((np.asarray(offsets, dtype=np.int64) + np.int64(KEY_ONE - SIGN)).astype(U64) | U64(SIGN))


def _in_bin(rng, b, cnt):
    """cnt distinct offsets of flat bin b"""
    low = rng.choice(FLAT_W - 2, size=cnt, replace=False) + 1          # (never a bin's first or last offset: those are placed by hand)
    return b * FLAT_W + low.astype(np.int64)


def _place(n, on_sample, elsewhere, rng):
    """distances with `on_sample` (BS_S values) on the sample rows and `elsewhere` (n - BS_S values) on the others, both shuffled"""
    on_sample, elsewhere = np.asarray(on_sample, dtype=np.float64), np.asarray(elsewhere, dtype=np.float64)
    assert on_sample.size == BS_S and elsewhere.size == n - BS_S
    d = np.empty(n)
    rows = sample_rows(n)
    mask = np.zeros(n, dtype=bool)
    mask[rows] = True
    d[rows] = rng.permutation(on_sample)
    d[~mask] = rng.permutation(elsewhere)
    return d


def _split(vals, n_sample, rng):
    vals = rng.permutation(np.asarray(vals))
    return vals[:n_sample], vals[n_sample:]


def _flat_case(n, K, small, big, rng, pin_sample=(0,)):
    """`small`: flat offsets (keys at or below hi), `big`: distances above hi.  3000 of the sample rows hold small keys (q <= 2184
    for any K of the bin path), the offsets of pin_sample among them (offset 0: lo is the key of 1.0)."""
    small = np.asarray(small, dtype=np.int64)
    pin = np.asarray(pin_sample, dtype=np.int64)
    rest = small.copy()
    for p in pin:
        rest = np.delete(rest, np.nonzero(rest == p)[0][0])
    s_on, s_off = _split(rest, 3000 - pin.size, rng)
    b_on, b_off = _split(big, BS_S - 3000, rng)
    return _place(n, np.concatenate((flat(pin), flat(s_on), b_on)), np.concatenate((flat(s_off), b_off)), rng), K


def chi(rng, n):
    return np.sqrt((rng.normal(size=(n, 8)) ** 2).sum(axis=1))


def lognormal(rng, n):
    return np.exp(3.0 * rng.normal(size=n))


def _big(rng, m):
    return 2.0 + 1e6 * rng.random(m)


def case_kth_last_eq_hi(n=16384, K=8192):
    """four keys in each of the 2048 flat bins: exactly K keys at or below hi (tot == K), the K-th key is the last of bin 2047 and
    equals hi; hi + 1 sits on 40 rows and stays out"""
    rng = np.random.default_rng(101)
    small = np.concatenate([_in_bin(rng, b, 4) for b in range(FLAT_BINS)])
    small[-1] = (1 << 40) - 1                                           # the key hi itself
    small[0] = 0
    big = _big(rng, n - K)
    big[:40] = flat([1 << 40])[0]                                       # hi + 1
    return _flat_case(n, K, small, big, rng)


def case_kth_first_K1(n=16384, K=1):
    """K = 1: the smallest key is the first of bin 0, which holds 200 more; need == 1"""
    rng = np.random.default_rng(102)
    small = np.concatenate([[0], _in_bin(rng, 0, 200)] + [_in_bin(rng, b, 3) for b in range(1, FLAT_BINS)])
    return _flat_case(n, K, small, _big(rng, n - small.size), rng)


def case_kth_first_mid(n=16384, K=3001):
    """3000 keys in bins 0..599, then bin 700 with 300 keys: the K-th key is its first (need == 1), empty bins in between"""
    rng = np.random.default_rng(103)
    small = np.concatenate([_in_bin(rng, b, 5) for b in range(600)] + [_in_bin(rng, 700, 300)] +
                           [_in_bin(rng, b, 2) for b in range(701, FLAT_BINS)])
    small[0] = 0
    return _flat_case(n, K, small, _big(rng, n - small.size), rng)


def case_ties_straddle(n=16384, K=3000):
    """bin 500 holds 20 smaller keys, 60 keys equal to T and 20 larger; 2950 keys below the bin: the cut takes 30 of the 60 ties,
    those of the lowest rows"""
    rng = np.random.default_rng(104)
    below = np.concatenate([_in_bin(rng, b, 6) for b in range(490)] + [_in_bin(rng, 495, 10)])
    T = 500 * FLAT_W + (FLAT_W >> 1)
    inbin = np.concatenate((500 * FLAT_W + 1 + np.arange(20), np.full(60, T), T + 1 + np.arange(20)))
    above = np.concatenate([_in_bin(rng, b, 2) for b in range(501, FLAT_BINS)])
    small = np.concatenate((below, inbin, above))
    small[0] = 0
    assert below.size == 2950
    return _flat_case(n, K, small, _big(rng, n - small.size), rng)


def case_below_lo(n=16384, K=2500):
    """+0, the smallest subnormal, 0.5 and 1 - 2^-53 on rows the sample does not read: all below lo (the key of 1.0), all in bin 0"""
    rng = np.random.default_rng(105)
    small = np.concatenate([_in_bin(rng, b, 2) for b in range(FLAT_BINS)])
    small[0] = 0
    d, K = _flat_case(n, K, small, _big(rng, n - small.size), rng)
    mask = np.ones(n, dtype=bool)
    mask[sample_rows(n)] = False
    rows = np.nonzero(mask & (d > 2.0))[0][:40]
    tiny = dists_of(np.array([SIGN, SIGN | 1, keys_of(np.array([0.5]))[0], KEY_ONE - 1], dtype=U64))
    d[rows] = np.tile(tiny, 10)
    return d, K


def case_bin_1024(n=16384, K=3000, m=1024):
    """m equal keys in bin 300 (1024: the most one work-group sorts; 1025: overflow), 1500 keys below them, K inside a later bin"""
    rng = np.random.default_rng(106)
    small = np.concatenate([_in_bin(rng, b, 5) for b in range(300)] + [np.full(m, 300 * FLAT_W + 12345)] +
                           [_in_bin(rng, b, 3) for b in range(301, FLAT_BINS)])
    small[0] = 0
    return _flat_case(n, K, small, _big(rng, n - small.size), rng)


def case_overflow_1025():
    return case_bin_1024(m=1025)


def case_crowded_above(n=16384, K=3000):
    """1100 keys in bin 2000, far above b*: counted, never sorted, no give-up"""
    rng = np.random.default_rng(107)
    small = np.concatenate([_in_bin(rng, b, 4) for b in range(1500)] + [_in_bin(rng, 2000, 1100)])
    small[0] = 0
    return _flat_case(n, K, small, _big(rng, n - small.size), rng)


def case_shift0(n=16384, K=4000):
    """every key at or below hi within 4094 of it: shift == 0, a bin per key value"""
    rng = np.random.default_rng(108)
    m = 12000
    o = (1 << 40) - 1 - rng.integers(0, 4095, size=m)
    o[0] = (1 << 40) - 1 - 4094                                         # lo, on a sample row
    o[1] = (1 << 40) - 1                                                # hi
    return _flat_case(n, K, o, _big(rng, n - m), rng, pin_sample=(o[0],))


def case_short(n=16384, K=5000):
    """small keys on 1376 sample rows only, every other row 1e6: q = 1375, hi is a small key's bound, tot = 1376 < K"""
    rng = np.random.default_rng(109)
    d = np.full(n, 1e6)
    rows = rng.permutation(sample_rows(n))[:1376]
    d[rows] = 1.0 + rng.random(1376)
    return d, K


def case_crowded_above_chi(n=65536, K=6000):
    """chi distances; 1100 keys equal to a value between the K-th key and hi, on rows the sample does not read"""
    rng = np.random.default_rng(110)
    d = chi(rng, n)
    m = bin_model(d, K)
    s = np.sort(d)
    v = 0.5 * (s[K + 200] + float(dists_of(np.array([m["hi"]], dtype=U64))[0]))
    mask = np.ones(n, dtype=bool)
    mask[sample_rows(n)] = False
    rows = np.nonzero(mask & (d > v))[0][:1100]
    d[rows] = v
    return d, K


def case_random(kind, n, K, seed):
    rng = np.random.default_rng(seed)
    return (chi if kind == "chi" else lognormal)(rng, n), K


# name -> (constructor, what the model must say: verdict and the stated properties, checked by check_case on the CPU)
CASES = {
    "kth_last_eq_hi": (case_kth_last_eq_hi, "ok", ("kth_last", "tot_eq_K", "eq_hi", "hi_plus_1", "K_8192")),
    "kth_first_K1": (case_kth_first_K1, "ok", ("kth_first", "K_1")),
    "kth_first_mid": (case_kth_first_mid, "ok", ("kth_first", "empty_bins")),
    "ties_straddle": (case_ties_straddle, "ok", ("ties_straddle",)),
    "below_lo": (case_below_lo, "ok", ("below_lo",)),
    "bin_1024": (case_bin_1024, "ok", ("bin_1024",)),
    "crowded_above": (case_crowded_above, "ok", ("crowded_above",)),
    "crowded_above_chi": (case_crowded_above_chi, "ok", ("crowded_above",)),
    "shift0": (case_shift0, "ok", ("shift0",)),
    "overflow_1025": (case_overflow_1025, "overflow", ()),
    "short": (case_short, "short", ()),
    "n_16384_plus_4095": (lambda: case_random("chi", 16384 + 4095, 7000, 201), "ok", ("unsampled_tail",)),
    "n_131072": (lambda: case_random("lognormal", 131072, 20000, 202), "ok", ()),
    "n_131073": (lambda: case_random("chi", 131073, 65536, 203), "ok", ("hist_clamped",)),
    "n_8x131072_plus_1": (lambda: case_random("chi", 8 * 131072 + 1, 100000, 204), "ok", ("hist_clamped", "hist_second_round")),
    "big_chi": (lambda: case_random("chi", (1 << 19) + 2, (1 << 18) + 1, 205), "ok", ()),
    "big_lognormal": (lambda: case_random("lognormal", (1 << 19) + 2, (1 << 18) + 1, 206), "ok", ()),
    "big_2_20": (lambda: case_random("chi", 1 << 21, 1 << 20, 207), "ok", ()),
}


def check_case(name, d, K, m):
    """the model's record m of case `name` has the verdict and every property the case states"""
    _, verdict, props = CASES[name]
    assert m["verdict"] == verdict, (name, m["verdict"], m["tot"], m["crowded"])
    n = d.size
    k = keys_of(d)
    order = reference_order(d)
    bins, counts, offs = m["bins"], m["counts"], m["offs"]
    srows = np.zeros(n, dtype=bool)
    srows[sample_rows(n)] = True
    for p in props:
        if p == "kth_last":
            assert m["need"] == counts[m["bstar"]] > 1
        elif p == "kth_first":
            assert m["need"] == 1 and counts[m["bstar"]] > 1
        elif p == "tot_eq_K":
            assert m["tot"] == K < n
        elif p == "eq_hi":
            assert int(k[order[K - 1]]) == m["hi"]
        elif p == "hi_plus_1":
            assert int((k == U64(m["hi"] + 1)).sum()) >= 1
        elif p == "K_8192":
            assert K == 8192 and n == 16384
        elif p == "K_1":
            assert K == 1
        elif p == "empty_bins":
            assert (counts[:m["bstar"]] == 0).any()
        elif p == "ties_straddle":
            T = k[order[K - 1]]
            eq = np.nonzero(k == T)[0]
            taken = int((k[order[:K]] == T).sum())
            assert 0 < taken < eq.size and (bins[eq] == m["bstar"]).all()
            assert (k[bins == m["bstar"]] < T).any() and (k[bins == m["bstar"]] > T).any()
        elif p == "below_lo":
            below = k < U64(m["lo"])
            assert below.sum() >= 4 and not srows[below].any() and (bins[below] == 0).all()
            assert int(k.min()) == SIGN                                     # +0 among them
        elif p == "bin_1024":
            full = np.nonzero(counts == BS_CAP)[0]
            assert full.size and full[0] <= m["bstar"]
        elif p == "crowded_above":
            assert (counts[m["bstar"] + 1:] > BS_CAP).any() and m["crowded"] == []
        elif p == "shift0":
            assert m["shift"] == 0 and int((k == U64(m["hi"])).sum()) >= 1
        elif p == "unsampled_tail":
            assert sample_rows(n).max() < BS_S * (n // BS_S) < n
        elif p == "hist_clamped":
            assert (n + 255) // 256 > HIST_BLOCKS
        elif p == "hist_second_round":
            assert n > 8 * HIST_BLOCKS * 256
        else:
            raise AssertionError("unknown property %s" % p)
    if verdict == "overflow":
        assert m["crowded"] and counts[m["crowded"]].max() == BS_CAP + 1 and m["tot"] >= K
    if verdict == "short":
        assert m["tot"] == 1376 and not m["crowded"]
    if name.startswith("big_"):
        assert m["nbins"] == BS_NB_BIG
