"""Weight vectors that shape the serving chain of the device alias build (abcsmc_amd/csrc/alias_dev.hip), and what the build's
exact-integer model (scripts/alias_scan_proto.py, imported, not copied) says about each of them: the table, whether the
speculation verifies (the table is then built on the device) and how many smalls, bigs and chain steps there are.

Shared by tests/test_alias_cases_cpu.py (the model against the oracle) and tests/test_gpu_alias_branches.py (the kernels
against the oracle, the fallbacks against the model)."""
import functools
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_proto():
    spec = importlib.util.spec_from_file_location("alias_scan_proto", os.path.join(ROOT, "scripts", "alias_scan_proto.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


proto = _load_proto()

KINDS = ["ascending", "descending", "one_big", "one_big_first", "one_big_last", "one_hot", "alternating", "smalls_then_bigs",
         "bigs_then_smalls", "handover_chain", "mostly_zero", "zero_head", "zero_tail", "one_small", "small_integers",
         "powers_of_two", "exactly_full", "exactly_full_shuffled"]
FULL_KINDS = ("exactly_full", "exactly_full_shuffled")
# every size at which a work-group of 256 threads with two (512) or four (1024) elements each is full, one short or one over,
# the smallest tables, and a few blocks with a one-element tail
EDGE_SIZES = [2, 3, 4, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 4097]


def weights(kind, K, seed=0):
    """a valid weight vector (finite, non-negative, not all zero) of K entries; deterministic in (kind, K, seed)"""
    rng = np.random.default_rng([KINDS.index(kind) if kind in KINDS else 99, K, seed])
    U = rng.random(K)
    if kind == "uniform":                                   # (the plain case the structured ones are measured against)
        w = U
    elif kind == "ascending":
        w = np.sort(0.05 + U)
    elif kind == "descending":
        w = np.sort(0.05 + U)[::-1].copy()
    elif kind in ("one_big", "one_big_first", "one_big_last"):       # one big serves every small
        w = 1e-4 + 1e-3 * U
        w[{"one_big": K // 3, "one_big_first": 0, "one_big_last": K - 1}[kind]] = float(K)
    elif kind == "one_hot":
        w = np.zeros(K)
        w[(2 * K) // 3] = 1.0
    elif kind == "alternating":                             # small, big, small, big, ...
        w = np.where(np.arange(K) % 2 == 0, 0.1 + 0.1 * U, 1.0 + U)
    elif kind == "smalls_then_bigs":
        w = np.where(np.arange(K) < K // 2, 0.1 + 0.1 * U, 1.0 + U)
    elif kind == "bigs_then_smalls":
        w = np.where(np.arange(K) < K // 2, 1.0 + U, 0.1 + 0.1 * U)
    elif kind == "handover_chain":                          # every big serves about one small and is demoted
        w = 1.0 + 0.3 * U
        w[rng.permutation(K)[:K // 2]] *= 0.02
    elif kind == "mostly_zero":                             # 90 % zeros
        w = 0.05 + U
        w[rng.permutation(K)[:min(K - 1, (9 * K + 9) // 10)]] = 0.0
    elif kind == "zero_head":
        w = 0.05 + U
        w[:K // 3] = 0.0
    elif kind == "zero_tail":
        w = 0.05 + U
        w[K - K // 3:] = 0.0
    elif kind == "one_small":
        w = np.ones(K)
        w[K // 2] = 0.5
    elif kind == "small_integers":
        w = rng.integers(1, 8, K).astype(np.float64)
    elif kind == "powers_of_two":
        w = np.ldexp(1.0, rng.integers(-20, 20, K))
    elif kind in FULL_KINDS:
        # a quarter 1, half 2, a quarter 3 (K = 4: [1, 2, 2, 3]): the total is 2 K exactly, a 2 sits exactly at the mean, and a 3
        # that serves a 1 is left with EXACTLY the mean -- GSL's third branch (neither small nor big any more)
        q = max(1, K // 4)
        w = np.concatenate([np.full(q, 1.0), np.full(K - 2 * q, 2.0), np.full(q, 3.0)])
        if kind == "exactly_full_shuffled":
            w = w[rng.permutation(K)]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(w, dtype=np.float64)


def blocked_prefix_sums(w, block=512):
    """approximate prefix sums in the device's order: inside every block of `block` elements, then across the blocks"""
    w = np.asarray(w, dtype=np.float64)
    out = np.empty_like(w)
    before = 0.0
    for lo in range(0, w.size, block):
        c = np.cumsum(w[lo:lo + block])
        out[lo:lo + block] = before + c
        before += float(c[-1])
    return out


def model(w):
    """what the exact model says about the weights w: a dict with
         on_device  True: the speculation verifies, the device builds the table; False: a check fails, the host builds it; None: the
                    verdict depends on the order in which the APPROXIMATE prefix sums of the total's chain are accumulated
                    (np.cumsum against blocks of 512) -- nothing may be asserted about such a cell
         reason     the model's Fallback text ("" on the device)
         F, A       the model's table with GSL's KNUTH_CONVENTION applied as abc_alias_table applies it (None where it falls back)
         ns, nb, nsteps"""
    wl = [float(x) for x in w]
    K = len(wl)
    info = {}
    out = {"on_device": True, "reason": "", "F": None, "A": None, "ns": None, "nb": None, "nsteps": None}
    try:
        _, F, A = proto.alias_by_scan(wl, info=info)
        out["F"] = (np.array(F) + np.arange(K, dtype=np.float64)) / float(K)
        out["A"] = np.array(A, dtype=np.uint64)
    except proto.Fallback as e:
        out["on_device"], out["reason"] = False, str(e)
    out.update(info)
    try:                                                     # (only the total's chain reads the approximate sums)
        proto.total_by_scan(wl, approx=blocked_prefix_sums(w))
        blocked_ok = True
    except proto.Fallback:
        blocked_ok = False
    sum_ok = out["on_device"] or not (out["reason"].startswith("sum") or out["reason"] in ("total", "weight", "first weight below the grid"))
    if blocked_ok != sum_ok:
        out["on_device"] = None
    return out


# Cells (kind, K) whose verdict differed between the two summation orders at seed 0 and were re-seeded (none so far).
RESEED = {}

# Cells the MODEL sends to the host (the table is still asserted there, the verdict is not).  Every exactly_full cell belongs
# here by construction: a big left with exactly the mean fails "expected no demotion" (the device leaves GSL's third branch to
# the host on purpose, k_al_serve_apply).  The others are listed by name, with the model's reason.
EXPECT_HOST = {
    # K a power of two: the mean is a binade boundary, and the one big ends its chain within a few grid units of it -- the level
    # speculated from the exact sums is one off, the claimed value would need 54 bits
    ("one_big_first", 512): "claimed value not representable",
    ("one_big_last", 1024): "claimed value not representable",
    # the same boundary, met by the last hand-over (its IEEE operation on the claimed operands gives another double)
    ("small_integers", 512): "step 510 (h)",
    # integer weights whose total is 4 K: a 7 that serves a 1 is left with exactly the mean, GSL's third branch as in exactly_full
    ("small_integers", 2049): "expected no demotion at 0",
    # outside the grid of block edges, used by the resampling test: the hot entry goes down from 1 by the mean, 1 / 20000, and after
    # 10000 steps stands at 0.5 up to the chain's rounding drift -- a binade boundary again, the level cannot be told from the exact sums
    ("one_hot", 20000): "claimed value not representable",
}
RESAMPLE_SIZES = [19999, 20000]                  # ABC_ALIAS_DEV_MIN_K - 1 (the host's table) and ABC_ALIAS_DEV_MIN_K
RESAMPLE_KINDS = ["one_hot", "mostly_zero", "handover_chain"]


def expect_host(kind, K):
    return kind in FULL_KINDS or (kind, K) in EXPECT_HOST


def two_valued(ns, nb, seed=0):
    """ns smalls and nb bigs in random places: a small and a big value with a little noise (0.2 and 2, ten per cent)"""
    rng = np.random.default_rng([77, ns, nb, seed])
    K = ns + nb
    w = np.concatenate([0.2 * (1.0 + 0.1 * rng.random(ns)), 2.0 * (1.0 + 0.1 * rng.random(nb))])[rng.permutation(K)]
    return np.ascontiguousarray(w)


@functools.lru_cache(maxsize=None)
def block_edge_cases(elems):
    """[(label, w, model(w))]: the number of smalls, of bigs and of chain steps each exactly B - 1, B, B + 1 and 2 B (B = 256 * elems,
    the elements of a work-group) while K is at least two off every multiple of B.  The chain of such weights serves every small
    and demotes every big but the last, nsteps = K - 1: the nsteps cases have K = target + 1 (on an edge only for B - 1)."""
    B = 256 * elems
    other = B // 2 + 37
    out = []
    for t, T in (("B-1", B - 1), ("B", B), ("B+1", B + 1), ("2B", 2 * B)):
        for q, (ns, nb) in (("ns", (T, other)), ("nb", (other, T)), ("nsteps", ((T + 1) - (T + 1) * 2 // 5, (T + 1) * 2 // 5))):
            w = two_valued(ns, nb)
            w.setflags(write=False)
            out.append(("%s=%s" % (q, t), w, model(w)))
    return out


@functools.lru_cache(maxsize=None)
def cell(kind, K):
    """(w, model(w)) of one cell of the grid, computed once per process; the arrays are read-only"""
    w = weights(kind, K, RESEED.get((kind, K), 0))
    w.setflags(write=False)
    m = model(w)
    for a in (m["F"], m["A"]):
        if a is not None:
            a.setflags(write=False)
    return w, m
