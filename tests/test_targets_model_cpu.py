"""CPU checks of tests/_targets_model.py: the copy of launch_rank_targets' host decisions is held to the text of
abcsmc_amd/csrc/targets.hip and pinned on both sides of every threshold; the constructed give-up inputs of
tests/test_gpu_targets_branches.py are shown, by the reference alone, to land where they are meant to; and the exact model of one
target's selection is checked by brute force on small sets with ties, zeros, subnormals and +inf."""
import os
import re

import numpy as np
import pytest

import _targets_model as TM
from _project_dispatch import NOT_A_SHAPE, fused_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src():
    return open(os.path.join(ROOT, "abcsmc_amd", "csrc", "targets.hip")).read()


def _launcher():
    src = _src()
    body = src[src.index("int launch_rank_targets("):]
    return body[:body.index("int launch_row_weights_check(")]


# ---- the copy against the source text -------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    src = _src()
    num = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert (num("TG_S"), num("TG_NB"), num("TG_CAP"), num("TG_CSTRIDE")) == (TM.TG_S, TM.TG_NB, TM.TG_CAP, TM.TG_CSTRIDE)
    m = re.search(r"const size_t TG_CHUNK_BYTES = \(size_t\)(\d+) << (\d+);", src)
    assert int(m.group(1)) << int(m.group(2)) == TM.TG_CHUNK_BYTES == 512 * 1024 * 1024
    # a chunk's bytes per target, the clamp of the two grid-stride kernels, the thresholds of the groups
    assert "const size_t per = p.C * 24 + (TG_NB + 1) * 4;" in src
    assert src.count("if (blocks > 4096) blocks = 4096;") == 2 and TM.ROW_BLOCKS == 4096
    assert "size_t groups = (rb >= 2048) ? 1 : (2048 + rb - 1) / rb;" in src
    assert "const size_t rb = (N + 256 * tg_rpt(kc) - 1) / (256 * tg_rpt(kc));" in src
    # the sample's positions and the plan's arithmetic
    assert "return (size_t)j * stride + stride / 2;" in src and "const size_t stride = n / (size_t)ns;" in src
    assert "const double qd = f * TG_S + 4.0 * sqrt(TG_S * f * (1.0 - f)) + 8.0;" in src
    assert "const double frac = (p.q + 1.0) / TG_S + 8.0 * sqrt(p.q + 1.0) / TG_S;" in src
    assert "const double cap = frac * (double)N + 256.0;" in src


def test_candidate_instances_and_rows_per_thread():
    body = _launcher()
    cases = re.findall(r"(case (\d+)|default): TG_CAND\((\d+)\); break;", body)
    got = [(int(c[1]) if c[1] else None, int(c[2])) for c in cases]
    assert got == [(1, 1), (2, 2), (4, 4), (8, 8), (16, 16), (32, 32), (None, 0)]
    assert tuple(kc for _, kc in got) == TM.KCS
    assert "hipLaunchKernelGGL((k_tg_cand<KCV, tg_rpt(KCV)>)" in body
    m = re.search(r"constexpr int tg_rpt\(int kc\) \{ return (.*?); \}", _src()).group(1)
    assert m == "(kc == 0 || kc >= 32) ? 1 : (32 / kc > 4 ? 4 : 32 / kc)"
    expr = lambda kc: 1 if (kc == 0 or kc >= 32) else (4 if 32 // kc > 4 else 32 // kc)
    assert [TM.tg_rpt(kc) for kc in TM.KCS] == [expr(kc) for kc in TM.KCS] == [4, 4, 4, 4, 2, 1, 1]
    assert [TM.tg_kc(A) for A in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)] == [1, 2, 4, 4, 8, 8, 16, 16, 32, 32, 0, 0]
    assert [TM.tg_kco(A) for A in (1, 3, 9, 32, 33, 40)] == [1, 4, 16, 32, 33, 40]


def test_no_kernel_the_mirror_does_not_name():
    body = _launcher()
    launched = set(re.findall(r"\b(k_tg_[a-z0-9_]+)", body))
    assert launched == set(TM.KERNELS), launched ^ set(TM.KERNELS)
    assert set(re.findall(r"\b(k_[a-z0-9_]+)", body)) == launched                   # and nothing under another name
    defined = set(re.findall(r"__global__ [^\n]*void (k_tg_[a-z0-9_]+)\(", _src()))
    assert defined == launched
    # the rows' scores: the projection's fused pass on the whole set, else k_tg_row_scores
    assert "launch_project_distance_scores(ctx, X, N, ldx, M, P, A, model, dtmp, S, N, 0, nullptr) != 0" in body


# ---- both sides of every threshold -------------------------------------------------------------------------------------------------
def test_plan_thresholds():
    for K in (1, 17, 4096):
        for ex in (False, True):
            assert TM.tg_plan(4096, K, ex) == (4096, K - 1, 4096)
    assert TM.tg_plan(4095, 17, False) == (4095, 16, 4095) and TM.tg_plan(1, 1, False) == (1, 0, 1)
    for K in (1, 50, 4097):
        ns, q, C = TM.tg_plan(4097, K, False)
        assert ns == 4096
    assert np.array_equal(TM.sample_rows(4097, 4096), np.arange(4096))                   # stride 1, offset 0
    assert np.array_equal(TM.sample_rows(8192, 4096), 2 * np.arange(4096) + 1)           # stride 2, offset 1
    assert np.array_equal(TM.sample_rows(8191, 4096), np.arange(4096))
    assert np.array_equal(TM.sample_rows(12289, 4096), 3 * np.arange(4096) + 1)
    assert np.array_equal(TM.sample_rows(1000, 1000), np.arange(1000))
    assert [TM.tg_sample_row(j, 1048833, 4096) for j in (0, 1, 4095)] == [128, 384, 4095 * 256 + 128]
    assert TM.tg_plan(8192, 100, False)[1:] == (86, 579)
    assert TM.tg_plan(8192, 3000, False)[1:] == (1631, 4166)
    assert TM.tg_plan(4097, 50, False)[2] == 417
    assert TM.tg_plan(4097, 4097, False)[1:] == (4095, 4097)
    assert TM.tg_plan(1048833, 1000, False)[1:] == (19, 14538)
    # an exclusion anywhere in the call asks for one key more
    assert TM.tg_plan(8192, 99, True) == TM.tg_plan(8192, 100, False)
    assert TM.tg_plan(4097, 4096, True)[1:] == (4095, 4097)
    # the capacity never falls below K, and reaches N before K does
    for N in (4097, 8192, 100000, 2097409):
        for K in (1, 17, N // 10, N // 2, N - 1, N):
            ns, q, C = TM.tg_plan(N, K, False)
            assert K <= C <= N and 0 <= q <= 4095 and q + 1 >= min(4096, K * 4096 // N)


def test_chunks_and_groups():
    assert TM.tg_chunk(4095, 10 ** 6) == 5042 and TM.tg_chunk(4095, 5042) == 5042 and TM.tg_chunk(4095, 7) == 7
    p = TM.launch_plan(4095, 1, 1, 5100, 33, True)
    assert (p["plan"], p["C"], p["bc"], p["nchunks"]) == ("exact", 4095, 5042, 2)
    assert [(c["c0"], c["nb"]) for c in p["chunks"]] == [(0, 5042), (5042, 58)]
    # 4095 rows, four per thread: 4 row blocks, 512 groups of 10 targets, the last of 5042 - 5040 + ... = 2 targets
    assert p["chunks"][0] == {"rb": 4, "groups": 505, "tgs": 10, "last": 2, "c0": 0, "nb": 5042}
    assert p["chunks"][1] == {"rb": 4, "groups": 58, "tgs": 1, "last": 1, "c0": 5042, "nb": 58}
    assert p["ragged"] and p["groups"] == [58, 505]
    p = TM.launch_plan(4095, 1, 1, 5042, 33, False)
    assert p["nchunks"] == 1
    # one group: 2048 row blocks or more
    assert TM.tg_groups(2048 * 1024, 1, 3) == {"rb": 2048, "groups": 1, "tgs": 3, "last": 3}
    assert TM.tg_groups(2048 * 1024 - 1024, 1, 3)["groups"] == 2 and TM.tg_groups(2048 * 1024 - 1024, 1, 3)["last"] == 1
    assert TM.tg_groups(2097409, 1, 3) == {"rb": 2049, "groups": 1, "tgs": 3, "last": 3}
    assert TM.tg_groups(2048 * 256, 32, 3)["groups"] == 1 and TM.tg_groups(2048 * 256 - 1, 0, 3)["groups"] == 1
    assert TM.tg_groups(2047 * 256, 40, 3)["groups"] == 2
    # fewer targets than groups: one target each; seven targets over the 1000 rows of a width case
    assert TM.tg_groups(1000, 1, 7) == {"rb": 1, "groups": 7, "tgs": 1, "last": 1}
    assert TM.tg_groups(1000, 8, 1) == {"rb": 1, "groups": 1, "tgs": 1, "last": 1}
    # the second trips of k_tg_row_scores and k_tg_dist_one
    assert not TM.launch_plan(1048576, 1, 1, 3, 10, False)["second_trip"]
    assert TM.launch_plan(1048577, 1, 1, 3, 10, False)["second_trip"] and TM.launch_plan(2097409, 1, 1, 3, 1000, False)["second_trip"]


def test_scoring_kernel():
    f = lambda N, M, A, ldx=None, al=True: TM.scoring_kernel(N, N + 2 if ldx is None else ldx, al, M, A)
    assert f(4098, 24, 8) == ("dist2_lds", 8) and f(4098, 24, 16) == ("dist2_lds", 16) and f(4098, 24, 24) == ("mfma", 2, "stage")
    for A in (8, 16, 24):
        assert f(4098, 24, A, al=False) == TM.ROW_SCORES and f(4098, 24, A, ldx=4101) == TM.ROW_SCORES
        assert f(4097, 24, A, ldx=4100) == TM.ROW_SCORES
    for A in (1, 2, 3, 4, 33, 40):
        assert f(4098, 24, A) == TM.ROW_SCORES
    assert fused_plan(4098, 4100, True, 24, 8, 0, 4098) != NOT_A_SHAPE
    assert f(1000, 9, 9) == ("dist2_lds", 16) and f(1000, 6, 5) == ("dist2_lds", 8) and f(1000, 17, 17) == ("mfma", 2, "stage")


# ---- keys and the pre-filter -------------------------------------------------------------------------------------------------------
def test_keys_preserve_the_order():
    v = np.array([0.0, 5e-324, 2.2250738585072014e-308, 1.0, np.nextafter(1.0, 2.0), 1e300, 1.7976931348623157e308, np.inf, np.nan])
    k = TM.key_of(TM.canonical(v))
    assert np.all(k[1:] > k[:-1]) and int(k[0]) == TM.KEY_ZERO and int(k[-2]) == TM.KEY_INF and int(k[-1]) < TM.PAD
    assert np.array_equal(TM.dist_of(k)[:-1], v[:-1]) and np.isnan(TM.dist_of(k)[-1])
    neg = np.array([-np.nan]).view(np.uint64) | np.uint64(1 << 63)
    assert int(TM.key_of(neg.view(np.float64))[0]) < TM.KEY_ZERO                         # a NaN with the sign bit: below +0
    assert TM.t2_of(TM.KEY_ZERO - 1) == -1.0 and TM.t2_of(TM.KEY_INF) == np.inf and TM.t2_of(TM.PAD) == np.inf


def test_prefilter_never_removes_a_candidate():
    """d2 <= t2 (or NaN) holds for every squared distance whose rooted key is at or below the threshold key: thresholds of +0,
    subnormal, ordinary, huge and +inf, and squared distances a few ulp on either side of the threshold's square"""
    rng = np.random.default_rng(12)
    tds = [0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1.4916681462400413e-154, 1e-100, 0.1, 1.0, np.nextafter(1.0, 0.0), 3.0,
           1e100, 1.3407807929942596e154, np.nextafter(1.3407807929942597e154, np.inf), 1e200, 1.7976931348623157e308, np.inf]
    tds += list(10.0 ** rng.uniform(-160, 160, 200)) + list(rng.uniform(0.5, 2.0, 200))
    removed_some = False
    for td in tds:
        tkey = int(TM.key_of(np.array([td]))[0])
        t2 = TM.t2_of(tkey)
        with np.errstate(over="ignore", under="ignore"):
            sq = np.float64(td) * np.float64(td)
            d2 = [0.0, 5e-324, sq, np.inf, np.nan, 1.7976931348623157e308]
            for start in (sq, np.nextafter(np.float64(td), np.inf) ** 2):
                up = dn = start
                for _ in range(6):
                    up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
                    d2 += [up, dn]
            d2 = np.array([v for v in d2 if not v < 0.0])
            keys = TM.key_of(TM.canonical(np.sqrt(d2)))
        inside = keys <= np.uint64(tkey)
        passed = TM.prefilter(d2, t2)
        assert passed[inside].all(), (td, d2[inside & ~passed])
        assert passed[np.isnan(d2)].all()
        removed_some = removed_some or (~passed).any()
    assert removed_some                                                               # (it is a filter)


# ---- the constructed give-up inputs ---------------------------------------------------------------------------------------------------
def _m1(z, t, seed=3, ncomp=1):
    mean, sd, r = TM.m1_record(seed)
    return TM.m1_distances(TM.m1_x(z, mean, sd), mean, sd, r, TM.m1_x(t, mean, sd), ncomp)


def test_constructed_overflow_and_short():
    d = _m1(TM.split_rows(8192, 1, "sample"), 0.0)
    assert TM.select_model(d, 100)[:3] == ("overflow", 4183, 579)
    assert TM.select_model(d, 99, excl=5000)[:3] == ("overflow", 4182, 579)           # (an unsampled row: one candidate fewer)
    odd = int(np.flatnonzero(np.arange(8192) % 2 == 1)[np.argmin(d[1::2])])
    assert TM.select_model(d, 99, excl=odd)[:3] == ("overflow", 4183, 579)            # (a sampled one: the next key passes instead)
    d = _m1(TM.split_rows(8192, 2, "others"), 0.0)
    assert TM.select_model(d, 3000)[:3] == ("short", 1632, 4166)
    v = TM.select_model(d, 2999, excl=int(TM.reference_order(d)[7]))
    assert v[0] == "short" and v[1] == 1632 and v[2] == 4166           # (the excluded row is a sampled one: one key more passes)
    # the same rows seen by an ordinary K: the sample is still unrepresentative, and the model says which way it fails
    assert TM.select_model(_m1(TM.split_rows(8192, 1, "sample"), 0.0), 3000)[0] == "overflow"


def test_constructed_ties():
    z = TM.tied_rows(3000, 1500, 4)
    d = _m1(z, 0.0)
    order = TM.reference_order(d)
    assert np.array_equal(order[:1500], np.arange(1, 3000, 2)) and len(np.unique(d[order[:1500]])) == 1 and d[order[0]] > 0
    for K in (1, 1200, 1501, 3000):
        v = TM.select_model(d, K)
        assert v[0] == "bin" and v[3] >= 1500 and v[1] >= max(K, 1500) and v[2] == 3000, (K, v)
    for K, ex in ((1, 1), (1200, 7), (1501, 2), (2999, 0), (1499, 2999)):
        v = TM.select_model(d, K, excl=ex)
        assert v[0] == "bin" and v[3] >= 1499, (K, ex, v)
    # targets equal to the tied rows: distance exactly 0, everything in bin 0
    d0 = _m1(z, 0.25)
    assert np.count_nonzero(d0 == 0.0) == 1500 and TM.select_model(d0, 10)[0] == "bin"


def test_ordinary_rows_are_selected_on_the_device():
    d = _m1(TM.ordinary_rows(3000, 5), 0.3)
    for K in (1, 17, 3000):
        v = TM.select_model(d, K)
        assert v[0] == "ok" and v[1] == K and v[3] <= TM.TG_CAP, (K, v)
    v = TM.select_model(d, 2999, excl=int(TM.reference_order(d)[40]))
    assert v[0] == "ok" and v[1] == 2999
    for N, K in ((8192, 100), (8192, 3000), (4097, 50), (12289, 50)):
        v = TM.select_model(_m1(TM.ordinary_rows(N, N), -0.2), K)
        assert v[0] == "ok" and K <= v[1] <= v[2], (N, K, v)


def test_pad_key_threshold_and_full_rankings():
    d = _m1(TM.ordinary_rows(4097, 6), 0.1)
    # an excluded row inside the sample at K = N - 1: the threshold is the pad key, the bins span the whole key range
    s = TM.select_detail(d, 4096, excl=10)
    assert (s["verdict"], s["c"], s["C"], s["tkey"], s["shift"]) == ("bin", 4096, 4097, TM.PAD, 53) and s["lo"] == TM.KEY_ZERO
    # ... outside the sample (the last row): the sample's largest key, and every row beyond it is missed
    last = TM.select_detail(d, 4096, excl=4096)
    assert last["tkey"] == int(TM.key_of(d[:4096]).max()) and last["c"] == 4096 - int((d[:4096] > d[:4096].max()).sum()) == 4096
    # K = N on a sampled plan: short unless the sample holds the largest key
    z = TM.ordinary_rows(8192, 7)
    big = int(np.argmax(np.abs(z)))
    z[[big, 0]] = z[[0, big]]                                                        # the farthest row: row 0, an unsampled one
    d = _m1(z, 0.0)
    assert int(np.argmax(d)) == 0
    assert TM.select_model(d, 8192)[0] == "short" and TM.select_model(d, 8192)[1] < 8192
    z2 = z.copy()
    z2[[0, 1]] = z2[[1, 0]]                                                          # ... row 1, a sampled one
    v = TM.select_model(_m1(z2, 0.0), 8192)
    assert v[:3] == ("ok", 8192, 8192) and v[3] <= TM.TG_CAP                         # (all rows pass, spread over 2047 bins)


def test_no_component():
    for N, want in ((1000, "ok"), (1024, "ok"), (1025, "bin"), (3000, "bin"), (4096, "bin")):
        d = _m1(TM.ordinary_rows(N, 8), 0.0, ncomp=0)
        assert not d.view(np.uint64).any()
        for K in (1, N // 2, N):
            v = TM.select_model(d, K)
            assert v == (want, N, N, N), (N, K, v)
    # (a sampled plan sees N equal keys at the threshold: more than the segment holds until K nears N)
    d = np.zeros(4097)
    assert TM.select_model(d, 1) == ("overflow", 4097, 297, 0) and TM.select_model(d, 4097) == ("bin", 4097, 4097, 4097)
    assert [TM.tg_ncomp(h, 8) for h in (0.0, -3.0, 13.0, 2.9, 8.0, 7.0, -0.5)] == [0, 0, 8, 2, 8, 7, 0]


# ---- the model by brute force --------------------------------------------------------------------------------------------------------
def test_model_brute_force():
    """200 small sets with ties, zeros, subnormals and +inf: under "ok" the first K candidates by (key, row) are the reference's
    first K, the K-th key lies in bin bstar with need = K - offs[bstar], and the bins up to bstar hold exactly the keys the
    device sorts; under every verdict the count and the threshold are what a plain scan gives"""
    rng = np.random.default_rng(2024)
    seen = set()
    for it in range(200):
        N = int(rng.integers(1, 601))
        d = np.abs(rng.normal(size=N)) * 10.0 ** rng.integers(-3, 4)
        for val, share in ((0.0, 0.1), (5e-324, 0.05), (1e-310, 0.05), (np.inf, 0.1)):
            if rng.random() < 0.5:
                d[rng.random(N) < share] = val
        if rng.random() < 0.6 and N > 3:                                   # ties: copies of a few values
            src = rng.integers(0, N, size=max(N // 3, 1))
            d[rng.integers(0, N, size=src.size)] = d[src]
        if it % 10 == 0:
            d[:] = d[0]
        K = int(rng.integers(1, N + 1))
        excl = int(rng.integers(0, N)) if (rng.random() < 0.4 and N > 1) else None
        if excl is not None and K > N - 1:
            K = N - 1
        s = TM.select_detail(d, K, excl)
        seen.add(s["verdict"])
        keys = [int(k) for k in TM.key_of(d)]
        rows = [r for r in range(N) if r != excl]
        ref = sorted(rows, key=lambda r: (keys[r], r))
        assert list(TM.reference_order(d, excl)) == ref
        # N <= 4096: the exact plan -- the threshold is the K-th key itself, and nothing overflows or falls short
        assert s["tkey"] == keys[ref[K - 1]] and s["lo0"] == keys[ref[0]] and s["C"] == N
        assert s["c"] == sum(1 for r in rows if keys[r] <= s["tkey"]) >= K
        assert s["verdict"] in ("ok", "bin")
        cand = sorted((int(r) for r in s["cand"]), key=lambda r: (keys[r], r))
        assert cand[:K] == ref[:K]
        lo, sh = s["lo"], s["shift"]
        bin_of = lambda k: 0 if k <= lo else (k - lo) >> sh
        assert lo <= s["lo0"] and bin_of(s["tkey"]) <= TM.TG_NB - 1
        assert sh == 0 or ((s["tkey"] - lo) >> (sh - 1)) >= TM.TG_NB - 1
        hist = [0] * (TM.TG_NB + 1)
        for r in cand:
            hist[bin_of(keys[r])] += 1
        assert hist == list(s["hist"])
        bstar = bin_of(keys[ref[K - 1]])
        assert bstar == s["bstar"] and s["need"] == K - int(s["offs"][bstar]) and 1 <= s["need"] <= hist[bstar]
        assert s["maxbin"] == max(hist[:bstar + 1]) and (s["verdict"] == "bin") == (s["maxbin"] > TM.TG_CAP)
        # the bins are ordered as the keys are: sorting each bin by (key, row) and keeping need of the last gives the first K
        out = []
        for b in range(bstar + 1):
            members = sorted((r for r in cand if bin_of(keys[r]) == b), key=lambda r: (keys[r], r))
            out += members[:s["need"]] if b == bstar else members
        assert out == ref[:K]
    assert seen == {"ok"} or seen == {"ok", "bin"}


def test_model_on_sampled_plans():
    """the same by brute force where the threshold comes from a sample: N just above 4096 and at strides 2 and 3, with ties"""
    rng = np.random.default_rng(77)
    for N in (4097, 8191, 8192, 12289):
        d = np.abs(rng.normal(size=N))
        d[rng.integers(0, N, size=200)] = d[rng.integers(0, N, size=200)]
        keys = TM.key_of(d)
        for K, excl in ((1, None), (50, None), (50, 17), (N // 10, None), (N - 1, 3), (N, None)):
            s = TM.select_detail(d, K, excl)
            ns, q, C = TM.tg_plan(N, K, excl is not None)
            stride = N // 4096
            rows = np.arange(4096) * stride + stride // 2
            sk = np.sort(np.where(rows == (-1 if excl is None else excl), np.uint64(TM.PAD), keys[rows]))
            assert s["tkey"] == int(sk[q]) and s["lo0"] == int(sk[0])
            ok = keys <= sk[q]
            if excl is not None:
                ok[excl] = False
            assert s["c"] == int(ok.sum()) and s["C"] == C
            want = "overflow" if s["c"] > C else "short" if s["c"] < K else None
            assert (s["verdict"] == want) if want else (s["verdict"] in ("ok", "bin"))
            if s["verdict"] == "ok":
                ref = TM.reference_order(d, excl)
                cand = s["cand"][np.argsort(keys[s["cand"]], kind="stable")]
                assert np.array_equal(cand[:K], ref[:K])


def test_one_metric_distances_are_the_oracles(oracle):
    """m1_distances (plain numpy) against the oracle's projection with exact observed scores, bit for bit: rows over many scales,
    a row equal to the target, +inf and NaN rows"""
    for seed in range(5):
        mean, sd, r = TM.m1_record(seed)
        z = np.random.default_rng(seed).normal(size=2000) * 10.0 ** np.random.default_rng(seed + 9).integers(-8, 8, size=2000)
        x = TM.m1_x(z, mean, sd)
        x[7], x[8], t = np.inf, np.nan, x[11]
        d = TM.m1_distances(x, mean, sd, r, t)
        o = TM.target_scores([t], np.array([mean]), np.array([sd]), np.array([[r]]), 1)
        ref = oracle.project_distance(x.reshape(-1, 1), [mean], [sd], np.array([[r]]), 1, o)
        assert d[11] == 0.0 and np.isposinf(d[7]) and np.isnan(d[8]) and np.isnan(ref[8])
        fin = np.isfinite(ref)
        assert np.array_equal(d[fin].view(np.uint64), ref[fin].view(np.uint64)) and np.array_equal(np.isposinf(d), np.isposinf(ref))
