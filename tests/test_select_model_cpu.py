"""CPU checks of tests/_select_model.py: the copy of the selection's host decisions is held to the text of
abcsmc_amd/csrc/select.hip and pinned on both sides of every threshold; the constructed inputs of tests/test_gpu_select_branches.py
are shown, by the model alone, to land where they are meant to; and the exact model of one bin selection is checked by brute force
on small random and tie-heavy sets."""
import os
import re

import numpy as np
import pytest

import _select_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src():
    return open(os.path.join(ROOT, "abcsmc_amd", "csrc", "select.hip")).read()


# ---- the copy against the source text -------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    src = _src()
    num = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert (num("BS_NB"), num("BS_NB_BIG"), num("BS_S"), num("BS_CAP"), num("SC_N")) == (
        SM.BS_NB, SM.BS_NB_BIG, SM.BS_S, SM.BS_CAP, SM.SC_N)
    assert "constexpr size_t SC_MAX_N = (size_t)1 << 18;" in src and SM.SC_MAX_N == 1 << 18
    assert num("CP_ITEMS") * 256 == SM.CP_CHUNK and "constexpr int CP_CHUNK = 256 * CP_ITEMS;" in src
    assert num("ST_ITEMS") * 256 == SM.ST_CHUNK and "constexpr int ST_CHUNK = 256 * ST_ITEMS;" in src
    assert src.count("if (hb > 512) hb = 512;") == 3 and SM.HIST_BLOCKS == 512
    assert src.count("size_t hb = (n + 255) / 256;") == 3


def test_dispatch_lines_are_the_sources():
    src = _src()
    assert ("const bool bins = !ctx->sel_force_radix && n >= 4 * (size_t)BS_S && 2 * K <= n && K <= ((size_t)1 << 20);" in src)
    assert "const int nbins = K <= ((size_t)1 << 18) ? BS_NB : BS_NB_BIG;" in src
    assert (SM.BIG_K, SM.MAX_BIN_K) == (1 << 18, 1 << 20)
    assert "if (nbins == BS_NB) hipLaunchKernelGGL(k_bs_scan<BS_NB / 1024>" in src
    assert "else hipLaunchKernelGGL(k_bs_scan<BS_NB_BIG / 1024>" in src
    # the radix path and the sorts
    assert "if (K == n) {\n        hipLaunchKernelGGL(k_init_pairs" in src
    assert "if (n <= 1) return ABC_OK;" in src
    assert "if (byte_lo == 0 && byte_hi == 8 && n <= SC_MAX_N) {" in src
    assert "const unsigned nc = (unsigned)((n + SC_N - 1) / SC_N);" in src and "if (nc == 1) {" in src
    assert "const int nb = (int)((n + ST_CHUNK - 1) / ST_CHUNK);" in src
    assert src.count("const int nb = (int)((n + CP_CHUNK - 1) / CP_CHUNK);") == 3
    assert "const int per = (nb + 255) / 256, i0 = t * per;" in src
    assert "for (int b0 = 0; b0 < m; b0 += 256) {" in src
    assert "for (unsigned r0 = 0; r0 < W; r0 += 8) {" in src
    # the counters: one bin selection per call of the bin path, one give-up where the function's own check reads a set flag
    body = src[src.index("int launch_select_smallest("):src.index("int abc_select_check_queue(")]
    assert body.count("ctx->sel_bin_selections++;") == 1 and body.count("ctx->sel_bin_giveups++;") == 1
    assert body.index("if (!bins) return select_by_radix") < body.index("ctx->sel_bin_selections++;") < body.index("select_by_bins(")
    assert body.index("if (defer_check) return ABC_OK;") < body.index("if (!failed) return ABC_OK;") < body.index("ctx->sel_bin_giveups++;")


def test_sample_and_bounds_are_the_sources():
    src = _src()
    assert "const size_t stride = n / BS_S;" in src
    assert "dv[j] = dist[(size_t)(t + 1024 * j) * stride + stride / 2];" in src
    assert "for (int j = 0; j < BS_S / 1024; j++)" in src and "__launch_bounds__(1024) void k_bs_sample" in src
    assert "const double f = (double)K / (double)n;" in src
    assert "double qd = f * BS_S + 4.0 * sqrt(BS_S * f * (1.0 - f)) + 8.0;" in src
    assert "unsigned int q = (qd >= (double)(BS_S - 1)) ? BS_S - 1 : (unsigned int)qd;" in src
    assert "const int shift = 56 - 8 * pass;" in src and "for (int pass = 0; pass < 3; pass++) {" in src
    assert "const unsigned long long lo = mn, hi = s_prefix | ~mask;" in src
    assert "while (shift < 63 && (span >> shift) >= (unsigned long long)(nbins - 1)) shift++;" in src
    assert "return (k <= lo) ? 0 : (int)((k - lo) >> shift);" in src
    assert "if (i0 + u * stride < n && k <= hi) atomicAdd(&lh[bs_bin(k, lo, shift)], 1u);" in src
    assert ("if ((unsigned long long)off < K && K <= (unsigned long long)off + c[j]) "
            "{ bs->bstar = BPT * t + j; bs->need = K - off; }") in src
    assert "if ((unsigned long long)off < K && c[j] > (unsigned int)BS_CAP) s_fail = 1;" in src
    assert "const int fail = (s_fail || (unsigned long long)tot < K) ? 1 : 0;" in src
    assert "return (b >> 63) ? ~b : (b | 0x8000000000000000ull);" in src
    # the 48 bits of an index the chunk sort keeps, and the refusal in front of it
    assert "oidx[base + e] = si[e] & 0x0000ffffffffffffull;" in src and SM.IDX_LIMIT == 1 << 48
    api = open(os.path.join(ROOT, "abcsmc_amd", "csrc", "api.hip")).read()
    assert api.count("CHECK_IDX48(ctx, \"abc_select_smallest_dev\", idx_base, n);") == 1
    assert api.count("CHECK_IDX48(ctx, \"abc_select_compact_dev\", idx_base, n);") == 1
    assert "const uint64_t lim48_ = (uint64_t)1 << 48;" in api


def test_sample_rows_are_the_kernels():
    for n in (16384, 16384 + 4095, 131073, (1 << 19) + 2):
        stride = n // 4096
        rows = sorted((t + 1024 * j) * stride + stride // 2 for t in range(1024) for j in range(4))
        assert rows == SM.sample_rows(n).tolist() and rows[-1] < n
    assert SM.sample_rows(16384)[:3].tolist() == [2, 6, 10]


def test_q_is_bounded_on_the_bin_path():
    """2 K <= n: qd <= 2184, the clamp to BS_S - 1 never binds"""
    worst = max(SM.sample_q(n, n // 2) for n in (16384, 16385, 1 << 21, 10 ** 7))
    assert worst == 2184
    assert SM.sample_q(16384, 1) == 10 and SM.sample_q(16384, 5000) == 1375 and SM.sample_q(16384, 8192) == 2184
    assert SM.sample_q(100, 100) == SM.BS_S - 1                             # (f = 1: only outside the bin path)


# ---- both sides of every threshold -------------------------------------------------------------------------------------------------
def test_path_thresholds():
    assert SM.select_path(16383, 1) == "radix" and SM.select_path(16384, 1) == "bins/4096"
    assert SM.select_path(16384, 8192) == "bins/4096" and SM.select_path(16384, 8193) == "radix"
    assert SM.select_path(16385, 8192) == "bins/4096" and SM.select_path(16385, 8193) == "radix"      # 2 K = n + 1
    for n in (1 << 20, (1 << 20) + 1):
        assert SM.select_path(n, n // 2) == "bins/16384" and SM.select_path(n, n // 2 + 1) == "radix"
    assert SM.select_path(1 << 22, 1 << 18) == "bins/4096" and SM.select_path(1 << 22, (1 << 18) + 1) == "bins/16384"
    assert SM.select_path((1 << 19) + 2, (1 << 18) + 1) == "bins/16384" and SM.select_path((1 << 19) + 1, (1 << 18) + 1) == "radix"
    assert SM.select_path(1 << 22, 1 << 20) == "bins/16384" and SM.select_path(1 << 22, (1 << 20) + 1) == "radix"
    assert SM.select_path(1 << 21, 1 << 20) == "bins/16384"
    assert SM.select_path(16384, 1, force_radix=True) == "radix"
    assert SM.radix_plan(5000, 5000) == "init_pairs" and SM.radix_plan(5000, 4999) == "six_pass"


def test_sort_thresholds():
    got = [SM.sort_plan(K) for K in (1, 2, 4096, 4097, 1 << 18, (1 << 18) + 1)]
    assert got == ["none", "chunk", "chunk", "chunks+merge", "chunks+merge", "lsd"]
    assert SM.sort_plan(0) == "none"
    assert [SM.merge_rounds(n) for n in (4097, 32768, 32769, 1 << 18)] == [1, 1, 2, 8]


def test_grid_clamps():
    assert [SM.hist_blocks(n) for n in (1, 256, 257, 131072, 131073, 10 ** 7)] == [1, 1, 2, 512, 512, 512]
    assert not SM.launch_plan(131072, 1000)["hist_clamped"] and SM.launch_plan(131073, 1000)["hist_clamped"]
    assert [SM.cp_blocks(n) for n in (1, 2048, 2049, 524288, 524289)] == [1, 1, 2, 256, 257]
    assert [SM.scan_slabs(m) for m in (1, 256, 257)] == [1, 1, 2]
    assert [SM.st_blocks(n) for n in (2048, 2049, 524288, 524289)] == [1, 2, 256, 257]
    assert [SM.st_per(nb) for nb in (1, 256, 257, 513)] == [1, 1, 2, 3]
    p = SM.launch_plan(526337, 263169)
    assert p == {"path": "radix", "hist_blocks": 512, "hist_clamped": True, "radix": "six_pass", "sort": "lsd", "cp_blocks": 258,
                 "scan_slabs": 2, "st_blocks": 129, "st_per": 1}
    assert SM.launch_plan(16384, 8192) == {"path": "bins/4096", "hist_blocks": 64, "hist_clamped": False, "nbins": 4096}


def test_keys_are_order_preserving_and_invertible():
    d = np.array([0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 0.5, 1.0, 1.0 + 2.0 ** -52, 3.0, 1e308, np.inf])
    k = SM.keys_of(d)
    assert (np.diff(k.astype(object)) > 0).all() and int(k[0]) == SM.SIGN and int(k[5]) == SM.KEY_ONE
    assert np.array_equal(SM.dists_of(k).view(np.uint64), d.view(np.uint64))
    assert SM.flat([0, 1 << 40, -1]).tolist() == [1.0, 1.0 + 2.0 ** -12, 1.0 - 2.0 ** -53]


# ---- the model by brute force ------------------------------------------------------------------------------------------------------
def _small_sets():
    rng = np.random.default_rng(5)
    for trial in range(300):
        n = int(rng.integers(4096, 12000))
        kind = trial % 5
        if kind == 0:
            d = np.abs(rng.normal(size=n))
        elif kind == 1:
            d = np.round(np.abs(rng.normal(size=n)), 1 + trial % 3)                  # massive ties
        elif kind == 2:
            d = np.abs(rng.normal(size=n)) * 2.0 ** rng.integers(-40, 40, size=n)
            d[rng.integers(0, n, 20)] = 0.0
            d[rng.integers(0, n, 20)] = np.inf
            d[rng.integers(0, n, 20)] = 5e-324
            d[rng.integers(0, n, 20)] = 1e308
        elif kind == 3:
            d = SM.flat(rng.integers(0, 1 << 40, size=n))
            d[rng.integers(0, n, n // 3)] = d[0]
        else:
            p = np.full(n, 0.05)                                                     # small keys mostly where the sample looks:
            p[SM.sample_rows(n)] = 0.5                                               # it overrates their share, short and ok both occur
            d = np.where(rng.random(n) < p, 1.0 + rng.random(n), 1e6 + rng.random(n))
        yield d, int(rng.integers(1, n // 2 + 1))


def test_model_by_brute_force():
    """an independent sort: `ok` means every bin up to b* holds at most BS_CAP keys and at least K keys are <= hi, the kept keys are
    the reference's first K, and the two give-up verdicts mean what they say"""
    seen = set()
    for d, K in _small_sets():
        m = SM.bin_model(d, K)
        seen.add(m["verdict"])
        k = [int(x) for x in SM.keys_of(d)]
        n = len(k)
        stride = n // 4096
        sample = sorted(k[i * stride + stride // 2] for i in range(4096))
        assert m["lo"] == sample[0] and m["hi"] == (sample[m["q"]] | ((1 << 40) - 1)) and m["hi"] >> 40 == sample[m["q"]] >> 40
        assert m["shift"] == 0 or ((m["hi"] - m["lo"]) >> (m["shift"] - 1)) >= 4095
        assert ((m["hi"] - m["lo"]) >> m["shift"]) < 4095
        srt = sorted(k)
        n_le_hi = sum(1 for x in srt if x <= m["hi"])
        assert n_le_hi == m["tot"]
        binof = lambda x: 0 if x <= m["lo"] else (x - m["lo"]) >> m["shift"]
        if n_le_hi < K:
            assert m["verdict"] in ("short", "overflow") and m["bstar"] is None
            if m["verdict"] == "short":
                assert not m["crowded"]
            continue
        bstar = binof(srt[K - 1])                                          # bins are monotone in the key: the K-th key's bin
        fill = {}
        for x in srt[:n_le_hi]:
            fill[binof(x)] = fill.get(binof(x), 0) + 1
        crowded = sorted(b for b, c in fill.items() if b <= bstar and c > SM.BS_CAP)
        assert (m["bstar"], m["crowded"]) == (bstar, crowded)
        assert m["need"] == K - sum(c for b, c in fill.items() if b < bstar)
        assert m["verdict"] == ("overflow" if crowded else "ok")
        if m["verdict"] == "ok":
            assert n_le_hi >= K and all(c <= SM.BS_CAP for b, c in fill.items() if b <= bstar)
            # what the device keeps: whole bins below b*, the first `need` of b* by (key, row) = the reference's first K
            o = SM.reference_order(d)[:K]
            assert (m["bins"][o] <= bstar).all() and (m["bins"][o] >= 0).all()
            assert int((m["bins"][o] == bstar).sum()) == m["need"]
    assert seen == {"ok", "overflow", "short"}


# ---- the constructed inputs of the GPU tests ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SM.CASES))
def test_constructed_case_lands_where_it_is_meant_to(name):
    d, K = SM.CASES[name][0]()
    assert d.dtype == np.float64 and not np.isnan(d).any() and not np.signbit(d).any()
    assert SM.select_path(d.size, K).startswith("bins")
    SM.check_case(name, d, K, SM.bin_model(d, K))
    d2, K2 = SM.CASES[name][0]()                                            # the constructors are deterministic
    assert K2 == K and np.array_equal(d2.view(np.uint64), d.view(np.uint64))


def test_issue_figures():
    """the figures the constructed give-ups were designed to: tot = 1376 at (16384, 5000); 1024 equal keys pass, 1025 do not"""
    d, K = SM.case_short()
    m = SM.bin_model(d, K)
    assert (d.size, K, m["tot"], m["q"], m["verdict"]) == (16384, 5000, 1376, 1375, "short")
    d, K = SM.case_bin_1024()
    assert SM.bin_model(d, K)["verdict"] == "ok" and K == 3000
    d, K = SM.case_overflow_1025()
    m = SM.bin_model(d, K)
    assert m["verdict"] == "overflow" and m["counts"][m["crowded"][0]] == 1025
    d, K = SM.case_crowded_above_chi()
    m = SM.bin_model(d, K)
    assert (d.size, K, m["verdict"]) == (65536, 6000, "ok") and m["counts"].max() >= 1100


def test_flat_layout():
    """the key-exact cases' frame: shift 29, hi = key(1.0) + 2^40 - 1, lo = key(1.0)"""
    for name in ("kth_last_eq_hi", "kth_first_K1", "kth_first_mid", "ties_straddle", "below_lo", "bin_1024", "crowded_above"):
        d, K = SM.CASES[name][0]()
        m = SM.bin_model(d, K)
        assert (m["lo"], m["hi"], m["shift"]) == (SM.KEY_ONE, SM.KEY_ONE + (1 << 40) - 1, SM.FLAT_SHIFT), name
