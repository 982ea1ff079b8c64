"""Every branch of the selection of the K smallest distances and of its sorts (abcsmc_amd/csrc/select.hip) against the stable
argsort of the keys, bit for bit.  Every call goes straight to abc_select_smallest_dev, abc_sort_pairs_dev,
abc_merge_sorted_runs_dev or abc_select_*_dev.

Per call (_select): the outputs sit inside sentinel-filled buffers with guard words on both sides, the input is compared afterwards,
idx and dist are compared as uint64 views -- nothing here has a tolerance.  The case states the path and the verdict it means to
reach and _run_select holds that to the mirror and the exact model (tests/_select_model.py) BEFORE the call; afterwards
Context.select_stats() must have risen by exactly (1, 0) for a bin selection that holds, (1, 1) for one that gives up (overflow,
short) and (0, 0) for the radix path.  Every call is made twice, the second time directly after a call of a different verdict (a
give-up behind an `ok` or a radix call, an `ok` behind a give-up), so that the workspace and the fail word hold the other branch's
leftovers.  A give-up is a designed, flagged branch: it must return the reference result all the same.

The constructed inputs are tests/_select_model.CASES; tests/test_select_model_cpu.py pins their verdicts without a GPU.
test_cases_cover_every_branch holds the union of what the cases state to the list of branches."""
import numpy as np
import pytest

import _select_model as SM

pytestmark = pytest.mark.gpu

GUARD = 8
IDX_SENTINEL = 0x5A5A5A5A5A5A5A5A
DIST_SENTINEL = -1.0            # (no distance is negative)
UNSUPPORTED = -4                # ABC_ERR_UNSUPPORTED
STATED = set()

BRANCHES = {
    # the bin path: instance and verdict, the K-th key's place, the edges of [lo, hi], the bins' filling, the arguments, the sizes
    "bins/4096:ok", "bins/4096:overflow", "bins/4096:short", "bins/16384:ok",
    "kth_last", "kth_first", "ties_straddle", "below_lo", "eq_hi", "hi_plus_1", "tot_eq_K", "bin_1024", "crowded_above", "shift0",
    "empty_bins", "dist_null", "idx_base", "K_1", "K_mid", "K_8192",
    "unsampled_tail", "hist_exact", "hist_clamped", "hist_second_round", "big_smallest", "big_2_20",
    # the radix path
    "radix:init_pairs", "radix:six_pass", "radix:K_n_minus_1", "radix:n_lt_16384", "radix:2K_n_plus_1", "radix:K_gt_2_20",
    "radix:low9", "radix:top_digit", "radix:ties_cp_chunks", "radix:ties_past_slab", "radix:uniform_trip",
    # the sorts
    "sort:none", "sort:chunk", "sort:chunks+merge", "sort:merge_second_round", "sort:lsd", "sort:lsd_per_gt_1",
    "sort_pairs:2", "sort_pairs:4095", "sort_pairs:4096", "sort_pairs:4097", "sort_pairs:32769", "sort_pairs:2^18",
    "sort_pairs:2^18+1", "sort_pairs:lsd_gt_256_blocks",
    # the merge of sorted runs, the distributed protocol, the 48 bits of an index
    "merge:W1", "merge:W2", "merge:W8", "merge:W9", "merge:W17", "merge:len1", "merge:len_odd", "merge:len_pow2",
    "merge:ties_across_runs", "merge:padding",
    "protocol:ties_span_shards", "protocol:idle_shard",
    "idx48:chunk_exact", "idx48:merge_exact", "idx48:bins_exact", "idx48:refused", "idx48:compact_refused",
}


def _state(*names):
    STATED.update(names)
    return names


def _u(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- one call ----------------------------------------------------------------------------------------------------------------------
def _select(gpu_ctx, dd, n, K, base, with_dist):
    """abc_select_smallest_dev on the device tensor dd -> (idx as uint64, dist or None, what select_stats rose by)"""
    import torch
    from abcsmc_amd._lib import lib
    ibuf = torch.full((2 * GUARD + K,), IDX_SENTINEL, dtype=torch.int64, device="cuda:0")
    dbuf = torch.full((2 * GUARD + K,), DIST_SENTINEL, dtype=torch.float64, device="cuda:0")
    gpu_ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    before = gpu_ctx.select_stats()
    gpu_ctx.check(lib().abc_select_smallest_dev(gpu_ctx.handle, dd.data_ptr(), n, K, base, ibuf.data_ptr() + 8 * GUARD,
                                                dbuf.data_ptr() + 8 * GUARD if with_dist else None))
    torch.cuda.synchronize()
    after = gpu_ctx.select_stats()
    ib, db = ibuf.cpu().numpy(), dbuf.cpu().numpy()
    assert (ib[:GUARD] == IDX_SENTINEL).all() and (ib[GUARD + K:] == IDX_SENTINEL).all(), "idx written outside its K words"
    assert (db[:GUARD] == DIST_SENTINEL).all() and (db[GUARD + K:] == DIST_SENTINEL).all(), "dist written outside its K words"
    if not with_dist:
        assert (db == DIST_SENTINEL).all()
    return ib[GUARD:GUARD + K].view(np.uint64), (db[GUARD:GUARD + K] if with_dist else None), (after[0] - before[0], after[1] - before[1])


_DIRTY = {}


def _dirty(gpu_ctx, kind):
    """a small call of a known verdict, run between the two calls of a case: "overflow" (16384 equal keys) or "ok" (chi)"""
    import torch
    if not _DIRTY:
        d_ok, K = SM.case_random("chi", 16384, 100, 9)
        assert SM.bin_model(d_ok, K)["verdict"] == "ok"
        d_ov = np.full(16384, 2.5)
        assert SM.bin_model(d_ov, K)["verdict"] == "overflow" and SM.select_path(16384, K) == "bins/4096"
        _DIRTY["ok"] = (d_ok, torch.from_numpy(d_ok).cuda(), SM.reference_order(d_ok)[:K].astype(np.uint64), (1, 0))
        _DIRTY["overflow"] = (d_ov, torch.from_numpy(d_ov).cuda(), np.arange(K, dtype=np.uint64), (1, 1))
    d, dd, ref, stats = _DIRTY[kind]
    idx, dist, rose = _select(gpu_ctx, dd, d.size, ref.size, 0, True)
    assert rose == stats, (kind, rose)
    assert np.array_equal(idx, ref) and np.array_equal(_u(dist), _u(d[ref.astype(np.int64)]))


def _run_select(gpu_ctx, oracle, d, K, path, verdict=None, base=0, with_dist=True, plan=None, model=None):
    """the case (d, K) must reach `path` (and, on the bin path, `verdict`; on the radix path, the entries of `plan`) by the mirror;
    then the call, a call of another verdict, the call again -- each checked against the reference"""
    import torch
    n = d.size
    got = SM.launch_plan(n, K)
    assert got["path"] == path, got
    if path == "radix":
        assert verdict is None
        assert {k: got[k] for k in (plan or {})} == (plan or {}), got
    else:
        m = model if model is not None else SM.bin_model(d, K)
        assert m["verdict"] == verdict and m["nbins"] == got["nbins"], (m["verdict"], m["tot"], m["crowded"])
    want = SM.expected_stats(path, verdict)
    ref = oracle.ordered(d)[:K]
    assert np.array_equal(ref, SM.reference_order(d)[:K].astype(np.uint64))         # the oracle's order is the stable argsort
    ref_idx = ref + np.uint64(base)
    ref_dist = _u(d[ref.astype(np.int64)])
    dd = torch.from_numpy(d).cuda()
    for rep in range(2):
        idx, dist, rose = _select(gpu_ctx, dd, n, K, base, with_dist)
        print("n=%d K=%d %s %s call %d: select_stats rose by %s, expected %s" % (n, K, path, verdict, rep, rose, want))
        assert rose == want, "call %d: select_stats rose by %s, the mirror and the model say %s" % (rep, rose, want)
        bad = np.nonzero(idx != ref_idx)[0]
        assert bad.size == 0, "call %d: %d of %d indices differ, first at %d: %d, reference %d" % (
            rep, bad.size, K, bad[0], idx[bad[0]], ref_idx[bad[0]])
        if with_dist:
            assert np.array_equal(_u(dist), ref_dist), "call %d: distances differ" % rep
        assert np.array_equal(_u(dd.cpu().numpy()), _u(d)), "the input was written"
        if rep == 0:
            _dirty(gpu_ctx, "ok" if want == (1, 1) else "overflow")


# ---- the bin path ------------------------------------------------------------------------------------------------------------------
# name of _select_model.CASES -> (path, idx_base, dist_out given, what the case states beyond CASES' own properties)
BIN_CASES = {
    "kth_last_eq_hi": ("bins/4096", 0, True, ()),
    "kth_first_K1": ("bins/4096", 0, True, ()),
    "kth_first_mid": ("bins/4096", 0, True, ("K_mid",)),
    "ties_straddle": ("bins/4096", 7_000_000_000, True, ("idx_base", "K_mid")),
    "below_lo": ("bins/4096", 0, False, ("dist_null",)),
    "bin_1024": ("bins/4096", 0, True, ()),
    "crowded_above": ("bins/4096", 0, True, ()),
    "crowded_above_chi": ("bins/4096", 12345, True, ("idx_base",)),
    "shift0": ("bins/4096", 0, True, ()),
    "overflow_1025": ("bins/4096", 3, True, ("idx_base",)),
    "short": ("bins/4096", 0, True, ()),
    "n_16384_plus_4095": ("bins/4096", 0, True, ()),
    "n_131072": ("bins/4096", 0, True, ("hist_exact",)),
    "n_131073": ("bins/4096", 0, True, ()),
    "n_8x131072_plus_1": ("bins/4096", 0, False, ("dist_null",)),
    "big_chi": ("bins/16384", 1 << 40, True, ("big_smallest", "idx_base")),
    "big_lognormal": ("bins/16384", 0, True, ("big_smallest",)),
    "big_2_20": ("bins/16384", 0, True, ("big_2_20",)),
}
for _name, (_path, _base, _wd, _extra) in BIN_CASES.items():
    _state("%s:%s" % (_path, SM.CASES[_name][1]), *SM.CASES[_name][2])
    _state(*_extra)
assert set(BIN_CASES) == set(SM.CASES)


@pytest.mark.parametrize("name", list(BIN_CASES))
def test_bin_selection(gpu_ctx, oracle, name):
    path, base, with_dist, _ = BIN_CASES[name]
    build, verdict, _ = SM.CASES[name]
    d, K = build()
    m = SM.bin_model(d, K)
    SM.check_case(name, d, K, m)                        # the stated properties, by the model
    if name == "n_131072":
        assert not SM.launch_plan(d.size, K)["hist_clamped"] and SM.hist_blocks(d.size) == SM.HIST_BLOCKS
    _run_select(gpu_ctx, oracle, d, K, path, verdict, base=base, with_dist=with_dist, model=m)


# ---- the radix path ----------------------------------------------------------------------------------------------------------------
def _tie_heavy(rng, n):
    """rounded values (massive ties), 80 binades, zeros, subnormals, huge, inf"""
    d = np.abs(rng.normal(size=n)) * 2.0 ** rng.integers(-40, 40, size=n)
    d = np.where(rng.integers(0, 4, size=n) == 0, np.round(np.abs(rng.normal(size=n)), 2), d)
    for v in (0.0, np.inf, 5e-324, 1e308):
        d[rng.integers(0, n, max(n // 200, 1))] = v
    return d


def _r_ties_cp_chunks(rng):
    """10000 rows = 5 CP_CHUNK blocks: 3000 below, 4000 equal to the threshold all over, K takes 2500 of them"""
    d = rng.permutation(np.concatenate((np.full(3000, 0.25) + rng.random(3000) * 0.1, np.full(4000, 0.5), np.full(3000, 1.0))))
    return d, 5500


def _r_ties_past_slab(rng):
    """258 CP_CHUNK blocks, two slabs of k_scan_u32: 700 ties at the threshold, 400 of them in the last 3000 rows (blocks 256 and
    257), all but five taken"""
    n, less = 526337, 263000
    d = np.full(n, 2.0) + rng.random(n)
    rows = rng.permutation(n - 3000)
    d[rows[:less]] = rng.random(less)
    d[rows[less:less + 300]] = 1.5
    d[n - 3000 + rng.permutation(3000)[:400]] = 1.5
    return d, less + 695


RADIX_CASES = {
    # name: (builder(rng) -> (d, K), plan entries the mirror must confirm, what the case states)
    "K_eq_n": (lambda r: (_tie_heavy(r, 5000), 5000), {"radix": "init_pairs", "sort": "chunks+merge"},
               ("radix:init_pairs", "sort:chunks+merge")),
    "K_eq_n_minus_1": (lambda r: (_tie_heavy(r, 5000), 4999), {"radix": "six_pass", "sort": "chunks+merge"},
                       ("radix:six_pass", "radix:K_n_minus_1")),
    "K_1": (lambda r: (_tie_heavy(r, 16383), 1), {"radix": "six_pass", "sort": "none"}, ("sort:none", "radix:n_lt_16384")),
    "n_16383": (lambda r: (_tie_heavy(r, 16383), 4096), {"radix": "six_pass", "sort": "chunk", "hist_blocks": 64},
                ("radix:n_lt_16384", "sort:chunk")),
    "2K_n_plus_1": (lambda r: (SM.chi(r, 20001), 10001), {"radix": "six_pass", "sort": "chunks+merge", "merge_rounds": 1},
                    ("radix:2K_n_plus_1",)),
    "low9": (lambda r: (SM.flat(r.integers(0, 512, size=3000)), 1000), {"radix": "six_pass", "sort": "chunk"}, ("radix:low9",)),
    "top_digit": (lambda r: (SM.dists_of((r.integers(0, 1024, size=2000).astype(np.uint64) << np.uint64(53)) | np.uint64(SM.SIGN)), 700),
                  {"radix": "six_pass", "sort": "chunk"}, ("radix:top_digit",)),
    "ties_cp_chunks": (_r_ties_cp_chunks, {"radix": "six_pass", "cp_blocks": 5, "sort": "chunks+merge"}, ("radix:ties_cp_chunks",)),
    "ties_past_slab": (_r_ties_past_slab, {"radix": "six_pass", "cp_blocks": 258, "scan_slabs": 2, "sort": "lsd", "st_per": 1},
                       ("radix:ties_past_slab", "sort:lsd")),
    "n_131073": (lambda r: (_tie_heavy(r, 131073), 70000), {"radix": "six_pass", "hist_clamped": True, "sort": "chunks+merge",
                                                           "merge_rounds": 3}, ("radix:uniform_trip", "sort:merge_second_round")),
    "K_2_20_plus_1": (lambda r: (SM.lognormal(r, (1 << 21) + 2), (1 << 20) + 1), {"radix": "six_pass", "sort": "lsd", "st_per": 3},
                      ("radix:K_gt_2_20", "sort:lsd_per_gt_1")),
}
for _c in RADIX_CASES.values():
    _state(*_c[2])


@pytest.mark.parametrize("name", list(RADIX_CASES))
def test_radix_selection(gpu_ctx, oracle, name):
    build, plan, _ = RADIX_CASES[name]
    d, K = build(np.random.default_rng(sorted(RADIX_CASES).index(name) + 300))
    if name == "K_2_20_plus_1":
        assert 2 * K <= d.size and SM.select_path(d.size, K - 1) == "bins/16384"      # only K > 2^20 keeps it off the bins
    if name in ("ties_cp_chunks", "ties_past_slab"):
        k = SM.keys_of(d)
        o = SM.reference_order(d)
        T = k[o[K - 1]]
        eq = np.nonzero(k == T)[0]
        taken = int((k[o[:K]] == T).sum())
        assert 0 < taken < eq.size and len(set((eq // SM.CP_CHUNK).tolist())) >= 3
        if name == "ties_past_slab":
            assert o[:K].max() // SM.CP_CHUNK >= 256 and (eq[:taken] // SM.CP_CHUNK >= 256).any()
    _run_select(gpu_ctx, oracle, d, K, "radix", base=1 << 33 if name == "K_eq_n" else 0, plan=plan)


# ---- the sorts ---------------------------------------------------------------------------------------------------------------------
SORT_SIZES = {2: "sort_pairs:2", 4095: "sort_pairs:4095", 4096: "sort_pairs:4096", 4097: "sort_pairs:4097", 32769: "sort_pairs:32769",
              1 << 18: "sort_pairs:2^18", (1 << 18) + 1: "sort_pairs:2^18+1", 526337: "sort_pairs:lsd_gt_256_blocks"}
_state(*SORT_SIZES.values())


@pytest.mark.parametrize("n", list(SORT_SIZES))
def test_sort_pairs_is_stable_by_key(gpu_ctx, n):
    """abc_sort_pairs_dev: a stable sort by key alone -- the values do not ascend, equal keys keep their input order -- at both sides
    of one chunk, of the second round of the eight-wide merge and of the chunk sort's reach, and an LSD sort of more than 256 blocks"""
    import torch
    from abcsmc_amd._lib import lib
    want = {2: "chunk", 4095: "chunk", 4096: "chunk", 4097: "chunks+merge", 32769: "chunks+merge", 1 << 18: "chunks+merge",
            (1 << 18) + 1: "lsd", 526337: "lsd"}[n]
    assert SM.sort_plan(n) == want
    if n == 32769:
        assert SM.merge_rounds(n) == 2 and SM.merge_rounds(n - 1) == 1
    if n == 526337:
        assert SM.st_blocks(n) > 256 and SM.st_per(SM.st_blocks(n)) == 2
    rng = np.random.default_rng(n)
    key = _tie_heavy(rng, n) if n > 2 else np.array([3.0, 3.0])
    val = rng.integers(0, 1 << 48, size=n, dtype=np.int64)                # any 48-bit value, in no order
    val[rng.integers(0, n, 2)] = (1 << 48) - 1
    o = np.argsort(SM.keys_of(key), kind="stable")
    if n > 2:
        ks = SM.keys_of(key)[o]
        assert (np.diff(val[o])[ks[1:] == ks[:-1]] < 0).any()              # ties whose values descend
    else:
        val[:] = (9, 4)
    for rep in range(2):
        kbuf = torch.full((2 * GUARD + n,), DIST_SENTINEL, dtype=torch.float64, device="cuda:0")
        vbuf = torch.full((2 * GUARD + n,), IDX_SENTINEL, dtype=torch.int64, device="cuda:0")
        kbuf[GUARD:GUARD + n] = torch.from_numpy(key).cuda()
        vbuf[GUARD:GUARD + n] = torch.from_numpy(val).cuda()
        gpu_ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        before = gpu_ctx.select_stats()
        gpu_ctx.check(lib().abc_sort_pairs_dev(gpu_ctx.handle, kbuf.data_ptr() + 8 * GUARD, vbuf.data_ptr() + 8 * GUARD, n))
        torch.cuda.synchronize()
        assert gpu_ctx.select_stats() == before
        kb, vb = kbuf.cpu().numpy(), vbuf.cpu().numpy()
        assert (kb[:GUARD] == DIST_SENTINEL).all() and (kb[GUARD + n:] == DIST_SENTINEL).all()
        assert (vb[:GUARD] == IDX_SENTINEL).all() and (vb[GUARD + n:] == IDX_SENTINEL).all()
        assert np.array_equal(_u(kb[GUARD:GUARD + n]), _u(key[o])), "call %d: keys" % rep
        assert np.array_equal(vb[GUARD:GUARD + n], val[o]), "call %d: values (stable order)" % rep
        if rep == 0:
            _dirty(gpu_ctx, "overflow")


# ---- the merge of sorted runs ------------------------------------------------------------------------------------------------------
MERGE_CASES = [(1, 37), (2, 1), (2, 64), (8, 37), (9, 64), (9, 1), (17, 37), (17, 256)]
_state(*["merge:W%d" % W for W, _ in MERGE_CASES], "merge:len1", "merge:len_odd", "merge:len_pow2", "merge:ties_across_runs",
       "merge:padding")


@pytest.mark.parametrize("W,length", MERGE_CASES)
def test_merge_sorted_runs(gpu_ctx, W, length):
    """W runs of `length` pairs, each sorted by (key, idx) with idx ascending in the run number, few distinct keys (equal keys across
    runs: the lower run first), every run padded with (+inf, 2^62) sentinels from a length of its own: the result is the stable sort
    of the concatenation"""
    import torch
    from abcsmc_amd._lib import lib
    rng = np.random.default_rng(100 * W + length)
    key = np.full((W, length), np.inf)
    idx = np.full((W, length), 1 << 62, dtype=np.int64)
    for q in range(W):
        fill = length if (q % 3 == 0 or length == 1) else int(rng.integers(0, length + 1))     # (a run may be all padding)
        kq = np.round(rng.random(fill) * 6) / 4.0
        kq[rng.random(fill) < 0.1] = np.inf                                                     # real +inf keys in front of the padding
        rows = np.sort(rng.choice(1000, size=fill, replace=False)) + 1000 * q
        o = np.lexsort((rows, SM.keys_of(kq)))
        key[q, :fill], idx[q, :fill] = kq[o], rows[o]
    key, idx = key.reshape(-1), idx.reshape(-1)
    n = W * length
    o = np.argsort(SM.keys_of(key), kind="stable")
    if W > 1 and length > 1:
        ks = SM.keys_of(key)
        assert len(set(ks.tolist())) < n                                  # equal keys across runs
    kin, iin = torch.from_numpy(key).cuda(), torch.from_numpy(idx).cuda()
    for rep in range(2):
        kbuf = torch.full((2 * GUARD + n,), DIST_SENTINEL, dtype=torch.float64, device="cuda:0")
        ibuf = torch.full((2 * GUARD + n,), IDX_SENTINEL, dtype=torch.int64, device="cuda:0")
        gpu_ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        gpu_ctx.check(lib().abc_merge_sorted_runs_dev(gpu_ctx.handle, kin.data_ptr(), iin.data_ptr(), W, length,
                                                      kbuf.data_ptr() + 8 * GUARD, ibuf.data_ptr() + 8 * GUARD))
        torch.cuda.synchronize()
        kb, ib = kbuf.cpu().numpy(), ibuf.cpu().numpy()
        assert (kb[:GUARD] == DIST_SENTINEL).all() and (kb[GUARD + n:] == DIST_SENTINEL).all()
        assert (ib[:GUARD] == IDX_SENTINEL).all() and (ib[GUARD + n:] == IDX_SENTINEL).all()
        assert np.array_equal(_u(kb[GUARD:GUARD + n]), _u(key[o])) and np.array_equal(ib[GUARD:GUARD + n], idx[o]), "call %d" % rep
        assert np.array_equal(_u(kin.cpu().numpy()), _u(key)) and np.array_equal(iin.cpu().numpy(), idx)


# ---- the distributed protocol ------------------------------------------------------------------------------------------------------
def test_distributed_protocol_ties_span_shards_and_a_shard_wins_nothing(gpu_ctx, oracle):
    """three shards: the middle one holds only large keys and wins nothing, the threshold's 100 ties sit half in the first and half
    in the last shard; K takes the first shard's 50 and 20 of the last one's"""
    from test_gpu_parity import _distributed_select_replay
    _state("protocol:ties_span_shards", "protocol:idle_shard")
    rng = np.random.default_rng(77)
    n_loc, W = 5000, 3
    d = 5.0 + rng.random(n_loc * W)
    for q in (0, 2):
        rows = q * n_loc + rng.permutation(n_loc)
        d[rows[:1000]] = rng.random(1000)
        d[rows[1000:1050]] = 1.0
    before = gpu_ctx.select_stats()
    out = _distributed_select_replay(gpu_ctx, oracle, d, n_loc, W, (2070, 2001, 2100, 1))
    assert gpu_ctx.select_stats() == before
    cnt, take = out[2070]
    assert [c[0] for c in cnt] == [1000, 0, 1000] and [c[1] for c in cnt] == [50, 0, 50] and take == [50, 0, 20]
    assert out[2001][1] == [1, 0, 0] and out[2100][1] == [50, 0, 50]


# ---- the 48 bits of an index -------------------------------------------------------------------------------------------------------
IDX48_SHAPES = {"chunk": (5000, 3000, "radix", "chunk", "idx48:chunk_exact"), "merge": (6000, 5000, "radix", "chunks+merge", "idx48:merge_exact"),
                "bins": (16384, 5000, "bins/4096", None, "idx48:bins_exact")}
_state(*[s[4] for s in IDX48_SHAPES.values()], "idx48:refused", "idx48:compact_refused")


@pytest.mark.parametrize("shape", list(IDX48_SHAPES))
def test_index_base_up_to_two_to_the_48(gpu_ctx, oracle, shape):
    """idx_base = 2^48 - n: every index exact, on both chunk-sorted shapes of the radix path and on a bin shape; one more is refused
    with ABC_ERR_UNSUPPORTED and a message, nothing written, nothing counted"""
    import torch
    from abcsmc_amd import _lib
    n, K, path, sort, _ = IDX48_SHAPES[shape]
    d = SM.chi(np.random.default_rng(48 + n), n)
    if sort:
        assert SM.launch_plan(n, K)["sort"] == sort
    _run_select(gpu_ctx, oracle, d, K, path, "ok" if path != "radix" else None, base=SM.IDX_LIMIT - n)
    assert int(SM.reference_order(d)[:K].max()) + SM.IDX_LIMIT - n >= SM.IDX_LIMIT - 16          # the top rows are among the winners
    dd = torch.from_numpy(d).cuda()
    before = gpu_ctx.select_stats()
    ibuf = torch.full((K,), IDX_SENTINEL, dtype=torch.int64, device="cuda:0")
    dbuf = torch.full((K,), DIST_SENTINEL, dtype=torch.float64, device="cuda:0")
    for base in (SM.IDX_LIMIT - n + 1, SM.IDX_LIMIT + 1, (1 << 64) - 1):
        with pytest.raises(_lib.AbcError) as e:
            gpu_ctx.check(_lib.lib().abc_select_smallest_dev(gpu_ctx.handle, dd.data_ptr(), n, K, base, ibuf.data_ptr(), dbuf.data_ptr()))
        assert e.value.code == UNSUPPORTED and "2^48" in str(e.value) and "abc_select_smallest_dev" in str(e.value)
    torch.cuda.synchronize()
    assert gpu_ctx.select_stats() == before
    assert (ibuf.cpu().numpy() == IDX_SENTINEL).all() and (dbuf.cpu().numpy() == DIST_SENTINEL).all()


def test_compact_refuses_an_index_base_beyond_two_to_the_48(gpu_ctx):
    import torch
    from abcsmc_amd import _lib
    n = 5000
    dd = torch.from_numpy(SM.chi(np.random.default_rng(1), n)).cuda()
    st = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    ibuf = torch.full((16,), IDX_SENTINEL, dtype=torch.int64, device="cuda:0")
    dbuf = torch.full((16,), DIST_SENTINEL, dtype=torch.float64, device="cuda:0")
    with pytest.raises(_lib.AbcError) as e:
        gpu_ctx.check(_lib.lib().abc_select_compact_dev(gpu_ctx.handle, dd.data_ptr(), n, st.data_ptr(), 8, 8, SM.IDX_LIMIT - n + 1,
                                                        ibuf.data_ptr(), dbuf.data_ptr()))
    assert e.value.code == UNSUPPORTED and "2^48" in str(e.value) and "abc_select_compact_dev" in str(e.value)
    torch.cuda.synchronize()
    assert (ibuf.cpu().numpy() == IDX_SENTINEL).all() and (dbuf.cpu().numpy() == DIST_SENTINEL).all()


# ---- the closing test --------------------------------------------------------------------------------------------------------------
def test_cases_cover_every_branch():
    _state("protocol:ties_span_shards", "protocol:idle_shard")          # (stated inside its test: holds when that test is deselected)
    assert STATED == BRANCHES, (sorted(BRANCHES - STATED), sorted(STATED - BRANCHES))
