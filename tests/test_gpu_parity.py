"""GPU parity tests proper: every stage of the HIP path, called through the C ABI, against the CPU
oracle on the same seeded inputs.  Bar: bit-exact for selection indices, resampled parents and
seeds; <= 1e-6 relative for floating point (tolerances written per assertion; most are far tighter)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-6          # BASELINE.json north_star: "float within 1e-6 rel"


@pytest.fixture(autouse=True)
def _default_kde_mode(request):
    """tests that switch the weight kernel leave the shared context in its default mode, pass or fail"""
    yield
    if "gpu_ctx" in request.fixturenames:
        from abcsmc_amd import _lib
        request.getfixturevalue("gpu_ctx").set_kde_mode(_lib.KDE_AUTO)


def _wl(M, P, N, seed=12345):
    from abcsmc_amd import synthetic
    wl = synthetic.Workload(M, P, seed)
    X, Y = wl.rows(0, N)
    return wl, X, Y, wl.observed()


def _near_tie_ok(idx_a, idx_b, dist_full, tol=1e-9):
    """two orderings agree except where the oracle's distances are within tol (relative)"""
    bad = np.nonzero(idx_a != idx_b)[0]
    for k in bad:
        da, db = dist_full[int(idx_a[k])], dist_full[int(idx_b[k])]
        if abs(da - db) > tol * max(abs(da), abs(db), 1e-300):
            return False
    return True


# ---------------------------------------------------------------------------------------------------
# ranking (AbcUtil.cpp:408-458)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,P,A,f", [
    (1000, 7, 5, 0, 0.5),        # ragged small
    (5000, 32, 16, 8, 0.5),      # BASELINE config shape
    (1001, 12, 3, 3, 0.37),      # odd leading dimension -> scalar-load path, odd split
    (300, 2, 2, 0, 0.5),         # dice-sized (config 1)
    (4097, 20, 1, 4, 0.9),       # single response (P == 1 branch of the PLS loop)
    (777, 40, 24, 10, 1.0),      # f = 1: empty validation set
    (4000, 64, 32, 8, 0.5),      # BASELINE configs[3] shape (6 column blocks, Y'Y blocks skipped)
    (3000, 128, 16, 32, 0.5),    # BASELINE configs[4] shape: 144 columns -> grouped Gram launches, 32 components
    (1500, 100, 28, 12, 0.5),    # ragged wide set
    (4000, 40, 20, 6, 0.5),      # 4 column blocks: the four-wave LDS-DMA Gram kernel (one trailing parameter-only block)
    (2002, 70, 9, 5, 0.45),      # 5 column blocks, parameters share the last block with metrics; split inside a tile
    (3000, 50, 30, 6, 0.4),      # 5 column blocks, last one parameters only
    (2001, 64, 32, 8, 0.5),      # 6 blocks, odd row count: the VGPR-staged kernel (LDS-DMA needs 16-byte row pairs)
    (90, 50, 14, 4, 0.5),        # 4 blocks, fewer rows than one 64-row tile per partition
    (1000, 80, 16, 6, 1.0),      # 6 blocks, f = 1: empty validation partition on the four-wave kernel
    (600, 130, 20, 10, 0.5),     # 150 columns: grouped pairs through the pointer-table mode, 4 groups
    (900, 300, 12, 6, 0.5),      # 312 columns: beyond the LDS-resident model fit's former 160-column limit
    (1200, 600, 16, 8, 0.5),     # 616 columns: the PLS work arrays live in global memory (> 160 KB), 13 column groups
    (1500, 90, 70, 5, 0.5),      # 70 responses: the memory-resident eigen-squaring (the register-resident one stops at 64)
    (800, 40, 100, 3, 0.6),      # more responses than metrics
    (2000, 17, 2, 3, 0.5),       # smallest set on the four-wave latency-tuned fit (k_pls_fit16), two responses
    (2500, 64, 16, 16, 0.5),     # k_pls_fit16, X'X in LDS at its largest, as many components as responses
    (1800, 65, 13, 7, 0.5),      # k_pls_fit16 on eight waves, X'X in registers with ragged quarter rows (qb = 17)
    (1500, 127, 16, 12, 0.45),   # ... odd leading dimension just below the register limit
    (1500, 129, 5, 9, 0.5),      # ... just above it: X'X read from global memory
    (700, 40, 16, 40, 0.5),      # as many components as metrics (XY exhausted after 16: the rest are rounding-level directions)
    (2502, 37, 20, 20, 0.5),     # 17..32 components: the projection on the fp64 matrix pipe; metrics not a multiple of four, rows not of 64
    (1111, 50, 24, 24, 0.5),     # ... odd row count: the last row through the scalar kernel
    (130, 128, 30, 30, 0.5),     # ... fewer rows than one work-group, 128 metrics
])
def test_particle_ranking_pls(gpu_ctx, oracle, N, M, P, A, f):
    wl, X, Y, obs = _wl(M, P, N)
    _ranking_pls_against_oracle(gpu_ctx, oracle, X, Y, obs, f, A)


def test_particle_ranking_pls_unrepresentative_pilot(gpu_ctx, oracle):
    """the first 256 rows -- the rows the statistics' shift is taken from -- 1e3 sigma away from the rest (a grid-ordered first
    set): the one-pass record then carries every value ~1e3 sigma off centre (tests/test_gpu_stats.py bounds its centred
    covariance); the model must still hold the oracle's loadings to 1e-6"""
    wl, X, Y, obs = _wl(32, 16, 4000)
    X[:256] += 1e3 * X.std(axis=0)
    Y[:256] += 1e3 * Y.std(axis=0)
    _ranking_pls_against_oracle(gpu_ctx, oracle, np.asfortranarray(X), np.asfortranarray(Y), obs, 0.5, 8)


def _ranking_pls_against_oracle(gpu_ctx, oracle, X, Y, obs, f, A):
    from abcsmc_amd import abcutil
    g = abcutil.particle_ranking_PLS(X, Y, obs, f, max_comp=A, details=True, ctx=gpu_ctx)
    o = oracle.particle_ranking_pls(X, Y, obs, f, A)
    assert g["ncomp"] == o["ncomp"]
    assert np.allclose(g["mean"], o["mean"], rtol=1e-12)
    assert np.allclose(g["sd"], o["sd"], rtol=1e-11)
    nc = o["ncomp"]
    # loadings: 1e-6 relative to the column norm (same sign convention on both sides)
    for k in range(nc):
        assert np.linalg.norm(g["R"][:, k] - o["R"][:, k]) <= RTOL * np.linalg.norm(o["R"][:, k]), k
    # staged bit-exactness: oracle projection fed the GPU's model == GPU distances, and so the order
    with np.errstate(invalid="ignore", divide="ignore"):
        zobs = np.where(g["sd"] == 0, 0.0, (obs - g["mean"]) / g["sd"])
    so = np.array([_fma_dot(zobs, g["R"][:, k]) for k in range(nc)])
    d_staged = oracle.project_distance(X, g["mean"], g["sd"], g["R"], nc, so)
    order_staged = oracle.ordered(d_staged)
    assert np.array_equal(g["idx"], order_staged), "selection indices not bit-exact given the same model"
    assert np.array_equal(g["dist"], d_staged[order_staged.astype(int)]), "distances not bit-exact"
    # end-to-end against the independent oracle model: equal up to near-ties, distances to 1e-6
    assert np.allclose(g["dist"], o["dist"][g["idx"].astype(int)], rtol=RTOL)
    assert _near_tie_ok(g["idx"], o["idx"], o["dist"])


def test_pls_fit_random_shapes_match_oracle_and_repeat_bitwise(gpu_ctx, oracle):
    """the latency-tuned model fit (k_pls_fit16: five barriers per component, per-wave recomputation instead of cross-wave
    reductions, register-resident X'X) on 36 random shapes (2..16 and 17..32 responses): loadings against the oracle's independent algorithm, and the
    whole model record bit-identical between two runs of the same input (a missing barrier shows up as run-to-run noise)"""
    from abcsmc_amd import abcutil
    rng = np.random.default_rng(20260103)
    for case in range(36):
        M = int(rng.integers(17, 141))
        P = int(rng.integers(2, 17)) if case < 24 else int(rng.integers(17, 33))      # one / two 16 x 16 blocks per side of XY'XY
        A = int(rng.integers(1, min(M, 20) + 1))
        N = int(rng.integers(400, 2500))
        f = float(rng.choice([0.4, 0.5, 0.63, 1.0]))
        wl, X, Y, obs = _wl(M, P, N, seed=1000 + case)
        g = abcutil.particle_ranking_PLS(X, Y, obs, f, max_comp=A, details=True, ctx=gpu_ctx)
        g2 = abcutil.particle_ranking_PLS(X, Y, obs, f, max_comp=A, details=True, ctx=gpu_ctx)
        tag = (case, M, P, A, N, f)
        for key in ("R", "mean", "sd", "dist"):
            assert np.array_equal(g[key], g2[key]), (tag, key)
        assert np.array_equal(g["idx"], g2["idx"]) and g["ncomp"] == g2["ncomp"], tag
        o = oracle.particle_ranking_pls(X, Y, obs, f, A)
        assert g["ncomp"] == o["ncomp"], tag
        for k in range(o["ncomp"]):
            assert np.linalg.norm(g["R"][:, k] - o["R"][:, k]) <= RTOL * np.linalg.norm(o["R"][:, k]), (tag, k)
        assert np.allclose(g["dist"], o["dist"][g["idx"].astype(int)], rtol=RTOL), tag


def _fma_dot(a, b):
    """m-ascending fma chain in float64 (matches orc_* and the kernels) using exact arithmetic"""
    from fractions import Fraction
    s = 0.0
    for x, y in zip(a, b):
        s = float(Fraction(float(x)) * Fraction(float(y)) + Fraction(s))
    return s


@pytest.mark.parametrize("N,M", [(1000, 7), (4099, 32), (50, 3)])
def test_particle_ranking_simple(gpu_ctx, oracle, N, M):
    from abcsmc_amd import abcutil
    wl, X, Y, obs = _wl(M, 4, N)
    g = abcutil.particle_ranking_simple(X, Y, obs, details=True, ctx=gpu_ctx)
    oi, od = oracle.particle_ranking_simple(X, obs)
    assert np.allclose(g["dist"], od[g["idx"].astype(int)], rtol=1e-11)
    assert _near_tie_ok(g["idx"], oi, od)
    assert sorted(g["idx"].tolist()) == list(range(N))


def test_ranking_top_k_is_prefix_of_full_order(gpu_ctx):
    from abcsmc_amd import abcutil
    wl, X, Y, obs = _wl(16, 8, 6000)
    full = abcutil.particle_ranking_PLS(X, Y, obs, 0.5, ctx=gpu_ctx)
    for K in (1, 7, 600, 5999):
        top = abcutil.particle_ranking_PLS(X, Y, obs, 0.5, K=K, ctx=gpu_ctx)
        assert np.array_equal(top, full[:K])


def test_ranking_zero_variance_metric(gpu_ctx, oracle):
    from abcsmc_amd import abcutil
    wl, X, Y, obs = _wl(6, 3, 500)
    X[:, 2] = 3.25                     # constant column: declared z = 0 (reference divides by 0)
    g = abcutil.particle_ranking_PLS(X, Y, obs, 0.5, details=True, ctx=gpu_ctx)
    o = oracle.particle_ranking_pls(X, Y, obs, 0.5, 0)
    assert g["sd"][2] == 0.0 and g["ncomp"] == o["ncomp"]
    assert np.allclose(g["dist"], o["dist"][g["idx"].astype(int)], rtol=RTOL)


def test_ranking_rejects_bad_arguments(gpu_ctx):
    from abcsmc_amd import abcutil, _lib
    wl, X, Y, obs = _wl(6, 3, 100)
    with pytest.raises(ValueError):
        abcutil.particle_ranking_PLS(X, Y, obs, 0.0, ctx=gpu_ctx)          # assert at AbcUtil.cpp:428
    with pytest.raises(_lib.AbcError):
        abcutil.particle_ranking_PLS(X, Y, obs, 0.5, K=101, ctx=gpu_ctx)
    with pytest.raises(_lib.AbcError):
        abcutil.particle_ranking_PLS(X, Y, obs, 0.5, max_comp=7, ctx=gpu_ctx)   # more components than metrics


# ---------------------------------------------------------------------------------------------------
# selection / sort (ranker.h order semantics)
# ---------------------------------------------------------------------------------------------------
def _select(gpu_ctx, d, K, base=0):
    import torch
    from abcsmc_amd._lib import lib
    dd = torch.from_numpy(d).cuda()
    idx = torch.empty(K, dtype=torch.int64, device="cuda")
    out = torch.empty(K, dtype=torch.float64, device="cuda")
    gpu_ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    gpu_ctx.check(lib().abc_select_smallest_dev(gpu_ctx.handle, dd.data_ptr(), d.size, K, base, idx.data_ptr(),
                                                out.data_ptr()))
    torch.cuda.synchronize()
    return idx.cpu().numpy().astype(np.uint64), out.cpu().numpy()


@pytest.mark.parametrize("n,K", [(1, 1), (5, 5), (5, 2), (2048, 100), (2049, 2049), (100000, 10000),
                                 (100000, 99999), (65537, 1)])
def test_select_smallest_random(gpu_ctx, oracle, n, K):
    rng = np.random.default_rng(n * 31 + K)
    d = np.abs(rng.normal(size=n)) * 10.0 ** rng.integers(-3, 4, size=n)
    idx, out = _select(gpu_ctx, d, K)
    ref = oracle.ordered(d)[:K]
    assert np.array_equal(idx, ref)
    assert np.array_equal(out, d[ref.astype(int)])


@pytest.mark.parametrize("n,K,kind", [(200000, 20000, "chi"), (200000, 1, "chi"), (50000, 25000, "lognormal"),
                                      (1000000, 100000, "chi"), (65536, 300, "ties_at_threshold"), (100000, 5000, "outliers"),
                                      (16384, 8192, "chi"), (300000, 150000, "binades"),
                                      (10_000_000, 1_000_000, "chi"), (4_000_000, 1 << 20, "lognormal"), (3_000_000, 300_000, "binades")])
def test_select_smallest_sampled_bins(gpu_ctx, oracle, n, K, kind):
    """large sets, at most half kept: the sampled-range bin selection (k_bs_*) instead of radix select + sort; same array.
    Round 4: up to 2^20 winners (16384 bins beyond 2^18: the 1e6 winners of configs[3] at its stated size)"""
    rng = np.random.default_rng(n + 7 * K)
    if kind == "chi":
        d = np.sqrt((rng.normal(size=(n, 8)) ** 2).sum(axis=1))            # distances in an 8-dimensional score space
    elif kind == "lognormal":
        d = np.exp(3.0 * rng.normal(size=n))
    elif kind == "binades":
        d = np.abs(rng.normal(size=n)) * 2.0 ** rng.integers(-40, 40, size=n)
    elif kind == "outliers":
        d = np.abs(rng.normal(size=n)) + 1.0
        d[rng.integers(0, n, 50)] = np.inf
        d[rng.integers(0, n, 50)] = 1e300
        d[rng.integers(0, n, 5)] = 0.0
    else:
        d = np.abs(rng.normal(size=n))
        t = np.partition(d, K - 1)[K - 1]
        d[rng.integers(0, n, 500)] = t                                     # 500 more keys equal to the K-th: lowest indices win
    idx, out = _select(gpu_ctx, d, K, base=12345)
    ref = oracle.ordered(d)[:K]
    assert np.array_equal(idx, ref + np.uint64(12345))
    assert np.array_equal(out, d[ref.astype(int)])


def test_generation_with_massive_distance_ties_repeats_with_the_radix_select(gpu_ctx, oracle):
    """2048 copies of each of 16 particles: every bin of the sampled-range selection overflows, the generation notices at its
    final synchronisation and repeats itself with the radix select; the result is the oracle's"""
    import torch
    from abcsmc_amd import abcutil, device, _lib
    M, P, A, reps = 6, 3, 2, 2048
    wl, X0, Y0, obs = _wl(M, P, 16)
    X, Y = np.asfortranarray(np.tile(X0, (reps, 1))), np.asfortranarray(np.tile(Y0, (reps, 1)))
    N, K, Nn = X.shape[0], 5000, 4096
    spec = wl.prior_spec()
    dev = "cuda:0"
    gen = device.Generation(N, M, P, K, 0, Nn, 0.5, A, multivariate=False, device=dev)
    r = abcutil.rng(99)
    sel0, rep0 = gen.ctx.select_stats(), gen.ctx.generation_repeats()
    gen.run(device.colmajor(X, dev), device.colmajor(Y, dev), device.colmajor(obs, dev),
            device.priors_to_device(_lib.make_priors(spec), dev), r)
    torch.cuda.synchronize()
    # the bin path did answer first (a selection counted), its give-up was the generation's to find (none counted by the selection
    # itself) and cost exactly one repeat of the generation
    sel1, rep1 = gen.ctx.select_stats(), gen.ctx.generation_repeats()
    assert sel1[0] - sel0[0] >= 1 and sel1[1] == sel0[1] and rep1[1] - rep0[1] == 1
    o = oracle.rng(99)
    ref = oracle.generation(X, Y, obs, oracle.make_priors(spec), K, Nn, o, None, None, None, train_frac=0.5, max_comp=A,
                            multivariate=False)
    assert np.array_equal(gen.idx.cpu().numpy().astype(np.uint64), ref["idx"])
    assert np.array_equal(gen.parent.cpu().numpy().astype(np.uint64), ref["parent"])
    import ctypes as C
    r2 = abcutil.rng(99)                                   # the repeated call must not have advanced the stream twice
    _lib.lib().abc_rng_jump(C.byref(r2), 2 * Nn)
    assert (r.s1, r.s2, r.s3) == (r2.s1, r2.s2, r2.s3)


def test_weighted_generation_with_distance_ties_repeats_before_the_alias_build(gpu_ctx, oracle):
    """the same degenerate distances (16 distinct metric rows, 2048 copies each) in a WEIGHTED, MULTIVARIATE generation: the
    give-up flag of the bin selection reaches the host at its wait for the weights, the generation repeats itself with the radix
    select before any alias table, draw or proposal of the placeholder winners is queued; results are the oracle's, the rng
    advanced once, no phantom give-ups"""
    import torch
    from abcsmc_amd import abcutil, device, _lib
    M, P, A, reps = 6, 3, 2, 2048
    wl, X0, Y0, obs = _wl(M, P, 16)
    X = np.asfortranarray(np.tile(X0, (reps, 1)))
    _, Y = wl.rows(100, 100 + 16 * reps)                        # distinct parameter rows: the posterior covariance is regular
    N, K, Kp, Nn = X.shape[0], 5000, 300, 4096
    spec = wl.prior_spec()
    prev = wl.previous_set(Kp)
    dev = "cuda:0"
    gpu_ctx.perturb_giveups(reset=True)
    gen = device.Generation(N, M, P, K, Kp, Nn, 0.5, A, multivariate=True, device=dev, ctx=gpu_ctx)
    r = abcutil.rng(99)
    gen.run(device.colmajor(X, dev), device.colmajor(Y, dev), device.colmajor(obs, dev),
            device.priors_to_device(_lib.make_priors(spec), dev), r, *(device.colmajor(a, dev) for a in prev))
    torch.cuda.synchronize()
    o = oracle.rng(99)
    ref = oracle.generation(X, Y, obs, oracle.make_priors(spec), K, Nn, o, *prev, train_frac=0.5, max_comp=A, multivariate=True)
    assert np.array_equal(gen.idx.cpu().numpy().astype(np.uint64), ref["idx"])
    assert np.allclose(gen.w.cpu().numpy(), ref["w"], rtol=RTOL)
    assert np.array_equal(gen.parent.cpu().numpy().astype(np.uint64), ref["parent"])
    assert np.isfinite(device.to_numpy(gen.next)).all()
    r2 = abcutil.rng(99)
    _lib.lib().abc_rng_jump(C.byref(r2), 2 * Nn)
    assert (r.s1, r.s2, r.s3) == (r2.s1, r2.s2, r2.s3)
    assert gpu_ctx.perturb_giveups() == 0


def test_select_smallest_ties_and_offsets(gpu_ctx, oracle):
    rng = np.random.default_rng(4)
    d = rng.integers(0, 50, size=30000).astype(np.float64)      # massive ties: index tie-break decides
    for K in (1, 599, 600, 601, 15000, 30000):
        idx, out = _select(gpu_ctx, d, K, base=7_000_000_000)
        ref = oracle.ordered(d)[:K]
        assert np.array_equal(idx, ref + np.uint64(7_000_000_000))
    d[:] = 2.5                                                    # all equal
    idx, _ = _select(gpu_ctx, d, 1234)
    assert np.array_equal(idx, np.arange(1234, dtype=np.uint64))
    d = np.array([0.0, 1e-310, 5e-324, 1e308, np.inf, 3.0])       # zero, subnormals, huge, inf
    idx, _ = _select(gpu_ctx, d, 6)
    assert np.array_equal(idx, oracle.ordered(d))


def test_sort_pairs(gpu_ctx, oracle):
    import torch
    from abcsmc_amd._lib import lib
    rng = np.random.default_rng(8)
    key = np.round(np.abs(rng.normal(size=50000)), 2)
    val = rng.permutation(50000).astype(np.int64)
    k, v = torch.from_numpy(key.copy()).cuda(), torch.from_numpy(val.copy()).cuda()
    gpu_ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    gpu_ctx.check(lib().abc_sort_pairs_dev(gpu_ctx.handle, k.data_ptr(), v.data_ptr(), key.size))
    torch.cuda.synchronize()
    o = np.argsort(key, kind="stable")
    assert np.array_equal(k.cpu().numpy(), key[o]) and np.array_equal(v.cpu().numpy(), val[o])


def _tie_heavy_keys(rng, n):
    """distances with every kind of trouble: rounded values (massive ties), 80 binades, zeros, subnormals, huge, inf"""
    d = np.abs(rng.normal(size=n)) * 2.0 ** rng.integers(-40, 40, size=n)
    q = rng.integers(0, 4, size=n)
    d = np.where(q == 0, np.round(np.abs(rng.normal(size=n)), 2), d)       # ~300 distinct values over a quarter of the keys
    d[rng.integers(0, n, 200)] = 0.0
    d[rng.integers(0, n, 200)] = np.inf
    d[rng.integers(0, n, 200)] = 5e-324
    d[rng.integers(0, n, 200)] = 1e308
    return d


@pytest.mark.parametrize("n", [(1 << 18) + 1, 500_000, 1_000_000, 2_500_000])
def test_sort_pairs_beyond_the_chunk_sort(gpu_ctx, n):
    """more than SC_MAX_N = 2^18 pairs: the eight 8-bit LSD radix passes (k_sort_hist / k_sort_scan / k_sort_scatter with
    n / ST_CHUNK histogram blocks under the one-block scan, select.hip: sort_pairs_u64) -- the path K = 1e6 winners of
    BASELINE configs[3] and any 2-rank run of it (K / G = 5e5) take.  Stable order = numpy's stable argsort"""
    import torch
    from abcsmc_amd._lib import lib
    rng = np.random.default_rng(n)
    key = _tie_heavy_keys(rng, n)
    val = rng.permutation(n).astype(np.int64)
    k, v = torch.from_numpy(key.copy()).cuda(), torch.from_numpy(val.copy()).cuda()
    gpu_ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    gpu_ctx.check(lib().abc_sort_pairs_dev(gpu_ctx.handle, k.data_ptr(), v.data_ptr(), key.size))
    torch.cuda.synchronize()
    o = np.argsort(key, kind="stable")
    assert np.array_equal(k.cpu().numpy(), key[o]) and np.array_equal(v.cpu().numpy(), val[o])


@pytest.mark.parametrize("n,K,kind", [
    ((1 << 18) + 1, (1 << 18) + 1, "ties"),     # K == n just beyond the chunk sort: full LSD sort of all keys
    (600_000, (1 << 18) + 1, "ties"),           # K one beyond the bin selection's reach (2 K <= n): radix select + LSD sort
    (1_000_000, 500_000, "chi"),                # 2 K == n, K > 2^18: radix select
    (1_000_000, 500_001, "ties"),               # 2 K > n
    (2_000_000, 1_000_000, "ties"),             # configs[3] winners on one GPU
    (3_000_000, 1_000_000, "ties_at_threshold"),
    (1_000_000, 1_000_000, "chi"),              # K == n
])
def test_select_smallest_beyond_two_to_the_18(gpu_ctx, oracle, n, K, kind):
    """K > 2^18 or 2 K > n: six-pass radix select (select.hip: select_by_radix), stable compaction, and for more than 2^18
    winners the LSD radix sort; indices and distances bit-exact against the oracle's (distance, index) order"""
    rng = np.random.default_rng(n + 13 * K)
    if kind == "chi":
        d = np.sqrt((rng.normal(size=(n, 8)) ** 2).sum(axis=1))
    elif kind == "ties":
        d = _tie_heavy_keys(rng, n)
    else:
        d = np.abs(rng.normal(size=n))
        t = np.partition(d, K - 1)[K - 1]
        d[rng.integers(0, n, 5000)] = t                 # 5000 more keys equal to the K-th: lowest indices win
    idx, out = _select(gpu_ctx, d, K, base=1 << 40)
    ref = oracle.ordered(d)[:K]
    assert np.array_equal(idx, ref + np.uint64(1 << 40))
    assert np.array_equal(out, d[ref.astype(np.int64)])


# ---------------------------------------------------------------------------------------------------
# doubled variance, weights, MVN setup
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,P", [(2, 1), (1000, 16), (4097, 5)])
def test_doubled_variance(gpu_ctx, oracle, K, P):
    from abcsmc_amd import abcutil
    th = np.random.default_rng(K).normal(size=(K, P)) * 50 + 1000
    assert np.allclose(abcutil.calculate_doubled_variance(th, ctx=gpu_ctx), oracle.doubled_variance(th), rtol=1e-10)


def _weights_case(P, K, Kp, seed):
    from abcsmc_amd import synthetic
    wl = synthetic.Workload(8, P, seed)
    _, th = wl.rows(0, K)
    th = np.asfortranarray(wl.mu_y + 0.4 * (th - wl.mu_y))
    tp, wp, dv = wl.previous_set(Kp)
    wp = np.random.default_rng(seed).random(Kp)
    wp /= np.linalg.norm(wp)
    return wl, th, tp, wp, dv


# The pair sums run on one of two kernels (include/abcsmc_hip.h: abc_ctx_set_kde_mode).  Tolerances, relative, per weight:
#   fp64 vector kernel                      1e-9  (measured ~1e-12)
#   split-operand matrix-pipe kernel (auto)  2.5e-7 (<= 2e-8 absolute in the base-2 exponent of a term; north star: 1e-6)
#   ... at 17..32 parameters (two chunks)    3e-7 } (the limb products left out, h1.r2' + r2.h1', grow with sqrt(P))
#   ... at 33..64 parameters (three / four chunks)   7e-7 }
# Largest error over ~15 000 weights per parameter count, every count from 5 to 64, far rows, zero and sixty-binade weights
# (tests/fuzz/kde_accuracy_sweep.py -> profiles/history/r03_kde_accuracy.json): 2.15e-7 up to 16 parameters, 2.43e-7 at 17..32, 4.1e-7 at 33..64;
# over 980 whole generations at random shapes (tests/fuzz/generation_fuzz.py -> profiles/history/r03_generation_fuzz.json): 3.1e-7 / 3.1e-7 / 5.2e-7.
# (the bounds below are for THESE tests' fixed seeds; the kernel's error budget for a weight that one term dominates is 5e-7 / 5.5e-7 / 8e-7)
KDE_TOL = {"fp64": 1e-9, "auto": 2.5e-7}


def _kde_tol(mode, P):
    if mode != "auto":
        return KDE_TOL[mode]
    return 7e-7 if 32 < P <= 64 else 3e-7 if 16 < P <= 32 else KDE_TOL[mode]


class _kde_mode:
    def __init__(self, ctx, mode):
        self.ctx, self.mode = ctx, mode

    def __enter__(self):
        from abcsmc_amd import _lib
        self.ctx.set_kde_mode(_lib.KDE_FP64 if self.mode == "fp64" else _lib.KDE_AUTO)

    def __exit__(self, *a):
        from abcsmc_amd import _lib
        self.ctx.set_kde_mode(_lib.KDE_AUTO)


@pytest.mark.parametrize("mode", ["auto", "fp64"])
@pytest.mark.parametrize("P,K,Kp", [(16, 700, 900), (2, 100, 64), (5, 1, 130), (32, 300, 257), (3, 2500, 70), (48, 200, 150),
                                    (9, 513, 31), (20, 65, 1000), (13, 1, 40), (33, 130, 97), (64, 257, 300), (57, 64, 1030),
                                    (70, 90, 80),
                                    # either side of the parameter counts up to which the norm pieces ride in spare K-slots (13, 29, 61)
                                    (13, 200, 333), (14, 200, 333), (29, 150, 260), (30, 150, 260), (61, 100, 140), (62, 100, 140),
                                    # ... and of the three-chunk kernels of round 6 (33..45 folded, 46..48 not, 49 four chunks again)
                                    (45, 100, 140), (46, 100, 140), (49, 100, 140)])
def test_weight_predictive_prior(gpu_ctx, oracle, P, K, Kp, mode):
    from abcsmc_amd import abcutil, _lib
    wl, th, tp, wp, dv = _weights_case(P, K, Kp, 77 + P)
    spec = wl.prior_spec()
    with _kde_mode(gpu_ctx, mode):
        w = abcutil.weight_predictive_prior(_lib.make_priors(spec), th, tp, wp, dv, ctx=gpu_ctx)
        # the split-operand kernel takes 5..64 parameters (padded to 8, 16, 32 or 64 columns) unless fp64 was asked for
        expect_split = mode == "auto" and 5 <= P <= 64
        assert gpu_ctx.kde_last_kernel() == (_lib.KDE_RAN_SPLIT if expect_split else _lib.KDE_RAN_FP64)
    ref = oracle.weights_importance(oracle.make_priors(spec), th, tp, wp, dv)
    assert np.all(ref > 0)
    assert np.allclose(w, ref, rtol=RTOL, atol=0)
    print("P = %d K = %d K' = %d %s: max rel err %.2e" % (P, K, Kp, mode, np.max(np.abs(w - ref) / ref)))
    assert np.max(np.abs(w - ref) / ref) < _kde_tol(mode, P)
    assert np.linalg.norm(w) == pytest.approx(1.0, rel=1e-12)          # L2, not L1 (AbcUtil.cpp:583)


@pytest.mark.parametrize("K,Kp,P", [(300, 257, 3), (1000, 700, 16), (129, 64, 40)])
def test_weight_epanechnikov_extension(gpu_ctx, oracle, K, Kp, P):
    """ABC_WEIGHT_EPANECHNIKOV (an extension without a reference counterpart: AbcUtil.cpp:476 only names it) against its
    oracle restatement; off by default; particles outside every previous particle's support get weight 0; a converged
    parameter (dv' = 0) takes no part"""
    from abcsmc_amd import abcutil, _lib
    wl, th, tp, wp, dv = _weights_case(P, K, Kp, 7)
    spec = wl.prior_spec()
    dv = dv.copy()
    if P > 4:
        dv[2] = 0.0
    th = th.copy()
    th[5] = th[5] + 40 * np.sqrt(np.where(dv > 0, dv, 1.0))            # far from everything: no support
    pri, opri = _lib.make_priors(spec), oracle.make_priors(spec)
    w_gauss = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx) if P <= 4 or dv[2] != 0 else None
    gpu_ctx.set_weight_kernel(_lib.WEIGHT_EPANECHNIKOV)
    try:
        w = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx)
    finally:
        gpu_ctx.set_weight_kernel(_lib.WEIGHT_GAUSSIAN)
    ref = oracle.weights_epanechnikov(opri, th, tp, wp, dv)
    assert w[5] == 0.0 and ref[5] == 0.0
    ok = ref > 0
    assert ok.sum() > K // 2 and np.allclose(w[ok], ref[ok], rtol=1e-9) and np.array_equal(w == 0, ref == 0)
    assert np.linalg.norm(w) == pytest.approx(1.0, rel=1e-12)
    if w_gauss is not None:
        assert not np.allclose(w, w_gauss, rtol=1e-3)                   # it is a different kernel


@pytest.mark.parametrize("P", [16, 13, 12, 7])
def test_weight_split_kernel_accuracy_and_zero_weights(gpu_ctx, oracle, P):
    """the split-operand kernel on a set large enough for many column slices and tiles: against the oracle and against
    the fp64 kernel; previous particles of weight exactly 0 (inside the exact range) contribute exactly nothing.  Up to 13
    parameters run the seven-MFMA variant (norm pieces in the spare K-slots of the limb operands), 14..16 the nine-MFMA one"""
    from abcsmc_amd import abcutil, _lib
    K, Kp = 3000, 5000
    wl, th, tp, wp, dv = _weights_case(P, K, Kp, 4242)
    wp = wp.copy()
    wp[::97] = 0.0
    pri = _lib.make_priors(wl.prior_spec())
    ref = oracle.weights_importance(oracle.make_priors(wl.prior_spec()), th, tp, wp, dv)
    w = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx)
    assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_SPLIT
    with _kde_mode(gpu_ctx, "fp64"):
        w64 = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx)
        assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_FP64
    err, err64 = np.abs(w - ref) / ref, np.abs(w64 - ref) / ref
    print("split kernel: max rel err %.2e (rms %.2e); fp64 kernel: %.2e" % (err.max(), np.sqrt((err ** 2).mean()), err64.max()))
    assert err64.max() < 1e-9 and err.max() < KDE_TOL["auto"]
    keep = wp != 0.0
    w2 = abcutil.weight_predictive_prior(pri, th, tp[keep], wp[keep], dv, ctx=gpu_ctx)
    assert np.max(np.abs(w2 - w) / w) < KDE_TOL["auto"]


@pytest.mark.parametrize("P,K,Kp,heavy", [(16, 2500, 6000, False), (14, 1300, 4000, True), (32, 1500, 5000, False), (64, 700, 3000, True),
                                          (48, 900, 3100, True), (46, 700, 2000, False)])      # (three chunks, round 6)
def test_weight_split_kernel_with_tiles_in_the_order_of_the_norm_tops(gpu_ctx, oracle, monkeypatch, P, K, Kp, heavy):
    """full 16-parameter chunks and enough pairs: the previous set's tiles are filled in the order of the rows' norm tops and the
    kernel subtracts top and batch reference in one MFMA step (KS_TOPN; forced here at a test's size).  Against the oracle and the fp64
    kernel, with zero weights and far rows; `heavy`: previous weights over 60 binades, so that the sparse ends of the order make
    wide tiles (handled the plain way inside the same kernel); bit-identical when repeated; equal to the plain variant's
    weights to the kernel's tolerance"""
    from abcsmc_amd import abcutil, _lib
    wl, th, tp, wp, dv = _weights_case(P, K, Kp, 77 + P)
    wp = wp.copy()
    if heavy:
        wp *= np.exp2(np.random.default_rng(3).uniform(-60, 0, Kp))
    wp[::101] = 0.0
    th, tp = th.copy(), tp.copy()
    unit = np.sqrt(dv) / np.sqrt(np.log2(np.e))
    th[5, 2] += 12.0 * unit[2]
    tp[9, P - 1] -= 11.0 * unit[P - 1]
    pri = _lib.make_priors(wl.prior_spec())
    ref = oracle.weights_importance(oracle.make_priors(wl.prior_spec()), th, tp, wp, dv)
    monkeypatch.setenv("ABC_KDE_TOPN_MIN_PAIRS", "1e30")
    w_plain = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx)
    monkeypatch.setenv("ABC_KDE_TOPN_MIN_PAIRS", "0")
    w = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx)
    assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_SPLIT
    w2 = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx)
    monkeypatch.delenv("ABC_KDE_TOPN_MIN_PAIRS")
    ok = ref > 0
    err = np.abs(w - ref)[ok] / ref[ok]
    print("P = %d tiles by norm top: max rel err %.2e (rms %.2e); against the plain variant %.2e" %
          (P, err.max(), np.sqrt((err ** 2).mean()), np.max(np.abs(w - w_plain)[ok] / ref[ok])))
    assert ok.sum() >= K - 1 and err.max() < _kde_tol("auto", P) and np.array_equal(w == 0, ref == 0)
    assert np.array_equal(w, w2)
    assert np.max(np.abs(w - w_plain)[ok] / ref[ok]) < 2 * _kde_tol("auto", P)


@pytest.mark.parametrize("P,K,Kp", [(40, 2100, 3000), (64, 1500, 4100), (47, 1100, 2100)])
def test_weight_split_kernel_accuracy_at_33_to_64_parameters(gpu_ctx, oracle, P, K, Kp):
    """33..64 parameters: three (up to 48 parameters, round 6) or four 16-parameter chunks per pair (19-21 / 25-27 matrix instructions
    per 1024 pairs), the previous tiles staged in LDS and shared by a work-group's waves, many tiles and column slices, an odd and
    an even number of previous tiles per slice; against the oracle and the fp64 kernel, with previous weights of exactly 0 and one
    far row on each side"""
    from abcsmc_amd import abcutil, _lib
    wl, th, tp, wp, dv = _weights_case(P, K, Kp, 1000 + P)
    wp = wp.copy()
    wp[::89] = 0.0
    th, tp = th.copy(), tp.copy()
    unit = np.sqrt(dv) / np.sqrt(np.log2(np.e))
    th[11, 3] += 12.0 * unit[3]                                   # a far new particle (fix-up in fp64)
    tp[17, P - 1] -= 11.0 * unit[P - 1]                           # a far previous particle
    pri = _lib.make_priors(wl.prior_spec())
    ref = oracle.weights_importance(oracle.make_priors(wl.prior_spec()), th, tp, wp, dv)
    w = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx)
    assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_SPLIT
    with _kde_mode(gpu_ctx, "fp64"):
        w64 = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx)
        assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_FP64
    ok = ref > 0
    err, err64 = np.abs(w - ref)[ok] / ref[ok], np.abs(w64 - ref)[ok] / ref[ok]
    print("P = %d split kernel: max rel err %.2e (rms %.2e); fp64 kernel: %.2e" % (P, err.max(), np.sqrt((err ** 2).mean()), err64.max()))
    assert ok.sum() >= K - 1 and err64.max() < 1e-9 and err.max() < _kde_tol("auto", P)
    assert np.array_equal(w == 0, ref == 0)


def test_weight_split_kernel_staging_does_not_change_the_sums():
    """33..64 parameters since round 6: the previous tiles are staged in LDS (k_kde_split_lds, two or three waves per SIMD) instead
    of being held in registers (k_kde_split, one wave per SIMD), and up to 48 parameters three chunks are stored and multiplied
    instead of four.  The staging changes where an operand comes from, not one matrix step: at 49..64 parameters the weights were the
    register kernel's BIT FOR BIT, and so were the four-chunk LDS kernel's at 33..48; the three-chunk kernels (the fourth chunk's
    products were exact zeros; the norm pieces ride in another chunk's spare slots up to 45 parameters, and 46..48 lose the folded
    variant) agreed with them far inside the kernel's error budget.  The register kernel and the four-chunk setting at 33..48 are
    retired: the sha256 of the weights the LDS kernels gave when they were checked against them are pinned here, and the kernels
    must still give exactly those bits."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pinned = {
        33: ("96a2168854e07ecad9ce4d478bddd7a6b694f7de6e9a375764b592fe766d6eb2", 1.87226878815456246e+01),
        45: ("00386d60c187b095d648f980c35ec568d192ded136e25727728b59a875fee828", 1.19730772430102377e+01),
        46: ("1442f5bca7a83db2aaeb35bf2a152af7fd163edb6283af18ec22a4049000de35", 7.47766780147603427e+00),
        48: ("a7aba27b0a5648ed4076a363f59983f2b2a31f981a1f5d6fdf22b9adbd7550d0", 1.13914449815631329e+01),
        49: ("e11ac59afd1b850fae4789d48b3592add83b08183967ba3162fa38ef663f259b", 3.82582272153152703e+00),
        61: ("7112143a4faeab0a5ad7af2b132e5320ac1e9afae9f8c817f4941a954d485e9f", 1.77819062987579901e+00),
        62: ("3eb48bcaad21ce3aa96e824f2b0cee95525f450afe489767a6896ac81ca6f39f", 2.32794576292930167e+00),
        64: ("6e1abd4e257763a792fd7fe5f55b6c92938550ab6f68809661d5daafb3e5639f", 1.00941719085734221e+01),
    }
    counts = [str(P) for P in pinned]
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "_kde_worker.py")] + counts, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ABC_DIAG="1"), cwd=root)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = [l.split() for l in p.stdout.splitlines() if l.startswith("KDE ")]
    assert [r[1] for r in rows] == counts
    for r in rows:
        P = int(r[1])
        assert r[2] == pinned[P][0], (P, float(r[3]), pinned[P][1])


@pytest.mark.parametrize("P", [16, 11])
def test_weight_split_kernel_range_edges(gpu_ctx, oracle, P):
    """rows OUTSIDE the range the split-operand kernel is exact on (a scaled coordinate above 8, a squared norm above 400, a
    previous weight outside [2^-300, 2^100]: weights.hip, KS_BOUND, KS_NORM2, KS_LW_CAP, KS_LW_MIN), written when the range was
    wider: every row moved here -- 9.0 to 9.5 scaled units from the centre, then one coordinate 10.6 units out --, and the
    previous weights 1e-150 (-log2: 498) and 1e-200, are 'far' under today's bounds.  Such a ROW leaves the matrix work and its
    pairs are added in fp64 by the fix-up kernels: the call stays on the split kernel and still matches the oracle, with more
    and more far rows from step to step.  The edges themselves, from both sides and through the kernel word, are in
    tests/test_gpu_weights_branches.py (test_range_edges_of_the_new_rows, test_range_edges_of_the_previous_weights,
    test_whole_range_shifted_to_its_edges)"""
    from abcsmc_amd import abcutil, _lib
    K, Kp = 400, 600
    wl, th, tp, wp, dv = _weights_case(P, K, Kp, 99)
    spec = [(_lib.PRIOR_GAUSS, 0.0, 1e9)] * P
    pri, opri = _lib.make_priors(spec), oracle.make_priors(spec)
    unit = np.sqrt(dv) / np.sqrt(np.log2(np.e))          # one scaled unit of parameter p (weights.hip: k_wscale)
    centre = tp.mean(axis=0)
    th, tp, wp = th.copy(), tp.copy(), wp.copy()
    th[5, :] = centre + 9.3 * unit * np.where(np.arange(P) % 2, 1.0, -1.0)      # every coordinate ~9.3 units out
    th[6, 3] = centre[3] - 9.5 * unit[3]
    tp[7, :] = centre + 9.0 * unit                                            # a previous particle equally far
    tp[8, :] = th[5, :] + 0.3 * unit                                          # ... and one next to the far current one
    wp[9], wp[10] = 1e-150, 0.0
    ref = oracle.weights_importance(opri, th, tp, wp, dv)
    w = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx)
    assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_SPLIT
    assert np.all(ref > 0) and np.max(np.abs(w - ref) / ref) < KDE_TOL["auto"]
    th2 = th.copy()
    th2[6, 3] = centre[3] - 10.6 * unit[3]                                    # a far new particle
    ref2 = oracle.weights_importance(opri, th2, tp, wp, dv)
    w2 = abcutil.weight_predictive_prior(pri, th2, tp, wp, dv, ctx=gpu_ctx)
    assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_SPLIT
    assert np.max(np.abs(w2 - ref2) / ref2) < KDE_TOL["auto"]
    assert abs(w2[6] - ref2[6]) / ref2[6] < KDE_TOL["fp64"]                  # the far row itself: summed in fp64
    wp3 = wp.copy()
    wp3[9] = 1e-200                                                           # a far previous particle
    ref3 = oracle.weights_importance(opri, th, tp, wp3, dv)
    w3 = abcutil.weight_predictive_prior(pri, th, tp, wp3, dv, ctx=gpu_ctx)
    assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_SPLIT
    assert np.max(np.abs(w3 - ref3) / ref3) < KDE_TOL["auto"]


@pytest.mark.parametrize("P", [16, 10])
def test_weight_far_rows_are_fixed_up_row_by_row(gpu_ctx, oracle, P):
    """particles outside the split-operand kernel's exact range on BOTH sides, scattered over tiles and slices: far new
    particles next to far previous ones (their mutual term dominates both sums), a far previous particle next to ordinary
    new ones, previous particles of weight 0 among the far ones.  Everything stays on the split kernel + fix-ups and
    matches the oracle; the result is bit-reproducible; with more far rows than the fix-ups take, the fp64 kernel runs."""
    from abcsmc_amd import abcutil, _lib
    K, Kp = 1500, 2100
    wl, th, tp, wp, dv = _weights_case(P, K, Kp, 1234)
    spec = [(_lib.PRIOR_GAUSS, 0.0, 1e9)] * P
    pri, opri = _lib.make_priors(spec), oracle.make_priors(spec)
    unit = np.sqrt(dv) / np.sqrt(np.log2(np.e))
    centre = tp.mean(axis=0)
    th, tp, wp = th.copy(), tp.copy(), wp.copy()
    rng = np.random.default_rng(7)
    far_i = [3, 40, 41, 777, 1499]
    far_j = [0, 65, 1000, 2099, 2098]
    for n, (i, j) in enumerate(zip(far_i, far_j)):
        d = rng.normal(size=P)
        d *= (12.0 + 3 * n) / np.abs(d).max()             # largest coordinate 12..24 units out
        th[i, :] = centre + d * unit
        tp[j, :] = th[i, :] + 0.2 * unit * rng.normal(size=P)          # a far neighbour: the dominant term of row i
    tp[500, 2] = centre[2] + 10.4 * unit[2]               # far in ONE coordinate, otherwise among the ordinary particles
    wp[[65, 300, 301]] = 0.0
    ref = oracle.weights_importance(opri, th, tp, wp, dv)
    w = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx)
    assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_SPLIT
    assert np.all(ref > 0) and np.max(np.abs(w - ref) / ref) < KDE_TOL["auto"]
    w_again = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx)
    assert np.array_equal(w, w_again)                      # fixed summation orders (sorted far list, block trees)
    with _kde_mode(gpu_ctx, "fp64"):
        w64 = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx)
    assert np.max(np.abs(w64 - ref) / ref) < KDE_TOL["fp64"]
    # too many far new particles (> K/16 + 32): the fp64 kernel takes the call
    th_many = th.copy()
    th_many[::8, 0] = centre[0] + 11.0 * unit[0]
    refm = oracle.weights_importance(opri, th_many, tp, wp, dv)
    wm = abcutil.weight_predictive_prior(pri, th_many, tp, wp, dv, ctx=gpu_ctx)
    assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_FP64
    assert np.max(np.abs(wm - refm) / refm) < KDE_TOL["fp64"]


@pytest.mark.parametrize("P", [16, 12, 24, 30, 40, 64])
def test_weight_far_row_in_one_coordinate_whichever_it_is(gpu_ctx, oracle, P):
    """a NEW particle that is far in exactly ONE coordinate, for every coordinate in turn (and one PREVIOUS particle likewise): a
    row of the limb-tile kernel is dealt out to several lanes, eight parameters each, and all of them have to learn that the row
    is far -- until the end of round 3 only the lane holding the coordinate did when that was not the first one (`flag ||
    shuffle` skipped the exchange in the lanes whose flag was set), the row's weight came out wrong by orders of magnitude
    and, through the normalisation, every other weight with it.  Against the oracle."""
    from abcsmc_amd import abcutil, _lib
    K, Kp = 350, 401
    wl, th0, tp0, wp, dv = _weights_case(P, K, Kp, 4321 + P)
    spec = [(_lib.PRIOR_GAUSS, 0.0, 1e4)] * P                # (flat enough, and its P-fold product stays a normal number)
    pri, opri = _lib.make_priors(spec), oracle.make_priors(spec)
    unit = np.sqrt(dv) / np.sqrt(np.log2(np.e))
    worst = 0.0
    for idx in range(P):
        th, tp = th0.copy(), tp0.copy()
        th[3 + idx, idx] += 11.0 * unit[idx]
        tp[(7 * idx + 5) % Kp, P - 1 - idx] -= 10.0 * unit[P - 1 - idx]
        ref = oracle.weights_importance(opri, th, tp, wp, dv)
        w = abcutil.weight_predictive_prior(pri, th, tp, wp, dv, ctx=gpu_ctx)
        assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_SPLIT
        assert np.all(ref > 0)
        err = np.max(np.abs(w - ref) / ref)
        worst = max(worst, err)
        assert err < _kde_tol("auto", P), (idx, err)
    print("P = %d: one far coordinate at a time, worst rel err %.2e" % (P, worst))


def test_weight_kernels_agree_on_random_shapes(gpu_ctx):
    """randomised shapes (every padded width 8 / 16 / 32, row counts that are not multiples of the 32-row tiles, the 64-row
    waves or the 256-row work-groups, several column slices) and row sub-ranges as the sharded driver uses them
    (abc_weights_raw_dev with k0 > 0): the split-operand kernel against the fp64 kernel of the same library"""
    import torch
    from abcsmc_amd import _lib, device, sharded, synthetic
    rng = np.random.default_rng(2024)
    be = sharded.HipBackend("cuda:0", gpu_ctx)
    for case in range(24):
        P = int(rng.integers(5, 33))
        K = int(rng.integers(1, 2500))
        Kp = int(rng.integers(2, 6000))
        wl = synthetic.Workload(4, P, seed=1000 + case)
        _, th = wl.rows(0, K)
        th = np.asfortranarray(wl.mu_y + 0.45 * (th - wl.mu_y))
        tp, _, dv = wl.previous_set(Kp)
        wp = rng.random(Kp) ** 4 + 1e-12
        if case % 3 == 0:
            wp[rng.integers(0, Kp, size=max(1, Kp // 50))] = 0.0
        k0 = int(rng.integers(0, K))
        kn = int(rng.integers(1, K - k0 + 1))
        dth, dtp, dwp, ddv = (device.colmajor(a, "cuda:0") for a in (th, tp, wp, dv))
        dpri = device.priors_to_device(_lib.make_priors(wl.prior_spec()), "cuda:0")
        out = {}
        for mode in ("auto", "fp64"):
            with _kde_mode(gpu_ctx, mode):
                o = torch.zeros(kn, dtype=torch.float64, device="cuda:0")
                be.weights_raw(dpri, dth, k0, kn, dtp, dwp, ddv, o)
                torch.cuda.synchronize()
                assert gpu_ctx.kde_last_kernel() == (_lib.KDE_RAN_SPLIT if mode == "auto" else _lib.KDE_RAN_FP64)
                out[mode] = o.cpu().numpy()
        ok = out["fp64"] > 0
        assert ok.any() and np.all(np.isfinite(out["auto"]))
        err = np.abs(out["auto"][ok] - out["fp64"][ok]) / out["fp64"][ok]
        assert err.max() < KDE_TOL["auto"], (case, P, K, Kp, k0, kn, err.max())
        assert np.array_equal(out["auto"] == 0, out["fp64"] == 0)


@pytest.mark.parametrize("P,K,Kp,epan", [(70, 300, 257, False), (130, 200, 300, False), (100, 150, 200, True)])
def test_weight_more_than_64_parameters(gpu_ctx, oracle, P, K, Kp, epan):
    """the reference's loops take any number of parameters (AbcUtil.cpp:556-581): beyond 64 the generic fp64 kernel"""
    from abcsmc_amd import abcutil, _lib
    rng = np.random.default_rng(P + K)
    th = rng.normal(size=(K, P)) * 0.5 + 3.0
    tp = rng.normal(size=(Kp, P)) * 0.7 + 3.0
    wp = rng.random(Kp) + 0.1
    wp /= np.linalg.norm(wp)
    dv = 2.0 * tp.var(axis=0, ddof=1)
    spec = [(_lib.PRIOR_GAUSS, 3.0, 4.0) if p % 2 else (_lib.PRIOR_UNIF_REAL, -10.0, 10.0) for p in range(P)]
    if epan:
        gpu_ctx.set_weight_kernel(_lib.WEIGHT_EPANECHNIKOV)
    try:
        w = abcutil.weight_predictive_prior(_lib.make_priors(spec), th, tp, wp, dv, ctx=gpu_ctx)
    finally:
        gpu_ctx.set_weight_kernel(_lib.WEIGHT_GAUSSIAN)
    ref = (oracle.weights_epanechnikov if epan else oracle.weights_importance)(oracle.make_priors(spec), th, tp, wp, dv)
    m = ref > 0
    assert np.array_equal(m, w > 0) and np.max(np.abs(w[m] - ref[m]) / ref[m]) < 1e-9


def test_weight_uniform_first_set(gpu_ctx):
    from abcsmc_amd import abcutil
    w = abcutil.weight_predictive_prior(None, np.zeros((123, 4)), ctx=gpu_ctx)
    assert np.array_equal(w, np.full(123, 1.0 / 123))


def test_weight_converged_parameter_and_prior_support(gpu_ctx, oracle):
    from abcsmc_amd import abcutil, _lib
    wl, th, tp, wp, dv = _weights_case(4, 200, 150, 5)
    th[:, 1] = 7.0
    tp[:, 1] = 7.0
    tp[::7, 1] = 8.0                     # some previous particles differ: factor 0 (declared deviation)
    dv[1] = 0.0
    spec = wl.prior_spec()
    spec[1] = (_lib.PRIOR_UNIF_INT, 1, 10)
    spec[2] = (_lib.PRIOR_UNIF_REAL, float(np.median(th[:, 2])), float(th[:, 2].max() + 1))   # half outside support
    w = abcutil.weight_predictive_prior(_lib.make_priors(spec), th, tp, wp, dv, ctx=gpu_ctx)
    assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_FP64            # a converged parameter: the guarded fp64 loop
    ref = oracle.weights_importance(oracle.make_priors(spec), th, tp, wp, dv, 0)
    assert (ref == 0).sum() > 10 and np.array_equal(w == 0, ref == 0)
    assert np.allclose(w, ref, rtol=RTOL)


@pytest.mark.parametrize("mode", ["auto", "fp64"])
def test_weight_far_particles_and_zero_weights(gpu_ctx, oracle, mode):
    """the weight kernel's guarded loop: a previous particle 1e7 proposal-sigmas away (its exponent leaves the int32
    range of the fast 2^x split), previous weights that are exactly 0, and a current particle so far from everything
    that its denominator underflows -- same values as the per-factor reference formula"""
    from abcsmc_amd import abcutil, _lib
    wl, th, tp, wp, dv = _weights_case(6, 300, 200, 11)
    spec = [(_lib.PRIOR_GAUSS, 0.0, 1e9)] * 6
    tp = tp.copy(); wp = wp.copy(); th = th.copy()
    tp[5, :] += 1e7 * np.sqrt(dv)            # contributes exactly 0 to every sum
    wp[7] = 0.0
    wp[8] = 0.0
    ref = oracle.weights_importance(oracle.make_priors(spec), th, tp, wp, dv)
    gpu_ctx.set_kde_mode(_lib.KDE_FP64 if mode == "fp64" else _lib.KDE_AUTO)
    w = abcutil.weight_predictive_prior(_lib.make_priors(spec), th, tp, wp, dv, ctx=gpu_ctx)
    assert np.all(np.isfinite(ref)) and np.all(ref > 0)
    assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_FP64
    assert np.max(np.abs(w - ref) / ref) < 1e-9       # the far row sends BOTH modes through the guarded fp64 loop
    # the same set with the far / zero-weight particles REMOVED gives the same weights: they really contribute nothing
    # (without the far row the auto mode runs the split-operand kernel: its tolerance applies)
    keep = np.ones(200, bool); keep[[5, 7, 8]] = False
    w2 = abcutil.weight_predictive_prior(_lib.make_priors(spec), th, tp[keep], wp[keep], dv, ctx=gpu_ctx)
    assert gpu_ctx.kde_last_kernel() == (_lib.KDE_RAN_FP64 if mode == "fp64" else _lib.KDE_RAN_SPLIT)
    assert np.max(np.abs(w2 - w) / w) < (1e-12 if mode == "fp64" else KDE_TOL["auto"])
    # one current particle 60 sigmas out in every coordinate: every term underflows to 0 in both implementations
    th[3, :] += 60 * np.sqrt(dv)
    raw = abcutil.weight_predictive_prior(_lib.make_priors(spec), th, tp, wp, dv, ctx=gpu_ctx)
    gpu_ctx.set_kde_mode(_lib.KDE_AUTO)
    rref = oracle.weights_importance(oracle.make_priors(spec), th, tp, wp, dv)
    assert np.array_equal(np.isfinite(raw), np.isfinite(rref))


@pytest.mark.parametrize("K,P", [(400, 6), (50, 16), (5000, 32), (33, 1), (900, 100), (700, 200)])
def test_setup_mvn_sampler(gpu_ctx, oracle, K, P):
    from abcsmc_amd import abcutil
    rng = np.random.default_rng(K + P)
    th = rng.normal(size=(K, P)) @ rng.normal(size=(P, P)) + rng.normal(size=P) * 100
    L = abcutil.setup_mvn_sampler(th, ctx=gpu_ctx)
    rc, Lo, cov = oracle.mvn_setup(th)
    assert rc == 0
    assert np.allclose(L, Lo, rtol=1e-7, atol=1e-9 * np.abs(Lo).max())
    assert np.allclose(np.tril(L) @ np.tril(L).T, cov, rtol=1e-8, atol=1e-9 * np.abs(cov).max())


def test_setup_mvn_sampler_not_spd(gpu_ctx):
    from abcsmc_amd import abcutil, _lib
    th = np.ones((20, 3))
    th[:, 0] = np.arange(20)
    with pytest.raises(_lib.AbcError) as e:
        abcutil.setup_mvn_sampler(th, ctx=gpu_ctx)        # reference: GSL_EDOM abort; here an error code
    assert e.value.code == -3


# ---------------------------------------------------------------------------------------------------
# resampling (bit-exact) and perturbation (distributional)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n,seed", [(1, 10, 1), (37, 5000, 2), (1000, 100000, 3), (4096, 64, 4), (513, 65, 5),
                                      (300001, 200000, 6)])       # >= 2e5: the threaded passes of the alias build
def test_resample_bit_exact(gpu_ctx, oracle, K, n, seed):
    from abcsmc_amd import abcutil
    w = np.random.default_rng(seed).random(K) ** 3
    if K > 5:
        w[3] = 0.0
    r, o = abcutil.rng(seed), oracle.rng(seed)
    for _ in range(seed):                 # start somewhere inside the stream
        abcutil.rng_get(r)
        oracle.rng_get(o)
    idx = abcutil.gsl_rng_nonuniform_int(r, n, w, ctx=gpu_ctx)
    ref = oracle.resample(o, w, n)
    assert np.array_equal(idx, ref)
    assert (r.s1, r.s2, r.s3) == (o.s1, o.s2, o.s3)      # both consumed exactly n outputs
    assert np.array_equal(np.bincount(idx.astype(int), minlength=K), np.bincount(ref.astype(int), minlength=K))


def _alias_weights(kind, K, rng):
    if kind == "uniform":
        w = rng.random(K)
    elif kind == "lognormal1.5":
        w = np.exp(1.5 * rng.normal(size=K))
    elif kind == "lognormal3":
        w = np.exp(3.0 * rng.normal(size=K))
    elif kind == "zeros":
        w = rng.random(K) ** 3
        w[rng.integers(0, K, max(1, K // 50))] = 0.0
    elif kind == "near_mean":
        w = np.full(K, 1.0 / K) * (1 + 1e-9 * rng.normal(size=K))      # everything within 1e-9 of the mean
    elif kind == "few_values":
        w = np.round(rng.random(K) * 8) / 8.0 + 0.125                   # nine distinct values: exact ties abound
    else:
        w = np.ones(K)                                                   # "equal": every entry exactly at the mean
    return w / np.linalg.norm(w)


@pytest.mark.parametrize("kind", ["uniform", "lognormal1.5", "lognormal3", "zeros", "near_mean", "few_values", "equal"])
def test_device_alias_table_is_gsls_table_bit_for_bit(gpu_ctx, oracle, kind):
    """The Walker alias table of the resampling step, built on the GPU by verified prefix scans (csrc/alias_dev.hip), against
    the oracle's gsl_ran_discrete_preproc (sequential): every cut-off F[k] (bit pattern) and every alias A[k], for 2 .. 1e6
    weights of seven kinds -- and the build's own verification must hold (no fallback to the host)"""
    rng = np.random.default_rng(["uniform", "lognormal1.5", "lognormal3", "zeros", "near_mean", "few_values", "equal"].index(kind))
    gpu_ctx.alias_stats(reset=True)
    sizes = [2, 3, 7, 64, 1000, 4097, 100_000, 300_001] + ([1_000_000] if kind in ("uniform", "lognormal1.5") else [])
    for K in sizes:
        w = _alias_weights(kind, K, rng)
        F, A, on_device = gpu_ctx.alias_table(w)
        oF, oA = oracle.discrete_preproc(w)
        assert np.array_equal(A, oA), (kind, K)
        assert np.array_equal(F.view(np.uint64), oF.view(np.uint64)), (kind, K)
        # Weights within 1e-9 of uniform leave the speculation margins of a few grid units near the chain's end (and at a power-of-two
        # K the mean itself is a binade boundary): the build's verification then sends some tables to the host -- measured with
        # scripts/alias_scan_proto.py: 0.5 % of such tables at K = 64, 0.7 % at 20000, 11 % at 32768; 0 of 900 for the other kinds.
        assert on_device == 1 or kind == "near_mean", (kind, K)
    builds, fallbacks = gpu_ctx.alias_stats()
    assert builds == len(sizes) and (fallbacks == 0 or (kind == "near_mean" and fallbacks <= 2))


def test_device_alias_table_falls_back_outside_its_grid(gpu_ctx, oracle):
    """weights spread over more than 2^44 (a first weight of 1e-30 of the others'): the device build says so and the host's
    sequential build delivers the table -- still GSL's; and ABC_ALIAS_HOST never touches the device build"""
    from abcsmc_amd import _lib
    rng = np.random.default_rng(3)
    w = rng.random(5000)
    w[0] = 1e-30
    gpu_ctx.alias_stats(reset=True)
    F, A, on_device = gpu_ctx.alias_table(w)
    oF, oA = oracle.discrete_preproc(w)
    assert on_device == 0 and gpu_ctx.alias_stats() == (1, 1)
    assert np.array_equal(A, oA) and np.array_equal(F.view(np.uint64), oF.view(np.uint64))
    gpu_ctx.set_alias_mode(_lib.ALIAS_HOST)
    try:
        F, A, on_device = gpu_ctx.alias_table(rng.random(3000))
        assert on_device == 0 and gpu_ctx.alias_stats(reset=True) == (1, 1)
    finally:
        gpu_ctx.set_alias_mode(_lib.ALIAS_DEVICE)


@pytest.mark.parametrize("K", [5000, 30000])
@pytest.mark.parametrize("bad", ["two_inf", "nan", "negative", "inf_and_nan"])
def test_device_alias_table_with_unusable_weights_goes_to_the_host(gpu_ctx, bad, K):
    """non-finite / negative weights: the first launches of the device build flag them, and NOTHING behind the flag
    may run on them -- a non-finite "big" has grid value 0, the excess sums then decrease, the rank searches stop being a
    bijection onto the chain's steps and the serving kernels would follow unwritten indices out of bounds.  The kernels now
    return at the flag; the table comes from the host's sequential build, the same bytes as with ABC_ALIAS_HOST.  (Also part of
    the poisoned-workspace slice of tests/test_gpu_fuzz.py, where unwritten step records are 0xff..ff indices.)"""
    from abcsmc_amd import _lib
    rng = np.random.default_rng(11)
    w = rng.random(K)
    if bad == "two_inf":
        w[[7, K // 2]] = np.inf
    elif bad == "nan":
        w[K // 3] = np.nan
    elif bad == "negative":
        w[K - 2] = -0.25
    else:
        w[3], w[K - 1] = np.inf, np.nan
    gpu_ctx.alias_stats(reset=True)
    F, A, on_device = gpu_ctx.alias_table(w)
    assert on_device == 0 and gpu_ctx.alias_stats() == (1, 1)
    gpu_ctx.set_alias_mode(_lib.ALIAS_HOST)
    try:
        hF, hA, _ = gpu_ctx.alias_table(w)
    finally:
        gpu_ctx.set_alias_mode(_lib.ALIAS_DEVICE)
        gpu_ctx.alias_stats(reset=True)
    assert np.array_equal(A, hA) and np.array_equal(F.view(np.uint64), hF.view(np.uint64))
    # ... and the context is fine afterwards: a well-posed table right behind it is built on the device and is GSL's
    w2 = rng.random(K)
    F2, A2, on2 = gpu_ctx.alias_table(w2)
    gpu_ctx.set_alias_mode(_lib.ALIAS_HOST)
    try:
        hF2, hA2, _ = gpu_ctx.alias_table(w2)
    finally:
        gpu_ctx.set_alias_mode(_lib.ALIAS_DEVICE)
        gpu_ctx.alias_stats(reset=True)
    assert on2 == 1 and np.array_equal(A2, hA2) and np.array_equal(F2.view(np.uint64), hF2.view(np.uint64))


def test_sample_mvn_predictive_priors(gpu_ctx, oracle):
    from abcsmc_amd import abcutil, _lib
    rng = np.random.default_rng(21)
    K, P, n = 300, 4, 200000
    th = np.column_stack([rng.normal(5, 1, K), np.round(rng.uniform(3, 18, K)), rng.uniform(0.2, 0.8, K),
                          rng.normal(0, 2, K)])
    spec = [(_lib.PRIOR_GAUSS, 5.0, 3.0), (_lib.PRIOR_UNIF_INT, 1, 20), (_lib.PRIOR_UNIF_REAL, 0.0, 1.0),
            (_lib.PRIOR_GAUSS, 0.0, 10.0)]
    w = rng.random(K)
    L = abcutil.setup_mvn_sampler(th, ctx=gpu_ctx)
    r, o = abcutil.rng(99), oracle.rng(99)
    out, parent, seeds = abcutil.sample_mvn_predictive_priors(r, n, w, th, _lib.make_priors(spec), L, seeds=True,
                                                              ctx=gpu_ctx)
    oout, opar, _ = oracle.sample_mvn_predictive_priors(o, n, w, th, oracle.make_priors(spec), L)
    assert np.array_equal(parent, opar)                                  # bit-exact parents
    # seeds: the taus2 outputs right after the n resampling draws
    o2 = oracle.rng(99)
    for _ in range(n):
        oracle.rng_get(o2)
    assert np.array_equal(seeds[:1000], np.array([oracle.rng_get(o2) for _ in range(1000)], dtype=np.uint64))
    # support / recast
    assert np.all(out[:, 1] == np.round(out[:, 1])) and out[:, 1].min() >= 1 and out[:, 1].max() <= 20
    assert out[:, 2].min() >= 0.0 and out[:, 2].max() <= 1.0
    # distribution: same moments as the reference stream's proposals (both truncated the same way)
    for p in range(P):
        sd = oout[:, p].std()
        assert abs(out[:, p].mean() - oout[:, p].mean()) < 5 * sd / np.sqrt(n) * 2
        assert abs(out[:, p].std() / sd - 1) < 0.02
    dg, do = out - th[parent.astype(int)], oout - th[opar.astype(int)]
    assert np.allclose(np.corrcoef(dg[:, [0, 3]].T), np.corrcoef(do[:, [0, 3]].T), atol=0.02)


def test_sample_predictive_priors_independent(gpu_ctx, oracle):
    from abcsmc_amd import abcutil, _lib
    rng = np.random.default_rng(22)
    K, P, n = 200, 3, 100000
    th = np.column_stack([rng.normal(5, 1, K), np.round(rng.uniform(3, 18, K)), rng.uniform(0.45, 0.55, K)])
    spec = [(_lib.PRIOR_GAUSS, 5.0, 3.0), (_lib.PRIOR_UNIF_INT, 1, 20), (_lib.PRIOR_UNIF_REAL, 0.4, 0.6)]
    w = np.full(K, 1.0 / K)
    dv = abcutil.calculate_doubled_variance(th, ctx=gpu_ctx)
    r, o = abcutil.rng(5), oracle.rng(5)
    out, parent = abcutil.sample_predictive_priors(r, n, w, th, _lib.make_priors(spec), dv, ctx=gpu_ctx)
    oout, opar, _ = oracle.sample_predictive_priors(o, n, w, th, oracle.make_priors(spec), dv)
    assert np.array_equal(parent, opar)
    assert out[:, 2].min() >= 0.4 and out[:, 2].max() <= 0.6
    assert np.all(out[:, 1] == np.round(out[:, 1]))
    for p in range(P):
        assert abs(out[:, p].mean() - oout[:, p].mean()) < 0.02 * oout[:, p].std() + 1e-3
        assert abs(out[:, p].std() / oout[:, p].std() - 1) < 0.02


def _assert_standard_normal(z, tag):
    """z: (n, P) recovered deviates of the device noise stream, n = 1e6.  What the sample size supports: a 1 % scale error in
    the normals fails the variance bound by 14 standard errors"""
    from scipy import stats
    n, P = z.shape
    assert np.all(np.abs(z) <= 6.77), tag                              # the stream's stated truncation, |z| <= 6.76
    for p in range(P):
        v = z[:, p]
        ks = stats.kstest(v, "norm")
        assert ks.pvalue > 1e-3, (tag, p, ks)                          # Kolmogorov-Smirnov against N(0, 1)
        assert abs(v.mean()) < 5.0 / np.sqrt(n), (tag, p, v.mean())
        assert abs(v.var() - 1.0) < 0.005, (tag, p, v.var())           # standard error sqrt(2 / n) = 0.0014
        kurt = np.mean((v - v.mean()) ** 4) / v.var() ** 2
        assert abs(kurt - 3.0) < 0.03, (tag, p, kurt)                  # standard error sqrt(24 / n) = 0.005
        assert abs(stats.skew(v)) < 0.0125, (tag, p)                   # standard error sqrt(6 / n) = 0.0025
        for t in (3.0, 4.0):                                           # tail counts within 5 sigma of the binomial
            q = 2.0 * stats.norm.sf(t)
            c = np.count_nonzero(np.abs(v) > t)
            assert abs(c - n * q) < 5.0 * np.sqrt(n * q * (1 - q)), (tag, p, t, c, n * q)
    cc = np.corrcoef(z.T)
    assert np.max(np.abs(cc - np.eye(P))) < 0.005, (tag, cc)           # independent coordinates (standard error 0.001)


@pytest.mark.parametrize("P", [4, 16])
def test_device_noise_stream_is_standard_normal(gpu_ctx, P):
    """The default proposals draw from Philox4x32-10 + Box-Muller on the f32 transcendental hardware (resample.hip: normal4;
    radius from all 32 bits of its word: |z| <= 6.76, deviates carry f32 rounding).  With priors that never reject, the
    deviates are recovered from 1e6 proposals -- z = L^-1 (x - parent) for MULTIVARIATE (AbcUtil.cpp:122-143), z = (x - parent) /
    sqrt(dv) per coordinate for INDEPENDENT (AbcUtil.cpp:145-158, Priors.h:19-43) -- and held to N(0, 1): KS, mean, variance to
    0.5 %, kurtosis, skewness, 3 / 4 sigma tail counts, cross-coordinate correlation"""
    from scipy.linalg import solve_triangular
    from abcsmc_amd import abcutil, _lib
    g = np.random.default_rng(40 + P)
    K, n = 200, 1_000_000
    mix = g.normal(size=(P, P)) / np.sqrt(P) + np.eye(P)
    th = g.normal(size=(K, P)) @ mix * 10.0 ** g.integers(-2, 3, size=P)          # correlated posterior, scales 1e-2 .. 1e2
    spec = [(_lib.PRIOR_GAUSS, 0.0, 1e9)] * P                                       # support = everything: no rejection
    w = g.random(K)
    L = abcutil.setup_mvn_sampler(th, ctx=gpu_ctx)
    out, parent = abcutil.sample_mvn_predictive_priors(abcutil.rng(7), n, w, th, _lib.make_priors(spec), L, ctx=gpu_ctx)[:2]
    z = solve_triangular(np.tril(L), (out - th[parent.astype(np.int64)]).T, lower=True).T
    _assert_standard_normal(z, "mvn")
    dv = abcutil.calculate_doubled_variance(th, ctx=gpu_ctx)
    out, parent = abcutil.sample_predictive_priors(abcutil.rng(8), n, w, th, _lib.make_priors(spec), dv, ctx=gpu_ctx)[:2]
    z = (out - th[parent.astype(np.int64)]) / np.sqrt(dv)
    _assert_standard_normal(z, "independent")
    assert gpu_ctx.perturb_giveups() == 0


class _noise_mode:
    def __init__(self, ctx, mode):
        self.ctx, self.mode = ctx, mode

    def __enter__(self):
        self.ctx.set_noise_mode(self.mode)

    def __exit__(self, *a):
        from abcsmc_amd import _lib
        self.ctx.set_noise_mode(_lib.NOISE_DEVICE)


@pytest.mark.parametrize("multivariate", [True, False])
def test_reference_stream_proposals_bit_exact(gpu_ctx, oracle, multivariate):
    """ABC_NOISE_REFERENCE_STREAM: the proposals consume the taus2 stream exactly as the reference does (polar Box-Muller per
    coordinate on uniform_pos draws, whole-vector / per-coordinate rejection, AbcUtil.cpp:122-158, Priors.h:19-43), the seeds
    follow the noise (AbcSmc.cpp:535): values, parents, seeds and the final rng state equal the oracle's bit for bit.
    Narrow priors make rejections (data-dependent consumption) frequent."""
    from abcsmc_amd import abcutil, _lib
    g = np.random.default_rng(31)
    K, P, n = 257, 5, 6000
    th = np.column_stack([g.normal(5, 1, K), np.round(g.uniform(3, 18, K)), g.uniform(0.3, 0.7, K), g.normal(0, 2, K),
                          g.normal(-3, 0.5, K)])
    spec = [(_lib.PRIOR_GAUSS, 5.0, 3.0), (_lib.PRIOR_UNIF_INT, 1, 20), (_lib.PRIOR_UNIF_REAL, 0.25, 0.75),
            (_lib.PRIOR_GAUSS, 0.0, 10.0), (_lib.PRIOR_UNIF_REAL, -4.2, -1.5)]
    w = g.random(K)
    rc, L, _ = oracle.mvn_setup(th)                       # one factor for both sides: this test is about the stream
    assert rc == 0
    dv = oracle.doubled_variance(th)
    r, o = abcutil.rng(1234), oracle.rng(1234)
    with _noise_mode(gpu_ctx, _lib.NOISE_REFERENCE_STREAM):
        if multivariate:
            out, parent, seeds = abcutil.sample_mvn_predictive_priors(r, n, w, th, _lib.make_priors(spec), L, seeds=True, ctx=gpu_ctx)
            oout, opar, rej = oracle.sample_mvn_predictive_priors(o, n, w, th, oracle.make_priors(spec), L)
        else:
            out, parent, seeds = abcutil.sample_predictive_priors(r, n, w, th, _lib.make_priors(spec), dv, seeds=True, ctx=gpu_ctx)
            oout, opar, rej = oracle.sample_predictive_priors(o, n, w, th, oracle.make_priors(spec), dv)
    oseeds = np.array([oracle.rng_get(o) for _ in range(n)], dtype=np.uint64)
    assert np.array_equal(parent, opar)
    assert np.array_equal(out, oout)                      # bit for bit
    assert np.array_equal(seeds, oseeds)
    assert (r.s1, r.s2, r.s3) == (o.s1, o.s2, o.s3)
    if multivariate:
        assert rej > 100                                  # the stream position really was data dependent
    # the default mode is untouched: same parents, different (Philox) noise
    r2 = abcutil.rng(1234)
    out2, parent2 = abcutil.sample_mvn_predictive_priors(r2, n, w, th, _lib.make_priors(spec), L, ctx=gpu_ctx)[:2]
    assert np.array_equal(parent2, opar) and not np.array_equal(out2, oout)


def test_reference_stream_generation(gpu_ctx, oracle):
    """abc_generation_dev in reference-stream mode against oracle.generation: selection, parents, seeds and the rng state bit
    for bit; the proposals to the rounding of the covariance factor (the device's reduction order differs from the
    oracle's in the last bits; integer-valued priors would make them identical, see the dice fit in tests/test_shell.py)"""
    import torch
    from abcsmc_amd import abcutil, device, _lib
    N, M, P, K, Kp, Nn, A = 3000, 12, 5, 300, 250, 2500, 4
    wl, X, Y, obs = _wl(M, P, N, 99)
    spec = wl.prior_spec()
    prev = wl.previous_set(Kp)
    dev = "cuda:0"
    gen = device.Generation(N, M, P, K, Kp, Nn, 0.5, A, multivariate=True, device=dev, ctx=gpu_ctx)
    r, o = abcutil.rng(77), oracle.rng(77)
    with _noise_mode(gpu_ctx, _lib.NOISE_REFERENCE_STREAM):
        gen.run(device.colmajor(X, dev), device.colmajor(Y, dev), device.colmajor(obs, dev),
                device.priors_to_device(_lib.make_priors(spec), dev), r, *(device.colmajor(a, dev) for a in prev))
        torch.cuda.synchronize()
    ref = oracle.generation(X, Y, obs, oracle.make_priors(spec), K, Nn, o, *prev, train_frac=0.5, max_comp=A, multivariate=True)
    assert np.array_equal(gen.idx.cpu().numpy().astype(np.uint64), ref["idx"])
    assert np.array_equal(gen.parent.cpu().numpy().astype(np.uint64), ref["parent"])
    assert np.array_equal(gen.seeds.cpu().numpy().astype(np.uint64), ref["seeds"])
    assert (r.s1, r.s2, r.s3) == (o.s1, o.s2, o.s3)
    assert np.allclose(device.to_numpy(gen.next), ref["next"], rtol=1e-9, atol=0)
    assert gpu_ctx.perturb_giveups() == 0


def test_perturb_giveups_are_counted(gpu_ctx):
    """a prior so narrow that no proposal can land in it: the device emits the (valid) parent after 16384 whole-vector
    rejections and says so through abc_perturb_giveups (the reference would never return, AbcUtil.cpp:132)"""
    from abcsmc_amd import abcutil, _lib
    K, n = 16, 40
    th = np.column_stack([np.full(K, 0.5), np.linspace(-1, 1, K)])
    spec = [(_lib.PRIOR_UNIF_REAL, 0.5, 0.5 + 1e-300), (_lib.PRIOR_GAUSS, 0.0, 5.0)]
    L = np.asfortranarray(np.array([[1.0, 0.0], [0.0, 1.0]]))
    gpu_ctx.perturb_giveups(reset=True)
    out, parent = abcutil.sample_mvn_predictive_priors(abcutil.rng(3), n, np.full(K, 1.0 / K), th, _lib.make_priors(spec), L, ctx=gpu_ctx)[:2]
    assert gpu_ctx.perturb_giveups() == n
    assert np.array_equal(out, th[parent.astype(int)])
    assert gpu_ctx.perturb_giveups(reset=True) == n and gpu_ctx.perturb_giveups() == 0


def test_generation_reports_giveups_through_a_count_not_a_status(gpu_ctx):
    """abc_generation_dev with a prior no proposal can land in: the call completes -- every proposal is its (valid) parent --
    and returns ABC_OK (the ABI has no positive status: `if (rc)` stays a valid failure test); abc_generation_giveups holds the
    count of THAT call, which the Python driver turns into a warning; the next, well-posed
    generation returns ABC_OK again (the reference would never return, AbcUtil.cpp:132)"""
    import torch
    from abcsmc_amd import abcutil, device, _lib
    N, M, P, K, Nn, A = 2000, 8, 3, 200, 48, 2
    wl, X, Y, obs = _wl(M, P, N)
    spec = wl.prior_spec()
    a0 = float(Y[:, 0].max()) + 10.0 * float(Y[:, 0].std())          # a zero-width prior far from every particle
    spec[0] = (_lib.PRIOR_UNIF_REAL, a0, a0 + 1e-300)
    dev = "cuda:0"
    gpu_ctx.perturb_giveups(reset=True)
    gen = device.Generation(N, M, P, K, 0, Nn, 0.5, A, multivariate=False, device=dev, ctx=gpu_ctx)     # INDEPENDENT: no covariance needed
    args = (device.colmajor(X, dev), device.colmajor(Y, dev), device.colmajor(obs, dev))
    with pytest.warns(_lib.AbcWarning, match="gave up on %d proposal" % Nn):
        gen.run(*args, device.priors_to_device(_lib.make_priors(spec), dev), abcutil.rng(3))
    torch.cuda.synchronize()
    import ctypes as C
    last = C.c_uint64(0)
    assert _lib.lib().abc_generation_giveups(gpu_ctx.handle, C.byref(last)) == 0 and last.value == Nn
    assert gpu_ctx.perturb_giveups() == Nn
    nxt = device.to_numpy(gen.next)
    assert np.all(nxt[:, 0] == a0) and np.isfinite(nxt).all()        # the prior mean of the zero-width prior (Priors.h:23-31)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                               # a well-posed generation: no warning
        gen.run(*args, device.priors_to_device(_lib.make_priors(wl.prior_spec()), dev), abcutil.rng(3))
    assert _lib.lib().abc_generation_giveups(gpu_ctx.handle, C.byref(last)) == 0 and last.value == 0
    assert gpu_ctx.perturb_giveups(reset=True) == Nn


@pytest.mark.parametrize("multivariate,P", [(True, 48), (False, 48), (True, 150), (False, 150), (True, 64), (True, 47)])
def test_samplers_wide_parameter_sets(gpu_ctx, oracle, multivariate, P):
    """33..64 parameters: multivariate noise on the 64-wide instance of the proposal kernel (round 6; the factor through the scalar
    cache, the padded columns not drawn), independent noise on the streaming kernel; more than 64 the chunked one (the reference's
    loops have no size limit): same parents, same support rules, same spread"""
    from abcsmc_amd import abcutil, _lib
    rng = np.random.default_rng(23)
    K, n = 500, 30000
    cols, spec = [], []
    for p in range(P):
        if p % 3 == 0:
            cols.append(rng.normal(p, 1.0, K)); spec.append((_lib.PRIOR_GAUSS, float(p), 5.0))
        elif p % 3 == 1:
            cols.append(np.round(rng.uniform(40, 60, K))); spec.append((_lib.PRIOR_UNIF_INT, 0, 100))
        else:
            cols.append(rng.uniform(0.3, 0.7, K)); spec.append((_lib.PRIOR_UNIF_REAL, 0.0, 1.0))
    th = np.column_stack(cols)
    w = rng.random(K)
    r, o = abcutil.rng(77), oracle.rng(77)
    if multivariate:
        L = abcutil.setup_mvn_sampler(th, ctx=gpu_ctx)
        out, parent = abcutil.sample_mvn_predictive_priors(r, n, w, th, _lib.make_priors(spec), L, ctx=gpu_ctx)[:2]
        oout, opar, _ = oracle.sample_mvn_predictive_priors(o, n, w, th, oracle.make_priors(spec), L)
    else:
        dv = abcutil.calculate_doubled_variance(th, ctx=gpu_ctx)
        out, parent = abcutil.sample_predictive_priors(r, n, w, th, _lib.make_priors(spec), dv, ctx=gpu_ctx)[:2]
        oout, opar, _ = oracle.sample_predictive_priors(o, n, w, th, oracle.make_priors(spec), dv)
    assert np.array_equal(parent, opar)
    assert out.shape == (n, P) and np.all(np.isfinite(out))
    for p in range(P):
        if p % 3 == 1:
            assert np.all(out[:, p] == np.round(out[:, p])) and out[:, p].min() >= 0 and out[:, p].max() <= 100
        if p % 3 == 2:
            assert out[:, p].min() >= 0.0 and out[:, p].max() <= 1.0
        dg, do = out[:, p] - th[parent.astype(int), p], oout[:, p] - th[opar.astype(int), p]
        assert abs(dg.std() / do.std() - 1) < 0.04, p
        assert abs(dg.mean() - do.mean()) < 6 * do.std() / np.sqrt(n) + 1e-9, p
    if multivariate:      # the proposal keeps the posterior's correlations
        dg, do = out - th[parent.astype(int)], oout - th[opar.astype(int)]
        assert np.allclose(np.corrcoef(dg[:, [0, 3, 6, 45]].T), np.corrcoef(do[:, [0, 3, 6, 45]].T), atol=0.04)
        assert np.allclose(np.corrcoef(dg[:, [1, P - 2, P - 1]].T), np.corrcoef(do[:, [1, P - 2, P - 1]].T), atol=0.04)     # (the last columns of the factor)


# ---------------------------------------------------------------------------------------------------
# whole generation, device resident (AbcSmc.cpp:634-664, 1041-1066, 490-518)
# ---------------------------------------------------------------------------------------------------
def _run_generation(N, M, P, K, Kp, Nn, A, multivariate, seed=67890, rule=1):      # (rule 1: the drop-in's default, _lib.RULE_DEFAULT = the Wilcoxon reduction)
    import torch
    from abcsmc_amd import abcutil, device, _lib
    wl, X, Y, obs = _wl(M, P, N)
    spec = wl.prior_spec()
    prev = wl.previous_set(Kp) if Kp else (None, None, None)
    dev = "cuda:0"
    gen = device.Generation(N, M, P, K, Kp, Nn, 0.5, A, rule=rule, multivariate=multivariate, device=dev)
    r = abcutil.rng(seed)
    gen.run(device.colmajor(X, dev), device.colmajor(Y, dev), device.colmajor(obs, dev),
            device.priors_to_device(_lib.make_priors(spec), dev), r,
            *(device.colmajor(a, dev) if a is not None else None for a in prev))
    torch.cuda.synchronize()
    return wl, X, Y, obs, spec, prev, gen, r


_DEVICE_SET = {}


def _device_set(N, M, P):
    """the synthetic set of seed 12345 generated on the GPU and its download, kept for the NEXT test that asks for the same shape
    (round 6: the three tests at configs[3]'s stated size each generated and downloaded the same 7.7 GB; one entry is kept)"""
    from abcsmc_amd import synthetic
    key = (N, M, P)
    if key not in _DEVICE_SET:
        _DEVICE_SET.clear()
        wl = synthetic.Workload(M, P, 12345)
        dX, dY = wl.rows_device(0, N, "cuda:0")
        _DEVICE_SET[key] = (wl, dX, dY, dX.cpu().numpy().T, dY.cpu().numpy().T)     # (N, c) column-major views of the downloads
    return _DEVICE_SET[key]


def _run_generation_device_inputs(N, M, P, K, Kp, Nn, A, multivariate, seed=67890, rule=1):
    """_run_generation with the synthetic set generated ON the GPU (synthetic.Workload.rows_device: numpy takes minutes at
    1e7 rows) and downloaded for the oracle: both sides see the same bits"""
    import torch
    from abcsmc_amd import abcutil, device, synthetic, _lib
    dev = "cuda:0"
    wl, dX, dY, X, Y = _device_set(N, M, P)
    obs = wl.observed()
    spec = wl.prior_spec()
    dprev = wl.previous_set_device(Kp, dev)
    prev = (dprev[0].cpu().numpy().T, dprev[1].cpu().numpy(), dprev[2].cpu().numpy())
    gen = device.Generation(N, M, P, K, Kp, Nn, 0.5, A, rule=rule, multivariate=multivariate, device=dev)
    r = abcutil.rng(seed)
    gen.run(dX, dY, device.colmajor(obs, dev), device.priors_to_device(_lib.make_priors(spec), dev), r, *dprev)
    torch.cuda.synchronize()
    return wl, X, Y, obs, spec, prev, gen, r


@pytest.mark.parametrize("multivariate,Kp,P", [(True, 400, 16), (False, 400, 16), (True, 0, 16), (True, 400, 12), (False, 400, 7)])
def test_generation_matches_oracle(gpu_ctx, oracle, multivariate, Kp, P):
    from abcsmc_amd import device
    N, M, K, Nn, A = 3000, 32, 400, 3000, 8
    wl, X, Y, obs, spec, prev, gen, r = _run_generation(N, M, P, K, Kp, Nn, A, multivariate)
    o = oracle.rng(67890)
    ref = oracle.generation(X, Y, obs, oracle.make_priors(spec), K, Nn, o, *prev, train_frac=0.5, max_comp=A,
                            multivariate=multivariate)
    assert gen.ncomp.value == ref["ncomp"]
    assert np.array_equal(gen.idx.cpu().numpy().astype(np.uint64), ref["idx"])
    assert np.allclose(gen.w.cpu().numpy(), ref["w"], rtol=RTOL)
    assert np.allclose(gen.dv.cpu().numpy(), ref["dv"], rtol=1e-9)
    assert np.array_equal(device.to_numpy(gen.theta), Y[ref["idx"].astype(int)])
    assert np.array_equal(gen.parent.cpu().numpy().astype(np.uint64), ref["parent"])
    # seeds (device noise): the taus2 outputs right behind the Nn resampling draws -- queued on the side stream BEHIND the previous
    # set's prologue in weighted generations, complete when the call returns all the same
    o2 = oracle.rng(67890)
    for _ in range(Nn):
        oracle.rng_get(o2)
    assert np.array_equal(gen.seeds.cpu().numpy().astype(np.uint64), np.array([oracle.rng_get(o2) for _ in range(Nn)], dtype=np.uint64))
    if multivariate:
        L = device.to_numpy(gen.L)
        assert np.allclose(np.tril(L), np.tril(ref["L"]), rtol=1e-7, atol=1e-12)
    nxt = device.to_numpy(gen.next)
    assert nxt.shape == (Nn, P) and np.isfinite(nxt).all()
    for p in range(P):                                       # proposals respect the prior support
        k, a, b = spec[p]
        if k == 2:
            assert nxt[:, p].min() >= a and nxt[:, p].max() <= b


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("multivariate", [True, False])
def test_reference_posterior_rows_ranking_and_generation(gpu_ctx, oracle, rule, multivariate):
    """The one real data set the reference ships: the 1000 posterior rows of examples/scratch/posterior.sqlite (5 parameters x 7
    metrics of a dengue model fit; tests/golden/posterior_rows.npz, exported by tests/golden/make_reference_fixtures.py).  Ranking
    (PLS under both component rules, and the simple ranking) and a whole weighted generation on it against the oracle: component
    count, selection, parents and seeds bit for bit, distances / weights / doubled variance / proposal factor to 1e-6 or better.
    The database holds no observed metrics: the mean metrics of its fifty best-ranked rows stand in for them; the previous
    predictive prior is the rows ranked 200..349 with uniform weights."""
    import os
    import torch
    from abcsmc_amd import abcutil, device, _lib
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posterior_rows.npz"))
    X, Y, rank = np.asfortranarray(d["metrics"]), np.asfortranarray(d["parameters"]), d["posterior_rank"]
    N, M = X.shape
    P = Y.shape[1]
    assert (N, M, P) == (1000, 7, 5) and sorted(rank) == list(range(1000))
    obs = X[rank < 50].mean(axis=0)
    g = abcutil.particle_ranking_PLS(X, Y, obs, 0.5, rule=rule, details=True, ctx=gpu_ctx)
    o = oracle.particle_ranking_pls(X, Y, obs, 0.5, rule=rule)
    assert g["ncomp"] == o["ncomp"]
    assert np.allclose(g["dist"], o["dist"][g["idx"].astype(int)], rtol=RTOL) and _near_tie_ok(g["idx"], o["idx"], o["dist"])
    gs = abcutil.particle_ranking_simple(X, Y, obs, details=True, ctx=gpu_ctx)
    os_idx, os_dist = oracle.particle_ranking_simple(X, obs)
    assert np.allclose(gs["dist"], os_dist[gs["idx"].astype(int)], rtol=1e-12) and _near_tie_ok(gs["idx"], os_idx, os_dist)
    # a weighted generation: 200 kept, 150 previous rows, 1000 proposals
    K, Nn = 200, 1000
    prev_rows = np.argsort(rank, kind="stable")[200:350]
    th_prev = np.asfortranarray(Y[prev_rows])
    w_prev = np.full(len(prev_rows), 1.0 / len(prev_rows))
    dv_prev = 2.0 * th_prev.var(axis=0, ddof=1)
    spec = [(_lib.PRIOR_UNIF_REAL, float(Y[:, p].min() - Y[:, p].std()), float(Y[:, p].max() + Y[:, p].std())) for p in range(P)]
    dev = "cuda:0"
    gen = device.Generation(N, M, P, K, len(prev_rows), Nn, 0.5, 0, rule=rule, multivariate=multivariate, device=dev, ctx=gpu_ctx)
    r = abcutil.rng(424242)
    gen.run(device.colmajor(X, dev), device.colmajor(Y, dev), device.colmajor(obs, dev), device.priors_to_device(_lib.make_priors(spec), dev), r,
            device.colmajor(th_prev, dev), device.colmajor(w_prev, dev), device.colmajor(dv_prev, dev))
    torch.cuda.synchronize()
    orng = oracle.rng(424242)
    ref = oracle.generation(X, Y, obs, oracle.make_priors(spec), K, Nn, orng, th_prev, w_prev, dv_prev, train_frac=0.5, max_comp=0, rule=rule,
                            multivariate=multivariate)
    assert gen.ncomp.value == ref["ncomp"]
    assert np.array_equal(gen.idx.cpu().numpy().astype(np.uint64), ref["idx"])
    assert np.allclose(gen.w.cpu().numpy(), ref["w"], rtol=RTOL) and np.allclose(gen.dv.cpu().numpy(), ref["dv"], rtol=1e-9)
    assert np.array_equal(gen.parent.cpu().numpy().astype(np.uint64), ref["parent"])
    if multivariate:
        assert np.allclose(np.tril(device.to_numpy(gen.L)), np.tril(ref["L"]), rtol=1e-7, atol=1e-12)
    nxt = device.to_numpy(gen.next)
    assert np.isfinite(nxt).all()
    for p in range(P):
        assert nxt[:, p].min() >= spec[p][1] and nxt[:, p].max() <= spec[p][2]


def test_generation_with_40_parameters_matches_oracle(gpu_ctx, oracle):
    """a whole weighted, MULTIVARIATE generation at 40 parameters / 48 metrics: the model fit beyond 32 responses, the pair sums
    on the four-chunk split kernel, 64-wide perturbation -- selection, parents bit for bit, weights to the 33..64-parameter bound"""
    from abcsmc_amd import device, _lib
    N, M, P, K, Kp, Nn, A = 4000, 48, 40, 500, 450, 4000, 6
    wl, X, Y, obs, spec, prev, gen, r = _run_generation(N, M, P, K, Kp, Nn, A, True)
    assert gpu_ctx.kde_last_kernel() == _lib.KDE_RAN_SPLIT
    o = oracle.rng(67890)
    ref = oracle.generation(X, Y, obs, oracle.make_priors(spec), K, Nn, o, *prev, train_frac=0.5, max_comp=A, multivariate=True)
    assert gen.ncomp.value == ref["ncomp"]
    assert np.array_equal(gen.idx.cpu().numpy().astype(np.uint64), ref["idx"])
    w = gen.w.cpu().numpy()
    assert np.max(np.abs(w - ref["w"]) / ref["w"]) < _kde_tol("auto", P)
    assert np.allclose(gen.dv.cpu().numpy(), ref["dv"], rtol=1e-9)
    assert np.array_equal(gen.parent.cpu().numpy().astype(np.uint64), ref["parent"])
    assert np.allclose(np.tril(device.to_numpy(gen.L)), np.tril(ref["L"]), rtol=1e-7, atol=1e-12)
    assert np.isfinite(device.to_numpy(gen.next)).all()


def test_generation_repeats_its_proposals_when_the_device_alias_build_fails(gpu_ctx, oracle, monkeypatch):
    """abc_generation_dev queues the draws and the proposals behind the device-built resampling table without waiting for the
    build's verdict; when the verdict (read at the generation's final synchronisation) says the table is unusable, the draws and
    the proposals are repeated with the host's table.  ABC_ALIAS_FORCE_FAIL makes a (correct) build report failure: parents,
    weights and seeds must still be the oracle's, and the fallback must have been counted"""
    from abcsmc_amd import device
    monkeypatch.setenv("ABC_ALIAS_FORCE_FAIL", "1")
    N, M, P, K, Kp, Nn, A = 220000, 32, 16, 22000, 500, 30000, 8          # (the device build takes tables from 20000 entries)
    ctx = gpu_ctx
    ctx.alias_stats(reset=True)
    wl, X, Y, obs, spec, prev, gen, r = _run_generation(N, M, P, K, Kp, Nn, A, True)
    builds, fallbacks = ctx.alias_stats(reset=True)
    monkeypatch.delenv("ABC_ALIAS_FORCE_FAIL")
    assert builds >= 1 and fallbacks == builds
    o = oracle.rng(67890)
    ref = oracle.generation(X, Y, obs, oracle.make_priors(spec), K, Nn, o, *prev, train_frac=0.5, max_comp=A, multivariate=True)
    assert np.array_equal(gen.idx.cpu().numpy().astype(np.uint64), ref["idx"])
    assert np.allclose(gen.w.cpu().numpy(), ref["w"], rtol=RTOL)
    assert np.array_equal(gen.parent.cpu().numpy().astype(np.uint64), ref["parent"])
    nxt = device.to_numpy(gen.next)
    assert np.isfinite(nxt).all()
    # the repeated proposals are the ones a host-table generation makes: same Philox keys, same parents
    from abcsmc_amd import _lib
    ctx.set_alias_mode(_lib.ALIAS_HOST)
    try:
        wl2, X2, Y2, obs2, spec2, prev2, gen2, r2 = _run_generation(N, M, P, K, Kp, Nn, A, True)
    finally:
        ctx.set_alias_mode(_lib.ALIAS_DEVICE)
    assert np.array_equal(device.to_numpy(gen2.next), nxt) and np.array_equal(gen2.parent.cpu().numpy(), gen.parent.cpu().numpy())
    assert (r.s1, r.s2, r.s3) == (r2.s1, r2.s2, r2.s3)


@pytest.mark.parametrize("N,M,P,K,Kp,A", [(20000, 32, 16, 2000, 2000, 8), (6000, 64, 32, 600, 600, 8), (4000, 128, 16, 400, 400, 32)])
def test_generation_repeats_bit_identically(gpu_ctx, N, M, P, K, Kp, A):
    """two runs of the same generation (side stream, deferred moments, host alias build between them) give the same bits in
    every output: weights, proposals, parents, seeds, factor -- the three BASELINE column shapes"""
    from abcsmc_amd import device
    outs = []
    for _ in range(2):
        wl, X, Y, obs, spec, prev, gen, r = _run_generation(N, M, P, K, Kp, N, A, True)
        outs.append([gen.idx.cpu().numpy().copy(), gen.w.cpu().numpy().copy(), gen.dv.cpu().numpy().copy(),
                     gen.parent.cpu().numpy().copy(), device.to_numpy(gen.next).copy(), device.to_numpy(gen.L).copy(),
                     gen.seeds.cpu().numpy().copy() if hasattr(gen, "seeds") else np.zeros(1), int(gen.ncomp.value)])
    for a, b in zip(outs[0][:-1], outs[1][:-1]):
        assert np.array_equal(a, b)
    assert outs[0][-1] == outs[1][-1]


def test_first_set_alias_table_is_kept_per_size(gpu_ctx, oracle):
    """set 0 (uniform weights, AbcUtil.cpp:539-545): the alias table of K equal weights is built while the GPU ranks and kept
    for the next call with the same K; a different K, and a weighted set in between, must not see a stale table"""
    N, M, P, Nn, A = 3000, 12, 5, 3000, 4
    for K, Kp in [(400, 0), (400, 0), (250, 0), (400, 300), (250, 0), (400, 0)]:
        wl, X, Y, obs, spec, prev, gen, r = _run_generation(N, M, P, K, Kp, Nn, A, True)
        o = oracle.rng(67890)
        ref = oracle.generation(X, Y, obs, oracle.make_priors(spec), K, Nn, o, *prev, train_frac=0.5, max_comp=A,
                                multivariate=True)
        assert np.array_equal(gen.parent.cpu().numpy().astype(np.uint64), ref["parent"]), (K, Kp)
        assert np.allclose(gen.w.cpu().numpy(), ref["w"], rtol=RTOL)


def test_generation_full_size_properties(gpu_ctx):
    """BASELINE config 2 size (N = 1e5, M = 32, P = 16, A = 8): size-independent invariants."""
    from abcsmc_amd import device
    N, M, P, K, Kp, Nn, A = 100000, 32, 16, 10000, 10000, 100000, 8
    wl, X, Y, obs, spec, prev, gen, r = _run_generation(N, M, P, K, Kp, Nn, A, True)
    idx = gen.idx.cpu().numpy()
    dist = gen.dist.cpu().numpy()
    assert len(set(idx.tolist())) == K and idx.min() >= 0 and idx.max() < N
    assert np.all(np.diff(dist) >= 0)                                         # sortedness
    w = gen.w.cpu().numpy()
    assert np.all(w >= 0) and np.linalg.norm(w) == pytest.approx(1.0, rel=1e-10)
    parent = gen.parent.cpu().numpy()
    counts = np.bincount(parent, minlength=K)
    assert counts.sum() == Nn and parent.min() >= 0 and parent.max() < K      # checksum of resample counts
    # resample counts follow the weights (chi-square-ish sanity on the heaviest particles)
    top = np.argsort(-w)[:50]
    exp = Nn * w[top] / w.sum()
    assert np.all(np.abs(counts[top] - exp) < 6 * np.sqrt(exp) + 6)
    # idempotence: the same inputs and rng state give the same bits
    wl2, X2, Y2, obs2, spec2, prev2, gen2, r2 = _run_generation(N, M, P, K, Kp, Nn, A, True)
    assert np.array_equal(gen2.idx.cpu().numpy(), idx) and np.array_equal(gen2.w.cpu().numpy(), w)
    assert np.array_equal(gen2.parent.cpu().numpy(), parent)
    assert np.array_equal(device.to_numpy(gen2.next), device.to_numpy(gen.next))
    assert (r.s1, r.s2, r.s3) == (r2.s1, r2.s2, r2.s3)


# ---------------------------------------------------------------------------------------------------
# C++ facade with the reference's signatures (abcsmc_amd/cxx/AbcUtilHip.hpp)
# ---------------------------------------------------------------------------------------------------
def test_cxx_facade_demo(gpu_ctx, tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "facade_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(root, "abcsmc_amd", "cxx", "facade_demo.cpp"),
                           "-L" + os.path.join(root, "abcsmc_amd"), "-labcsmc_hip",
                           "-Wl,-rpath," + os.path.join(root, "abcsmc_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "facade ok" in out.stdout
    # ABC::set_component_rule: the facade's default is the Wilcoxon reduction; both rules rank as the oracle does under them
    # (the demo's data regenerated here from the same taus2 stream)
    from oracle import pyoracle as O
    assert "rules: default 1 invalid_rejected 1 same_as_default 1" in out.stdout
    N, M, P = 2000, 6, 3
    g = O.rng(42)
    X, Y = np.empty((N, M)), np.empty((N, P))
    for i in range(N):
        for p in range(P):
            Y[i, p] = O.rng_get(g) / 4294967296.0 * 10.0
        for m in range(M):
            X[i, m] = Y[i, m % P] * (1.0 + m) + O.rng_get(g) / 4294967296.0
    obs = np.array([5.0 * (1.0 + m) + 0.5 for m in range(M)])
    lines = {ln.split(":")[0]: [int(v) for v in ln.split(":")[1].split()] for ln in out.stdout.splitlines() if ln.startswith(("press:", "wilcoxon:"))}
    assert lines["press"] == [int(v) for v in O.particle_ranking_pls(X, Y, obs, 0.5, rule=O.RULE_MIN_PRESS)["idx"][:12]]
    assert lines["wilcoxon"] == [int(v) for v in O.particle_ranking_pls(X, Y, obs, 0.5, rule=O.RULE_WILCOXON)["idx"][:12]]
    # ABC::gsl_ran_trunc_normal / gsl_ran_trunc_mv_normal (AbcUtil.h:80-91), one row each on the shared taus2 stream: the oracle's
    # sample_predictive_priors / sample_mvn_predictive_priors of a one-row posterior, bit for bit, and the same stream position after
    from abcsmc_amd import _lib
    spec = [(_lib.PRIOR_UNIF_INT, 1, 1000), (_lib.PRIOR_UNIF_REAL, -2.0, 3.0), (_lib.PRIOR_GAUSS, 5.0, 10.0)]
    mu, s2 = np.array([[500.2, 2.9, 4.0]]), np.array([2500.0, 4.0, 1.5])
    r1 = O.rng(777)
    want = O.sample_predictive_priors(r1, 1, np.array([1.0]), np.asfortranarray(mu), O.make_priors(spec), s2)
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("trunc_normal:")][0].split()
    assert [float(v) for v in got[1:4]] == [float(v) for v in np.asarray(want[0]).ravel()], (got, want)
    assert int(got[5]) == O.rng_get(r1)
    L = np.asfortranarray(np.array([[40.0, 0, 0], [0.7, 1.9, 0], [-0.3, 0.4, 1.1]]))
    r2 = O.rng(778)
    want = O.sample_mvn_predictive_priors(r2, 1, np.array([1.0]), np.asfortranarray(mu), O.make_priors(spec), L)
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("trunc_mv_normal:")][0].split()
    assert [float(v) for v in got[1:4]] == [float(v) for v in np.asarray(want[0]).ravel()], (got, want)
    assert int(got[5]) == O.rng_get(r2)


# ---------------------------------------------------------------------------------------------------
# Wilcoxon-reduced component count ([PLS] optimal_num_components)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,P,A,f,seed", [(400, 10, 4, 0, 0.5, 1), (1000, 32, 16, 8, 0.5, 2), (250, 12, 3, 3, 0.6, 3),
                                             (3000, 20, 6, 6, 0.5, 4), (120, 8, 5, 5, 0.5, 5), (5000, 32, 16, 8, 0.5, 6),
                                             (600, 48, 70, 6, 0.5, 7),      # more than 64 responses
                                             (500, 44, 9, 40, 0.5, 8)])     # more than 32 components (scores in chunks of 32)
def test_particle_ranking_pls_wilcoxon_rule(gpu_ctx, oracle, N, M, P, A, f, seed):
    from abcsmc_amd import abcutil, _lib
    wl, X, Y, obs = _wl(M, P, N, seed)
    # noisier responses make later components insignificant, so the reduction actually bites
    rng = np.random.default_rng(seed)
    Y = np.asfortranarray(Y + rng.normal(size=Y.shape) * Y.std(0) * 1.5)
    g = abcutil.particle_ranking_PLS(X, Y, obs, f, max_comp=A, rule=_lib.RULE_WILCOXON, details=True, ctx=gpu_ctx)
    o = oracle.particle_ranking_pls(X, Y, obs, f, A, rule=oracle.RULE_WILCOXON)
    o0 = oracle.particle_ranking_pls(X, Y, obs, f, A, rule=oracle.RULE_MIN_PRESS)
    assert g["ncomp"] == o["ncomp"], (g["ncomp"], o["ncomp"], o0["ncomp"])
    assert np.allclose(g["dist"], o["dist"][g["idx"].astype(int)], rtol=RTOL)
    assert _near_tie_ok(g["idx"], o["idx"], o["dist"])


def test_wilcoxon_rule_reduces_somewhere(oracle):
    """sanity of the test design: at least one of the cases above is a genuine reduction"""
    hit = 0
    for (N, M, P, A, f, seed) in [(400, 10, 4, 0, 0.5, 1), (250, 12, 3, 3, 0.6, 3), (120, 8, 5, 5, 0.5, 5)]:
        wl, X, Y, obs = _wl(M, P, N, seed)
        rng = np.random.default_rng(seed)
        Y = np.asfortranarray(Y + rng.normal(size=Y.shape) * Y.std(0) * 1.5)
        a = oracle.particle_ranking_pls(X, Y, obs, f, A, rule=oracle.RULE_WILCOXON)["ncomp"]
        b = oracle.particle_ranking_pls(X, Y, obs, f, A, rule=oracle.RULE_MIN_PRESS)["ncomp"]
        assert a <= b
        hit += a < b
    assert hit >= 1


def _stats_record(gpu_ctx, X, Y, ntrain):
    """the sufficient-statistics record of [X | Y] through the staged entry points -> (shift, sums[2], G[2]) as numpy"""
    import torch
    from abcsmc_amd import device, sharded
    dev = "cuda:0"
    be = sharded.HipBackend(dev, gpu_ctx)
    N, M = X.shape
    P = Y.shape[1]
    dX, dY = device.colmajor(X, dev), device.colmajor(Y, dev)
    stats = be.zeros(be.stats_len(M, P))
    be.stats_shift(dX, dY, stats)
    be.stats_accumulate(dX, dY, 0, ntrain, stats)
    torch.cuda.synchronize()
    st = stats.cpu().numpy()
    C16 = 16 * ((M + P + 15) // 16)
    shift = st[2:2 + C16]
    sums = [st[2 + C16:2 + 2 * C16], st[2 + 2 * C16:2 + 3 * C16]]
    G = [st[2 + 3 * C16:2 + 3 * C16 + C16 * C16].reshape(C16, C16).T, st[2 + 3 * C16 + C16 * C16:2 + 3 * C16 + 2 * C16 * C16].reshape(C16, C16).T]
    return shift, sums, G


@pytest.mark.parametrize("N,M,P,kind", [(200_000, 128, 16, "plain"), (400_000, 120, 8, "plain"), (231_073, 140, 20, "plain"),
                                        (240_000, 128, 16, "spikes"), (240_000, 128, 16, "heavy"), (220_000, 113, 16, "constant"),
                                        (200_000, 144, 16, "plain"), (210_000, 112, 16, "spikes"), (2_000_000, 64, 32, "heavy"), (220_000, 100, 8, "heavy"), (240_000, 90, 20, "plain"),
                                        # the (C, CY) instantiations no case above reaches: (7, 2), (8, 2), (9, 0), (9, 2), (10, 0), (10, 2), (6, 1)
                                        (200_000, 73, 36, "plain"), (200_000, 89, 36, "plain"), (200_000, 131, 6, "plain"),
                                        (200_000, 105, 36, "plain"), (200_000, 147, 6, "plain"), (200_000, 121, 36, "plain"),
                                        (2_000_000, 69, 23, "plain")])
def test_wide_gram_on_the_i8_matrix_pipe(gpu_ctx, N, M, P, kind):
    """k_gram_i8 (round 4; round 5: four rows per thread in the conversion, two sets of byte planes, one barrier per tile -- 160 columns
    leave LDS for two raw tiles instead of three, 128 columns are two whole conversion rounds; 81..96 columns take it from 2e6 rows -- the
    configs[3] column shape): the Gram of 113..160 columns (from 200000 rows) from four signed bytes per value on v_mfma_i32_32x32x32_i8.
    Against numpy on the same shifted data: column sums and the diagonal (fp64 on the vector pipe) to rounding, the off-diagonal
    products -- exact integer arithmetic on values rounded to a 32-bit grid of 4 x a robust sample range, byte pairs below 2^-32 of the
    top pair dropped -- to 5e-10 of sqrt(G_aa G_bb) (it falls with the square root of the rows); with values far outside the sampled
    range (their rows go through k_gram_far in fp64), heavy tails, a column of tiny variance and a constant one; an odd row count
    (no 16-byte row pairs for the LDS-DMA staging) stays on the fp64 matrix pipe"""
    from abcsmc_amd import _lib
    from _gram_dispatch import GRAM_I8, kernel_for
    fam = kernel_for(M, P, N, N // 2, mode=GRAM_I8)
    assert fam[0] == ("i8" if N % 2 == 0 else "wide"), fam
    gpu_ctx.set_gram_mode(_lib.GRAM_I8)        # (round 6: ABC_GRAM_AUTO takes this kernel from 400 000 rows per partition only)
    wl, X, Y, obs = _wl(M, P, N, 21)
    rng = np.random.default_rng(3)
    if kind == "spikes":                      # a handful of values hundreds of times beyond anything the 4096 sampled rows hold
        for r, c, f in ((5, 3, 900.0), (N // 2 + 1, 77, -2000.0), (N - 2, M - 1, 1e6), (12345, 0, 50.0), (N // 2, 100, 1e4)):
            X[r, c] = X[:, c].mean() + f * X[:, c].std()
        Y[777, 2] = Y[:, 2].mean() - 300.0 * Y[:, 2].std()
    elif kind == "heavy":                     # Cauchy-tailed metrics: hundreds of far rows
        X[:, :8] = X[:, :8].mean(axis=0) + X[:, :8].std(axis=0) * rng.standard_cauchy(size=(N, 8))
    elif kind == "constant":                  # constant wherever the sample looks (every 19th row of the 4096 samples' stride), not elsewhere
        X[:, 5] = 3.25
        X[1::7, 5] = 3.25 + rng.normal(size=len(X[1::7, 5])) * 1e-3
        X[:, 9] = -1.0                       # ... and one that is constant throughout
    X, Y = np.asfortranarray(X), np.asfortranarray(Y)
    ntrain = N // 2
    try:
        shift, sums, G = _stats_record(gpu_ctx, X, Y, ntrain)
    finally:
        gpu_ctx.set_gram_mode(_lib.GRAM_AUTO)
    Z = np.hstack([X, Y])
    C = M + P
    worst, where, worst_vs_model = 0.0, "", 0.0
    from _gram_model import gram_error_bound
    for part, (a, b) in enumerate(((0, ntrain), (ntrain, N))):
        V = Z[a:b] - shift[:C]
        ref = V.T @ V
        sref = V.sum(axis=0)
        scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref))) + 1e-300
        assert np.allclose(sums[part][:C], sref, rtol=1e-10, atol=1e-13 * np.abs(V).sum(axis=0).max())
        assert np.allclose(np.diag(G[part])[:M], np.diag(ref)[:M], rtol=1e-12)                       # X'X diagonal: fp64
        assert np.allclose(np.diag(G[part])[M:C], np.diag(ref)[M:C], rtol=1e-12)                     # Y'Y diagonal
        blockXX = np.abs(G[part][:M, :M] - ref[:M, :M]) / scale[:M, :M]
        blockXY = np.abs(G[part][:M, M:C] - ref[:M, M:C]) / scale[:M, M:C]
        # the kernel's error model, per entry (tests/_gram_model.py: 4 x 2^-32 range_a range_b sqrt(rows), range_c as k_pilot_scale
        # takes it) -- the ONE contract of the header, the fuzzer and this test; an odd row count stays on the fp64 kernel
        ratio = np.abs(G[part][:M, :C] - ref[:M, :C]) / ((gram_error_bound(Z, shift[:C], a, b)[:M, :C] if N % 2 == 0 else 1e-13 * scale[:M, :C]) + 1e-300)
        np.fill_diagonal(ratio[:, :M], 0.0)
        worst_vs_model = max(worst_vs_model, float(ratio.max()))
        if max(blockXX.max(), blockXY.max()) > worst:
            worst = max(blockXX.max(), blockXY.max())
            full = np.abs(G[part][:M, :C] - ref[:M, :C]) / scale[:M, :C]
            wa, wb = np.unravel_index(np.argmax(full), full.shape)
            where = "partition %d, columns (%d, %d): %.17g against %.17g" % (part, wa, wb, G[part][wa, wb], ref[wa, wb])
        assert np.allclose(G[part][:M, :C], G[part][:C, :M].T)                                       # symmetric where both halves exist
    print("wide Gram %s N=%d: worst off-diagonal error %.2e of sqrt(G_aa G_bb) (%s) = %.2f x the error model's bound" % (kind, N, worst, where, worst_vs_model))
    assert worst_vs_model <= 1.0, (worst_vs_model, worst)


def test_gram_mode_is_a_public_setting(gpu_ctx):
    """abc_ctx_set_gram_mode (the precision of the wide sets' statistics was an internal switch): ABC_GRAM_FP64 sends
    a set the byte-limb kernel would take to the fp64 matrix pipe -- off-diagonal products to 1e-13 of sqrt(G_aa G_bb) instead of
    ~1e-10 --, ABC_GRAM_I8 brings the byte-limb kernel back (a different, less exact record), ABC_GRAM_AUTO takes it only where every
    partition holds 400 000 rows (round 6: the loadings-level contract, tests/fuzz/wide_model_fuzz.py), an unknown mode is refused"""
    from abcsmc_amd import _lib
    N, M, P = 200_000, 128, 16
    wl, X, Y, obs = _wl(M, P, N, 21)
    X, Y = np.asfortranarray(X), np.asfortranarray(Y)
    ntrain, C = N // 2, M + P
    Z = np.hstack([X, Y])

    def worst():
        shift, sums, G = _stats_record(gpu_ctx, X, Y, ntrain)
        w = 0.0
        for part, (a, b) in enumerate(((0, ntrain), (ntrain, N))):
            V = Z[a:b] - shift[:C]
            ref = V.T @ V
            scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref))) + 1e-300
            w = max(w, float((np.abs(G[part][:M, :C] - ref[:M, :C]) / scale[:M, :C]).max()))
        return w
    try:
        gpu_ctx.set_gram_mode(_lib.GRAM_FP64)
        e64 = worst()
        gpu_ctx.set_gram_mode(_lib.GRAM_I8)
        e8 = worst()
        gpu_ctx.set_gram_mode(_lib.GRAM_AUTO)         # (round 6: 1e5 rows per partition are fewer than the 400 000 the default asks for)
        eauto = worst()
    finally:
        gpu_ctx.set_gram_mode(_lib.GRAM_AUTO)
    print("wide Gram, 144 columns x 2e5 rows: worst off-diagonal error %.2e (ABC_GRAM_FP64), %.2e (ABC_GRAM_I8: byte limbs), %.2e (ABC_GRAM_AUTO)"
          % (e64, e8, eauto))
    assert e64 <= 1e-13 and 1e-13 < e8 <= 5e-10 and eauto <= 1e-13, (e64, e8, eauto)
    assert _lib.lib().abc_ctx_set_gram_mode(gpu_ctx.handle, 7) == _lib.lib().abc_ctx_set_gram_mode(None, 0) != 0


def _wilcoxon_per_response(gpu_ctx, oracle, X, Y, obs, A, f=0.5, near_ok=False):
    """The Wilcoxon reduction alone, through the staged entry points: statistics -> model under argmin PRESS -> abc_pls_wilcoxon_dev;
    the per-response component counts it leaves in the model record against the oracle's reduction RUN ON THE DEVICE'S OWN MODEL
    (its loadings, means and deviations: the residuals are then the same bits on both sides, and so is every rank sum).
    The call runs twice: as it always did, and with the per-test record on (abc_wx_last_record) -- the model record it leaves is
    the same bytes, and every test's count of non-zero differences, rank sum, bounds and verdict are held against the oracle's
    statistic (tests/_wx_record.py).  No bounds verdict may go unchecked because its reference p lies within 1e-9 of 0.1 -- the
    fixed seeds of the tests have none; near_ok (the fuzzer's random sets) only reports them."""
    import _wx_record
    N, M = X.shape
    P = Y.shape[1]
    on = _wx_record.run_reduction(gpu_ctx, X, Y, obs, A, f, record=True, both="off first")
    m0, m1, ntrain = on["m0"], on["m1_off"], on["ntrain"]
    assert on["m1"].tobytes() == m1.tobytes()
    L = len(m0) - 8
    Zx, Zy, R, Q, per_press = _wx_record.oracle_inputs(X, Y, m0, A, ntrain)
    per_wx = m1[L - P:L].astype(int)
    _, o_press = oracle.pls_optimal_components(Zx, Zy, R, Q, oracle.RULE_MIN_PRESS)
    _, o_wx = oracle.pls_optimal_components(Zx, Zy, R, Q, oracle.RULE_WILCOXON)
    if np.array_equal(per_press, o_press):                # (else the caller's first assertion fails: different tests on the two sides)
        ref = _wx_record.reference(oracle, X, Y, m0, A, ntrain)
        out = _wx_record.check_record(on["path"], on["rec"], ref, m1, P, label="N=%d P=%d A=%d" % (N, P, A))
        print("wilcoxon record: %d tests, path %d, %d sums taken, %d verdicts by the bounds (%d next to the threshold left out), levels %s"
              % (len(on["rec"]), on["path"], out["taken"], out["settled"], out["left_out"], sorted(out["levels"].items())))
        assert near_ok or (not ref["near"] and out["left_out"] == 0), ref["near"]
    return per_press, per_wx, o_press.astype(int), o_wx.astype(int), int(m1[0])


@pytest.mark.parametrize("N,M,P,A,kind", [
    (6000, 10, 4, 4, "plain"),             # 3000 validation rows: one bin, sorted as a whole in LDS
    (6000, 10, 4, 4, "pairs"),             # every validation row twice: tie groups of two, average ranks
    (6000, 12, 5, 5, "zeros"),             # responses the model predicts equally well at several counts: zero differences dropped
    (40_000, 16, 6, 8, "plain"),           # 2e4 validation rows: 16 bins
    (40_000, 16, 6, 8, "pairs"),
    (300_000, 32, 16, 8, "plain"),         # 1.5e5 rows, up to 112 tests: one group of tests, 37 tiles -- one row per thread (_wx_dispatch.py)
    (300_000, 24, 8, 16, "plain"),         # 9..16 components: 74 tiles of two rows per thread are fewer than 192 -- one row per thread
    (200_000, 40, 6, 24, "plain"),         # one row per thread (17..32 components)
    (300_000, 16, 4, 6, "copies50"),       # 50 distinct validation rows: tie groups of 3000, a few values per bin
    (300_000, 16, 4, 6, "copies8"),        # 8 distinct rows: groups of 18750 would outgrow a bin of the exact step -- but a tie group has one
                                           # sign, so level 0's bounds are points and settle every test (the record: path 0, one level); the
                                           # repeat on the sorted path is reached in test_gpu_wilcoxon.py (two distinct rows, every test forced)
    (10_000_000, 8, 2, 4, "plain"),        # 5e6 validation rows (configs[3]'s count): level 0 at four rows per thread (k_wx_sweep<8, 4, 0>)
])
def test_wilcoxon_reduction_per_response_binned_path(gpu_ctx, oracle, N, M, P, A, kind):
    """Round 4's binned rank sums (wilcoxon.hip): per response the reduced component count equals the oracle's, on plain data, on
    tie-heavy data (average ranks across tie groups that fill whole bins) and where a bin outgrows LDS (the reduction then repeats
    itself on the sorted path)"""
    wl, X, Y, obs = _wl(M, P, N, 11)
    rng = np.random.default_rng(7)
    Y = np.asfortranarray(Y + rng.normal(size=Y.shape) * Y.std(0) * 1.5)      # noisy responses: later components insignificant
    nt0 = N // 2
    if kind == "pairs":
        X[nt0 + 1:N:2], Y[nt0 + 1:N:2] = X[nt0:N - 1:2], Y[nt0:N - 1:2]
    elif kind == "zeros":
        Y[:, 0] = Y[:, 0].mean() + 1e-9 * rng.normal(size=N)                   # a response nothing predicts
        Y[nt0:, 1] = Y[nt0, 1]                                                  # ... and one that is constant on the validation rows
    elif kind.startswith("copies"):
        c = int(kind[6:])
        src = nt0 + (np.arange(N - nt0) % c)
        X[nt0:], Y[nt0:] = X[src], Y[src]
    X, Y = np.asfortranarray(X), np.asfortranarray(Y)
    gpu_ctx.alias_stats(reset=True)
    per_press, per_wx, o_press, o_wx, ncomp = _wilcoxon_per_response(gpu_ctx, oracle, X, Y, obs, A)
    assert np.array_equal(per_press, o_press), (per_press, o_press)           # (same argmin: else the tests below compare different things)
    assert np.array_equal(per_wx, o_wx), (per_wx, o_wx, per_press)
    assert ncomp == o_wx.max() and np.all(per_wx <= per_press)
    print("wilcoxon %s N=%d: PRESS optima %s -> %s" % (kind, N, per_press.tolist(), per_wx.tolist()))


def test_wilcoxon_paths_agree(gpu_ctx, oracle, tmp_path):
    """the binned path (tests settled by the bounds sweep where they can be), the same with every test through the exact sweeps
    (ABC_WX_NOBOUNDS), the sorted path (ABC_WX_SORTED) and a binned reduction forced to repeat itself on the sorted path
    (ABC_WX_FORCE_FAIL) leave the same component counts -- each in a process of its own (the switches are read once)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_parity as T\nfrom oracle import pyoracle as O\nfrom abcsmc_amd import _lib\n"
            "wl, X, Y, obs = T._wl(24, 8, 120000, 11)\nrng = np.random.default_rng(7)\n"
            "Y = np.asfortranarray(Y + rng.normal(size=Y.shape) * Y.std(0) * 1.5)\n"
            "r = T._wilcoxon_per_response(_lib.default_context(0), O, np.asfortranarray(X), Y, obs, 8)\n"
            "print('RESULT', r[1].tolist(), r[3].tolist(), r[4])\n") % (root, os.path.join(root, "tests"))
    outs, dbg = [], []
    for extra in ({}, {"ABC_WX_NOBOUNDS": "1"}, {"ABC_WX_SORTED": "1"}, {"ABC_WX_FORCE_FAIL": "1"}):
        env = dict(os.environ, ABC_DIAG="1", ABC_WX_DEBUG="1", **extra)
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
        outs.append([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][0])
        dbg.append([ln for ln in p.stderr.splitlines() if ln.startswith("WX_DEBUG")])
    assert outs[0] == outs[1] == outs[2] == outs[3], outs
    # the default run settled tests by their bounds and left some to the exact sweeps (noisy responses: statistics near the
    # threshold exist); with the switch every test is undecided
    import re
    m0 = re.search(r"rejected (\d+), passed (\d+), undecided (\d+)", dbg[0][0])
    m1 = re.search(r"rejected (\d+), passed (\d+), undecided (\d+)", dbg[1][0])
    print(dbg[0][0], "|", dbg[1][0])
    assert int(m0.group(1)) + int(m0.group(2)) > 0
    assert int(m1.group(1)) + int(m1.group(2)) == 0 and int(m1.group(3)) > 0
    got, want = eval(outs[0].split(" ", 1)[1].split("] ")[0] + "]"), eval("[" + outs[0].split("] [")[1].split("]")[0] + "]")
    assert got == want, (got, want)


def _generation_size_properties(gpu_ctx, oracle, N, M, P, K, Kp, Nn, A, kde_tol, device_inputs=False, oracle_model=True,
                                rule=0, multivariate=True):
    """A full generation at a BASELINE size.  (1) The PLS model at size: the oracle's own ranking of the same set (its
    independent algorithm) -- component count equal, every loading column within 1e-6 of the oracle's, the K winners the
    oracle's up to near-ties, their distances within 1e-6.  (2) Invariants that do not need the O(K K' P) oracle --
    sortedness, selection = the oracle's ordering of the device's own distances (bit-exact), L2 norm, weights of a few rows
    against the oracle formula restricted to those rows, parents = the oracle's resampling of the device's own weights
    (bit-exact), finite proposals inside the prior support, MVN factor against numpy."""
    from abcsmc_amd import abcutil, device
    run = _run_generation_device_inputs if device_inputs else _run_generation
    wl, X, Y, obs, spec, prev, gen, r = run(N, M, P, K, Kp, Nn, A, multivariate, rule=rule)
    idx, dist = gen.idx.cpu().numpy(), gen.dist.cpu().numpy()
    assert np.all(np.diff(dist) >= 0) and len(np.unique(idx)) == K
    # full distance vector through the staged entry point, then the oracle's argsort on those exact values
    g = abcutil.particle_ranking_PLS(X, Y, obs, 0.5, K=N, max_comp=A, rule=rule, details=True, ctx=gpu_ctx)
    assert g["ncomp"] == gen.ncomp.value and 1 <= g["ncomp"] <= A
    full = np.empty(N)
    full[g["idx"].astype(np.int64)] = g["dist"]
    ref = oracle.ordered(full)[:K]
    assert np.array_equal(idx.astype(np.uint64), ref)                       # bit-exact selection at full size
    assert np.array_equal(dist, full[ref.astype(np.int64)])
    if oracle_model:
        # the model against the oracle's independent fit of the same N rows (AbcUtil.cpp:423-458)
        # (under the Wilcoxon rule the oracle sorts the validation rows once per (response, candidate) test: ~0.1 s each at 5e5 rows)
        o = oracle.particle_ranking_pls(X, Y, obs, 0.5, A, rule=rule)
        assert g["ncomp"] == o["ncomp"], (g["ncomp"], o["ncomp"])
        assert np.allclose(g["mean"], o["mean"], rtol=1e-12) and np.allclose(g["sd"], o["sd"], rtol=1e-11)
        worst = max(np.linalg.norm(g["R"][:, k] - o["R"][:, k]) / np.linalg.norm(o["R"][:, k]) for k in range(o["ncomp"]))
        assert worst <= RTOL, worst                                         # loadings: 1e-6 of the column norm
        od = o["dist"]
        derr = float(np.max(np.abs(full - od) / od))
        assert derr <= RTOL, derr                                           # all N distances
        # the K winners are the oracle's up to near-ties: position by position the oracle's distance of the device's
        # winner equals the oracle's distance of its own winner to 1e-7 (a tenth of the bar; measured ~1e-10: the models
        # differ by rounding only)
        oi = o["idx"][:K].astype(np.int64)
        perr = float(np.max(np.abs(od[idx] - od[oi]) / od[oi]))
        ndiff = len(np.setdiff1d(idx, oi))
        print("model at size N=%d M=%d P=%d: ncomp %d, worst loading column %.2e, worst distance %.2e, winners: position "
              "error %.2e, %d of %d differ as sets" % (N, M, P, o["ncomp"], worst, derr, perr, ndiff, K))
        assert perr <= 1e-7, perr
        assert ndiff <= max(4, K // 1000), ndiff                            # ... and the sets differ at the cut only
        del o, od
    # the distances themselves: oracle projection with the device's model on a sample of rows
    w = gen.w.cpu().numpy()
    assert np.all(w >= 0) and abs(np.linalg.norm(w) - 1.0) < 1e-10
    theta = Y[idx]
    assert np.array_equal(device.to_numpy(gen.theta), theta)
    assert np.allclose(gen.dv.cpu().numpy(), 2.0 * theta.var(axis=0, ddof=1), rtol=1e-9)
    # weights at size: 64+ STRATIFIED rows -- the 16 heaviest, the 16 lightest non-zero, the 16 farthest
    # from the previous set's centre in units of its kernel width (where the split-operand kernel's far-row fix-ups live), 16
    # random ones and the five of earlier rounds -- against the oracle's formula on exactly those rows.  The device normalises by
    # the L2 norm of ALL K raw weights, which the oracle cannot afford (O(K K' P)): the constant is taken as the median ratio over
    # the sample, and EVERY sampled row has to agree with it to the kernel's tolerance (absolute relative error, not ratios to one row)
    order = np.argsort(w, kind="stable")
    nzw = order[w[order] > 0]
    far = np.argsort(-np.max(np.abs(theta - prev[0].mean(axis=0)) / np.sqrt(np.where(prev[2] > 0, prev[2], 1.0)), axis=1), kind="stable")[:16]
    rows = np.unique(np.concatenate([order[-16:], nzw[:16], far, np.random.default_rng(5).integers(0, K, 16), [0, 1, 777 % K, K // 2, K - 1]]))
    raw = oracle.weights_importance(oracle.make_priors(spec), theta[rows], prev[0], prev[1], prev[2])
    ok = (raw > 0) & (w[rows] > 0)
    assert np.array_equal(raw > 0, w[rows] > 0) and ok.sum() >= 48
    c = np.median(raw[ok] / w[rows][ok])
    werr = float(np.max(np.abs(raw[ok] / (c * w[rows][ok]) - 1.0)))
    print("weights at size: %d stratified rows, largest relative error %.2e (tolerance %.1e)" % (len(rows), werr, 2 * kde_tol))
    assert werr <= 2 * kde_tol, werr
    parent = gen.parent.cpu().numpy()
    assert np.bincount(parent, minlength=K).sum() == Nn and parent.max() < K
    # the resampled parents are exactly the oracle's for the device's own weights
    o = oracle.rng(67890)
    assert np.array_equal(parent.astype(np.uint64), oracle.resample(o, w, Nn))
    if multivariate:
        cov = np.cov(theta, rowvar=False, ddof=1)
        cov[np.diag_indices(P)] *= 2.0                                       # AbcUtil.cpp:475-479
        assert np.allclose(np.tril(device.to_numpy(gen.L)), np.linalg.cholesky(cov), rtol=1e-7, atol=1e-12 * np.abs(cov).max() ** 0.5)
    nxt = device.to_numpy(gen.next)
    assert np.isfinite(nxt).all()
    for p in range(P):
        k, a, b = spec[p]
        if k == 2:
            assert nxt[:, p].min() >= a and nxt[:, p].max() <= b
    # a proposal is its parent plus noise of the doubled posterior variance (distributional: Philox stream)
    d = nxt - theta[parent]
    assert np.allclose(d.std(axis=0) / np.sqrt(gen.dv.cpu().numpy()), 1.0, atol=0.05)
    if not multivariate:
        # INDEPENDENT noise (the reference's default, AbcSmc.cpp:419; Priors.h:19-33): per-coordinate truncated normals -- the
        # coordinates' noise is uncorrelated although the posterior's coordinates are not
        cc = np.corrcoef(d[:200_000].T)
        assert np.max(np.abs(cc - np.eye(P))) < 0.02, np.max(np.abs(cc - np.eye(P)))


def test_generation_config3_size_independent_noise(gpu_ctx, oracle):
    """BASELINE configs[2] with noise = INDEPENDENT, the reference's default (AbcSmc.cpp:419): the at-size properties of the
    MULTIVARIATE test (selection bit-exact, stratified weights, parents bit-exact, support) plus uncorrelated per-coordinate noise"""
    _generation_size_properties(gpu_ctx, oracle, 1_000_000, 32, 16, 100_000, 100_000, 1_000_000, 8, KDE_TOL["auto"],
                                multivariate=False, oracle_model=False)


def test_generation_config3_size_wilcoxon_rule(gpu_ctx, oracle):
    """BASELINE configs[2] under the Wilcoxon component rule (the drop-in default of the C++ facade): up to 112 tests
    over 5e5 validation rows each on the binned path; the oracle sorts each test's rows (about ten seconds in all)"""
    from abcsmc_amd import _lib
    _generation_size_properties(gpu_ctx, oracle, 1_000_000, 32, 16, 100_000, 100_000, 1_000_000, 8, KDE_TOL["auto"],
                                rule=_lib.RULE_WILCOXON)


def test_generation_config5_size_wilcoxon_rule(gpu_ctx, oracle):
    """BASELINE configs[4] (128 metrics, 32 components: up to 496 tests over 5e5 validation rows) under the Wilcoxon rule"""
    from abcsmc_amd import _lib
    _generation_size_properties(gpu_ctx, oracle, 1_000_000, 128, 16, 100_000, 100_000, 1_000_000, 32, KDE_TOL["auto"],
                                device_inputs=True, rule=_lib.RULE_WILCOXON)


def test_generation_config2_size_against_the_full_oracle(gpu_ctx, oracle):
    """BASELINE configs[1] (1e5 particles x 16 parameters x 32 metrics, 8 components; K = K' = 1e4) against the COMPLETE oracle
    generation under the drop-in's default rule -- at this size the oracle's O(K K' P) weight stage is affordable (1.6e9 density
    evaluations, ~20 s on one core), so nothing is sampled: component count, all K selection indices and all N_next parents bit for
    bit, every weight to 1e-6 relative, doubled variances, posterior rows"""
    from abcsmc_amd import device
    N, M, P, K, Kp, Nn, A = 100_000, 32, 16, 10_000, 10_000, 100_000, 8
    wl, X, Y, obs, spec, prev, gen, r = _run_generation(N, M, P, K, Kp, Nn, A, True)
    o = oracle.rng(67890)
    ref = oracle.generation(X, Y, obs, oracle.make_priors(spec), K, Nn, o, *prev, train_frac=0.5, max_comp=A, multivariate=True)
    assert gen.ncomp.value == ref["ncomp"]
    assert np.array_equal(gen.idx.cpu().numpy().astype(np.uint64), ref["idx"])
    w = gen.w.cpu().numpy()
    werr = float(np.max(np.abs(w - ref["w"]) / ref["w"]))
    print("configs[1] against the full oracle: ncomp %d, largest relative weight error %.2e over all %d weights" % (ref["ncomp"], werr, K))
    assert werr <= RTOL, werr
    assert np.allclose(gen.dv.cpu().numpy(), ref["dv"], rtol=1e-9)
    assert np.array_equal(device.to_numpy(gen.theta), Y[ref["idx"].astype(int)])
    assert np.array_equal(gen.parent.cpu().numpy().astype(np.uint64), ref["parent"])


@pytest.mark.parametrize("M,P,A,noise,Kp", [(20, 5, 10, 2.0, 500), (16, 3, 8, 1.5, 0), (16, 6, 8, 0.0, 500), (40, 4, 20, 1.0, 500),
                                            (40, 4, 20, 2.0, 0)])
def test_generation_speculates_on_the_component_count(gpu_ctx, oracle, M, P, A, noise, Kp):
    """Whole generations on sets the Wilcoxon cascade takes run the ranking BESIDE the reduction, on the component count the fit wrote
    (api.hip, round 5): the ranking's projection scores all A components in its one pass over X (every row's scores are kept, the
    validation rows' go to the cascade) and takes the distance over the fit's count.  The host looks at the cascade -- which takes the
    tests of a few responses that hold the largest count first (round 6) -- in front of the weight stage.  With noisy responses the
    reduction lowers the largest count: the distances are taken again from the kept scores, selection and gather run once more
    (round 5's default had queued everything up to the proposals by then and repeated the whole generation).
    With clean responses the count stands.  Either way every output equals the oracle's generation under the rule -- the parents too,
    so the repeat starts from the generator's state at entry -- and the count equals the oracle's, which in the noisy cases is below
    the argmin-PRESS count (checked: the speculation is wrong there and has to be repaired).  8 / 10 components: the vector
    projection kernels; 20: the fp64 matrix-pipe one."""
    from abcsmc_amd import _lib, abcutil, device, synthetic
    N, K, Nn = 60_000, 2_000, 5_000
    wl = synthetic.Workload(M, P, 4713 if M == 20 else 4711)
    X, Y = wl.rows(0, N)
    if noise:
        Y = np.asfortranarray(Y + np.random.default_rng(7).normal(size=Y.shape) * Y.std(0) * noise)
    obs, spec = wl.observed(), wl.prior_spec()
    prev = wl.previous_set(Kp) if Kp else (None, None, None)
    dev = "cuda:0"
    gen = device.Generation(N, M, P, K, Kp, Nn, 0.5, A, rule=_lib.RULE_WILCOXON, multivariate=True, device=dev, ctx=gpu_ctx)
    r = abcutil.rng(67890)
    dprev = [device.colmajor(a, dev) for a in prev] if Kp else []
    gpu_ctx.generation_repeats(reset=True)
    gen.run(device.colmajor(X, dev), device.colmajor(Y, dev), device.colmajor(obs, dev), device.priors_to_device(_lib.make_priors(spec), dev), r, *dprev)
    ranking_repeats, generation_repeats = gpu_ctx.generation_repeats(reset=True)
    o = oracle.rng(67890)
    ref = oracle.generation(X, Y, obs, oracle.make_priors(spec), K, Nn, o, *prev, train_frac=0.5, max_comp=A, rule=oracle.RULE_WILCOXON, multivariate=True)
    press = oracle.particle_ranking_pls(X, Y, obs, 0.5, A, rule=oracle.RULE_MIN_PRESS)["ncomp"]
    print("speculation: argmin PRESS keeps %d components, the Wilcoxon rule %d (noise %.1f); ranking repeated %d times, generation %d times"
          % (press, ref["ncomp"], noise, ranking_repeats, generation_repeats))
    if noise:
        assert ref["ncomp"] < press            # (the case the test is for: the count the ranking speculated on is wrong)
    # what the repair cost (abc_generation_repeats): a moved count = the three ranking stages ONCE more, a count that stands = nothing;
    # the generation itself is never repeated (round 5's default did that).  Under the diagnostic switch that forces the cascade to
    # fail the counts are that switch's own.
    import os
    if not os.environ.get("ABC_WX_FORCE_FAIL"):
        assert (ranking_repeats, generation_repeats) == ((1, 0) if ref["ncomp"] < press else (0, 0))
    assert gen.ncomp.value == ref["ncomp"]
    assert np.array_equal(gen.idx.cpu().numpy().astype(np.uint64), ref["idx"])
    assert np.allclose(gen.w.cpu().numpy(), ref["w"], rtol=RTOL)
    assert np.array_equal(device.to_numpy(gen.theta), Y[ref["idx"].astype(int)])
    assert np.array_equal(gen.parent.cpu().numpy().astype(np.uint64), ref["parent"])


def test_generation_repeats_itself_when_the_cascade_gives_up(gpu_ctx):
    """the cascade reports failure (ABC_WX_FORCE_FAIL: as if a bin of its exact step had outgrown LDS) when the generation looks at
    it in front of its weight stage: the reduction runs once more in stream order (which, forced to fail again, repeats itself on
    the sorted path), and the ranking with it.
    The speculation test's weighted and first-set cases in a process of their own (the switch is read once): every output the
    oracle's, parents included"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ABC_DIAG="1", ABC_WX_FORCE_FAIL="1")
    ids = ["tests/test_gpu_parity.py::test_generation_speculates_on_the_component_count[%s]" % i for i in ("20-5-10-2.0-500", "16-3-8-1.5-0", "16-6-8-0.0-500")]
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + ids, capture_output=True, text=True,
                       timeout=900, env=env, cwd=root)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "3 passed" in p.stdout, p.stdout[-500:]


def test_wilcoxon_reduction_at_config4_stated_size(gpu_ctx, oracle):
    """BASELINE configs[3] at its STATED size under the drop-in's default rule: 1e7 particles x 64 metrics x 32 responses x 8
    components = up to 224 tests over 5e6 validation rows, through the staged entry points on device-generated rows (the model under
    argmin PRESS, then abc_pls_wilcoxon_dev).  The component count of EVERY response is compared with the oracle's reduction run on the
    device's own model -- for 2 of the 32 responses: the oracle sorts 5e6 differences per (response, candidate) test, about a
    second each, and the 224 tests of all responses would take four minutes; the responses are independent of each other in the
    reduction (optimal_num_components works response by response)."""
    import torch
    from abcsmc_amd import _lib, device, sharded, synthetic
    lib = _lib.lib()
    N, M, P, A = 10_000_000, 64, 32, 8
    dev = "cuda:0"
    wl, dX, dY, _, _ = _device_set(N, M, P)
    dobs = device.colmajor(wl.observed(), dev)
    be = sharded.HipBackend(dev, gpu_ctx)
    ntrain = N // 2
    stats = be.zeros(be.stats_len(M, P))
    L = be.model_len(M, P, A)
    model = be.zeros(L + 8)
    be.stats_shift(dX, dY, stats)
    be.stats_accumulate(dX, dY, 0, ntrain, stats)
    be.pls_model(stats, dobs, M, P, A, _lib.RULE_MIN_PRESS, model)
    torch.cuda.synchronize()
    m0 = model.cpu().numpy().copy()
    gpu_ctx.check(lib.abc_pls_wilcoxon_dev(gpu_ctx.handle, dX.data_ptr(), dY.data_ptr(), N, N, N, M, P, A, ntrain, model.data_ptr()))
    torch.cuda.synchronize()
    m1 = model.cpu().numpy()
    off_mean, off_sd = 4, 4 + M + P
    off_R = off_sd + (M + P) + M + A
    off_Q = off_R + M * A
    off_per = L - P
    per_press, per_wx = m0[off_per:L].astype(int), m1[off_per:L].astype(int)
    mean, sd = m0[off_mean:off_mean + M + P], m0[off_sd:off_sd + M + P]
    R = np.asfortranarray(m0[off_R:off_R + M * A].reshape(A, M).T)
    Q = np.asfortranarray(m0[off_Q:off_Q + P * A].reshape(A, P).T)
    assert int(m1[0]) == per_wx.max() and np.all(per_wx <= per_press) and np.all(per_wx >= 1)
    cols = [5, 26]                                                   # (round 6: two responses instead of six -- ~1 s of sorting per test)
    Xv = dX[:, ntrain:].cpu().numpy().T                              # (N - ntrain, M) view of the download
    Zx = np.asfortranarray((Xv - mean[:M]) / sd[:M])
    del Xv
    Yv = dY[cols][:, ntrain:].cpu().numpy().T
    Zy = np.asfortranarray((Yv - mean[M:][cols]) / sd[M:][cols])
    Qc = np.asfortranarray(Q[cols])
    _, o_press = oracle.pls_optimal_components(Zx, Zy, R, Qc, oracle.RULE_MIN_PRESS)
    _, o_wx = oracle.pls_optimal_components(Zx, Zy, R, Qc, oracle.RULE_WILCOXON)
    assert np.array_equal(per_press[cols], o_press.astype(int)), (per_press[cols], o_press)
    assert np.array_equal(per_wx[cols], o_wx.astype(int)), (per_wx[cols], o_wx, per_press[cols])
    print("wilcoxon at configs[3] size: PRESS optima %s -> %s (responses %s against the oracle)" % (per_press.tolist(), per_wx.tolist(), cols))


def test_generation_config4_full_size_wilcoxon_rule_properties(gpu_ctx, oracle):
    """... and the whole generation at that size under the rule: the size-independent properties (selection = the oracle's ordering
    of the device's own distances bit for bit, stratified weights against the oracle's formula, parents = the oracle's resampling of
    the device's weights, support, factor) without the oracle's own model fit (test above: the reduction per response)"""
    from abcsmc_amd import _lib
    _generation_size_properties(gpu_ctx, oracle, 10_000_000, 64, 32, 1_000_000, 1_000_000, 10_000_000, 8, KDE_TOL["auto"],
                                device_inputs=True, oracle_model=False, rule=_lib.RULE_WILCOXON)


def test_generation_config3_size_properties(gpu_ctx, oracle):
    """BASELINE configs[2] (N = 1e6, M = 32, P = 16, A = 8, K = K' = 1e5), the configuration the metric is quoted on"""
    _generation_size_properties(gpu_ctx, oracle, 1_000_000, 32, 16, 100_000, 100_000, 1_000_000, 8, KDE_TOL["auto"])


def test_generation_config4_shard_size_properties(gpu_ctx, oracle):
    """BASELINE configs[3] (10 M x 32 parameters x 64 metrics on 8 GPUs) at the size of one GPU's shard: N = 1.25e6,
    K = K' = 1.25e5 -- the four-wave LDS-DMA Gram kernel (6 column blocks), two-chunk split-operand weight kernel"""
    _generation_size_properties(gpu_ctx, oracle, 1_250_000, 64, 32, 125_000, 125_000, 1_250_000, 8, KDE_TOL["auto"])


def test_generation_config4_full_size_on_one_gpu(gpu_ctx, oracle):
    """BASELINE configs[3] at its STATED size on one MI355X: N = 1e7 particles x 32 parameters x 64 metrics, K = K' = 1e6
    (AbcSmc.cpp:645-646: the reference keeps whatever K the configuration says), N_next = 1e7.  1e12 weight pairs; K = 1e6
    winners go through the radix select and the LSD radix sort; inputs generated on the device (7.7 GB)"""
    _generation_size_properties(gpu_ctx, oracle, 10_000_000, 64, 32, 1_000_000, 1_000_000, 10_000_000, 8, KDE_TOL["auto"],
                                device_inputs=True)


def test_generation_config5_full_size_on_one_gpu(gpu_ctx, oracle):
    """BASELINE configs[4] at its STATED size on one MI355X: N = 1e6 particles x 16 parameters x 128 metrics, 32 PLS
    components, K = K' = 1e5, N_next = 1e6"""
    _generation_size_properties(gpu_ctx, oracle, 1_000_000, 128, 16, 100_000, 100_000, 1_000_000, 32, KDE_TOL["auto"],
                                device_inputs=True)


def test_generation_config5_shard_size_properties(gpu_ctx, oracle):
    """BASELINE configs[4] (1 M x 128 metrics, 32 PLS components on 8 GPUs) at the size of one GPU's shard: N = 1.25e5,
    K = K' = 12500 -- 144 columns: grouped Gram launches, eight-wave model fit with 32 components"""
    _generation_size_properties(gpu_ctx, oracle, 125_000, 128, 16, 12_500, 12_500, 125_000, 32, KDE_TOL["auto"])


# ---------------------------------------------------------------------------------------------------
# degenerate sizes: must neither hang nor fault, and agree with the oracle where the oracle is finite
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,P", [(2, 1, 1), (3, 1, 1), (5, 2, 1), (4, 3, 2), (17, 1, 3), (64, 5, 5), (129, 16, 16)])
def test_ranking_tiny_sets(gpu_ctx, oracle, N, M, P):
    from abcsmc_amd import abcutil
    rng = np.random.default_rng(N * 100 + M * 10 + P)
    Y = np.asfortranarray(rng.normal(size=(N, P)))
    X = np.asfortranarray(Y[:, :1] @ rng.normal(size=(1, M)) + 0.1 * rng.normal(size=(N, M)))
    obs = X[0] * 0.9
    A = min(M, P)
    g = abcutil.particle_ranking_PLS(X, Y, obs, 0.5, details=True, ctx=gpu_ctx)
    o = oracle.particle_ranking_pls(X, Y, obs, 0.5, 0)
    assert sorted(g["idx"].tolist()) == list(range(N))
    if np.isfinite(o["dist"]).all() and np.isfinite(g["dist"]).all():
        assert g["ncomp"] == o["ncomp"]
        assert np.allclose(g["dist"], o["dist"][g["idx"].astype(int)], rtol=1e-6, atol=1e-12)
    s = abcutil.particle_ranking_simple(X, Y, obs, details=True, ctx=gpu_ctx)
    oi, od = oracle.particle_ranking_simple(X, obs)
    assert np.allclose(s["dist"], od[s["idx"].astype(int)], rtol=1e-9, atol=1e-12)


def test_generation_tiny(gpu_ctx, oracle):
    N, M, P, K, Kp, Nn, A = 40, 3, 2, 10, 8, 25, 2
    wl, X, Y, obs, spec, prev, gen, r = _run_generation(N, M, P, K, Kp, Nn, A, True)
    o = oracle.rng(67890)
    ref = oracle.generation(X, Y, obs, oracle.make_priors(spec), K, Nn, o, *prev, train_frac=0.5, max_comp=A)
    assert np.array_equal(gen.idx.cpu().numpy().astype(np.uint64), ref["idx"])
    assert np.allclose(gen.w.cpu().numpy(), ref["w"], rtol=RTOL)
    assert np.array_equal(gen.parent.cpu().numpy()[:Nn].astype(np.uint64), ref["parent"])


def _distributed_select_replay(gpu_ctx, oracle, d, n_loc, W, Ks):
    """The sharded driver's exact selection (6 all-reduced radix histograms, tie hand-out by global row, padded
    gather, stable merge sort) replayed in one process over W emulated shards of n_loc rows, for every K of Ks; checked against
    the oracle's order -> {K: (per shard [#below, #equal], per shard ties taken)}"""
    import torch
    from abcsmc_amd import sharded
    be = sharded.HipBackend("cuda:0", gpu_ctx)
    shards = [torch.from_numpy(d[q * n_loc:(q + 1) * n_loc].copy()).cuda() for q in range(W)]
    seen = {}
    for K in Ks:
        st = [be.zeros(8, torch.int64) for _ in range(W)]
        hs = [be.zeros(2048, torch.int32) for _ in range(W)]
        for q in range(W):
            be.select_begin(K, st[q], hs[q])
        for p in range(6):
            for q in range(W):
                be.select_hist(shards[q], st[q], p, hs[q])
            tot = sum(hs)                                                  # the all-reduce
            for q in range(W):
                hs[q].copy_(tot)
                be.select_pick(st[q], p, hs[q], K)
        assert all(torch.equal(st[0], s) for s in st)
        cnt = []
        for q in range(W):
            c = be.zeros(2, torch.int64)
            be.select_count(shards[q], st[q], c)
            cnt.append(c.cpu().tolist())
        remaining = K - sum(c[0] for c in cnt)
        take = []
        for q in range(W):
            tq = min(cnt[q][1], max(remaining, 0))
            take.append(tq)
            remaining -= tq
        assert remaining == 0
        idxs, dists = [], []
        for q in range(W):
            nw = cnt[q][0] + take[q]
            io, do = be.zeros(max(nw, 1), torch.int64), be.zeros(max(nw, 1))
            be.select_compact(shards[q], st[q], cnt[q][0], take[q], q * n_loc, io, do)
            idxs.append(io[:nw])
            dists.append(do[:nw])
        # as the sharded driver does it: every shard sorts its own winners, pads to the longest run with sentinels,
        # the runs are laid out back to back (the all-gather) and merged by ranking
        maxw = max(max(i.numel() for i in idxs), 1)
        ri, rd = be.zeros(W * maxw, torch.int64), be.zeros(W * maxw)
        for q in range(W):
            if idxs[q].numel() > 1:
                be.sort_pairs(dists[q], idxs[q])
            ri[q * maxw:(q + 1) * maxw].fill_(1 << 62)
            rd[q * maxw:(q + 1) * maxw].fill_(float("inf"))
            ri[q * maxw:q * maxw + idxs[q].numel()].copy_(idxs[q])
            rd[q * maxw:q * maxw + idxs[q].numel()].copy_(dists[q])
        mi, md = be.zeros(W * maxw, torch.int64), be.zeros(W * maxw)
        be.merge_runs(rd, ri, W, maxw, md, mi)
        # and the single stable sort of the concatenation it replaces
        ci, cd = torch.cat(idxs).contiguous(), torch.cat(dists).contiguous()
        assert ci.numel() == K
        be.sort_pairs(cd, ci)
        torch.cuda.synchronize()
        ref = oracle.ordered(d)[:K]
        assert np.array_equal(ci.cpu().numpy().astype(np.uint64), ref), K
        assert np.array_equal(cd.cpu().numpy(), d[ref.astype(np.int64)])
        assert np.array_equal(mi[:K].cpu().numpy().astype(np.uint64), ref), K
        assert np.array_equal(md[:K].cpu().numpy(), d[ref.astype(np.int64)])
        assert bool(torch.all(mi[K:] == (1 << 62))) and bool(torch.all(torch.isinf(md[K:])))
        seen[K] = (cnt, take)
    return seen


def test_distributed_select_protocol_with_ties(gpu_ctx, oracle):
    """the replay over 3 emulated shards, on tie-heavy keys"""
    rng = np.random.default_rng(12)
    n_loc, W = 5000, 3
    d = np.round(np.abs(rng.normal(size=n_loc * W)) * 20) / 20.0          # ~80 distinct values: massive ties
    _distributed_select_replay(gpu_ctx, oracle, d, n_loc, W, (1, 37, 4999, 5000, 7501, 14999))


# ---------------------------------------------------------------------------------------------------
# error conventions of the C ABI (int status + message, never exit/abort)
# ---------------------------------------------------------------------------------------------------
def test_error_codes_and_messages(gpu_ctx):
    import ctypes as C
    from abcsmc_amd import _lib, abcutil
    L = _lib.lib()
    h = gpu_ctx.handle
    X = np.asfortranarray(np.random.default_rng(0).normal(size=(50, 4)))
    Y = np.asfortranarray(np.random.default_rng(1).normal(size=(50, 2)))
    idx = np.zeros(50, dtype=np.uint64)
    # null argument -> ABC_ERR_INVALID (-1)
    assert L.abc_particle_ranking_pls(h, None, None, None, 50, 4, 2, 0.5, 0, 0, 10, None, None, None, None, None, None) == -1
    assert b"null" in L.abc_last_error(h)
    # unknown component rule
    rc = L.abc_particle_ranking_pls(h, X.ctypes.data, Y.ctypes.data, X[0].copy().ctypes.data, 50, 4, 2, 0.5, 0, 7, 10,
                                    idx.ctypes.data, None, None, None, None, None)
    assert rc == -1 and b"rule" in L.abc_last_error(h)
    # more components than metrics -> ABC_ERR_INVALID (-1), not a crash
    X70 = np.asfortranarray(np.random.default_rng(2).normal(size=(200, 8)))
    Y70 = np.asfortranarray(np.random.default_rng(3).normal(size=(200, 4)))
    idx70 = np.zeros(10, dtype=np.uint64)
    rc = L.abc_particle_ranking_pls(h, X70.ctypes.data, Y70.ctypes.data, X70[0].copy().ctypes.data, 200, 8, 4, 0.5, 9,
                                    _lib.RULE_WILCOXON, 10, idx70.ctypes.data, None, None, None, None, None)
    assert rc == -1 and b"components" in L.abc_last_error(h)
    th = np.asfortranarray(np.random.default_rng(2).normal(size=(20, 70)))
    _stage_argument_checks(gpu_ctx)
    # a later valid call on the same context still works
    assert abcutil.calculate_doubled_variance(th[:, :3], ctx=gpu_ctx).shape == (3,)


def _stage_argument_checks(gpu_ctx):
    """the stage entry points that take a leading dimension refuse one below the row count, a set without columns and (the
    statistics) a set without metrics -- ABC_ERR_INVALID with a message, the caller's buffers untouched; n == 0 is an all-zero
    record (tests/test_gpu_stats.py::test_stats_record_of_no_rows)"""
    import torch
    from abcsmc_amd import _lib
    L = _lib.lib()
    h = gpu_ctx.handle
    n, M, P, A, K = 64, 4, 2, 2, 16
    X = torch.ones(n * M + n, dtype=torch.float64, device="cuda:0")
    Y = torch.ones(n * P + n, dtype=torch.float64, device="cuda:0")
    stats = torch.full((L.abc_stats_len(M, P),), float("nan"), dtype=torch.float64, device="cuda:0")
    model = torch.zeros(L.abc_model_len(M, P, A) + 8, dtype=torch.float64, device="cuda:0")
    dist = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    idx = torch.zeros(K, dtype=torch.int64, device="cuda:0")
    theta = torch.full((K * P + K,), -1.0, dtype=torch.float64, device="cuda:0")
    x, y, s = X.data_ptr(), Y.data_ptr(), stats.data_ptr()
    torch.cuda.synchronize()
    mp, dp, ip, tp = model.data_ptr(), dist.data_ptr(), idx.data_ptr(), theta.data_ptr()
    bad = [
        (lambda: L.abc_stats_shift_dev(h, x, y, n, n - 1, n, M, P, s), b"ldx"),
        (lambda: L.abc_stats_shift_dev(h, x, y, n, n, n - 1, M, P, s), b"ldy"),
        (lambda: L.abc_stats_shift_dev(h, x, y, n, n, n, 0, 0, s), b"no columns"),
        (lambda: L.abc_stats_shift_dev(h, x, y, n, n, n, 0, P, s), b"M == 0"),
        (lambda: L.abc_stats_accumulate_dev(h, x, y, n, n - 1, n, M, P, 0, n // 2, s), b"ldx"),
        (lambda: L.abc_stats_accumulate_dev(h, x, y, n, n, 1, M, P, 0, n // 2, s), b"ldy"),
        (lambda: L.abc_stats_accumulate_dev(h, x, y, n, n, n, 0, 0, 0, n // 2, s), b"no columns"),
        (lambda: L.abc_stats_accumulate_dev(h, x, y, n, n, n, 0, P, 0, n // 2, s), b"M == 0"),   # (was ABC_OK, record unwritten)
        (lambda: L.abc_pls_wilcoxon_dev(h, x, y, n, n - 1, n, M, P, A, n // 2, mp), b"ldx"),
        (lambda: L.abc_pls_wilcoxon_dev(h, x, y, n, n, n - 2, M, P, A, n // 2, mp), b"ldy"),
        (lambda: L.abc_pls_wilcoxon_dev(h, x, y, n, n, n, 0, 0, A, n // 2, mp), b"no columns"),
        (lambda: L.abc_project_distance_dev(h, x, n, n - 1, M, P, A, mp, 0, dp), b"ldx"),
        (lambda: L.abc_project_distance_dev(h, x, n, 0, M, P, A, mp, 1, dp), b"ldx"),
        (lambda: L.abc_project_distance_dev(h, x, n, n, 0, 0, A, mp, 0, dp), b"no columns"),
        (lambda: L.abc_gather_rows_dev(h, y, n, n - 1, P, ip, K, 0, tp, K), b"ldy"),
        (lambda: L.abc_gather_rows_dev(h, y, n, n, P, ip, K, 0, tp, K - 1), b"ldt"),
    ]
    for k, (call, word) in enumerate(bad):
        assert call() == -1, k
        msg = L.abc_last_error(h)
        assert word in msg, (k, msg)
    torch.cuda.synchronize()
    assert torch.isnan(stats).all() and torch.isnan(dist).all() and (theta == -1.0).all()
    # leading dimensions of an empty side are not looked at (P == 0: Y unused; M == 0 with P > 0: a projection of nothing)
    gpu_ctx.check(L.abc_stats_shift_dev(h, x, None, n, n, 0, M, 0, s))
    gpu_ctx.check(L.abc_gather_rows_dev(h, y, n, 0, 0, idx.data_ptr(), K, 0, theta.data_ptr(), 0))
    torch.cuda.synchronize()
