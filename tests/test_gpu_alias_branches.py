"""The device build of the resampling table (abcsmc_amd/csrc/alias_dev.hip) at every scan boundary and chain shape: tables whose
size, number of smalls, of bigs or of chain steps sits on the edge of a work-group, both compiled variants (two and four
elements per thread, chosen with ABC_ALIAS_ELEMS) at the same sizes, several hundred work-groups, structured weight vectors.

The reference is the oracle's sequential gsl_ran_discrete_preproc: every alias equal, every cut-off equal as a bit pattern.  The
build verifies itself and hides a mistake as a host fallback, so every cell also asserts WHERE the table was built: the build's
exact model (scripts/alias_scan_proto.py through tests/_alias_cases.py) says for every cell whether the speculation holds; the
cells it sends to the host are listed in _alias_cases.EXPECT_HOST (tests/test_alias_cases_cpu.py keeps that list honest)."""
import numpy as np
import pytest

import _alias_cases as ac

pytestmark = pytest.mark.gpu


def _same_table(F, A, oF, oA):
    return np.array_equal(A, oA) and np.array_equal(F.view(np.uint64), oF.view(np.uint64))


def _build_and_check(gpu_ctx, oracle, w, m, host_listed, what):
    """one table through Context.alias_table: the oracle's bits; built where the model says (unless the cell is listed)"""
    gpu_ctx.alias_stats(reset=True)
    F, A, on_device = gpu_ctx.alias_table(w)
    builds, fallbacks = gpu_ctx.alias_stats(reset=True)
    oF, oA = oracle.discrete_preproc(w)
    assert _same_table(F, A, oF, oA), what
    assert builds == 1 and fallbacks == 1 - on_device, (what, builds, fallbacks, on_device)
    if not host_listed:
        assert m["on_device"] is True and on_device == 1, (what, m["reason"], on_device)
    return F, A, on_device


def _set_elems(monkeypatch, elems):
    if elems is None:
        monkeypatch.delenv("ABC_ALIAS_ELEMS", raising=False)
    else:
        monkeypatch.setenv("ABC_ALIAS_ELEMS", str(elems))


@pytest.mark.parametrize("kind", ac.KINDS)
@pytest.mark.parametrize("elems", [2, 4])
def test_table_at_block_edges(gpu_ctx, oracle, monkeypatch, elems, kind):
    """K = 2, 3, 4 and one below, at and one above 256, 512, 1024, then 2049 and 4097, with either variant: a full work-group, a
    last work-group of one element, 2 K (the chain's launch) on its edge -- the `base + j < n` tails of all ten kernels"""
    _set_elems(monkeypatch, elems)
    for K in ac.EDGE_SIZES:
        if kind in ac.FULL_KINDS and K < 4:
            continue
        w, m = ac.cell(kind, K)
        _build_and_check(gpu_ctx, oracle, w, m, ac.expect_host(kind, K), (elems, kind, K))


@pytest.mark.parametrize("elems", [2, 4])
def test_smalls_bigs_and_steps_on_block_edges(gpu_ctx, oracle, monkeypatch, elems):
    """the number of smalls, of bigs and of chain steps each exactly B - 1, B, B + 1 and 2 B (B: the elements of a work-group)
    while K is not: k_al_psum_apply's early return and the coarse index (Dc, Xc) of a full / partly filled / one-element last
    block, rank_two_level's coarse search running off the end, the identity aggregates of k_al_serve_reduce"""
    _set_elems(monkeypatch, elems)
    for label, w, m in ac.block_edge_cases(elems):
        _build_and_check(gpu_ctx, oracle, w, m, False, (elems, label, w.size, m["ns"], m["nb"], m["nsteps"]))


@pytest.mark.parametrize("elems,K", [(2, 65536), (2, 65537), (2, 131072), (2, 131073), (2, 300000),
                                     (4, 262144), (4, 262145), (4, 300031), (4, 300032), (4, 300033),
                                     (None, 300000), (None, 300001)])
def test_many_work_groups(gpu_ctx, oracle, monkeypatch, elems, K):
    """more than 256 work-groups, where every thread of prefix_of_blocks composes several aggregates (two elements: nblk2 257
    from K = 65537, per = 3 at 300000; four: from 131073), and the natural dispatch edge at 300000 / 300001: the unset switch
    gives the bits of either forced variant (which therefore agree with each other)"""
    for kind in ("uniform", "handover_chain", "one_big"):
        w, m = ac.cell(kind, K)
        _set_elems(monkeypatch, elems)
        F, A, _ = _build_and_check(gpu_ctx, oracle, w, m, False, (elems, kind, K))
        if elems is None:
            for forced in (2, 4):
                _set_elems(monkeypatch, forced)
                F2, A2, _ = _build_and_check(gpu_ctx, oracle, w, m, False, (forced, kind, K))
                assert F2.tobytes() == F.tobytes() and A2.tobytes() == A.tobytes(), (forced, kind, K)


def test_exactly_full_goes_to_the_host(gpu_ctx, oracle):
    """a big left with EXACTLY the mean (GSL's third branch, neither small nor big any more): the device leaves it to the host
    (k_al_serve_apply's `c > mean`), so every such table is a counted fallback, GSL's table, the same bytes as with ALIAS_HOST
    -- and a plain table right behind it is built on the device again"""
    from abcsmc_amd import _lib
    for kind in ac.FULL_KINDS:
        for K in ac.EDGE_SIZES:
            if K < 4:
                continue
            w, m = ac.cell(kind, K)
            assert m["on_device"] is False and m["reason"].startswith("expected no demotion")
            gpu_ctx.alias_stats(reset=True)
            F, A, on_device = gpu_ctx.alias_table(w)
            assert on_device == 0 and gpu_ctx.alias_stats() == (1, 1), (kind, K)
            oF, oA = oracle.discrete_preproc(w)
            assert _same_table(F, A, oF, oA), (kind, K)
            gpu_ctx.set_alias_mode(_lib.ALIAS_HOST)
            try:
                hF, hA, _ = gpu_ctx.alias_table(w)
            finally:
                gpu_ctx.set_alias_mode(_lib.ALIAS_DEVICE)
            assert hF.tobytes() == F.tobytes() and hA.tobytes() == A.tobytes(), (kind, K)
            w2, m2 = ac.cell("ascending", K)
            _build_and_check(gpu_ctx, oracle, w2, m2, False, ("after", kind, K))


@pytest.mark.parametrize("n", [4097, 65])
@pytest.mark.parametrize("kind", ac.RESAMPLE_KINDS)
@pytest.mark.parametrize("K", ac.RESAMPLE_SIZES)
def test_resample_over_structured_tables(gpu_ctx, oracle, K, kind, n):
    """draws through the whole resampling call on either side of ABC_ALIAS_DEV_MIN_K: the host's table at 19999, at 20000 the
    device's with its verdict published by the draw kernel (k_alias_draw) -- parents and rng state the oracle's, no parent of
    weight zero, every parent of a one-hot vector the hot index"""
    from abcsmc_amd import abcutil
    w, m = ac.cell(kind, K)
    seed = 5 + n
    r, o = abcutil.rng(seed), oracle.rng(seed)
    gpu_ctx.alias_stats(reset=True)
    idx = abcutil.gsl_rng_nonuniform_int(r, n, w, ctx=gpu_ctx)
    builds, fallbacks = gpu_ctx.alias_stats(reset=True)
    ref = oracle.resample(o, w, n)
    assert np.array_equal(idx, ref)
    assert (r.s1, r.s2, r.s3) == (o.s1, o.s2, o.s3)
    assert np.all(w[idx.astype(np.int64)] > 0)
    if kind == "one_hot":
        assert np.all(idx == (2 * K) // 3)
    assert builds == (1 if K >= 20000 else 0)
    if K >= 20000 and not ac.expect_host(kind, K):
        assert m["on_device"] is True and fallbacks == 0, (m["reason"], fallbacks)
