"""Which projection kernels abc_project_distance_dev runs: a copy of the decisions of abc_project_plan
(abcsmc_amd/csrc/project_plan.h), the one plan behind the three launchers of abcsmc_amd/csrc/project.hip, so that a test can state
the kernel and branch it means to reach and check that it does.  tests/test_project_dispatch.py holds this copy against the plan
function itself, line by line over the cases tests/cxx/project_plan_probe.cpp prints, and against the kernel tables
(PROJECT_DIST2, PROJECT_DIST2_LDS, PROJECT_DIST) the launchers launch through; tests/test_gpu_project.py asserts through
it that its cases reach every kernel, every tail, both matrix-pipe layouts and the second trip of every grid-stride loop.

Kernels (the `main` and `tail` of plan):
    ("simple",)                 k_simple_dist
    ("wide", KCT)               k_project_dist_wide on KCT = 32 ceil(A / 32) padded components (more than 32)
    ("mfma", 2, layout)         k_project_mfma<2> (17..32 components, row pairs, at most 150 KiB of LDS); layout "stage": the LDS
                                in front of the observed scores is the epilogue's score stage (4 x 64 x 33 doubles), "loadings":
                                it is the loadings, means and deviations (M4 x 34 doubles, from M4 = 252 on)
    ("dist2_lds", KC)           k_project_dist2_lds<KC>: row pairs, the loadings in at most 64 KiB of LDS (KC 8, 16)
    ("dist2", KC)               k_project_dist2<KC>: row pairs, scalar operands
    ("dist", KC)                k_project_dist<KC>: one row per lane; the tail (the odd last row) of the pair kernels, and the only
                                kernel where row pairs are not possible

fused_plan mirrors launch_project_distance_scores (distances and the scores of the rows from row_test on in one pass).  Its
row_split > 0 form is not reached by the tests: the callers pass row_test > 0 only when the all-rows score buffer could not be
allocated (an odd N fails the launcher's own evenness condition first), so only row_test = 0 runs.
"""

LDS_PAIR = 64 * 1024            # bytes of dynamic LDS k_project_dist2_lds may ask for
LDS_MFMA = 150 * 1024           # ... and k_project_mfma<2>
MAX_BLOCKS = 256 * 16           # the clamp of the grid-stride kernels
MAX_BLOCKS_LDS = 1024           # ... of k_project_dist2_lds
STAGE = 4 * 64 * 33             # doubles of k_project_mfma<2>'s score stage: four waves x 64 rows x (32 + 1)


def kc_of(A):
    """the padded component count: the next power of two, beyond 32 the next multiple of 32"""
    KC = 1
    while KC < A:
        KC *= 2
    if KC > 32:
        KC = (A + 31) // 32 * 32
    return KC


def mfma_lds(M):
    """(doubles in front of the observed scores, bytes of dynamic LDS, layout) of k_project_mfma<2>"""
    M4 = (M + 3) & ~3
    load = M4 * 32 + 2 * M4
    main = load if load > STAGE else STAGE
    return main, (main + 32) * 8, "loadings" if load > STAGE else "stage"


def _blocks(rows, cap=MAX_BLOCKS):
    return min((rows + 255) // 256, cap)


def vec_ok(n, ldx, x_aligned, dist_aligned):
    """row pairs with 16-byte loads and stores are possible: an even leading dimension, X and dist on 16-byte boundaries, two rows"""
    return ldx % 2 == 0 and x_aligned and dist_aligned and n >= 2


def plan(n, ldx, x_aligned, dist_aligned, M, A, simple):
    """-> dict of what launch_project_distance queues for n rows of leading dimension ldx (x_aligned / dist_aligned: X and dist
    on a 16-byte boundary), M metrics, A components:
        main        the kernel of the rows taken in pairs (or of all rows: simple, wide), None where pairs are not possible
        tail        ("dist", KC) for the rows the main kernel leaves (the odd last one, or all of them), or None
        pad         k_pad_model runs
        lds         bytes of dynamic LDS of the main kernel
        grid        work-groups of the main kernel (of the tail where there is no main kernel)
        tail_grid   work-groups of the tail
        second      a thread of the main kernel (of the tail where there is no main kernel) takes a second trip through its
                    grid-stride loop
    n == 0 queues nothing."""
    return _plan(n, vec_ok(n, ldx, x_aligned, dist_aligned), M, A, simple)


def _plan(n, pairs, M, A, simple):
    out = {"main": None, "tail": None, "pad": False, "lds": 0, "grid": 0, "tail_grid": 0, "second": False}
    if n == 0:
        return out
    blocks = _blocks(n)
    if simple:
        out.update(main=("simple",), grid=blocks, second=n > blocks * 256)
        return out
    KC = kc_of(A)
    if KC > 32:
        out.update(main=("wide", KC), pad=True, grid=blocks, second=n > blocks * 256)
        return out
    npairs = n // 2 if pairs else 0
    ntail = n - 2 * npairs
    pblocks = _blocks(npairs)
    tblocks = _blocks(ntail)
    if ntail:
        out.update(tail=("dist", KC), tail_grid=tblocks)
    if KC == 32 and npairs:
        main, lb, layout = mfma_lds(M)
        if lb <= LDS_MFMA:
            out.update(main=("mfma", 2, layout), pad=ntail > 0, lds=lb, grid=(2 * npairs + 255) // 256)
            return out
    lds_kernel = KC in (8, 16) and (M * KC + KC) * 8 <= LDS_PAIR and npairs > 0
    out["pad"] = (not lds_kernel) or ntail > 0
    if npairs:
        if lds_kernel:
            pblocks = min(pblocks, MAX_BLOCKS_LDS)
            out.update(main=("dist2_lds", KC), lds=(M * KC + KC) * 8)
        else:
            out["main"] = ("dist2", KC)
        out.update(grid=pblocks, second=npairs > pblocks * 256)
    else:
        out.update(grid=tblocks, second=ntail > tblocks * 256)
    return out


NOT_A_SHAPE = "not a shape for it"


def fused_plan(n, ldx, aligned, M, A, row_test, sld):
    """the kernel launch_project_distance_scores runs -- ("dist2_lds", 8 | 16) or ("mfma", 2, layout) -- or NOT_A_SHAPE (it
    returns 1 and queues nothing: the caller scores the rows with a kernel of its own).  aligned: X, dist and S all on 16-byte
    boundaries; sld: the leading dimension of S."""
    KC = kc_of(A)
    vec_ok = (ldx % 2 == 0 and aligned and n >= 2 and n % 2 == 0 and row_test % 2 == 0 and sld % 2 == 0 and row_test < n)
    if not vec_ok or KC not in (8, 16, 32):
        return NOT_A_SHAPE
    if KC == 32:
        main, lb, layout = mfma_lds(M)
        return ("mfma", 2, layout) if lb <= LDS_MFMA else NOT_A_SHAPE
    if (M * KC + KC) * 8 > LDS_PAIR:
        return NOT_A_SHAPE
    return ("dist2_lds", KC)


def scores_plan(n, ldx, aligned, M, A):
    """what launch_project_scores runs for the n validation rows of the Wilcoxon rule -- (kernel, rows it takes), the kernel
    ("dist2_lds", 8 | 16) or ("mfma", 2, layout) -- or NOT_A_SHAPE (it returns 0 rows: the caller scores them all).  aligned: X and
    S both on 16-byte boundaries; S has n rows.  Unlike the fused pass it has a kernel for up to 4 components (the 8-wide one),
    and its matrix-pipe kernel takes the even part of an odd n."""
    KC = max(kc_of(A), 8)
    if not (ldx % 2 == 0 and aligned and n >= 2) or KC > 32:
        return NOT_A_SHAPE
    if KC == 32:
        main, lb, layout = mfma_lds(M)
        return (("mfma", 2, layout), n // 2 * 2) if lb <= LDS_MFMA else NOT_A_SHAPE
    if (M * KC + KC) * 8 > LDS_PAIR or n % 2:
        return NOT_A_SHAPE
    return ("dist2_lds", KC), n


def family(kernel):
    """a kernel without what the launch site does not name: ("wide", KCT) -> ("wide",), ("mfma", 2, layout) -> ("mfma", 2)"""
    if kernel is None:
        return None
    if kernel[0] == "wide":
        return ("wide",)
    if kernel[0] == "mfma":
        return kernel[:2]
    return kernel


def reachable(max_m=1100, max_a=97):
    """-> (main kernels, tails, tail-only kernels) launch_project_distance can reach over M, A up to the given sizes, every
    alignment and n in {1, 2, 3}; the main kernels in full (KCT, layout)"""
    mains, tails, only = set(), set(), set()
    aligns = [(ldx, xa, da) for ldx in (4, 5) for xa in (True, False) for da in (True, False)]
    # (the alignments count only through vec_ok: per n, the values it takes over all of them)
    cases = [(n, pairs) for n in (1, 2, 3) for pairs in sorted({vec_ok(n, *a) for a in aligns})]
    assert cases == [(1, False), (2, False), (2, True), (3, False), (3, True)]
    for simple in (False, True):
        for M in range(1, max_m + 1):
            for A in ([0] if simple else range(1, max_a + 1)):
                for n, pairs in cases:
                    p = _plan(n, pairs, M, A, simple)
                    if p["main"] is not None:
                        mains.add(p["main"])
                        if p["tail"] is not None:
                            tails.add(p["tail"])
                    elif p["tail"] is not None:
                        only.add(p["tail"])
    return mains, tails, only
