"""The tests' copy of the host decisions of abcsmc_amd/csrc/wilcoxon.hip: which path a reduction takes, how a level of the cascade
is cut into work-groups and batches, how many bins a fine level gets, and which k_wx_sweep<AM, R, MODE, 1024> instantiation a
launch is.  tests/test_wx_dispatch.py holds it against the source (the constants and thresholds are read out of the .hip text,
the instantiations out of the launch macros); tests/test_gpu_wilcoxon.py uses it to say which instantiations its cases reach.

The sweep kernel: AM = 8 / 16 / 32 by the components A (<= 8, <= 16, <= 32); MODE 0 = level 0 (192 logarithmic cells), MODE 1 = a
fine level, MODE 2 = the keys of the exact step; R = rows per thread.  The launch macros can produce 18 instantiations
(AM 8: R 4, 2, 1; AM 16: R 2, 1; AM 32: R 1; each in three modes).  Fifteen are reachable: the exact step always runs
R = rkeys(A) = 4 / 2 / 1, so <8, 2, 2>, <8, 1, 2> and <16, 1, 2> are compiled and never launched.  For MODE 0 and 1, wx_level_one
starts from R = 4 / 2 / 1 and halves it while (tiles of 1024 R rows) x (groups of tests) < 192 -- so R > 1 needs many rows or many
tests: at level 0 a group is 180 tests and the groups are counted from P (A - 1), the tests a set COULD have.

Which case reaches which instantiation (nv = validation rows; "forced" = every test kept open by ABC_WX_NOBOUNDS, in a child process):
    <8, 1, 0> <8, 1, 1>     every cascade case of 16 384 .. 16 391 rows with A = 8 (tests/_wx_worker.py: CASES_CASCADE)
    <16, 1, 0> <16, 1, 1>   ... with A = 16                 <32, 1, 0> <32, 1, 1>   ... with A = 32
    <8, 4, 2> <16, 2, 2> <32, 1, 2>   the same cases whenever a test reaches the exact step; all of them in the forced runs
    <8, 2, 1>               forced, CASES_MANY["a8_r2"]: 65 537 rows, 16 responses x 8 components (112 open tests in 2048 bins: 7 groups x 33 tiles)
    <8, 4, 1>               forced, CASES_MANY["a8_r4"]: 65 537 rows, 32 responses x 8 components (224 open tests: 14 groups x 17 tiles)
    <16, 2, 1>              forced, CASES_MANY["a16_r2"]: 65 537 rows, 8 responses x 16 components (120 open tests)
    <8, 2, 0>               test_large_level0_two_rows_per_thread[8]: 391 169 rows (191 x 2048 + 1), 2 responses x 8 components
    <16, 2, 0>              test_large_level0_two_rows_per_thread[16]: 391 169 rows, 2 responses x 16 components
    <8, 4, 0>               test_gpu_parity.py: test_wilcoxon_reduction_per_response_binned_path, 5e6 validation rows (4 components)
k_wx_ranks_big (the bins k_wx_ranks hands over: a sub-bin above WX_WALK keys, a bin above WX_CAP_S) is reached, by necessity, by
CASES_CASCADE["c8_copies"] in the forced runs (tests/_wx_worker.py says why); a bin above WX_CAP = 16 384 keys -- the repeat on the
sorted path -- by CASES_OUTGROW, forced.
The other existing cases (test_gpu_parity.py): 1.5e5 rows x 16 responses x 8 components, 1.5e5 x 8 x 16 and 1e5 x 6 x 24 run level 0
at R = 1 (<8, 1, 0>, <16, 1, 0>, <32, 1, 0>: one group of tests, 37 .. 74 tiles at R = 4 / 2); test_wilcoxon_paths_agree (6e4 rows x 8
responses x 8 components) <8, 1, 0>, <8, 1, 1> and, forced, <8, 4, 2>; the cases of 3000 and fewer validation rows, more than 32
components and ABC_WX_SORTED take the sorted path, which has no sweep.
"""
import math

WX_T = 1024
WX_NC0 = 192
WX_CSH = 17
WX_LDS = 144 << 10
WX_NBFMAX = 16384
WX_FIRST_MAX = 8
MAXSEG = 65535
WX_CAP, WX_CAP_S, WX_NS, WX_WALK, WX_PK = 16384, 4096, 1024, 48, 16
CASCADE_MIN_ROWS = 16384
GROUPS_FLOOR = 192               # R is halved while tiles x groups stays below this
RUNS_TARGET = 256                # runs of tiles x groups a launch aims at
BC_CAP = 96 << 20
XB_KEYS = 1 << 25
TARGET_DIV, TARGET_MIN = 3500, 2048

MODES = (0, 1, 2)


def cascade_applies(nv_total, P, A, force_sorted=False):
    """abc_wx_cascade_applies"""
    return (not force_sorted) and 2 <= A <= 32 and CASCADE_MIN_ROWS <= nv_total < (1 << 31) and P * (A - 1) <= MAXSEG


def path(nv_total, P, A, force_sorted=False):
    """'none' (nothing to reduce), 'cascade' or 'sorted' -- launch_wilcoxon"""
    if nv_total == 0 or A < 2 or P == 0:
        return "none"
    return "cascade" if cascade_applies(nv_total, P, A, force_sorted) else "sorted"


def rmax(A):
    return 4 if A <= 8 else (2 if A <= 16 else 1)


def rkeys(A):
    """rows per thread of the exact step's key sweep"""
    return 4 if A <= 8 else (2 if A <= 16 else 1)


def am_of(A):
    return 8 if A <= 8 else (16 if A <= 16 else 32)


def sweep_instantiation(A, R, mode):
    """wx_sweep: the (AM, R, MODE) it launches for a level geometry with R rows per thread"""
    if A <= 8:
        return (8, 4 if R == 4 else (2 if R == 2 else 1), mode)
    if A <= 16:
        return (16, 2 if R == 2 else 1, mode)
    return (32, 1, mode)


def instantiable():
    """what the launch macros WX_GO x WX_SW can produce"""
    return {(am, r, mode) for am, rs in ((8, (4, 2, 1)), (16, (2, 1)), (32, (1,))) for r in rs for mode in MODES}


def reachable():
    """... and what a run can launch: MODE 2 only at R = rkeys"""
    out = set()
    for A in (8, 16, 32):
        for mode in (0, 1):
            r = rmax(A)
            while r >= 1:
                out.add(sweep_instantiation(A, r, mode))
                r >>= 1
        out.add(sweep_instantiation(A, rkeys(A), 2))
    return out


def per_test_lds(NBX, mode):
    """level_queue: LDS bytes a test of a sweep work-group takes"""
    return NBX * 4 + (WX_NC0 * 4 if mode == 1 else 0) + 7 * 4 + 16


def level_one(nt, A, want, NBX, per_test, bc_bytes, fixed_slots=0):
    """wx_level_one -> dict(R, tiles, G, TG, RR, tpw, nslots)"""
    G = (WX_LDS - 1024) // per_test
    G = max(G, 1)
    G = min(G, want)
    ns = fixed_slots if fixed_slots > 0 else want
    g = {}
    for _ in range(8):
        TG = (ns + G - 1) // G
        R = rmax(A)
        while R > 1 and ((nt + WX_T * R - 1) // (WX_T * R)) * TG < GROUPS_FLOOR:
            R >>= 1
        tiles = (nt + WX_T * R - 1) // (WX_T * R)
        limit = 65535 // (WX_T * R)
        rr_target = max(RUNS_TARGET // TG, 1)
        tpw = min(max((tiles + rr_target - 1) // rr_target, 1), limit)
        RR = max((tiles + tpw - 1) // tpw, 1)
        g = dict(R=R, tiles=tiles, G=G, TG=TG, RR=RR, tpw=tpw, nslots=ns)
        rr_bytes = rr_target if (fixed_slots < 0 and RR < rr_target) else RR
        nbytes = rr_bytes * ns * NBX * 4
        if fixed_slots > 0:
            while g["RR"] * ns * NBX * 4 > bc_bytes and g["RR"] > 1 and g["tpw"] < limit:
                g["tpw"] += 1
                g["RR"] = (tiles + g["tpw"] - 1) // g["tpw"]
            break
        if nbytes <= bc_bytes or ns <= G:
            break
        fit = (bc_bytes // (rr_bytes * NBX * 4)) // G * G
        fit = max(fit, G)
        if fit >= ns:
            break
        ns = fit
    return g


def level(nt, nvt, sharded, A, want, NBX, per_test, bc_bytes):
    """wx_level"""
    if not sharded:
        return level_one(nt, A, want, NBX, per_test, bc_bytes, 0)
    allr = level_one(max(nvt, nt), A, want, NBX, per_test, bc_bytes, -1)
    return level_one(nt, A, want, NBX, per_test, bc_bytes, allr["nslots"])


def bc_bytes(nv, nseg_max, cap_kb=None):
    """wx_bc_bytes (cap_kb: ABC_WX_BC_CAP_KB)"""
    tiles = (nv + WX_T - 1) // WX_T
    b = max(tiles, 1) * max(nseg_max * 2048 * 4, 8 * WX_NBFMAX * 4)
    cap = (cap_kb << 10) if cap_kb and cap_kb > 0 else BC_CAP
    return min(b, cap) + (1 << 20)


def batches(nt, A, nact_host, NBX, mode, bcb, nvt=None, sharded=False):
    """the launches of level_queue over nact_host tests -> [geometry of each batch]"""
    out, lo = [], 0
    while lo < nact_host:
        g = level(nt, nt if nvt is None else nvt, sharded, A, nact_host - lo, NBX, per_test_lds(NBX, mode), bcb)
        # (level_queue refuses a launch whose counters do not fit the buffer: only a cap below one group of tests gets there)
        assert g["RR"] * g["nslots"] * NBX * 4 <= bcb, "%d runs x %d tests x %d bins do not fit the counter buffer" % (g["RR"], g["nslots"], NBX)
        out.append(g)
        lo += g["nslots"]
    return out


def pick_bins(nact, nvt):
    """wx_pick_bins"""
    open_per_bin = 126.0 * math.sqrt(nvt / 5.0e5)
    best, best_cost = 1024, 1e300
    nb = 16384
    while nb >= 1024:
        if not (nb > 1024 and nb * 4 > nvt):
            G = max((WX_LDS - 1024) // (nb * 4 + WX_NC0 * 4 + 7 * 4 + 16), 1)
            passes = float((nact + G - 1) // G)
            opn = min(open_per_bin / nb, 1.0)
            cost = passes + 1.5 * opn * nact
            if cost < best_cost:
                best_cost, best = cost, nb
        nb >>= 1
    return best


def xb(nvt):
    """tests of one batch of the exact step"""
    v = XB_KEYS // (nvt if nvt else 1)
    return 1 if v < 1 else (8 if v > 8 else v)


def target(nvt):
    """keys a bin of the exact step aims at"""
    return max((nvt + TARGET_DIV - 1) // TARGET_DIV, TARGET_MIN)


def nbcap(nvt):
    return nvt // target(nvt) + 2


def scores_kc(A):
    """the score kernels: k_wx_scores<KC> with KC the power of two >= A (at most 32), 'wide' (k_wx_scores_wide) above 32 components
    on the sorted path"""
    if A > 32:
        return "wide"
    kc = 1
    while kc < A:
        kc *= 2
    return kc


def first_r(P, A, stop_at_max):
    """responses whose tests go first (the largest count first); 0: every test at once"""
    if not (stop_at_max and P <= 1024 and A >= 2):
        return 0
    r = 32 // (A - 1)
    r = 2 if r < 2 else (4 if r > 4 else r)
    return 0 if r >= P else r


def second_fine_level(NBX, NBX_last, left):
    """fine_levels: a second fine level only for at most 32 tests and finer bins (NBX = pick_bins(left, nvt))"""
    return not (NBX <= NBX_last or left > 32)


def sweeps_of_run(nv, P, A, fine_levels, n_exact, cap_kb=None):
    """The instantiations a plain reduction (abc_pls_wilcoxon_dev: every test at level 0 at once) over nv rows launches:
    fine_levels = [(bins, tests entering the level), ...], n_exact = tests of the exact step.  -> (set of (AM, R, MODE), batches per level)"""
    bcb = bc_bytes(nv, P * (A - 1), cap_kb)
    out, nbatch = set(), []
    for mode, NBX, n in [(0, WX_NC0, P * (A - 1))] + [(1, b, n) for b, n in fine_levels]:
        bs = batches(nv, A, n, NBX, mode, bcb)
        nbatch.append(len(bs))
        out |= {sweep_instantiation(A, g["R"], mode) for g in bs}
    if n_exact > 0:
        out.add(sweep_instantiation(A, rkeys(A), 2))
    return out, nbatch
