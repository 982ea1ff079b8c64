/*
 * abcsmc_hip.h -- C ABI of the MI355X (gfx950) implementation of AbcSmc's per-generation
 * numerical hot path.  Plain pointers and sizes only; no C++/torch types cross this line.
 *
 * The reference has no FFI for its numerics: the boundary this library replaces is the set of
 * C++ free functions in namespace ABC declared in /root/reference/include/AbcSmc/AbcUtil.h:78-172
 * and called from /root/reference/src/AbcSmc.cpp:490-518, 634-640, 1041-1066.  Each entry point
 * below names the declaration it stands in for.  A C++ facade with the reference's own
 * signatures sits on top (abcsmc_amd/cxx/AbcUtilHip.hpp); INTEGRATION.md shows the binding a
 * reference maintainer would add.
 *
 * Conventions
 *   - all matrices are double, COLUMN-MAJOR with leading dimension = number of rows (Eigen's
 *     default layout for the reference's Mat2D): each metric / parameter is one contiguous
 *     particle-major vector.
 *   - functions WITHOUT the _dev suffix take HOST pointers (drop-in for the reference call
 *     sites); functions WITH _dev take DEVICE pointers (HBM-resident data, used by bench.py and
 *     the multi-GPU driver) and run asynchronously on the context's stream.
 *   - every function returns ABC_OK (0) or a negative abc_status; abc_last_error() gives text; there is no positive status
 *     (`if (rc)` is a valid failure test).  A generation whose outputs are complete and valid but in which the perturbation gave
 *     up on some proposals -- they are their (valid) parents or a prior mean; the reference would still be retrying,
 *     AbcUtil.cpp:132 -- returns ABC_OK and says so through abc_generation_giveups / abc_perturb_giveups.
 *     Nothing here calls exit() or throws (the reference exits/aborts).
 *   - one context per GPU and per host thread; calls on one context are serialised.
 *   - Diagnostic environment switches: the library reads NO environment variable unless ABC_DIAG=1 is set; beside it, the
 *     test / A-B switches listed in INTEGRATION.md section 6 act (ABC_WS_POISON: workspace pre-filled with a byte;
 *     ABC_ALIAS_FORCE_FAIL: the device alias build reports failure; kernel-path and fault-injection switches of the tests).
 *     None changes a result except by forcing a documented fall-back path.
 */
#ifndef ABCSMC_HIP_H
#define ABCSMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct abc_ctx abc_ctx;

typedef enum {
    ABC_OK = 0,
    ABC_ERR_INVALID = -1,       /* bad argument (reference: assert / exit)                   */
    ABC_ERR_HIP = -2,           /* HIP runtime failure                                        */
    ABC_ERR_NOT_SPD = -3,       /* covariance not positive definite (reference: GSL abort)    */
    ABC_ERR_UNSUPPORTED = -4,   /* size outside what the kernels are built for                */
    ABC_ERR_NOMEM = -5,
    ABC_ERR_COMM = -6           /* RCCL / caller-supplied collective failed, or librccl is missing */
} abc_status;

/* POD form of the concrete priors in Priors.h:46-110 (likelihood / recast / valid / mean). */
enum { ABC_PRIOR_GAUSS = 0, ABC_PRIOR_UNIF_INT = 1, ABC_PRIOR_UNIF_REAL = 2 };
typedef struct {
    int32_t kind;     /* ABC_PRIOR_*                               */
    int32_t pad_;
    double  a;        /* GAUSS: mean ; UNIF_*: min                 */
    double  b;        /* GAUSS: sd   ; UNIF_*: max                 */
} abc_prior;

/* gsl_rng_taus2 state (examples/include/examples.h:10); abc_rng_set == gsl_rng_set. */
typedef struct { uint32_t s1, s2, s3; } abc_rng;

/* PLS component-selection rule ([PLS] optimal_num_components, AbcUtil.cpp:447-449). */
enum { ABC_RULE_MIN_PRESS = 0, ABC_RULE_WILCOXON = 1 };

/* ---- context ----------------------------------------------------------------------- */
int  abc_ctx_create(int device, abc_ctx** out);
void abc_ctx_destroy(abc_ctx* ctx);
const char* abc_last_error(const abc_ctx* ctx);
/* Run on an existing hipStream_t (e.g. torch's current stream; NULL = HIP's default stream).
 * A new context runs on a private non-blocking stream until this is called;
 * abc_ctx_use_own_stream switches back to it. Both synchronise the stream being left. */
int  abc_ctx_set_stream(abc_ctx* ctx, void* hip_stream);
int  abc_ctx_use_own_stream(abc_ctx* ctx);
int  abc_ctx_synchronize(abc_ctx* ctx);
int  abc_version(void);
/* Which kernel evaluates the O(K K' P) pair sums of weight_predictive_prior (AbcUtil.cpp:556-581).
 * ABC_KDE_AUTO (default): 5 <= P <= 64 parameters run the split-operand kernel (pair dot products on the f16 matrix
 * pipe from three limbs per coordinate, 1.4e-8 rms / 7e-8 max (P <= 16), 2e-8 / 9e-8 (P <= 32), ~3e-8 / 1.3e-7 (P <= 64) absolute
 * error in the base-2 exponent of a term; the terms are evaluated in f32, sixteen at a time, and summed in fp64: 5e-8 rms / 2e-7
 * max relative on such a partial sum; error budget of a weight that one term dominates (all of it at its worst): 5e-7 up to 16 parameters, 5.5e-7 at 17..32, 8e-7 at 33..64; the fixed-seed tests hold 2.5e-7 / 3e-7 / 7e-7 (largest
 * error over ~15 000 weights per parameter count, every count from 5 to 64: 2.2e-7 / 2.4e-7 / 4.1e-7, profiles/history/r03_kde_accuracy.json; in 980 whole generations at random shapes 3.1e-7 / 3.1e-7 / 5.2e-7, profiles/history/r03_generation_fuzz.json),
 * budget 1e-6; rows it cannot represent exactly are summed in fp64, sets it cannot take fall back by themselves); P < 5 and
 * 64 < P run the fp64 kernel (at 64 parameters it is 10 times slower: 63.5 against 6.35 ms per 1e10 pairs; round 6: above 32
 * parameters the previous tiles are staged in LDS -- the same matrix steps on the same operands, the same sums -- and 33..48
 * parameters take three 16-parameter chunks instead of four).
 * ABC_KDE_FP64: always the fp64 vector kernel (<= 1e-12 relative). */
enum { ABC_KDE_AUTO = 0, ABC_KDE_FP64 = 1 };
int  abc_ctx_set_kde_mode(abc_ctx* ctx, int mode);
/* Which kernel takes the sufficient statistics (column sums, Gram blocks) of WIDE sets: 97..160 columns (metrics + parameters), and,
 * from 2 000 000 rows, 81..96 columns whose last one or two 16-column blocks hold parameters only (80 + 16, 64 + 32: configs[3]).
 * The byte-limb kernel (csrc/gram.hip: k_gram_i8, the i8 matrix pipe) rounds every value to a 32-bit fixed-point grid per column.
 * Row counts, column sums and the Gram DIAGONAL stay exact; an off-diagonal entry obeys ONE error model (tests/_gram_model.py, the
 * bound the fixed tests and tests/fuzz/wide_gram_fuzz.py assert per entry):
 *     |G_ab - exact| <= 2^-32 (4 range_a range_b sqrt(rows) + range_a |S_b| + range_b |S_a|),
 * range_c = the column's grid (4 x a robust size of |x - shift| among 4096 sampled rows, rounded up to a power of two: 10 .. 19
 * sigma for Gaussian-like columns), S_c = the partition's sum of x - shift_c: 2e-10 of sqrt(G_aa G_bb) at 2e5 rows for Gaussian-like
 * columns (measured: 0.06 .. 0.1 of the bound), 1.5e-9 beside a column whose mass sits in one value.  That noise is harmless at the
 * Gram's scale but is AMPLIFIED in the loadings of components that fit noise (cross products sqrt(rows) below that scale, close
 * eigenvalues): tests/fuzz/wide_model_fuzz.py holds every USED loading column against the oracle's fit and found 4.3e-6 (fp64
 * kernels: 4e-10) at 66 000 training rows x 29 responses x 30 components, against the 1e-6 of BASELINE.json; with 450 000 rows and
 * more in each partition the worst of 64 fuzzed sets is 2.6e-7 (profiles/r06_wide_model_fuzz*.json).  Hence:
 * ABC_GRAM_AUTO (default): the byte-limb kernel only where EVERY non-empty partition (training rows, validation rows) OF THE WHOLE
 *   SET has at least 400 000 rows -- the sharded generation decides from N_total and the training fraction, so every rank and the
 *   unsharded run of the same set take the same kernel; a rank whose own shard the kernel cannot take (odd row count, columns not
 *   16-byte aligned, fewer than 4096 rows) accumulates ITS rows in fp64 --, the fp64 kernels everywhere else.  Rows outside a
 *   column's grid ("far" rows) are summed in fp64 by a serial side kernel: sets with heavy tails in many rows should use ABC_GRAM_FP64.
 * ABC_GRAM_FP64: the fp64 kernels always (products on the fp64 matrix pipe, ~1e-15 of sqrt(G_aa G_bb)); 1.5x the time of the i8
 *   kernel at 1e6 rows x 144 columns.  With it the sharded generation's statistics equal the unsharded ones to rounding of the order
 *   of summation (distances within 1e-12); under the byte-limb kernel the two differ by the fixed-point noise above (each rank
 *   rounds on its own grid), selection indices still agree up to near-ties.
 * ABC_GRAM_I8: the byte-limb kernel from 200 000 rows in the whole set (round 5's default; A/B runs, the kernel's own tests): Gram
 *   entries within the model above, loadings NOT held to 1e-6. */
enum { ABC_GRAM_AUTO = 0, ABC_GRAM_FP64 = 1, ABC_GRAM_I8 = 2 };
int  abc_ctx_set_gram_mode(abc_ctx* ctx, int mode);
/* Which of the two kernels produced the pair sums of the most recent weight call on this context (synchronises). */
enum { ABC_KDE_RAN_NONE = 0, ABC_KDE_RAN_FP64 = 1, ABC_KDE_RAN_SPLIT = 2 };
int  abc_kde_last_kernel(abc_ctx* ctx, int* which);
/* What the last Wilcoxon reduction on this context (abc_pls_wilcoxon_dev, the Wilcoxon rule of a ranking or a generation) computed
 * for each of its (response, candidate) tests, in plan order: responses ascending, candidates a' = 1 .. a* - 1 of each.  Off by
 * default; abc_ctx_set_wx_record(ctx, 1) switches it on for the calls that follow (a device buffer of the context then takes one
 * record per test; with it off the reduction's kernels get null pointers and nothing else about a launch changes).
 *   nz                    non-zero paired differences; valid once a level or the sorted path has seen the test (n_levels > 0, or a
 *                         path other than ABC_WX_PATH_CASCADE)
 *   level_bins/lo2/hi2    for each level of the cascade of bounds the test went through, in order: its bins and the interval
 *                         [lo2, hi2] of TWICE the signed rank sum that the level's counts leave (n_levels may exceed
 *                         ABC_WX_REC_LEVELS: the levels beyond are not kept)
 *   verdict               0 rejected / 1 passed by the bounds, 2 undecided by them, 3 left open as not needed (largest count first)
 *   passed                the pass / fail the decision used (an undecided test whose sum was never taken: not meaningful)
 *   W, w_taken            the signed rank sum, and whether the exact step or the sorted path actually took it
 * path: how the call ended.  abc_wx_last_record synchronises; ntests = 0 and path = ABC_WX_PATH_NONE while nothing is recorded. */
enum { ABC_WX_REC_LEVELS = 6 };
enum { ABC_WX_PATH_NONE = -1, ABC_WX_PATH_CASCADE = 0, ABC_WX_PATH_CASCADE_THEN_SORTED = 1, ABC_WX_PATH_SORTED = 2 };
typedef struct abc_wx_test_record {
    int32_t response, candidate, optimum, n_levels;
    int32_t verdict, passed, w_taken, pad_;
    uint64_t nz;
    double W;
    int64_t level_bins[ABC_WX_REC_LEVELS], level_lo2[ABC_WX_REC_LEVELS], level_hi2[ABC_WX_REC_LEVELS];
} abc_wx_test_record;
int  abc_ctx_set_wx_record(abc_ctx* ctx, int on);
int  abc_wx_last_record(abc_ctx* ctx, abc_wx_test_record* out, size_t cap, size_t* ntests, int* path);
/* Kernel of the importance weights (weight_predictive_prior, set > 0).  ABC_WEIGHT_GAUSSIAN (default) is the reference's product
 * of Gaussian factors (AbcUtil.cpp:572-576).  ABC_WEIGHT_EPANECHNIKOV is an EXTENSION with no reference counterpart (the
 * reference only mentions the name in a comment, AbcUtil.cpp:476; BASELINE.json's north_star asks for it): the radial
 * Epanechnikov kernel of the same covariance, K = max(0, 1 - r2 / (P' + 4)), r2 = sum_p (theta_ip - theta'_jp)^2 / dv'_p over the
 * P' parameters with dv'_p != 0; a particle without support among the previous ones gets weight 0.  fp64 vector kernel. */
enum { ABC_WEIGHT_GAUSSIAN = 0, ABC_WEIGHT_EPANECHNIKOV = 1 };
int  abc_ctx_set_weight_kernel(abc_ctx* ctx, int kernel);
/* Which stream the Gaussian noise of the proposals comes from (sample_*_predictive_priors, abc_generation_dev).
 * ABC_NOISE_DEVICE (default): counter-based Philox stream keyed by (rng state, draw, attempt), evaluated on the device -- same
 *   distribution as the reference, different numbers; the simulator seeds are the taus2 outputs right after the resampling draws.
 * ABC_NOISE_REFERENCE_STREAM: the shared taus2 stream consumed EXACTLY as the reference does (AbcUtil.cpp:122-158,
 *   Priors.h:19-43: polar Box-Muller on gsl_rng_uniform_pos per coordinate, whole-vector / per-coordinate rejection, then one
 *   gsl_rng_get per row for the seeds, AbcSmc.cpp:535): proposals, seeds and the final rng state equal a CPU run of the
 *   reference bit for bit.  Inherently sequential -- a host loop inside the library, ~50 ns per normal; not available to the
 *   row-sliced entry points (abc_perturb_dev, abc_generation_sharded_dev). */
enum { ABC_NOISE_DEVICE = 0, ABC_NOISE_REFERENCE_STREAM = 1 };
int  abc_ctx_set_noise_mode(abc_ctx* ctx, int mode);
/* Where the Walker alias table of the resampling step (gsl_ran_discrete_preproc, AbcUtil.cpp:111-120) is built.
 * ABC_ALIAS_DEVICE (default): on the GPU, as two verified prefix scans (csrc/alias_dev.hip) -- the same table bit for bit; when
 *   its verification does not hold (or the weights are outside its grid: negative, non-finite, spread over more than 2^44) the
 *   host builds the table instead, and abc_alias_stats counts it.
 * ABC_ALIAS_HOST: always on the host (the sequential algorithm, the GPU idle meanwhile): round 2's path, kept for A/B runs. */
enum { ABC_ALIAS_DEVICE = 0, ABC_ALIAS_HOST = 1 };
int  abc_ctx_set_alias_mode(abc_ctx* ctx, int mode);
/* device builds queued / of those found unusable (rebuilt on the host) since the context was created or the last reset */
int  abc_alias_stats(abc_ctx* ctx, uint64_t* device_builds, uint64_t* host_fallbacks, int reset);
/* The table itself, for inspection: F (K doubles, GSL's KNUTH_CONVENTION applied: (F[k] + k) / K) and A (K uint64) from weights in
 * host memory, built as the context's alias mode says; *on_device = 1 when the device build was used (0: host, incl. fallback). */
int  abc_alias_table(abc_ctx* ctx, const double* w, size_t K, double* F, uint64_t* A, int* on_device);
/* Proposals the perturbation gave up on since the context was created (or since the last reset): multivariate rows whose
 * 16384 whole-vector draws were all rejected (the valid parent is emitted; the reference would retry for ever,
 * AbcUtil.cpp:132) plus independent-noise coordinates that fell back to the prior mean after 1000 tries (the reference prints
 * an error line per fallback, Priors.h:27-29).  Synchronises. */
int  abc_perturb_giveups(abc_ctx* ctx, uint64_t* count, int reset);
/* ... and how many of them the most recent abc_generation_dev / abc_generation_sharded_dev call on this context added (the sharded
 * call: those of THIS rank's slice of the proposals; 0 after a clean generation; the value the host already holds at the call's
 * end: no synchronisation). */
int  abc_generation_giveups(const abc_ctx* ctx, uint64_t* count);
/* What the speculation on the component count cost since the context was created (or the last reset).  A whole generation under
 * ABC_RULE_WILCOXON ranks on the count the fit wrote while the reduction of AbcUtil.cpp:447-449 runs beside it;
 * when the reduction lowers the LARGEST per-response count -- the one the distances use, AbcUtil.cpp:449 -- the projection, the
 * selection and the gather run once more with it (*ranking_repeats), and when the reduction itself gives up on its fast path, or a
 * degenerate selection has to be redone by radix select, the generation starts over (*generation_repeats).  Both 0 on clean
 * responses; neither changes a result.  No synchronisation. */
int  abc_generation_repeats(abc_ctx* ctx, uint64_t* ranking_repeats, uint64_t* generation_repeats, int reset);
/* Which path the selection of the K smallest distances took since the context was created (or the last reset).  *bin_selections:
 * selections queued on the sampled-range bin path, by any caller (abc_select_smallest_dev, a generation, a rank of the sharded
 * driver, the exact single-target path of abc_rank_targets_dev); every other selection is a radix select.  *bin_giveups: of those,
 * the ones whose give-up flag (a bin of more than 1024 keys at or below the K-th key's bin, or fewer than K keys at or below the
 * sampled bound) was read by the selection's own check, which then repeated it with the radix select: abc_select_smallest_dev
 * and the single-target path.  The generation drivers read the flag at a later synchronisation of their own and report their
 * repeat through abc_generation_repeats, not here.  Host-side counters; neither changes a result.  No synchronisation. */
int  abc_select_stats(abc_ctx* ctx, uint64_t* bin_selections, uint64_t* bin_giveups, int reset);
/* The context's scratch arena as the most recent entry point left it.  Every call first reserves an upper bound of the device
 * scratch it will take and then allocates from it block by block; the arena only grows.  *reserved: the arena's size in bytes;
 * *asked: the bound that call reserved, before it is rounded up to 1 MiB; *peak: the highest offset any allocation of that call
 * reached, counted at every allocation, so that space a call hands back and takes again counts once.  peak <= asked <= reserved
 * after every call that returned ABC_OK; the tests hold every entry point to it (tests/test_gpu_arena.py).  Where the Wilcoxon
 * reduction repeats itself on its sorted path it works in a temporary arena of its own: peak then keeps counting against that
 * arena, and may pass asked, which bounds the context's own arena only.  An entry point that takes nothing from the arena (the
 * setters and getters, abc_stats_shift_dev, abc_gather_rows_dev, ...) leaves the three values as the call before it did; all are 0
 * on a new context.  Any pointer may be NULL.  Host-side values, no synchronisation; nothing about a result depends on them. */
int  abc_ws_info(const abc_ctx* ctx, size_t* reserved, size_t* asked, size_t* peak);
/* Optional per-stage timing: HIP events recorded on the context's stream around each stage
 * (and around the k_gram / k_kde kernels alone).  abc_timing_read synchronises, then returns the
 * number of stages; names[i] is a static string, ms[i] the accumulated device time, host_ms[i]
 * accumulated host-side time (alias-table build), count[i] the number of launches; reset != 0 clears.
 * on: 0 = off, 1 = every stage (an event pair per stage: ~10 us of host / dispatch gap each, i.e. ~0.15 ms per generation),
 *     2 = only the brackets around the k_gram and k_kde kernels (what bench.py's roofline needs inside its timed region). */
int  abc_timing_enable(abc_ctx* ctx, int on);
int  abc_timing_read(abc_ctx* ctx, const char** names, double* ms, double* host_ms, long long* count,
                     int max_stages, int reset);
/* What an event pair around a single kernel reports beyond the kernel's own execution time (dispatch and
 * end-of-kernel release latencies), measured with empty kernels on the context's stream.  bench.py reports the
 * k_gram duration both raw and with this subtracted; rocprofv3's kernel duration is the arbiter. */
int  abc_timing_overhead(abc_ctx* ctx, int reps, double* overhead_ms);

/* ---- RNG (gsl_rng_set / gsl_rng_get on taus2) ------------------------------------------- */
void     abc_rng_set(abc_rng* r, unsigned long seed);
uint32_t abc_rng_get(abc_rng* r);
/* advance the state by n outputs in O(log n) (taus2 is GF(2)-linear) */
void     abc_rng_jump(abc_rng* r, uint64_t n);

/* ======================================================================================== */
/* HOST-pointer entry points (drop-in for the AbcUtil.h free functions)                     */
/* ======================================================================================== */

/* ABC::particle_ranking_PLS (AbcUtil.h:149-153, AbcUtil.cpp:423-458).
 * X: N x M metrics, Y: N x P parameters, obs: M observed metrics.  Returns the first K entries
 * of the ascending-distance ordering (the caller keeps only those: AbcSmc.cpp:645-646); K = N
 * gives the whole vector the reference returns.  max_comp <= 0 -> min(M,P).
 * Optional outputs (NULL to skip): dist[K], ncomp, R[M*A], mean[M], sd[M]. */
int abc_particle_ranking_pls(abc_ctx* ctx, const double* X, const double* Y, const double* obs,
                             size_t N, size_t M, size_t P, double train_frac, int max_comp,
                             int rule, size_t K, uint64_t* idx, double* dist, int32_t* ncomp,
                             double* R, double* mean, double* sd);

/* ABC::particle_ranking_simple (AbcUtil.h:144-147, AbcUtil.cpp:408-421) */
int abc_particle_ranking_simple(abc_ctx* ctx, const double* X, const double* obs, size_t N,
                                size_t M, size_t K, uint64_t* idx, double* dist);

/* ABC::calculate_doubled_variance (AbcUtil.h:168-170, AbcUtil.cpp:528-537); theta K x P */
int abc_calculate_doubled_variance(abc_ctx* ctx, const double* theta, size_t K, size_t P, double* dv);

/* ABC::weight_predictive_prior, set 0 (AbcUtil.h:155-158, AbcUtil.cpp:539-545) */
int abc_weight_predictive_prior_uniform(abc_ctx* ctx, size_t K, double* w);

/* ABC::weight_predictive_prior, set > 0 (AbcUtil.h:160-166, AbcUtil.cpp:547-586): Gaussian-kernel
 * importance weights, L2-normalised.  theta K x P, theta_prev Kp x P, w_prev[Kp], dv_prev[P]. */
int abc_weight_predictive_prior(abc_ctx* ctx, const abc_prior* priors, const double* theta, size_t K,
                                size_t P, const double* theta_prev, size_t Kp, const double* w_prev,
                                const double* dv_prev, double* w);

/* ABC::setup_mvn_sampler (AbcUtil.h:128-130, AbcUtil.cpp:462-488): L is P x P column-major, lower
 * triangle + diagonal = Cholesky factor of the doubled-diagonal covariance, strict upper triangle =
 * covariance entries (as gsl_linalg_cholesky_decomp1 leaves them). */
int abc_setup_mvn_sampler(abc_ctx* ctx, const double* theta, size_t K, size_t P, double* L);

/* ABC::gsl_rng_nonuniform_int / sample_posterior (AbcUtil.h:78, 110-114; AbcUtil.cpp:111-120,
 * 366-375): n weighted draws of parent rows; consumes exactly n outputs of rng (bit-exact with
 * gsl_ran_discrete on taus2) and advances it. */
int abc_sample_posterior(abc_ctx* ctx, abc_rng* rng, const double* w, size_t K, size_t n, uint64_t* idx);

/* ABC::sample_mvn_predictive_priors (AbcUtil.h:132-137, AbcUtil.cpp:391-404, 122-143) and
 * ABC::sample_predictive_priors (AbcUtil.h:121-126, AbcUtil.cpp:377-389, 145-158).
 * out: n x P proposals; parent (optional): n parent rows; seeds (optional): n simulator seeds
 * (AbcSmc.cpp:535).  Parent indices are bit-exact with the reference stream; the Gaussian noise
 * comes from a counter-based generator keyed by (rng state, particle), i.e. it is distributed as
 * the reference's but is not the same stream (DESIGN.md "Declared deviations"). */
int abc_sample_mvn_predictive_priors(abc_ctx* ctx, abc_rng* rng, size_t n, const double* w,
                                     const double* theta, size_t K, size_t P, const abc_prior* priors,
                                     const double* L, double* out, uint64_t* parent, uint64_t* seeds);
int abc_sample_predictive_priors(abc_ctx* ctx, abc_rng* rng, size_t n, const double* w,
                                 const double* theta, size_t K, size_t P, const abc_prior* priors,
                                 const double* dv, double* out, uint64_t* parent, uint64_t* seeds);

/* ======================================================================================== */
/* DEVICE-pointer entry points                                                               */
/* ======================================================================================== */

/* One SMC generation turn-over with everything resident in HBM
 * (AbcSmc.cpp:634-664 rank+truncate, :1041-1066 dv+weights, :490-518 proposals, :535 seeds). */
typedef struct {
    size_t N, M, P;            /* this set: particles, metrics, parameters                   */
    size_t K, Kp, Nnext;       /* pred-prior size, previous pred-prior size (0 = set 0), next */
    double train_frac;
    int32_t max_comp, rule, multivariate, reserved;
} abc_generation_cfg;

typedef struct {               /* all DEVICE pointers; optional ones may be NULL              */
    const double* X;           /* N x M                                                       */
    const double* Y;           /* N x P                                                       */
    const double* obs;         /* M                                                           */
    const abc_prior* priors;   /* P                                                           */
    const double* theta_prev;  /* Kp x P  (NULL for set 0)                                    */
    const double* w_prev;      /* Kp                                                          */
    const double* dv_prev;     /* P                                                           */
    uint64_t* idx;             /* K   selected particle rows, ascending distance              */
    double*   dist;            /* K   their distances (optional)                              */
    double*   theta;           /* K x P gathered posterior (optional)                         */
    double*   w;               /* K   weights                                                 */
    double*   dv;              /* P   doubled variance                                        */
    double*   L;               /* P x P Cholesky factor (multivariate; optional)              */
    double*   next;            /* Nnext x P proposals                                         */
    uint64_t* parent;          /* Nnext parent rows (optional)                                */
    uint64_t* seeds;           /* Nnext simulator seeds (optional)                            */
} abc_generation_io;

int abc_generation_dev(abc_ctx* ctx, const abc_generation_cfg* cfg, const abc_generation_io* io,
                       abc_rng* rng, int32_t* ncomp_host);

/* ---- stage-level device entry points (used by the sharded multi-GPU driver) -- */

/* Doubles needed for one sufficient-statistics record for (M,P):
 *   [ n_train, n_test, shift[C16], sum_train[C16], sum_test[C16], G_train[C16*C16], G_test[C16*C16] ]
 * with C16 = 16*ceil((M+P)/16).  Records from different row shards that used the same shift are
 * combined by plain addition of everything after shift[]; records about different shifts are re-centred first
 * (abc_generation_sharded_dev all-gathers the ranks' records, each about its own pilot shift, and merges them). */
size_t abc_stats_len(size_t M, size_t P);
/* Column-major arguments of the stage entry points below (statistics, Wilcoxon reduction, projection, gather): every call with
 * M + P == 0, with a leading dimension below the row count (ldx < n with M > 0, ldy < n with P > 0, ldt < K with P > 0)
 * returns ABC_ERR_INVALID with a message (the gather has no M: P == 0 is a no-op there); rows [n, ld) of a column take no part
 * in any result.  The statistics calls refuse M == 0 (ABC_ERR_INVALID): the record is built around the metrics' X'X block.
 * n == 0 gives an all-zero record.
 * Record entries: padding columns (M+P .. C16) are 0 in the shift, the sums and both Grams; the off-diagonal Y'Y entries
 * are either the products or 0 (the fp64 kernels skip whole 16-column blocks that hold parameters only). */
/* pilot shift (mean of the first min(n,256) local rows) -> stats record's shift[] */
int abc_stats_shift_dev(abc_ctx* ctx, const double* X, const double* Y, size_t n, size_t ldx,
                        size_t ldy, size_t M, size_t P, double* stats);
/* one pass over the local rows: column sums + Gram of the shifted [X|Y], train rows =
 * global rows < n_train_global.  row0 = global index of local row 0. */
int abc_stats_accumulate_dev(abc_ctx* ctx, const double* X, const double* Y, size_t n, size_t ldx,
                             size_t ldy, size_t M, size_t P, uint64_t row0, uint64_t n_train_global,
                             double* stats);
/* model record length in doubles, and the fit: z-score moments, kernel-PLS deflation (type 2),
 * PRESS on the test statistics, component choice, observed scores. */
size_t abc_model_len(size_t M, size_t P, size_t A);
int abc_pls_model_dev(abc_ctx* ctx, const double* stats, const double* obs, size_t M, size_t P,
                      size_t A, int rule, double* model);
/* optional second step of the fit for rule ABC_RULE_WILCOXON: reduces the per-response PRESS optima using the
 * validation rows [row_test, n) of THIS device (single-GPU sets only) and rewrites ncomp in the model record */
int abc_pls_wilcoxon_dev(abc_ctx* ctx, const double* X, const double* Y, size_t n, size_t ldx, size_t ldy,
                         size_t M, size_t P, size_t A, size_t row_test, double* model);
int abc_model_ncomp(abc_ctx* ctx, const double* model, size_t M, size_t P, size_t A, int32_t* ncomp);
/* "simple" model: only means / sds / z-scored obs (AbcUtil.cpp:412-416) */
int abc_simple_model_dev(abc_ctx* ctx, const double* stats, const double* obs, size_t M, size_t P,
                         double* model);
/* per-row distance to the observed scores (AbcUtil.cpp:453-455, or :419 when simple != 0) */
int abc_project_distance_dev(abc_ctx* ctx, const double* X, size_t n, size_t ldx, size_t M, size_t P,
                             size_t A, const double* model, int simple, double* dist);
/* K smallest of dist[n] in ascending (dist, index) order: idx[K] (local row + idx_base), dist[K] (dist_out may be NULL).
 * Limit: idx_base + n <= 2^48 (ABC_ERR_UNSUPPORTED beyond: the sort of up to 2^18 winners keeps 48 bits of an index). */
int abc_select_smallest_dev(abc_ctx* ctx, const double* dist, size_t n, size_t K, uint64_t idx_base,
                            uint64_t* idx, double* dist_out);
/* Distributed exact selection: every shard histograms its keys for pass p = 0..5 (digits of the
 * IEEE bit pattern, high to low), the caller all-reduces hist (2048 x int32) over the shards, then every shard
 * picks the same digit; after pass 5 `state` holds the global K-th smallest key.  count -> {#below, #equal} per
 * shard (the caller decides how many ties each shard takes, lowest global rows first); compact -> that shard's
 * winners (dist, row + idx_base) in row order.  state: 8 x int64, hist: 2048 x int32 (zeroed by begin / pick).
 * Limit of compact: idx_base + n <= 2^48 (ABC_ERR_UNSUPPORTED beyond), as what sorts its output keeps 48 bits of an index. */
int abc_select_begin_dev(abc_ctx* ctx, uint64_t K, int64_t* state, int32_t* hist);
int abc_select_hist_dev(abc_ctx* ctx, const double* dist, size_t n, const int64_t* state, int pass, int32_t* hist);
int abc_select_pick_dev(abc_ctx* ctx, int64_t* state, int pass, int32_t* hist, uint64_t K);
int abc_select_count_dev(abc_ctx* ctx, const double* dist, size_t n, const int64_t* state, int64_t* counts);
int abc_select_compact_dev(abc_ctx* ctx, const double* dist, size_t n, const int64_t* state, uint64_t n_less,
                           uint64_t ties_take, uint64_t idx_base, uint64_t* idx_out, double* dist_out);
/* stable sort of n (key, idx) pairs by key alone: equal keys keep their input order, whatever their idx; used to merge per-shard
 * winners.  Limit: every idx below 2^48 -- up to 2^18 pairs the sort keeps 48 bits of idx and returns the rest as zeros, without
 * an error (the values are on the device, the host cannot see them). */
int abc_sort_pairs_dev(abc_ctx* ctx, double* key, uint64_t* idx, size_t n);
/* merge n_runs runs of run_len pairs, each sorted by (key, idx), laid out back to back, into one sorted
 * sequence (ties: lower run first = a stable sort of the concatenation).  Out-of-place. */
int abc_merge_sorted_runs_dev(abc_ctx* ctx, const double* key, const uint64_t* idx, int n_runs, size_t run_len,
                              double* key_out, uint64_t* idx_out);
/* theta[i, :] = Y[idx[i] - idx_base, :] for idx in [idx_base, idx_base + n_local), else untouched */
int abc_gather_rows_dev(abc_ctx* ctx, const double* Y, size_t n_local, size_t ldy, size_t P,
                        const uint64_t* idx, size_t K, uint64_t idx_base, double* theta, size_t ldt);
int abc_doubled_variance_dev(abc_ctx* ctx, const double* theta, size_t K, size_t P, double* dv);
/* un-normalised importance weights for rows [k0, k0+kn) of theta (sharded KDE); w_raw[kn] */
int abc_weights_raw_dev(abc_ctx* ctx, const abc_prior* priors, const double* theta, size_t K, size_t P,
                        size_t k0, size_t kn, const double* theta_prev, size_t Kp, const double* w_prev,
                        const double* dv_prev, double* w_raw);
/* w /= ||w||_2 (AbcUtil.cpp:583) */
int abc_normalize_l2_dev(abc_ctx* ctx, double* w, size_t K);
int abc_setup_mvn_sampler_dev(abc_ctx* ctx, const double* theta, size_t K, size_t P, double* L);
/* draws [i0, i0+n) of the reference's resampling stream: parent[i] for those draws; rng is the
 * state at draw 0 and is NOT advanced. w is a device pointer (the alias table is built on the
 * host exactly as gsl_ran_discrete_preproc, then cached in the context). */
int abc_resample_dev(abc_ctx* ctx, const abc_rng* rng, const double* w, size_t K, uint64_t i0,
                     size_t n, uint64_t* parent);
/* proposals for draws [i0, i0+n): out is n x P (ld = n) */
int abc_perturb_dev(abc_ctx* ctx, const abc_rng* rng, const double* theta, size_t K, size_t P,
                    const abc_prior* priors, const uint64_t* parent, uint64_t i0, size_t n,
                    int multivariate, const double* L_or_dv, double* out, uint64_t* seeds,
                    uint64_t seed_stream_offset);

/* ---- batched ranking: one fitted set, many observed targets -------------------------------------------------------------
 * Ranks the same N rows against B observed metric vectors with ONE statistics pass, ONE fit and ONE projection (cross-validation
 * of the ABC setup as cv4abc does it; one reference table against many data sets).  Target b's result equals, bit for bit
 * (indices and dist bits), the first K entries of abc_particle_ranking_pls(X, Y, targets[b], ...) with the same train_frac,
 * max_comp and rule: ascending (dist, row), ties by row, dist = sqrt(sum_{k < ncomp} (s_k - o_k)^2) as one fma chain in component
 * order, ncomp from the model header.
 * exclude (optional, B entries; UINT64_MAX = none): row exclude[b] is never ranked for target b, so its result equals the
 * single call's first K + 1 rows with that row removed.  DEVIATION from a leave-one-out refit: the fit is shared by all targets
 * and the excluded row still takes part in it (statistics, loadings, component choice); it only drops out of the ranking.
 * Non-finite target entries are refused (ABC_ERR_INVALID).  Both calls synchronise the context's stream. */
/* Device pointers, column-major.  model: a finished record of abc_pls_model_dev (+ abc_pls_wilcoxon_dev) for (M, P, A); its own
 * observed scores are ignored.  targets: B x M, leading dimension ldt >= B.  idx, dist: K x B (target b's K rows contiguous at
 * b K).  post_mean (optional): B x P row-major, post_mean[b P + j] = fp64 mean of Y[idx[b K + e], j] over e < K; Y (leading
 * dimension ldy) is read only for it.  exclude, dist, post_mean and Y may be NULL.  ABC_ERR_INVALID (with a message) for B == 0,
 * K == 0, K > N, K > N - 1 when a target excludes a row, an excluded row >= N other than UINT64_MAX, ldx < N, ldt < B, ldy < N
 * (with post_mean), M == 0, A == 0, and NULL X / model / targets / idx (Y with post_mean); ABC_ERR_NOMEM when the workspace cannot
 * be had; ABC_ERR_UNSUPPORTED for N >= 2^32. */
int abc_rank_targets_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M, size_t P,
                         const double* model, size_t A, const double* targets, size_t ldt, size_t B, const uint64_t* exclude,
                         size_t K, uint64_t* idx, double* dist, double* post_mean);
/* HOST-pointer drop-in: X N x M, Y N x P, targets B x M (ld = B), exclude B (optional); one upload, the fit of
 * abc_particle_ranking_pls, the batched ranking, one download.  idx / dist K x B, post_mean B x P (optional), ncomp (optional). */
int abc_particle_ranking_pls_targets(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                     const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                     const uint64_t* exclude, size_t K, uint64_t* idx, double* dist, double* post_mean,
                                     int32_t* ncomp);
/* Targets of the two calls above whose batched selection gave up (its sampled threshold let through fewer than K rows or more
 * than the candidate segment holds, or a bin of the exact step outgrew LDS) and that the exact single-target path recomputed,
 * since the context was created or the last reset.  Never changes a result. */
int abc_targets_fallbacks(abc_ctx* ctx, uint64_t* count, int reset);

/* ---- local-linear regression adjustment of the batched ranking (Beaumont, Zhang & Balding 2002) ------------------------------
 * The ranking of the two calls above (idx and dist bit for bit the same for the same arguments; dist may be NULL here), then for
 * every target b a weighted regression of its K retained rows' parameters on their PLS scores.  Definition, per target:
 *   rows e = 0..K-1 in ranking order (exclusion applied), distances d_e ascending, row numbers i_e; nc = the model's component
 *   count; o = the target's observed scores (abc_rank_targets_dev's formula); S[i, k] = score k of row i (the ranking's own).
 *   bandwidth   h = d_{K-1}
 *   weights     kernel 0 (Epanechnikov): w_e = 1 - (d_e / h)^2, computed as t = d_e / h, 1 - t * t (a row at distance h weighs 0);
 *               kernel 1 (rectangular): w_e = 1.  Kernel 0 takes the rectangular weights when h == 0 or every weight is 0 (K = 1,
 *               for example), and sets status bit 1.
 *   covariates  x_e[k] = S[i_e, k] - o_k, k < nc;  response theta_e = Y[i_e, :]
 *   fit         weighted means xbar, thetabar; centred moments C = sum w (x - xbar)(x - xbar)' (nc x nc) and
 *               c = sum w (x - xbar)(theta - thetabar)' (nc x P), from one pass shifted by the first retained row; beta = C^-1 c by
 *               the regression sweep operator (Goodnight 1979) in component order.  Pivot k is skipped (beta_k = 0) when C_kk after
 *               the earlier sweeps is <= 1e-10 x the original C_kk, or the original C_kk is <= 0; rank = the pivots kept.
 *               alpha = thetabar - beta' xbar: the fitted value at the observation, the adjusted posterior mean.
 *   adjusted    theta*_e[j] = theta_e[j] - sum_k beta_kj x_e[k], one fma chain in k order.
 * Every reduction's order depends on (K, nc, P) only: target b's outputs are the same bits alone (B = 1), inside any batch and
 * through either entry point (with the same model).  Limits: A <= 64, P <= 1024 (ABC_ERR_UNSUPPORTED beyond).  Argument checks
 * are those of the ranking plus ABC_ERR_INVALID for kernel not 0 / 1, NULL Y, ldy < N and NULL out. */
typedef struct {            /* every pointer optional (NULL: not written); device or host memory per the entry point          */
    double*  theta;         /* (B*K) x P row-major: row b*K + e = theta*_e of target b                                        */
    double*  weight;        /* B*K: w_e                                                                                       */
    double*  coef;          /* B x (A+1) x P row-major: [b][0][j] = alpha_j, [b][1+k][j] = beta_kj (0 for k >= nc or skipped) */
    int32_t* rank;          /* B: pivots kept                                                                                 */
    int32_t* status;        /* B: bit 0 = some pivot skipped, bit 1 = rectangular fallback, bit 2 = every weight 0 (row weights) */
} abc_adjust_out;
enum { ABC_KERNEL_EPANECHNIKOV = 0, ABC_KERNEL_RECTANGULAR = 1 };
/* Device pointers (as abc_rank_targets_dev; Y required), out's members in device memory. */
int abc_rank_targets_adjust_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                                size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                const uint64_t* exclude, size_t K, int kernel, uint64_t* idx, double* dist,
                                const abc_adjust_out* out);
/* HOST-pointer drop-in (as abc_particle_ranking_pls_targets), out's members in host memory; A = max_comp if it is positive,
 * otherwise min(M, P). */
int abc_particle_ranking_pls_targets_adjust(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                            const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                            const uint64_t* exclude, size_t K, int kernel, uint64_t* idx, double* dist,
                                            const abc_adjust_out* out, int32_t* ncomp);

/* ---- log and logit parameter transforms of the local-linear adjustment (R abc: transf = c("log", "logit"), logit.bounds) ------
 * The adjustment above regresses the parameters on their raw scale, so theta* = theta - beta' x can leave a parameter's support (a
 * rate below 0, a probability past 1).  With transforms set, the regression runs on a transformed scale and the adjusted rows are
 * carried back, so they stay inside the support.  Each parameter j has a kind; LOGIT also has finite bounds lo_j < hi_j.
 *   forward  NONE   t = y, copied bit for bit (signed zeros and NaNs pass through)
 *            LOG    t = log(y) for finite y > 0, otherwise NaN (y == 0 gives NaN, not -inf)
 *            LOGIT  t = log((y - lo) / (hi - y)) for lo < y < hi, otherwise NaN
 *   back     a NaN t gives NaN (tested first);  NONE y = t;  LOG y = exp(t);
 *            LOGIT  s = 1.0 / (1.0 + exp(-t)), y = fma(hi - lo, s, lo), then clamped to [lo, hi]; t = -inf gives lo, t = +inf gives hi
 * Every kernel takes these operations from one device header (csrc/transf_dev.h), so a value has the same bits wherever it is made.
 * With a setting active, the local-linear fit of a target is the definition above with theta_e = forward(Y[i_e, :]):
 *   coef (alpha, beta), rank and status are on the transformed scale; the weights are unchanged;
 *   the adjusted row is back(theta*_e): the bits abc_adjust_out.theta holds and the values v_e every product sees under method 1
 *   (summary, density, joint, draws, path summary).  Quantiles, densities, covariances, bandwidths and the smoothing of smoothed
 *   draws work on the parameter's own scale, after the back-transform: a density grid or a smoothed draw may still pass a bound, as
 *   in R.  An out-of-domain Y entry in a retained row makes that (target, parameter) NaN and nothing else, as a NaN parameter does.
 * Unchanged bit for bit whether or not a setting is active: idx, dist, the PLS fit of the host entries (fitted on the raw Y),
 * everything under method 0 (rejection), the path's post_mean and h, the generic abc_weighted_* entries, the generation path.
 * The setting lives in the context (as abc_ctx_set_weight_kernel's): it is copied at set time; NULL, P = 0 or every kind NONE turn
 * it off (the default).  ABC_ERR_INVALID at set time for P > 1024, a kind outside 0..2, NULL kind, and a LOGIT entry whose bounds
 * are NULL, non-finite or not lo < hi.  A call that regresses (abc_rank_targets_adjust_dev, the path calls that fit, every product
 * under method 1, and their host forms) under a setting with another P is refused with ABC_ERR_INVALID before anything is queued;
 * calls that do not regress ignore the setting.  The forward pass costs N x P x 8 bytes of workspace and one streaming kernel. */
enum { ABC_TRANSF_NONE = 0, ABC_TRANSF_LOG = 1, ABC_TRANSF_LOGIT = 2 };
typedef struct { size_t P; const int32_t* kind; const double* lo; const double* hi; } abc_param_transf_t;  /* host memory; lo / hi read
                                                                    for LOGIT entries only, may be NULL when there is none */
int abc_ctx_set_param_transf(abc_ctx* ctx, const abc_param_transf_t* tf);
/* The context's transforms over a column-major n x P matrix (V[i + ldv j] -> out[i + ldo j]); inverse != 0: the back direction; in
 * place is allowed; with nothing set it copies.  ABC_ERR_INVALID for NULL V / out, ldv < n, ldo < n, and P other than the setting's. */
int abc_param_transf_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t n, size_t P, int inverse, double* out, size_t ldo);
int abc_param_transf(abc_ctx* ctx, const double* V, size_t n, size_t P, int inverse, double* out);   /* host pointers, ld = n */
/* Entries of LOG / LOGIT columns that forward passes (those of the calls that regress and of abc_param_transf*) found outside
 * their domain, non-finite ones included, since the context was created or the last reset.  Never changes a result. */
int abc_param_transf_outside(abc_ctx* ctx, uint64_t* count, int reset);

/* ---- heteroscedastic variance correction of the local-linear adjustment (R abc: hcorr = TRUE) ----------------------------------
 * The adjustment above shifts the retained rows along the regression; their spread stays the pooled spread of the whole tolerance
 * window.  With this setting on, a second weighted regression models the log residual variance over the same covariates, and the
 * residual of every adjusted row is rescaled to the variance the model gives at the observation.  Per slot (a target b, or (b, t) on
 * a tolerance path with K = K_t rows) and per parameter j; x_e, w_e, alpha, beta, C, the kept pivots and the shift by the first
 * retained row are the first fit's, on the transformed scale when parameter transforms are set:
 *   1. v_e[j] = theta_e[j] - sum_k beta_kj x_e[k], the plain adjusted value (the bits the adjustment gives without the setting);
 *      r_e[j] = v_e[j] - alpha_j, one fp64 subtraction with the stored alpha_j.
 *   2. z_e[j] = 2 log|r_e[j]|  (R's log(residuals^2), without the underflow of the square).
 *   3. The first fit's weighted regression with z in place of theta: the same weights and covariates, the one-pass moment scheme
 *      shifted by the first retained row's x and z; C and its pivot decisions are the first fit's (same bits);
 *      c2 = sum w (x - xbar)(z - zbar)', g = C^-1 c2 by the same sweep, g_k = 0 for a skipped pivot;
 *      a_j = zbar_j - g_j' xbar: the log residual variance at the observation.  rank and status do not change.
 *   4. q = sum_k g_kj x_e[k] (an fma chain from 0.0 in k order), f = exp(-0.5 q) = sigma(observation) / sigma(x_e),
 *      theta**_e[j] = fma(r_e[j], f, alpha_j); under transforms the back-transform follows, unchanged.
 *   5. Parameter j of a slot is SKIPPED when K <= nc + 2 (the first fit interpolates, the residuals are rounding noise) or when any
 *      retained row, zero-weight rows included, has r_e[j] == 0 or non-finite (a constant parameter column, duplicated rows with
 *      h == 0, a NaN parameter; R's lsfit errors out on these).  Then the row is v_e[j], bit for bit the plain adjustment's,
 *      hcoef[slot][0][j] = NaN and hcoef[slot][1 + k][j] = 0.
 *   6. hcoef is laid out as coef: slots x (A + 1) x P, row 0 = a, row 1 + k = g_k (0 for k >= nc).
 * The correction applies wherever adjusted rows are made: abc_adjust_out.theta, and the values every product sees under method 1
 * (summary, density, joint, draws, path summary), in the device and the host entries alike, from one device function.
 * Unchanged under the setting: idx, dist, weight, coef (so alpha, the local-linear point estimate), rank, status, the path's
 * post_mean and h, everything under method 0, the generic abc_weighted_* entries, the generation path.  With the setting off (the
 * default) every output of every call keeps its bits.  The device exp and log are not bit-exact against a host library; batch
 * invariance is: a slot's outputs are the same bits alone, in any batch and through either entry point, and every reduction's
 * order depends on (K, nc, P) only.  On a tolerance path that holds of hcoef too: slot (b, t) is made as
 * abc_rank_targets_adjust_dev with K = K_t makes it (that call's order of sums, its first fit computed over again), so it has
 * that call's bits whatever K_max and the other tolerances are.  The path's own coef keeps its definition above (its sums'
 * order depends on K_max as well) and may differ from that first fit in its last bits; the values of the path summary take
 * alpha and beta from the path's coef and g from hcoef.
 * The setting lives in the context (as abc_ctx_set_param_transf's); calls that do not regress ignore it.  ABC_ERR_INVALID for on
 * outside 0 / 1.  Workspace: one more (1 + nc) x P moment block per row chunk. */
int abc_ctx_set_adjust_hcorr(abc_ctx* ctx, int on);
/* hcoef of the last regressing call made under the setting, copied to host memory: at most cap doubles (hcoef may be NULL when
 * cap = 0); *slots, *a1 = A + 1 and *P are always written, 0 / 0 / 0 while there is nothing.  Synchronises.  The record lives in a
 * device buffer of the context, allocated or grown only while the setting is on and freed with the context. */
int abc_adjust_last_hcorr(abc_ctx* ctx, double* hcoef, size_t cap, size_t* slots, size_t* a1, size_t* P);
/* (slot, parameter) pairs skipped by rule 5 since the context was created or the last reset. */
int abc_adjust_hcorr_skipped(abc_ctx* ctx, uint64_t* count, int reset);

/* ---- ridge adjustment with the penalty chosen by leave-one-out PRESS (R abc: method = "ridge") ---------------------------------
 * The local-linear fit breaks down where few rows are retained relative to the number of covariates, or where the covariates are
 * nearly collinear inside the tolerance window (PLS scores are orthogonal over the training rows, not over one target's K nearest
 * rows).  With this setting on, every call that regresses fits each slot once per penalty of an ascending list and keeps, per
 * parameter, the fit whose exact leave-one-out prediction error (PRESS) is smallest.  Per slot (a target b, or (b, t) on a
 * tolerance path with K = K_t) and per parameter j; w_e, x_e, the shift by the first retained row, W, xm, xbar, thetabar, C and c
 * are the plain fit's, on the transformed scale when parameter transforms are set:
 *   1. For every l, C^(l) = C except for the diagonal, C^(l)_kk = fma(lambda_l, C_kk, C_kk): lm.ridge's penalty, which scales
 *      every covariate to unit variance, written on the unscaled moments.
 *   2. beta_l = C^(l)^-1 c by the plain fit's sweep in component order; the skip rule is the plain fit's, applied to C^(l).
 *   3. alpha_l = thetabar - beta_l' xbar by the plain fit's chain.  For lambda_l == 0 beta_l and alpha_l are the plain fit's bits.
 *   4. M_l is the swept left block: the inverse over the kept pivots, the rows and columns of skipped pivots 0.
 *   5. For a row with w_e > 0, r_e[j] = v_e[j] - alpha_l[j], v_e the plain adjusted value with beta_l (rule 1 of the variance
 *      correction above, with the stored alpha_l).
 *   6. The leverage h_e = w_e (1 / W + q_e), q_e = xt_e' M_l xt_e with xt_e[k] = (x_e[k] - x_0[k]) - xm[k], the shifted, centred
 *      covariate of the moments: s_k = sum_m M_l[k][m] xt_e[m] (an fma chain from 0.0, m ascending), q_e = sum_k xt_e[k] s_k (an
 *      fma chain from 0.0, k ascending).
 *   7. PRESS_l[j] = sum over w_e > 0 of w_e (r_e[j] / (1 - h_e))^2, the exact leave-one-out residuals of the weighted ridge fit with
 *      an unpenalised intercept and the penalty matrix held fixed.  Rows of weight 0 take no part.
 *   8. If any contributing row has 1 - h_e <= 1e-10 (the fit interpolates), PRESS_l[j] = +inf for every j; a NaN counts as +inf.
 *   9. pick[j] = the smallest l with the smallest PRESS_l[j]; if every l is +inf, pick[j] = L - 1 and the pair counts as unscored.
 *  10. coef[:, j] = (alpha_pick, beta_pick); rows above nc are 0.
 * With L = 1 the same pass runs, the pick is trivial and the record holds that penalty's PRESS.  rank and status are those of the
 * call with the setting off (the pivots of the unpenalised C, the same bits), as are idx, dist and weight.  Everything that reads
 * coef sees the ridge fit: the adjusted rows, every product under method 1, the path summary, the back-transform, and the variance
 * correction, whose second fit stays unpenalised and models the residuals of the ridge fit.  On a tolerance path slot (b, t) of
 * coef, pick and press is made as abc_rank_targets_adjust_dev with K = K_t makes it (that call's order of sums) and has that
 * call's bits; the path's rank, status, post_mean and h keep theirs.  Every reduction's order depends on (K, nc, P, L) only: a
 * slot's outputs are the same bits alone, in any batch and through either entry point.  With the setting off (the default) every
 * output of every call keeps its bits.
 * lambda: host memory, copied; strictly ascending, every entry finite and >= 0, 1 <= L <= ABC_RIDGE_MAXL, else ABC_ERR_INVALID and
 * the setting stays as it was.  L = 0 or lambda = NULL turns the setting off.  Calls that do not regress ignore it.
 * Workspace: per target of a batch, L fits of 1 + nc + (1 + nc) P + nc^2 doubles and L P doubles per row tile. */
enum { ABC_RIDGE_MAXL = 8 };
int abc_ctx_set_adjust_ridge(abc_ctx* ctx, const double* lambda, size_t L);
/* The record of the last regressing call made under the setting, copied to host memory: pick (slots x P, at most cap_pick
 * entries) and press (slots x L x P, at most cap_press doubles; +inf: rule 8); either may be NULL when its cap is 0.  *slots, *L
 * and *P are always written, 0 / 0 / 0 while there is nothing.  Synchronises.  The record lives in device buffers of the context,
 * allocated or grown only while the setting is on and freed with the context. */
int abc_adjust_last_ridge(abc_ctx* ctx, int32_t* pick, size_t cap_pick, double* press, size_t cap_press,
                          size_t* slots, size_t* L, size_t* P);
/* (slot, parameter) pairs for which no penalty could be scored (rule 9) since the context was created or the last reset. */
int abc_adjust_ridge_unscored(abc_ctx* ctx, uint64_t* count, int reset);

/* ---- row importance weights of the batched ranking ------------------------------------------------------------------------------
 * Everything built on the batched ranking takes the N rows of the table for draws from the prior, as R's abc does: every retained
 * row counts the same, up to the kernel's factor.  The rows of an SMC generation from set 1 on are draws from the previous set's
 * perturbation kernel instead, and a reference table may come from any design that is not the prior; every posterior product then
 * estimates the wrong distribution, by an error that does not shrink with N or K.  The correction is the importance weight of the
 * row, omega_i = prior(theta_i) / proposal(theta_i), which depends on the row only and not on the target: for a generation it is
 * what abc_weight_predictive_prior / abc_weights_raw_dev compute for the N rows.  Any positive scale will do.
 * The setting holds N finite weights omega >= 0 with at least one positive.  While it is set, for every abc_rank_targets_*_dev /
 * abc_particle_ranking_pls_targets* entry:
 *   1. A call whose N differs from the stored count is ABC_ERR_INVALID.
 *   2. idx, dist, the fallback counter and the Epanechnikov fallback rule (distances only) keep every bit: the weights never
 *      influence which rows are retained.
 *   3. Entry e of a target weighs w_e = k_e * omega[i_e], one fp64 multiplication, k_e the kernel's weight as without the setting
 *      (1 under rejection, the rectangular kernel and the fallback).  abc_adjust_out.weight holds w_e, and every place that uses a
 *      weight uses w_e: the moments of the adjustment and of the path, the second fit of the variance correction, the leverages
 *      and PRESS of the ridge fit, the weights of every product under either method, the draws' cumulative weights and ess.
 *   4. post_mean of abc_rank_targets_dev and of the path is sum omega_e Y_e / sum omega_e.  abc_rank_targets_dev: thread t of 256
 *      takes the entries e = t, t + 256, ... ascending (numerator: one fma chain from 0; the weights' sum: a chain of additions),
 *      then both pass through the same halving tree.  The path: per parameter NS = 256 / min(P, 256) threads take every NS-th
 *      entry below K_t the same way, and their sums are added in thread order.  The order is fixed by K (and P) alone.
 *   5. Under method 0 the products are the weighted products of the retained rows with the weights omega[i_e]: the same kernels on
 *      the same values and weights as the generic entries (abc_weighted_*) given V = Y[idx[b]] and w = omega[idx[b]].  The path's
 *      summaries under method 0 take, per tolerance, the general kernels with K = K_t, as under method 1, so slot (b, t) has the
 *      bits of the summary call at K_t.
 *   6. A row with omega = 0 is an ordinary zero-weight row, as the Epanechnikov row at distance h is.  The variance correction's
 *      skip rule keeps its meaning: a zero or non-finite residual skips the parameter whatever the row's weight.
 *   7. The all-zero rule.  A slot whose retained rows all have w_e = 0 (W = 0) is not fitted: status gets bit 2 (value 4) beside
 *      the bits of their own rules (bit 0 when nc > 0: rank < nc), rank = 0, coef rows 0 .. nc and the target's theta rows are
 *      NaN, coef's rows beyond nc stay 0, weight is the zeros it is.  Under the variance correction every parameter of the slot is
 *      skipped and counted, and its hcoef record holds what a skipped parameter's holds: NaN in row 0, zeros below.  Under ridge
 *      every (slot, parameter) is unscored and counted, and the record holds pick = L - 1 and press = +inf for every penalty.
 *      post_mean of such a target is NaN.  In the products every floating-point output of the target is NaN (quantiles, cdf,
 *      grid, bandwidths, densities, modes, means, covariances, correlations, draws), its ess is 0 and its src entries are 0.  The
 *      other targets of the batch keep the bits they have in a batch without it.
 *   8. A target's outputs are the same bits alone, in any batch and through either entry point; reduction orders still depend on
 *      (K, nc, P) only.  omega[i_e] is one more 8-byte read per staged row, made where the row's weight is made.
 * Without the setting (the default) every call launches the kernel instances it launched before the setting existed and returns
 * the same bits.  The abc_weighted_* entries, the single-target rankings and the generation and sharded drivers are not affected.
 * R's abc has no such argument: it is this library's addition for tables that are not prior draws.
 * w (host memory) / w_dev (device memory): N doubles, copied, so the caller's buffer may be freed after the call.  One small kernel
 * counts the negative or non-finite and the positive entries and takes sum w and sum w^2, which the host reads here (the call
 * synchronises): a negative or non-finite weight, none positive, or weights so large that sum w or sum w^2 is not finite in fp64
 * (any positive scale will do short of that: rescale them) is ABC_ERR_INVALID and the setting stays as it was.  w = NULL or
 * N = 0 clears the setting. */
int abc_ctx_set_row_weights(abc_ctx* ctx, const double* w, size_t N);
int abc_ctx_set_row_weights_dev(abc_ctx* ctx, const double* w_dev, size_t N);
/* The setting: *N its count (0: off), *positive the number of positive weights, *ess = (sum w)^2 / sum w^2 of the whole table.
 * Any pointer may be NULL. */
int abc_row_weights_info(abc_ctx* ctx, size_t* N, size_t* positive, double* ess);

/* ---- tolerance path: one batched ranking, the rejection estimate and the local-linear fit at several tolerances ------------
 * What cv4abc does with tols = c(.005, .01, .05): ONE ranking at K_max = Ks[T-1] (idx and dist, K_max x B, are the bits of
 * abc_rank_targets_dev with K = K_max; dist may be NULL), and from it an estimate at every tolerance K_t of an ascending list.
 * The full (dist, row) order is nested, so rows e = 0..K_t-1 of that ranking are the ranking at K_t bit for bit.
 * Definition at tolerance t: the adjustment's definition above applied to rows e = 0..K_t-1 with h = d_{K_t-1}: the same weight
 * formula, the rectangular fallback evaluated on those K_t rows, the same shift by the first retained row, sweep and pivot rule.
 * post_mean is thetabar of the rectangular kernel over those rows (an fp64 mean).  Rows e >= K_t take NO part in tolerance t: they
 * are left out of its sums, not multiplied by a zero weight, so a non-finite parameter in a farther row never reaches a nearer
 * tolerance.
 * Every reduction's order depends on (K_max, K_t, nc, P) only: the outputs of (b, t) are the same bits alone, inside any batch,
 * through either entry point and whatever other tolerances the list holds (given its K_max).  A path of one tolerance, Ks = {K},
 * gives in coef, rank and status the bits of abc_rank_targets_adjust_dev with that K.
 * Limits and errors: those of the ranking (with K = K_max) and of the adjustment (A <= 64, P <= 1024), and ABC_ERR_INVALID for a
 * NULL path, NULL Ks, T = 0, T > 16, Ks[0] = 0 and a list that is not strictly ascending. */
typedef struct {
    const size_t* Ks; size_t T;  /* HOST memory in every entry: 1..16 strictly ascending tolerances, Ks[0] >= 1;
                                    K_max = Ks[T-1] obeys the ranking's limits (<= N, <= N-1 with an exclusion) */
    double*  post_mean;          /* B x T x P      rejection: fp64 mean of Y over the first K_t retained rows   */
    double*  coef;               /* B x T x (A+1) x P  loclinear at tolerance t, laid out as abc_adjust_out.coef */
    int32_t* rank;               /* B x T */
    int32_t* status;             /* B x T   bits as abc_adjust_out.status */
    double*  h;                  /* B x T   the bandwidth d_{K_t-1} (the bits of dist[b K_max + K_t - 1]) */
} abc_path;                      /* every output optional (NULL: not written); device or host memory per the entry point */
/* Device pointers (as abc_rank_targets_adjust_dev; Y required). */
int abc_rank_targets_path_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                              size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                              const uint64_t* exclude, int kernel, uint64_t* idx, double* dist, const abc_path* path);
/* HOST-pointer drop-in (as abc_particle_ranking_pls_targets_adjust), path's outputs in host memory. */
int abc_particle_ranking_pls_targets_path(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                          const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                          const uint64_t* exclude, int kernel, uint64_t* idx, double* dist,
                                          const abc_path* path, int32_t* ncomp);

/* ---- weighted posterior quantiles and CDF of the batched ranking ------------------------------------------------------------
 * A segment is one (target b, parameter j): values v_e and weights w_e, e = 0..K-1 in the ranking's row order, exclusion applied.
 *   method 0, rejection (ABC_POSTERIOR_REJECTION):  v_e = Y[i_e, j], w_e = 1 (the kernel argument is checked, no effect)
 *   method 1, loclinear (ABC_POSTERIOR_LOCLINEAR):  v_e = theta*_e[j], w_e = the adjustment's weight: the same bits that
 *             abc_adjust_out.theta / .weight hold for the same call (Epanechnikov, rectangular and the rectangular fallback)
 *   generic (abc_weighted_summary*):                 v_e = V[e + ldv j], w_e = w[e] (1 when w is NULL)
 * If any value of a segment is non-finite, all of that segment's outputs are NaN (other segments are unaffected).
 * The entries with w_e > 0, sorted ascending by the IEEE totalOrder of the value (-0.0 before +0.0), ties by e, are
 * u_0 .. u_{n-1} with weights om_r.
 *   W_r = om_0 + ... + om_r (reference: left to right in fp64; the device sums in another fixed order), W = W_{n-1}
 *   knots       p_r = fma(-0.5, om_r, W_r) / W
 *   quantile    q <= p_0: u_0;  q >= p_{n-1}: u_{n-1};  otherwise r = the largest index with p_r <= q,
 *               t = (q - p_r) / (p_{r+1} - p_r), Q(q) = fma(t, u_{r+1} - u_r, u_r).  With equal weights this is R's type 5
 *               ("hazen" in NumPy): the median of an even count is the midpoint of the middle two values.
 *   CDF at tau  F = fma(0.5, E, L) / W, L = sum of om_r over u_r < tau, E = sum over u_r == tau (IEEE equality: -0 == +0), both
 *               in sorted order; NaN tau gives NaN, +-inf gives 0 or 1.  Across well-calibrated cross-validation targets F is
 *               roughly uniform (the coverage diagnostic of Prangle et al. 2014).
 * This definition is the project's own, chosen to equal type 5 for equal weights.  R's abc package has its own convention for
 * weighted quantiles; it has not been checked against R.
 * With equal weights (method 0; method 1 with kernel 1 or the fallback; generic with w NULL) every W_r is an exact integer, so
 * the device's quantiles and CDF are the reference's bits.  With unequal weights the device's sums differ from the reference's
 * only by the rounding of another fixed summation order (|dW_r| <= 4 K 2^-53 W).  A target's outputs are the same bits on a
 * repeat run, alone (B = 1) and in any batch, and through the device and host entry points.
 * Outputs: quant B x nq x P row-major ([b][q][j]), cdf and truth B x P row-major (as post_mean); generic entry: quant nq x P,
 * cdf and truth P.  Limits as the adjustment's: A <= 64, P <= 1024 (ABC_ERR_UNSUPPORTED beyond); any K <= N. */
typedef struct {
    const double* probs;  size_t nq;  /* 1..64 finite levels in [0, 1], any order, repeats allowed; host memory in every entry */
    const double* truth;              /* optional; memory as the entry point's other arrays                                    */
    double* quant;                    /* optional                                                                             */
    double* cdf;                      /* optional; requires truth                                                             */
} abc_summary;
enum { ABC_POSTERIOR_REJECTION = 0, ABC_POSTERIOR_LOCLINEAR = 1 };
/* Device pointers (as abc_rank_targets_adjust_dev; Y required).  idx, dist and adj are optional; when given they receive the
 * bits of abc_rank_targets_dev / abc_rank_targets_adjust_dev for the same arguments (adj is ignored by method 0).  Besides the
 * ranking's and the adjustment's own checks, ABC_ERR_INVALID for method or kernel not 0 / 1, NULL sum, nq = 0 or > 64, a NaN
 * or out-of-range level, and cdf without truth.  Output members left NULL are not written. */
int abc_rank_targets_summary_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                                 size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                 const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx, double* dist,
                                 const abc_adjust_out* adj, const abc_summary* sum);
/* HOST-pointer drop-in (as abc_particle_ranking_pls_targets_adjust); every array of adj and sum in host memory. */
int abc_particle_ranking_pls_targets_summary(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                             const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                             const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx,
                                             double* dist, const abc_adjust_out* adj, const abc_summary* sum, int32_t* ncomp);
/* ---- tolerance path with summaries: weighted quantiles and the CDF at the truth at EVERY tolerance of one ranking -------------
 * What a user needs to choose the tolerance by cross-validation with cv4abc's default statistic (the median) and by the coverage
 * diagnostic (Prangle et al. 2014): the path call above and, from the same ranking at K_max, the summaries above at every K_t.
 * path is required and carries Ks and T; its five outputs stay optional and receive the bits of abc_rank_targets_path_dev for the
 * same arguments, as do idx and dist (both optional here).  sum is the abc_summary above with truth B x P,
 * quant B x T x nq x P ([b][t][q][j]) and cdf B x T x P; at least one of quant and cdf is required.
 * Definition: segment (b, t, j) is the summaries' segment built on rows e = 0..K_t-1 of the ranking at K_max.
 *   method 0: v_e = Y[i_e, j], w_e = 1.  The outputs are bit for bit those of abc_rank_targets_summary_dev with K = K_t.  (The
 *             values do not depend on t and ties break by e, so the (value, e) list sorted once at K_max and filtered by e < K_t is
 *             the sorted segment at K_t: one sort per (b, j) answers every tolerance.)
 *   method 1: v_e = theta*_e[j] with the coefficients of (b, t), the bits that path->coef[b][t] holds or would hold, and
 *             w_e = the adjustment's weight with h_t = d_{K_t-1}, the rectangular fallback evaluated on the first K_t distances as
 *             the path does.  With Ks = {K} quant and cdf are the bits of abc_rank_targets_summary_dev with that K, method 1.
 * Rows e >= K_t take no part in (b, t): a non-finite value in a farther row does not make a nearer tolerance NaN; one among the
 * first K_t entries makes that (b, t, j) NaN and nothing else.
 * Every reduction's order depends on (K_max, K_t, nc, P) only: (b, t) gives the same bits alone, in any batch, through either
 * entry, whatever the other tolerances of the list (given K_max) and whichever outputs are asked for.
 * Errors: the path's and the summaries' own, and ABC_ERR_INVALID for a NULL sum and for quant and cdf both NULL.  Limits:
 * A <= 64, P <= 1024, T <= 16, nq <= 64.  The caller sizes the outputs; nothing of size B K P is written. */
int abc_rank_targets_path_summary_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                                      size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                      const uint64_t* exclude, int method, int kernel, uint64_t* idx, double* dist,
                                      const abc_path* path, const abc_summary* sum);
/* HOST-pointer drop-in (as abc_particle_ranking_pls_targets_path); every array of path and sum in host memory. */
int abc_particle_ranking_pls_targets_path_summary(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                                  const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                                  const uint64_t* exclude, int method, int kernel, uint64_t* idx, double* dist,
                                                  const abc_path* path, const abc_summary* sum, int32_t* ncomp);

/* The same summaries of P given columns of K values (V[e + ldv j], device memory; w: K weights or NULL; truth, quant and cdf in
 * device memory).  ABC_ERR_INVALID also for K = 0, P = 0, ldv < K, NULL V, and weights that are negative, non-finite or all
 * zero (checked on the device; the call synchronises). */
int abc_weighted_summary_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t K, size_t P, const double* w,
                             const abc_summary* sum);
/* HOST-pointer form: V is K x P column-major (ldv = K); w, truth, quant and cdf in host memory. */
int abc_weighted_summary(abc_ctx* ctx, const double* V, size_t K, size_t P, const double* w, const abc_summary* sum);

/* ---- weighted posterior densities and modes of the batched ranking -----------------------------------------------------------
 * The marginal posterior density of every segment on a grid, a Gaussian kernel estimate as R's density() with bw.nrd0, and the
 * mode taken from it (summary.abc's "Weighted Mode").  A segment is that of the summaries above: values v_e and weights w_e,
 * e = 0..K-1 in the ranking's row order, exclusion applied; method 0 (rejection): Y rows, w = 1; method 1 (loclinear): theta*_e
 * with the adjustment's weights, the same bits as abc_adjust_out.theta / .weight; generic (abc_weighted_density*): V[e + ldv j],
 * w[e] (1 when w is NULL).  Only entries with w_e > 0 count.  If any value of a segment is non-finite, every output of that segment
 * is NaN (other segments are unaffected).
 *   moments     over the entries with w_e > 0: W = sum w, S2 = sum w^2, mean m = sum w v / W, n_eff = W^2 / S2,
 *               s^2 = sum w (v - m)^2 / (W - S2 / W): the n - 1 variance when the weights are equal; s = 0 when that denominator
 *               is <= 0 (a single entry).  The centred sum is taken about m in a second pass (the device: about u_min plus the
 *               mean of v - u_min), never as sum w v^2 - (sum w v)^2 / W.
 *   bandwidth   R's bw.nrd0: IQR = Q(0.75) - Q(0.25) by the weighted quantile definition above; lo = min(s, IQR / 1.34); if lo is
 *               0, lo = s; if that is 0, lo = |v of the first entry with w > 0 in ranking order|; if that is 0, lo = 1;
 *               h = bw_scale * 0.9 * lo * n_eff^(-1/5).  A given bandwidth (bw, one per segment) replaces the rule; bw_scale is
 *               not applied to it.  Two deviations from R: the IQR is type 5 here (R: type 7), and n_eff stands for length(x)
 *               (with equal weights n_eff = n).
 *   grid        u_min, u_max: the smallest and largest value with w > 0 (Q(0), Q(1)); lo_x = u_min - cut * h;
 *               step = ((u_max + cut * h) - lo_x) / (G - 1); x_g = fma((double)g, step, lo_x), g = 0..G-1.
 *   density     f(x_g) = sum_e w_e exp(-((x_g - v_e) / h)^2 / 2) / (W h sqrt(2 pi))
 *   mode        g* = the smallest g at which the device's own f is largest; mode = x_{g*}, mode_dens = f(x_{g*}).
 * Accuracy: |f_dev - f_ref| <= 1e-6 f_ref(x_g) + 1e-290 max_g f_ref, f_ref the long-double evaluation of the density at the
 * device's own h and grid (1e-6: the project's parity tolerance for weights).  The kernel's argument is formed in fp64; only the
 * factor 2^r, |r| <= 1/2, of each exponential is taken in f32.  bw_out agrees with a long-double evaluation of the rule to the
 * rounding of fixed-order sums of K terms and of the quantiles.
 * The order of every sum depends on (K, G) only and no floating-point atomics are involved: a target's outputs are the same bits
 * on a repeat run, alone (B = 1) and in any batch, through the device and host entry points, and whether or not dens is asked for.
 * This has not been checked against R.
 * Segment order: B x P row-major (as quant / cdf), P segments for the generic entry.  Limits as the summaries'. */
typedef struct {
    size_t G;            /* 2..4096 grid points per segment                                                                  */
    double cut;          /* finite, >= 0 (R: 3)                                                                              */
    double bw_scale;     /* finite, > 0 (R's adjust; 1)                                                                      */
    const double* bw;    /* optional: given bandwidths, one per segment, finite and > 0                                      */
    double* dens;        /* optional: [segment][g]                                                                           */
    double* grid;        /* optional: [segment][2] = lo_x, step                                                              */
    double* bw_out;      /* optional: h used                                                                                 */
    double* mode;        /* optional                                                                                         */
    double* mode_dens;   /* optional                                                                                         */
} abc_density;           /* memory of every array as the entry point's other arrays                                          */
/* Device pointers; the arguments of abc_rank_targets_summary_dev with den in place of sum.  idx, dist and adj are optional and
 * receive the bits of the plain calls.  Besides the ranking's, the adjustment's and the method / kernel checks, ABC_ERR_INVALID
 * for NULL den, G outside 2..4096, cut negative or non-finite, bw_scale <= 0 or non-finite, every output member NULL, and a given
 * bandwidth that is <= 0 or non-finite (checked on the device; the call then synchronises). */
int abc_rank_targets_density_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                                 size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                 const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx, double* dist,
                                 const abc_adjust_out* adj, const abc_density* den);
/* HOST-pointer drop-in (as abc_particle_ranking_pls_targets_summary); every array of adj and den in host memory. */
int abc_particle_ranking_pls_targets_density(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                             const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                             const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx,
                                             double* dist, const abc_adjust_out* adj, const abc_density* den, int32_t* ncomp);
/* The same densities of P given columns of K values (as abc_weighted_summary_dev, with its checks of V, ldv, K, P and w). */
int abc_weighted_density_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t K, size_t P, const double* w,
                             const abc_density* den);
/* HOST-pointer form: V is K x P column-major (ldv = K); w and den's arrays in host memory. */
int abc_weighted_density(abc_ctx* ctx, const double* V, size_t K, size_t P, const double* w, const abc_density* den);

/* ---- joint posterior of the batched ranking: covariances, correlations and pair densities -------------------------------------
 * What a pairs plot of a posterior draws, for every target at once: the weighted means, covariance and Pearson correlation matrix
 * of the P parameters, and for chosen pairs of parameters the two-dimensional Gaussian kernel density on a G x G grid with its
 * mode.  For target b the entries are e = 0..K-1 in the ranking's row order; the values v_e[j] and weights w_e are those of the
 * summaries and densities above (method 0 rejection, method 1 loclinear, generic: V[e + ldv j] and w[e], 1 when w is NULL).  Only
 * entries with w_e > 0 count.  A parameter j that holds any non-finite value is bad: every output that involves j is NaN (mean_j,
 * row and column j of cov and corr, grid and bw_out of j, dens / mode / mode_dens of every pair with j); the others are unaffected.
 *   moments     W = sum w, S2 = sum w^2, mean_j = sum w v_j / W,
 *               cov_ij = sum w (v_i - mean_i)(v_j - mean_j) / (W - S2 / W), the centred sum taken about the means in a second pass,
 *               never from raw second moments; cov is 0 everywhere when that denominator is <= 0 (a single entry).  This is
 *               numpy.cov(aweights = w).  One triangle is computed and mirrored: cov and corr are symmetric bit for bit.
 *   correlation corr_ij = cov_ij / (sqrt(cov_ii) sqrt(cov_jj)), clamped to [-1, 1]; corr_ii is exactly 1 when cov_ii > 0; corr_ij
 *               is NaN when either variance is 0.
 *   bandwidth h_j and grid (lo_x_j, step_j) of parameter j: the bits abc_*_density returns for the same segment with the same G,
 *               cut, bw_scale and bw (bw.nrd0 on the weighted moments and quantiles, as defined above); x_g = fma(g, step, lo_x).
 *   pair density, for a pair (i, j), i != j, i on the first grid axis (x), j on the second (y):
 *               f(x_g, y_g') = sum_e w_e exp(-((x_g - v_ei) / h_i)^2 / 2) exp(-((y_g' - v_ej) / h_j)^2 / 2) / (W 2 pi h_i h_j),
 *               the product-Gaussian estimate of MASS::kde2d.  The bandwidths are those of the marginal densities above, not
 *               kde2d's bandwidth.nrd.
 *   joint mode  the smallest flat index g G + g' at which the device's own f is largest: mode = (x_g, y_g'), mode_dens = f there.
 * Accuracy: |f_dev - f_ref| <= 1e-6 f_ref + 1e-290 max f_ref over the pair's grid, f_ref the long-double evaluation at the device's
 * own h and grids: each factor's argument is formed in fp64 and only 2^r, |r| <= 1/2, is taken in f32, as the marginal density's
 * terms.  mean within K 2^-52 max|v| and cov within 1e-9 sqrt(cov_ii cov_jj) of the long-double values.
 * The order of every sum depends on (K, P) only and no floating-point atomics are involved: a target's outputs are the same bits on
 * a repeat run, alone (B = 1) and in any batch, through the device and host entry points, whether or not dens is asked for, and for
 * a pair alone or among other pairs.  The pair (j, i) is computed on its own and equals the transpose of (i, j) within the accuracy
 * above, not bit for bit.  None of this has been checked against R.
 * Layout: mean [b][P]; cov, corr [b][P][P]; grid [b][P][2] = lo_x, step; bw_out [b][P]; dens [b][pair][g][g']; mode [b][pair][2];
 * mode_dens [b][pair]; the generic entries have one b.  The caller sizes dens: B npairs G^2 doubles, which is 3.9 GB for 1000
 * targets x 120 pairs x 64^2; the host entries stage it in the context's workspace as well.  Limits as the summaries': A <= 64,
 * P <= 1024, and a given pair list holds at most 2^22 pairs (ABC_ERR_UNSUPPORTED beyond). */
typedef struct {
    size_t G;                 /* 2..256 grid points per axis                                                                 */
    double cut, bw_scale;     /* as abc_density                                                                              */
    const double* bw;         /* optional: given bandwidths, one per (target, parameter), as abc_density                     */
    const int32_t* pairs;     /* optional, HOST memory in every entry: npairs x 2 = (i, j), 0 <= i, j < P, i != j;           */
    size_t npairs;            /*   NULL: all i < j in the order (0,1), (0,2), ..., (P-2,P-1), and npairs is ignored          */
    double *mean, *cov, *corr;        /* [b][P], [b][P][P], [b][P][P]                                                        */
    double* dens;                     /* [b][pair][g][g']                                                                    */
    double *grid, *bw_out;            /* [b][P][2], [b][P]: those of abc_density at this G                                   */
    double *mode, *mode_dens;         /* [b][pair][2], [b][pair]                                                             */
} abc_joint;                  /* every output optional, at least one required; memory as the entry point's other arrays     */
/* Device pointers; the arguments of abc_rank_targets_density_dev with jt in place of den.  idx, dist and adj are optional and
 * receive the bits of the plain calls.  Besides the ranking's, the adjustment's and the method / kernel checks, ABC_ERR_INVALID
 * for NULL jt, G outside 2..256, cut negative or non-finite, bw_scale <= 0 or non-finite, a pair index out of range or with
 * i == j, pairs given with npairs == 0, every output member NULL, and a given bandwidth that is <= 0 or non-finite (checked on the
 * device; the call then synchronises).  P = 1 with pairs NULL is valid: there are no pairs, and dens, mode and mode_dens are not
 * written. */
int abc_rank_targets_joint_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                               size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                               const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx, double* dist,
                               const abc_adjust_out* adj, const abc_joint* jt);
/* HOST-pointer drop-in (as abc_particle_ranking_pls_targets_density); every array of adj and jt in host memory. */
int abc_particle_ranking_pls_targets_joint(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                           const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                           const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx,
                                           double* dist, const abc_adjust_out* adj, const abc_joint* jt, int32_t* ncomp);
/* The same of P given columns of K values (as abc_weighted_density_dev, with its checks of V, ldv, K, P and w). */
int abc_weighted_joint_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t K, size_t P, const double* w, const abc_joint* jt);
/* HOST-pointer form: V is K x P column-major (ldv = K); w and jt's arrays in host memory. */
int abc_weighted_joint(abc_ctx* ctx, const double* V, size_t K, size_t P, const double* w, const abc_joint* jt);

/* ---- posterior draws of the batched ranking: weighted and smoothed bootstrap -------------------------------------------------
 * A posterior handed back as a sample: S rows per target, resampled from the target's K entries with the entries' weights (the
 * weighted bootstrap) and, on request, jittered by the marginal densities' bandwidths (the smoothed bootstrap: a sample of the
 * estimate that abc_*_density draws).  For a posterior predictive check, or to start a follow-up set per target.  For target b the
 * entries are e = 0..K-1 in the ranking's row order; the values v_e[j] and weights w_e are those of the products above (method 0
 * rejection: Y rows, w = 1; method 1 loclinear: theta*_e with the adjustment's weights; generic: V[e + ldv j] and w[e], 1 when w
 * is NULL).
 *   cumulative  c_e = w_0 + ... + w_e, an inclusive prefix sum in a fixed order that depends on K only (entries with w_e <= 0 add
 *               0); W = c_{K-1} is that same sum.  The order is a tree, not left to right: |c_e - exact| <= 4 K 2^-53 W, the
 *               bound of the summaries' sums.  c is non-decreasing, and c_e == c_{e-1} exactly when w_e == 0.  With equal weights
 *               c_e = e + 1 exactly.
 *   selection   of draw s of target b, t = stream[b] (b when stream is NULL): the Philox4x32-10 block of counter
 *               (lo32(t), hi32(t), s, 0) under the key (k0, k1) = (lo32(seed), hi32(seed)) gives the words x0..x3;
 *               m = (x0 << 21) | (x1 >> 11) (53 bits), u = m 2^-53, tau = u W (one rounding); src = the smallest e with
 *               c_e > tau.  An entry with w_e = 0 is never chosen.  With equal weights src = floor(u K), exact on both sides.
 *   values      smooth == 0: draws[b][s][j] = v_src[j], the bits of abc_adjust_out.theta / Y / V at that row.
 *               smooth == 1: draws[b][s][j] = fma(h_j, z_j, v_src[j]).  h_j is bit for bit the bandwidth that abc_*_density returns
 *               in bw_out for segment (b, j) with the same bw_scale and bw (bw.nrd0 on the weighted moments and quantiles; a given
 *               bandwidth replaces the rule).  z_j is deviate j mod 4 of the four normal deviates made of the Philox block of counter
 *               (lo32(t), hi32(t), s, 1 + j / 4): two Box-Muller pairs (x0, x1) and (x2, x3) evaluated in f32 (the radius from all
 *               32 bits of the first word of a pair, the angle from the top 24 bits of the second), the deviates of the device
 *               noise stream of abc_perturb_dev; they carry f32 rounding, about 1e-7 relative.
 *   bad         a parameter j with a non-finite value among a target's entries has h_j = NaN, as in the densities: its smoothed
 *               draws are NaN.  Plain draws copy the values as they are.  The other parameters are unaffected.
 *   ess         W^2 / S2, S2 = sum of w^2, over the entries with w > 0 (K with equal weights).
 * A draw depends on (seed, stream id, s) and its target's segment only.  So a target with the same stream id gets the same bits
 * alone (B = 1) and in any batch, on a repeat run, through the device and host entry points, and whichever output members are asked
 * for; a call with S' < S gives the first S' draws of the call with S; and two targets with different stream ids get independent
 * selections and noise.  A caller that splits a batch over several calls passes each target's own number in stream.  The context's
 * abc_rng is not used and not advanced.  No floating-point atomics are involved.
 * Not done here: the draws are not clipped to prior bounds, the smoothed bootstrap is not shrunk towards the mean (its variance is
 * the sample's plus h^2), and the kernel is a product of marginal ones (no correlated smoothing).
 * Layout: draws [b][s][j], src [b][s], bw_out [b][j], ess [b]; the generic entries have one b.  The caller sizes draws: B S P doubles;
 * the host entries stage it in the context's workspace as well.  Limits as the summaries': A <= 64, P <= 1024. */
typedef struct {
    size_t S;               /* draws per target, 1..2^24                                                                    */
    int smooth;             /* 0: weighted bootstrap (rows as they are); 1: smoothed bootstrap, + h_j z_j                   */
    double bw_scale;        /* smooth only: as abc_density (finite, > 0)                                                    */
    const double* bw;       /* smooth only, optional: given bandwidths, one per segment, as abc_density                     */
    uint64_t seed;          /* Philox key: k0 = lo32(seed), k1 = hi32(seed)                                                 */
    const uint64_t* stream; /* optional, B entries (1 for the generic entry): the stream id of target b;                    */
                            /* NULL: b.  HOST memory in every entry, as abc_joint.pairs                                     */
    double* draws;          /* optional: [b][s][j], B x S x P                                                               */
    uint64_t* src;          /* optional: [b][s], the position e in 0..K-1 (ranking order) the draw came from                */
    double* bw_out;         /* optional: [b][j], h used (smooth only; NaN when smooth == 0)                                 */
    double* ess;            /* optional: [b], W^2 / S2 over the entries with w > 0                                          */
} abc_draws;                /* at least one output required; memory of bw and the outputs as the entry point's other arrays */
/* Device pointers; the arguments of abc_rank_targets_density_dev with dr in place of den.  idx, dist and adj are optional and
 * receive the bits of the plain calls.  Besides the ranking's, the adjustment's and the method / kernel checks, ABC_ERR_INVALID
 * for NULL dr, S outside 1..2^24, smooth not 0 / 1, every output member NULL, and when smoothing bw_scale <= 0 or non-finite and
 * a given bandwidth that is <= 0 or non-finite (checked on the device; the call then synchronises). */
int abc_rank_targets_draws_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                               size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                               const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx, double* dist,
                               const abc_adjust_out* adj, const abc_draws* dr);
/* HOST-pointer drop-in (as abc_particle_ranking_pls_targets_density); every array of adj and dr in host memory. */
int abc_particle_ranking_pls_targets_draws(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                           const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                           const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx,
                                           double* dist, const abc_adjust_out* adj, const abc_draws* dr, int32_t* ncomp);
/* The same of P given columns of K values (as abc_weighted_density_dev, with its checks of V, ldv, K, P and w). */
int abc_weighted_draws_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t K, size_t P, const double* w, const abc_draws* dr);
/* HOST-pointer form: V is K x P column-major (ldv = K); w and dr's arrays in host memory. */
int abc_weighted_draws(abc_ctx* ctx, const double* V, size_t K, size_t P, const double* w, const abc_draws* dr);

/* ---- posterior entropy of the batched ranking: the k-nearest-neighbour estimate ------------------------------------------------
 * One number per target that says how concentrated its posterior is in all P parameters at once: the Kozachenko-Leonenko
 * k-nearest-neighbour entropy of the target's K entries, in the form of Singh et al. (2003) that the minimum-entropy criterion
 * of Nunes & Balding (2010) uses to choose summary statistics (abctools: AS.select, nn.ent).  It has NOT been checked against
 * abctools.  A Gaussian entropy from the joint product's covariance is no substitute for skewed, bounded or multimodal posteriors.
 * For one target the entries are e = 0..K-1 in the ranking's row order and their values v_e[j] are those of the products above,
 * bit for bit (method 0 rejection: the Y rows; method 1 loclinear: theta*_e, with the transforms, the variance correction and
 * the ridge adjustment when set; generic: V[e + ldv j]).  With n = K:
 *   scaled value  u_e[j] = v_e[j] / scale[j], a division (a generic call on a matrix divided beforehand gives the same bits);
 *                 without scale u_e[j] = v_e[j].
 *   distance      d2(e, f): acc = 0, then acc = fma(dl_j, dl_j, acc) for j ascending, dl_j = u_e[j] - u_f[j].
 *   neighbour     rho2_e = the k-th smallest of d2(e, f) over f != e; f != e is decided by position, not by value.
 *                 knn[e] = sqrt(rho2_e).
 *   entropy       H = c + coef S, S = sum_e log rho2_e, coef = P / (2 n) (one rounding) and
 *                 c = (P / 2) log pi - lgamma(P / 2 + 1) - psi(k) + log n, psi(k) = -gamma + sum_{m < k} 1 / m, made on the host in
 *                 double.  S is taken in a fixed order that depends on K only (entry e belongs to e mod 256; each class is summed
 *                 with e ascending, then the 256 class sums by a binary tree).
 *   zeros         the number of entries with rho2_e == 0, that is k or more exact duplicates; when zeros > 0, H = -inf.
 *   too few       K <= k: H = NaN, the target's knn NaN, zeros 0.
 *   bad           a non-finite scaled value among a target's entries makes that target's H and knn NaN and its zeros 0.  The
 *                 other targets are unaffected.  (Finite values whose distance overflows give rho2 = +inf the ordinary way.)
 * No floating-point atomics are used.  A target's outputs are the same bits on a repeat run, alone (B = 1) and in any batch,
 * through the device and host entry points, and whichever output members are asked for.  knn of a row-permuted generic V is the
 * permuted knn, bit for bit; H is not, because the order of its sum moves.
 * The estimator is for an unweighted sample, so the entries' weights must all be equal: ABC_ERR_UNSUPPORTED, with a message that
 * says which, for method 1 with the Epanechnikov kernel (pass the rectangular kernel), for a ranking call while row importance
 * weights are set on the context, and for a generic call with w non-NULL.  There is no entry for tolerance paths: a smaller
 * tolerance lowers the entropy almost by construction.
 * Layout: H [b], knn [b][e], zeros [b]; the generic entries have one b.  Limits as the summaries': A <= 64, P <= 1024; K is
 * limited by the workspace alone (B K (P + 1) doubles). */
typedef struct {
    int k;                 /* 1..8; abctools uses 4                                              */
    const double* scale;   /* optional, P finite values > 0, HOST memory in every entry          */
    double* H;             /* [b]                                                                */
    double* knn;           /* [b][e], B x K: distance to the k-th nearest neighbour              */
    uint64_t* zeros;       /* [b]                                                                */
} abc_entropy;             /* at least one output required; memory as the entry's other arrays   */
/* Device pointers; the arguments of abc_rank_targets_draws_dev with en in place of dr.  idx, dist and adj are optional and
 * receive the bits of the plain calls.  Besides the ranking's, the adjustment's and the method / kernel checks, ABC_ERR_INVALID
 * for NULL en, k outside 1..8, every output member NULL and a scale entry that is <= 0 or non-finite; ABC_ERR_UNSUPPORTED as
 * above. */
int abc_rank_targets_entropy_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                                 size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                 const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx, double* dist,
                                 const abc_adjust_out* adj, const abc_entropy* en);
/* HOST-pointer drop-in (as abc_particle_ranking_pls_targets_draws); every array of adj and en in host memory. */
int abc_particle_ranking_pls_targets_entropy(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                             const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                             const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx,
                                             double* dist, const abc_adjust_out* adj, const abc_entropy* en, int32_t* ncomp);
/* The same of P given columns of K values (as abc_weighted_draws_dev, with its checks of V, ldv, K and P); w must be NULL. */
int abc_weighted_entropy_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t K, size_t P, const double* w, const abc_entropy* en);
/* HOST-pointer form: V is K x P column-major (ldv = K); en's arrays in host memory. */
int abc_weighted_entropy(abc_ctx* ctx, const double* V, size_t K, size_t P, const double* w, const abc_entropy* en);

/* ---- highest-density intervals of the batched ranking: the shortest interval that holds a given mass --------------------------
 * The interval an analyst reports as "the 95 % credible interval" of a skewed, bounded posterior (the HPD interval or HDI, as
 * coda::HPDinterval), where the summaries' quantiles give equal-tailed intervals only.  A segment, its sorted entries
 * u_0 .. u_{n-1}, its knots p_r = fma(-0.5, om_r, W_r) / W and the quantile function Q(q) are the summaries' above; the device
 * takes the same sums in the same fixed order as the summaries, so p_r and W are the summary call's bits for the same segment.
 * For a mass m, 0 < m < 1, the candidates are numbered c = 2 r + kind, r = 0..n-1 (fl: one fp64 rounding):
 *   kind 0 (lower end on knot r):  plo = p_r,          phi = fl(p_r + m),  lo = u_r,     hi = Q(phi),  valid iff phi <= p_{n-1}
 *   kind 1 (upper end on knot r):  plo = fl(p_r - m),  phi = p_r,          lo = Q(plo),  hi = u_r,     valid iff plo >= p_0
 * with Q evaluated by the summaries' expressions (the largest r with p_r <= q, then t, then fma(t, u_{r+1} - u_r, u_r)).  The
 * result is the valid candidate with the smallest (hi - lo, c) in lexicographic order, the width in fp64: a total order, so the
 * answer does not depend on the shape of the reduction.  If no candidate is valid (n = 1, or m at least the knots' span):
 * lo = u_0, hi = u_{n-1}, plo = p_0, phi = p_{n-1}.  A non-finite value in the segment, or n = 0, makes all four outputs of that
 * segment NaN and affects nothing else.
 * Why: between the first and the last knot Q is piecewise linear, so Q(p + m) - Q(p) is piecewise linear in p with its breakpoints
 * exactly at these candidates, and a minimum lies on one of them; the search is restricted to [p_0, p_{n-1} - m] so that the flat
 * tails of Q cannot donate free mass.  The result is the exact minimiser for the project's own quantile convention, not a grid
 * approximation.  With equal weights and integer n m it is coda::HPDinterval's interval [x_i, x_{i + n m}]; a NumPy prototype
 * agreed with coda's rule on gamma-distributed samples, but it has NOT been compared with R itself.
 * Guarantees.  With equal weights (as the summaries': method 0; method 1 with kernel 1 or the fallback; generic with w NULL) the
 * outputs are the reference's bits.  A target gives the same bits on a repeat run, alone (B = 1) and in any batch, through the
 * device and host entries, and whichever outputs are requested.  (lo, hi) are the bits that the summary call on the same segment
 * returns for probs = {plo, phi}, as long as the knot at the winning end is not tied with a later knot (two neighbouring weights
 * both below the rounding of W can tie knots; the summary then answers from the last of them).  With unequal weights the knots
 * differ from the reference's by the rounding of the other summation order, as the summaries' do.
 * Layout: lo, hi, plo, phi B x nm x P row-major ([b][m][j]); generic entry nm x P.  Limits are the summaries': A <= 64,
 * P <= 1024 (ABC_ERR_UNSUPPORTED beyond), any K <= N.  There is no form for tolerance paths (abc_rank_targets_path_*) and none in
 * the sharded driver. */
typedef struct {
    const double* mass;  size_t nm;   /* 1..16 finite masses strictly inside (0, 1), any order; host memory in every entry */
    double* lo;  double* hi;          /* optional; B x nm x P ([b][m][j]); generic entry nm x P                           */
    double* plo; double* phi;         /* optional; the probabilities of the two ends, same layout                         */
} abc_hpd;                            /* at least one output required                                                      */
/* Device pointers; the arguments of abc_rank_targets_summary_dev with hd in place of sum.  idx, dist and adj are optional and
 * receive the bits of the plain calls.  Besides the ranking's, the adjustment's and the method / kernel checks, ABC_ERR_INVALID
 * for NULL hd, nm = 0 or > 16, NULL mass, a mass that is NaN or outside (0, 1), and all four outputs NULL. */
int abc_rank_targets_hpd_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M, size_t P,
                             const double* model, size_t A, const double* targets, size_t ldt, size_t B, const uint64_t* exclude,
                             size_t K, int method, int kernel, uint64_t* idx, double* dist, const abc_adjust_out* adj,
                             const abc_hpd* hd);
/* HOST-pointer drop-in (as abc_particle_ranking_pls_targets_summary); every array of adj and hd in host memory. */
int abc_particle_ranking_pls_targets_hpd(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                         const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                         const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx, double* dist,
                                         const abc_adjust_out* adj, const abc_hpd* hd, int32_t* ncomp);
/* The same of P given columns of K values (as abc_weighted_summary_dev, with its checks of V, ldv, K, P and w). */
int abc_weighted_hpd_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t K, size_t P, const double* w, const abc_hpd* hd);
/* HOST-pointer form: V is K x P column-major (ldv = K); w and hd's arrays in host memory. */
int abc_weighted_hpd(abc_ctx* ctx, const double* V, size_t K, size_t P, const double* w, const abc_hpd* hd);

/* ---- ABC-GLM posterior of the batched ranking (Leuenberger & Wegmann 2010): densities, moments and the evidence ---------------
 * ABCtoolbox's estimator on top of PLS.  On the retained rows a general linear model of the scores on the parameters is fitted;
 * the retained sample is taken as a mixture of sharp Gaussian peaks (the truncated prior) and multiplied analytically by the
 * Gaussian likelihood of the observation.  That gives smooth marginal posterior densities, posterior means and variances that
 * rest on no regression of parameters on statistics, and the marginal density of the observation (the evidence of model choice).
 * Inputs, per target b.  The ranking's rows e = 0..K-1 carry the parameter rows theta_e (P) = Y[i_e, :], the scores x_e (n = the
 * model's ncomp) and the observed scores o, exactly the covariates of abc_rank_targets_adjust_dev, and the weights w_e: the row
 * importance weight of i_e when row weights are set on the context, else 1.  Only entries with w_e > 0 count.  W = sum w,
 * S2 = sum w^2, n_eff = W^2 / S2.  Any non-finite theta or x among the counted rows makes every output of that target NaN and sets
 * status bit 2 (so does a non-finite theta in an uncounted row, with or without a given bw: abc_density's rule reads every
 * entry of a parameter's column before it looks at the weights).
 * Step 1, moments.  The weighted means thbar and xbar; in a second pass the centred weighted moments divided by W: M_thth (P x P),
 *   M_thx (P x n), M_xx (n x n).
 * Step 2, the GLM s = C theta + c0 + eps.  M_thth is factored by Cholesky in parameter order; a pivot <= 1e-10 of its own diagonal
 *   entry makes the target degenerate: status bit 0 and NaN outputs (the pivot is not skipped).  C = (M_thth^-1 M_thx)', n x P;
 *   c0 = xbar - C thbar; R = M_xx - M_xth M_thth^-1 M_thx; Sigma_s = R n_eff / (n_eff - P - 1).  n_eff <= P + 1, or a Cholesky
 *   pivot of Sigma_s <= 1e-10 of its diagonal entry, sets status bit 1 and writes NaN outputs.
 * Step 3, peaks.  Sigma_theta = diag(h_j^2), h_j the bandwidth of parameter j by abc_density's rule (bw.nrd0 on the weighted
 *   sample, times bw_scale); a given bw array (B x P) replaces the rule, as there.
 * Step 4, the posterior mixture, every theta taken relative to thbar (an exact reparametrisation that keeps the exponents small).
 *   Q = C' Sigma_s^-1 C + Sigma_theta^-1; T = Q^-1 by Cholesky; u = C' Sigma_s^-1 (o - xbar); v_e = u + Sigma_theta^-1 (theta_e - thbar);
 *   t_e = thbar + T v_e; log c_e = log w_e - [(theta_e - thbar)' Sigma_theta^-1 (theta_e - thbar) - v_e' T v_e] / 2;
 *   c^_e = exp(log c_e - max log c) / (the sum of that over the counted rows).
 * Step 5, products.  mean[j] = sum c^_e t_e[j]; var[j] = T_jj + sum c^_e (t_e[j] - mean[j])^2; ess = 1 / sum c^_e^2.
 *   Grid, per (b, j): lo_x = min_e t_e[j] - cut sqrt(T_jj); step = ((max_e t_e[j] + cut sqrt(T_jj)) - lo_x) / (G - 1);
 *   x_g = fma(g, step, lo_x).  Marginal density f_j(x_g) = sum_e c^_e exp(-(x_g - t_e[j])^2 / (2 T_jj)) / sqrt(2 pi T_jj), the
 *   term evaluated as abc_density's (fp64 argument; relative error of a term about 1e-7).  mode is the x_g of the smallest g at
 *   which the device's own f is largest, mode_dens that f.  Evidence: S = Sigma_s + C Sigma_theta C';
 *   log_md = log sum_e w_e N(o; c0 + C theta_e, S) - log W, by log-sum-exp with the Cholesky factor of S.
 *   Model outputs (optional): C (B x n x P), c0 (B x n), sigma_s (B x n x n), T (B x P x P), peaks t_e (B x K x P, [b][e][j]) and
 *   c = c^_e (B x K); peaks and c are written only when asked for.  C, c0 and sigma_s are packed at the model's n = ncomp; the
 *   caller's arrays hold room for n = min(A, 32).
 * Reduction order.  The order of every reduction depends on (K, n, P, G) only: a target's outputs are the same bits on a repeat,
 * alone or in any batch, through the device or the host entry, and with or without dens / peaks.
 * Limits: 1 <= P <= 32, 1 <= ncomp <= 32, A <= 64, G in 2..4096, cut >= 0 and finite, bw_scale > 0 and finite, at least one output;
 * each violation is ABC_ERR_INVALID with a message (ncomp is read from the model before anything is ranked).  A parameter
 * transform, the variance correction or ridge set on the context is ABC_ERR_UNSUPPORTED: ABC-GLM is not an adjustment, so those
 * settings have no meaning for it.
 * Deviations from ABCtoolbox: the peak widths come from abc_density's bandwidth rule instead of diracPeakWidth, the statistics are
 * the PLS scores instead of raw statistics, and all targets share one PLS fit.  NOT checked against ABCtoolbox itself. */
#define ABC_GLM_MAX 32
typedef struct {
    size_t G;                          /* grid points per parameter, 2..4096                                              */
    double cut, bw_scale;              /* as abc_density                                                                  */
    const double* bw;                  /* optional: given bandwidths h_j, B x P, finite and positive                      */
    double *dens;                      /* optional; B x P x G ([b][j][g])                                                 */
    double *lo_x, *step;               /* optional; B x P                                                                 */
    double *mode, *mode_dens;          /* optional; B x P                                                                 */
    double *mean, *var;                /* optional; B x P                                                                 */
    double *ess, *log_md;              /* optional; B                                                                     */
    double *C, *c0, *sigma_s, *T;      /* optional; B x n x P, B x n, B x n x n, B x P x P (row-major per target)         */
    double *peaks, *c;                 /* optional; B x K x P, B x K                                                      */
    int32_t* status;                   /* optional; B: bit 0 degenerate M_thth, bit 1 n_eff or Sigma_s, bit 2 non-finite; */
                                       /* one bit at most, the first of: non-finite input, n_eff <= P + 1 (also: no       */
                                       /* counted row), a pivot of M_thth, a pivot of Sigma_s                              */
} abc_glm;                             /* memory of every array as the entry point's other arrays                         */
/* Device pointers; the remaining arguments are those of abc_rank_targets_density_dev without method and kernel.  idx and dist are
 * optional and receive the bits of abc_rank_targets_dev.  The descriptor comes first: the call is a method of the request. */
int abc_glm_rank_targets_dev(const abc_glm* glm, abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N,
                             size_t M, size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                             const uint64_t* exclude, size_t K, uint64_t* idx, double* dist);
/* HOST-pointer drop-in (as abc_particle_ranking_pls_targets_density); every array of glm in host memory. */
int abc_glm_particle_ranking_pls_targets(const abc_glm* glm, abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M,
                                         size_t P, const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                         const uint64_t* exclude, size_t K, uint64_t* idx, double* dist, int32_t* ncomp);
/* The generic form for any retained sample with any statistics (B = 1): theta K x P (theta[e + ldv j]), stats K x n
 * (stats[e + lds k]), obs the n observed statistics, w the K weights (NULL: all 1; checked as abc_weighted_density_dev's).
 * ABC_ERR_INVALID for a NULL theta, stats or obs, K = 0, P or n outside 1..32, ldv < K or lds < K. */
int abc_glm_weighted_dev(const abc_glm* glm, abc_ctx* ctx, const double* theta, size_t ldv, const double* stats, size_t lds, size_t K,
                         size_t P, size_t n, const double* obs, const double* w);
/* HOST-pointer form: theta and stats column-major with ldv = lds = K; every array in host memory. */
int abc_glm_weighted(const abc_glm* glm, abc_ctx* ctx, const double* theta, const double* stats, size_t K, size_t P, size_t n,
                     const double* obs, const double* w);

/* ---- ABC-GLM posterior: exact quantiles and the CDF at a truth ---------------------------------------------------------------
 * The four ABC-GLM entries with one more descriptor, an abc_summary (probs, nq, truth, quant, cdf) right after glm; both come in
 * front of the context.  ABCtoolbox validates this estimator by the posterior quantile of the true parameter over many
 * pseudo-observed sets (Wegmann et al. 2010); cdf is that quantile.
 * Definition.  Every peak of parameter j has the one variance T_jj, so with sigma = sqrt(T_jj) the marginal CDF of step 4's mixture is
 *   F_j(x) = sum over the counted rows e (w_e > 0), in the ranking's order, of c^_e Phi((x - t_e[j]) / sigma),
 *   Phi(z) = erfc(-z / sqrt 2) / 2.
 * For a target of status 0:
 *   cdf[b][j] = F_j(truth[b][j]); a NaN truth gives NaN, -inf gives 0 and +inf gives 1.
 *   quant[b][q][j] = the x with F_j(x) = probs[q].  F_j is strictly increasing, so the root is unique.  It lies in
 *     [min_e t_e[j] + sigma z_q, max_e t_e[j] + sigma z_q], z_q = Phi^-1(probs[q]), because every peak lies between the two
 *     extremes.  The device closes that bracket (widened by 2^-49 of its terms and four doubles) with a safeguarded Newton
 *     iteration on its own evaluation of F_j until no double lies strictly between the ends, and returns the end whose F_j is
 *     nearer probs[q]: |F_j(quant) - probs[q]| is within the rounding of a K-term fp64 sum plus what one spacing of quant is
 *     worth in F_j (the density there times that spacing).
 * For a target whose status is not 0 every quant and cdf entry of that target is NaN; other targets are unaffected.
 * Phi is evaluated with the device library's fp64 erfc, not with the density's term (whose relative error is about 1e-7).
 * No sort, no knots and no interpolation convention enter: this is not abc_rank_targets_summary_dev's weighted sample quantile.
 * Reduction order.  The order of every sum depends on (K, n, P, nq) only, and there are no floating-point atomics.  A target's
 * quant and cdf are the same bits on a repeat, alone (B = 1) or in any batch, through the device and the host entry, whatever glm
 * outputs are asked for beside them, and for each level whatever other levels are in probs.  The glm outputs written by these
 * entries are bit for bit those of the corresponding entry above for the same arguments.
 * Arguments.  sum is required (NULL: ABC_ERR_INVALID).  Every output member of glm is optional here and all may be NULL; G, cut,
 * bw_scale and bw keep their meaning and their checks (G also when no grid output is asked for).  At least one of sum->quant,
 * sum->cdf and the outputs of glm is required.  probs in host memory in every entry, nq in 1..64, every level finite and STRICTLY
 * inside (0, 1) (the mixture's quantile at 0 or 1 is infinite; ABC_ERR_INVALID, although abc_summary allows both elsewhere), any
 * order, repeats allowed; probs and nq are read only when quant is given.  cdf without truth is ABC_ERR_INVALID.
 * Shapes as abc_summary's: quant B x nq x P ([b][q][j]), cdf and truth B x P; the generic entries nq x P and P.  Memory as the
 * entry point's other arrays.  Every other check, limit and refusal is that of the entry above that the new one extends, with
 * the same message, before anything is ranked.  Like the ABC-GLM posterior itself this is NOT checked against ABCtoolbox. */
int abc_glm_rank_targets_summary_dev(const abc_glm* glm, const abc_summary* sum, abc_ctx* ctx, const double* X, size_t ldx,
                                     const double* Y, size_t ldy, size_t N, size_t M, size_t P, const double* model, size_t A,
                                     const double* targets, size_t ldt, size_t B, const uint64_t* exclude, size_t K, uint64_t* idx,
                                     double* dist);
/* HOST-pointer drop-in: every array of glm and sum in host memory. */
int abc_glm_particle_ranking_pls_targets_summary(const abc_glm* glm, const abc_summary* sum, abc_ctx* ctx, const double* X,
                                                 const double* Y, size_t N, size_t M, size_t P, const double* targets, size_t B,
                                                 double train_frac, int max_comp, int rule, const uint64_t* exclude, size_t K,
                                                 uint64_t* idx, double* dist, int32_t* ncomp);
/* The generic forms (B = 1), as abc_glm_weighted_dev and abc_glm_weighted. */
int abc_glm_weighted_summary_dev(const abc_glm* glm, const abc_summary* sum, abc_ctx* ctx, const double* theta, size_t ldv,
                                 const double* stats, size_t lds, size_t K, size_t P, size_t n, const double* obs, const double* w);
int abc_glm_weighted_summary(const abc_glm* glm, const abc_summary* sum, abc_ctx* ctx, const double* theta, const double* stats,
                             size_t K, size_t P, size_t n, const double* obs, const double* w);

/* ---- Box-Cox transform of the metrics: the skewness search and the transform (ABC::optimize_box_cox, AbcUtil.cpp:89-109) ---------
 * PLS is linear; simulated metrics (counts, sizes, durations) are positive and right-skewed.  The reference searches, per metric, a
 * grid of exponents for the lambda whose transform (x^lambda - 1) / lambda has the smallest |skewness| (its ranking carries the
 * call as a TODO, AbcUtil.cpp:430).  This is that search for every column of a table at once, and the transform.  It is a pre-pass:
 * transform the table AND the targets, then hand both to any ranking call; no other entry point changes.
 * All arrays are fp64; matrices are column-major with a leading dimension, as in abc_param_transf_dev.
 * Grid (abc_box_cox_grid): the reference's loop, quirks included.  The three float arguments are widened to double; then
 *   lambda_0 = min, lambda_{k+1} = lambda_k + step in fp64, for as long as lambda_k <= max.  So the defaults (-5, 5, 0.1f) give 100
 *   values, not 101 (the last is 4.9000001475...), and never hit 0 (lambda_50 = 7.45e-8), because (double)0.1f != 0.1; (-2, 2, 0.5f)
 *   gives 9 values and hits 0 exactly.  ABC_ERR_INVALID for a count outside 1..ABC_BOX_COX_MAXL, a step that is non-finite or <= 0,
 *   non-finite bounds, NULL L, and a grid with cap below the count (grid may be NULL: the count alone).  The search calls take any
 *   grid of finite values, this one or the caller's own.
 * Per column j, with the caller's shifts c_j (NULL: zeros): z_i = x_ij + c_j, l_i = log z_i, lbar the mean of l.  For a grid value:
 *   lambda != 0: t_i = exp(lambda (l_i - lbar));  lambda == 0: t_i = l_i - lbar;
 *   skew(lambda) = sgn(lambda) (sum (t - tbar)^3 / N) / (sum (t - tbar)^2 / (N - 1))^(3/2), sgn(0) = +1.
 *   This is the reference's quantity, skewness((x^lambda - 1) / lambda): skewness does not change under a positive affine map and
 *   flips sign under a negative one.  The form above is evaluated where it is well conditioned (the reference's own double formula
 *   loses everything on a column of 1000 +- 50 at the far lambda, where x^-5 - 1 cancels).  The kernels take l_i - lbar as
 *   v_i - vbar with v_i = log1p((z_i - z_min) / z_min), which keeps the differences of the logs of a narrow column to full relative
 *   precision, and sum the moments in one sweep about the pilot t = 1 (d = expm1(lambda (l - lbar))), centred at the end.
 * Pick: ascending k, strict |skew_k| < |best| starting from +inf; a non-finite skew is never taken; if none is finite the pick is
 *   0 (all the reference's behaviour).  lambda_j = grid[pick_j], best_skew_j = skew[j][pick_j].
 * Status bits per column:
 *   bit 0  some z_i is non-finite or <= 0: lambda_j = 1, pick_j = -1, every skew NaN.  DEVIATION: the reference would return
 *          lambda_min, a destructive transform
 *   bit 1  min == max, a constant column (N = 1 lands here): every skew 0, pick 0 (the reference's `_v == 0` rule)
 *   bit 2  some skew of the grid was non-finite (an overflow at the far lambda) and was skipped
 * Apply: y = expm1(lambda l) / lambda for lambda != 0, y = l for lambda == 0, with l = log(x + c) in IEEE arithmetic: z == 0 gives
 *   -1 / lambda (lambda > 0) or -inf, z < 0 or NaN gives NaN.  Elementwise: element (i, j) depends on x_ij, lambda_j and c_j only.
 *   out may be X itself (same pointer and ld); it must not overlap otherwise.
 * Bits: every reduction order depends on N only and no floating-point atomics are used, so a column's outputs are the same bits on
 *   a repeat run, alone (M = 1) and among other columns, for any ldx, through the device and the host entry, and whichever
 *   optional outputs are asked for.
 * ABC_ERR_INVALID, with a message naming the entry point, for N, n or M equal to 0, ld < rows, NULL X / grid / out / out->lambda /
 * lambda, L outside 1..ABC_BOX_COX_MAXL and a non-finite grid value, lambda or shift; ABC_ERR_UNSUPPORTED for N or n >= 2^32;
 * ABC_ERR_NOMEM from the workspace (3 N M L / 2048 doubles of partial sums).  Nothing is launched by a refused call.  Both search
 * calls synchronise; abc_box_cox_dev is stream-ordered like abc_param_transf_dev (its host arrays are read before it returns).
 * Cost: N x M x L exponentials, fp64 vector work; the search is compute-bound, unlike everything else here. */
enum { ABC_BOX_COX_MAXL = 512 };
typedef struct {            /* every member optional except lambda; device or host memory per the entry point */
    double*  lambda;        /* M */
    double*  best_skew;     /* M */
    double*  skew;          /* M x L row-major: [j][k] */
    int32_t* pick;          /* M */
    int32_t* status;        /* M */
} abc_box_cox_out;
enum { ABC_BOX_COX_BAD = 1, ABC_BOX_COX_CONSTANT = 2, ABC_BOX_COX_SKIPPED = 4 };
int abc_box_cox_grid(float lambda_min, float lambda_max, float step, double* grid, size_t cap, size_t* L);   /* host only */
/* X in device memory (X[i + ldx j]); shift (M, or NULL) and grid (L) in HOST memory; out's members in device memory. */
int abc_optimize_box_cox_dev(abc_ctx* ctx, const double* X, size_t ldx, size_t N, size_t M, const double* shift, const double* grid,
                             size_t L, const abc_box_cox_out* out);
/* HOST-pointer form: X is N x M column-major (ld = N); out's members in host memory. */
int abc_optimize_box_cox(abc_ctx* ctx, const double* X, size_t N, size_t M, const double* shift, const double* grid, size_t L,
                         const abc_box_cox_out* out);
/* The transform of an n x M matrix (X[i + ldx j] -> out[i + ldo j]) in device memory; lambda (M) and shift (M, or NULL) in HOST
 * memory.  A B x M block of targets is transformed by the same call with n = B. */
int abc_box_cox_dev(abc_ctx* ctx, const double* X, size_t ldx, size_t n, size_t M, const double* lambda, const double* shift, double* out,
                    size_t ldo);
int abc_box_cox(abc_ctx* ctx, const double* X, size_t n, size_t M, const double* lambda, const double* shift, double* out);   /* host pointers, ld = n */

/* ======================================================================================== */
/* Multi-GPU: rows (particles) sharded over several GPUs of one node             */
/* ======================================================================================== */
/* The reference has no multi-device path (its MPI farm distributes simulator calls, AbcMPI.cpp:28-143, and is compiled
 * out); this is the particle sharding BASELINE.json's north_star asks for.  One context per GPU; a communicator is attached
 * to each context and the sharded entry points below run the same protocol on every rank:
 *   all-gather of the ranks' sufficient-statistics records (<= 0.35 MB each, merged on every rank), all-gather of the ranks'
 *   sorted local-top lists with their parameter rows (merged on every rank: the K smallest of the whole set), all-gather of the
 *   per-rank weight slices; resampling / perturbation need no exchange.  Small sets, K > N / 2 and massively tied distances take
 *   the radix protocol instead of the lists: six all-reduces of a 2048-bin histogram (exact global K-th distance) and
 *   all-gathers of the per-rank winner lists and rows.
 * Communicators: RCCL over xGMI (one process per GPU: abc_comm_unique_id + abc_comm_init_rank; or one process driving
 * several GPUs: abc_ctx_create_multi), or collectives supplied by the caller (abc_comm_init_callbacks: any transport; used
 * by the tests to run two ranks over gloo on one GPU). */
#define ABC_COMM_ID_BYTES 128
enum { ABC_DT_F64 = 0, ABC_DT_I32 = 1, ABC_DT_I64 = 2 };
/* every callback works on DEVICE buffers, in stream order of `hip_stream`, and returns 0 on success */
typedef struct {
    int (*all_reduce_sum)(void* user, void* buf, size_t count, int dtype, void* hip_stream);
    int (*all_gather)(void* user, const void* send, void* recv, size_t bytes_per_rank, void* hip_stream);
    int (*broadcast)(void* user, void* buf, size_t bytes, int root, void* hip_stream);
    void* user;
} abc_comm_callbacks;
/* rank 0 creates the id and hands its 128 bytes to the other ranks (any channel), then every rank calls init_rank */
int abc_comm_unique_id(void* id128);
int abc_comm_init_rank(abc_ctx* ctx, int world, int rank, const void* id128);
int abc_comm_init_callbacks(abc_ctx* ctx, int world, int rank, const abc_comm_callbacks* cb);
int abc_comm_destroy(abc_ctx* ctx);
/* 0 = none, 1 = RCCL, 2 = callbacks; world and rank of the attached communicator (1, 0 without one) */
int abc_comm_info(const abc_ctx* ctx, int* kind, int* world, int* rank);
/* one process, ndev GPUs: creates ndev contexts (out[0..ndev)) joined by RCCL communicators (ncclCommInitAll); each is then
 * driven from its own host thread (abc_generation_multi below does that); destroy every context with abc_ctx_destroy */
int abc_ctx_create_multi(const int* devices, int ndev, abc_ctx** out);

/* One generation turn-over with the rows of the set sharded over the ranks of ctx's communicator (every rank calls this with
 * its shard; the call is collective).  Global row g of the set lives on the rank with row0 <= g < row0 + n_local; the next
 * set's particles [next0, next0 + nnext_local) are proposed by this rank.  io: X, Y are the LOCAL rows (leading dimension
 * n_local); idx / dist / theta / w / dv / L are replicated outputs (global row numbers in idx); next / parent / seeds
 * hold this rank's nnext_local proposals (leading dimension nnext_local).  rng: the same state on every rank; advanced by
 * the 2 Nnext_total draws of the whole generation.  Results equal abc_generation_dev on the unsharded set bit for bit
 * (indices, parents, seeds) and to rounding of the reduction order (statistics -> model -> distances within 1e-12) -- for the wide
 * sets that take the byte-limb statistics kernel (abc_ctx_set_gram_mode: 97..160 columns, or 81..96 with parameters from 2 000 000
 * rows, and 400 000 rows in every partition of the whole set) under ABC_GRAM_FP64 only: that kernel rounds every rank's values on
 * the rank's own grid; indices then agree up to near-ties, distances to ~1e-7. */
typedef struct {
    size_t n_local, row0, N_total;        /* this rank's rows of the current set                      */
    size_t M, P;
    size_t K, Kp;                         /* pred-prior size, previous pred-prior size (0 = set 0)    */
    size_t nnext_local, next0, Nnext_total;
    double train_frac;
    int32_t max_comp, rule, multivariate, reserved;
} abc_sharded_cfg;
int abc_generation_sharded_dev(abc_ctx* ctx, const abc_sharded_cfg* cfg, const abc_generation_io* io, abc_rng* rng,
                               int32_t* ncomp_host);

/* HOST-pointer generation over the ndev contexts of abc_ctx_create_multi: splits the N rows into contiguous shards, uploads
 * them, runs abc_generation_sharded_dev on one host thread per GPU and collects the outputs.  Same argument meaning as
 * abc_generation_cfg / abc_generation_io with HOST pointers (X: N x M, Y: N x P, next: Nnext x P, column-major). */
int abc_generation_multi(abc_ctx* const* ctxs, int ndev, const abc_generation_cfg* cfg, const abc_generation_io* host_io,
                         abc_rng* rng, int32_t* ncomp);

#ifdef __cplusplus
}
#endif
#endif /* ABCSMC_HIP_H */
