// Internal declarations shared by the HIP translation units of libabcsmc_hip.so.
// gfx950 (MI355X, wave64) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/abcsmc_hip.h"

#define ABC_WAVE 64

// Diagnostic switches (include/abcsmc_hip.h, "Diagnostic environment switches"): an environment variable steers the library
// ONLY when ABC_DIAG=1 is set beside it -- a production process that happens to inherit ABC_WS_POISON or ABC_ALIAS_FORCE_FAIL
// from somebody's shell is not affected.  Every getenv of the library goes through here.
inline const char* abc_diag_env(const char* name) {
    static const bool on = [] { const char* d = getenv("ABC_DIAG"); return d && d[0] == '1'; }();
    return on ? getenv(name) : nullptr;
}

// The context's pinned, device-visible status block (ctx->status_pin).  A generation's status words go here: into pinned memory
// the small copies at its end are queued back to back behind ONE synchronisation; into pageable memory each one is a blocking
// round trip (17 + 50 us of gaps at the end of a generation, rocprofv3 timeline).  Kernels receive the members' addresses.
struct abc_wx_words {              // the Wilcoxon cascade's words (wilcoxon.hip); the kernels index them as pin_words[0..7]
    int left;                      // [0] tests left after a level: k_wx_bounds' last work-group, the host spins on it (preset to -1)
    int vmax_lo, vmax_hi;          // [1] [2] k_wx_bounds: the largest validation-row count of a rank, 31 bits each
    int ncomp;                     // [3] k_wx_bounds / k_wx_decide: the final component count
    int changed;                   // [4] ... and whether it differs from the fit's
    int decided;                   // [5] k_wx_bounds: the cascade needs no further level
    int n_rest;                    // [6] k_wx_bounds of the first half: the tests outside it
    int n_level;                   // [7] k_wx_bounds: the tests of this level's list
};
struct abc_status_block {
    double model_hdr[4];           // the model header (component count first): k_post_tail or k_status_words
    int spd;                       // Cholesky status
    int sel_fail;                  // the bin selection gave up (k_status_words, or the host from gather_sel_fail)
    int gather_sel_fail;           // ... as the gather behind the selection stores it
    int alias_fail;                // the device build of the resampling table did not verify (alias_dev.hip)
    unsigned long long giveups;    // the proposals' give-up counter, read back at a generation's end
    unsigned giveup_flag;          // raised by a proposal kernel that gives up (note_giveup, resample.hip)
    int spare;
    abc_wx_words wx;
    int repeat_sel_fail;           // the repeated selection's give-up flag (the first gather may still be writing gather_sel_fail)
};
static_assert(offsetof(abc_status_block, model_hdr) == 0 && offsetof(abc_status_block, spd) == 32 &&
              offsetof(abc_status_block, sel_fail) == 36 && offsetof(abc_status_block, gather_sel_fail) == 40 &&
              offsetof(abc_status_block, alias_fail) == 44 && offsetof(abc_status_block, giveups) == 48 &&
              offsetof(abc_status_block, giveup_flag) == 56 && offsetof(abc_status_block, wx) == 64 &&
              offsetof(abc_status_block, repeat_sel_fail) == 96, "status block layout");
static_assert(sizeof(abc_wx_words) == 8 * sizeof(int) && offsetof(abc_wx_words, n_level) == 7 * sizeof(int), "cascade words");
static_assert(sizeof(abc_status_block) <= 128, "status block size");

// timed stages (abc_timing_names in api.hip must match)
enum { ST_GRAM = 0, ST_STATS_REDUCE, ST_PLS_MODEL, ST_PROJECT, ST_SELECT, ST_SORT, ST_GATHER_DV, ST_KDE,
       ST_WEIGHTS_MISC, ST_MVN, ST_ALIAS_HOST, ST_RESAMPLE, ST_PERTURB, ST_COMM, ABC_NSTAGE };

struct abc_ctx {
    int device;
    hipStream_t stream;
    hipStream_t own_stream;
    char err[512];
    // device workspace arena (bump allocator, reset per API call)
    char* ws;
    size_t ws_bytes;
    size_t ws_off;
    size_t ws_asked;       // bytes the entry point passed to the last abc_ws_reserve, before the rounding (abc_ws_info)
    size_t ws_peak;        // largest ws_off an abc_ws_alloc has reached since then: the hand rewinds of ws_off do not lower it
    // pinned host scratch
    char* pin;
    size_t pin_bytes;
    abc_status_block* status_pin;      // pinned (above)
    // cached alias table (device) for the last weights vector handed to abc_resample_dev
    double* alias_F;
    uint32_t* alias_A;
    size_t alias_K;
    // alias table of K equal weights 1/K (set 0, AbcUtil.cpp:539-545): built once per K, kept (abc_uniform_alias)
    double* ualias_F;
    uint32_t* ualias_A;
    size_t ualias_cap, ualias_K;
    char* ualias_pin;      // its own pinned staging (the upload is asynchronous: the shared scratch may be reused before it ran)
    hipEvent_t ev_copy;    // marks the end of the weights' device-to-host copy (the host waits on it, not on the stream)
    // side stream of the fused drivers: the two taus2 streams of a generation (draws, seeds) depend on the rng state alone and
    // run there from the first launch on, beside the ranking chain (abc_rng_streams_early); ev_fork / ev_side order them
    hipStream_t side;
    hipStream_t wx_stream;             // the Wilcoxon reduction of a fused generation, beside the ranking that speculates on its outcome
    hipEvent_t ev_wx_fork, ev_wx_done, ev_wx_scores;
    hipEvent_t ev_fork, ev_side, ev_prev;
    hipEvent_t ev_theta, ev_moments;   // the posterior's moments on the side stream: start (rows gathered) and end
    bool side_forked;      // ev_fork of the current generation is recorded (abc_side_fork); cleared when the generation ends
    bool side_early_waited; // the main stream already waits for everything queued early on the side stream (ev_prev implies ev_side)
    // jump-ahead matrices for taus2 (device), built once
    uint32_t* jump_tab;
    // optional per-stage timing with HIP events recorded on ctx->stream (abc_timing_*)
    int timing;            // 0 off, 1 every stage, 2 only the two kernel brackets bench.py's roofline needs (k_gram, k_kde)
    int kde_mode;  // ABC_KDE_AUTO / ABC_KDE_FP64
    int gram_mode; // ABC_GRAM_AUTO / ABC_GRAM_FP64 (abc_ctx_set_gram_mode)
    int noise_mode;  // ABC_NOISE_DEVICE / ABC_NOISE_REFERENCE_STREAM
    int weight_kernel;  // ABC_WEIGHT_GAUSSIAN / ABC_WEIGHT_EPANECHNIKOV
    int alias_mode;     // ABC_ALIAS_DEVICE (default) / ABC_ALIAS_HOST
    int* alias_fail_dev;               // device flag of the last device build
    unsigned long long alias_dev_builds, alias_dev_fallbacks;   // device builds queued / found unusable (abc_alias_stats)
    unsigned long long* giveups_dev;   // proposals the perturbation gave up on (device counter, abc_perturb_giveups)
    unsigned long long giveups_host;   // ... and in the reference-stream host loop
    unsigned long long giveups_seen;   // device counter as of the last generation's end
    unsigned long long giveups_last_call;   // what the most recent generation added to it (abc_generation_giveups)
    unsigned long long giveups_dev_known;   // the device counter as the host last read it (re-read only when the pinned flag word says it moved)
    int timers_open;                   // StageTimers between their two events (the ring is only drained when none is)
    unsigned long long timing_dropped; // samples that found the ring full while a timer was open (abc_timing_read reports them)
    int* kde_which;  // device: which weight kernel produced the last sums (ABC_KDE_RAN_*), written by k_wfinish
    int* sel_fail_dev;       // device: the sampled-range bin selection gave up (select.hip); read by abc_select_check
    bool sel_bins_ran;       // the last launch_select_smallest took the bin path and has not been checked yet
    bool sel_force_radix;    // set by a caller that repeats its work after a failed bin selection
    unsigned long long sel_bin_selections, sel_bin_giveups;   // bin selections queued / found failed by launch_select_smallest's own check (abc_select_stats)
    unsigned long long targets_fallbacks;   // targets of abc_rank_targets_dev that took the exact single-target path
    // parameter transforms of the local-linear adjustment (abc_ctx_set_param_transf): one device allocation [lo | hi | kind] of tf_P
    // entries each, NULL / 0 while nothing is set; the forward passes' out-of-domain counter (device, abc_param_transf_outside)
    char* tf_buf;
    size_t tf_P;
    unsigned long long* tf_outside_dev;
    // heteroscedastic variance correction of the local-linear adjustment (abc_ctx_set_adjust_hcorr): the second fit of the last
    // regressing call made under it (device, hc_cap doubles, allocated and grown only while the setting is on; hc_slots x hc_a1 x
    // hc_P of it are the record, 0 while there is none) and the skip rule's counter (device, abc_adjust_hcorr_skipped)
    int hcorr;
    double* hc_buf;
    size_t hc_cap, hc_slots, hc_a1, hc_P;
    unsigned long long* hc_skipped_dev;
    // ridge adjustment (abc_ctx_set_adjust_ridge): the penalties (rg_L == 0: off), the record of the last regressing call made
    // under it (device; rg_pick rg_slots x rg_P, rg_press rg_slots x rg_Lrec x rg_P; allocated and grown only while the setting is on,
    // the counts 0 while there is none) and the counter of unscored pairs (device, abc_adjust_ridge_unscored)
    double rg_lambda[ABC_RIDGE_MAXL];
    size_t rg_L;
    int32_t* rg_pick;
    double* rg_press;
    size_t rg_cap_pick, rg_cap_press, rg_slots, rg_Lrec, rg_P;
    unsigned long long* rg_unscored_dev;
    // row importance weights of the batched ranking (abc_ctx_set_row_weights): the context's own copy of the rw_N weights (device;
    // rw_N == 0: off), the number of positive ones and (sum w)^2 / sum w^2, from the check made when they were set
    double* rw_dev;
    size_t rw_N, rw_pos;
    double rw_ess;
    unsigned long long wx_moved_counts, generation_repeats;      // abc_generation_repeats
    bool wx_gather_rows;     // diagnostic (ABC_DIAG=1 ABC_WX_GATHER=1, set at context creation): the sharded generation's Wilcoxon rule by
                             // gathering the validation rows on every rank (rounds 1-4) instead of the sharded cascade
    // the per-test record of the last Wilcoxon reduction (abc_ctx_set_wx_record / abc_wx_last_record): a device allocation of the
    // context, [256 bytes: tests, path | abc_wx_test_record x wx_rec_cap], NULL until a reduction runs with the switch on
    int wx_record;
    char* wx_rec_dev;
    size_t wx_rec_cap;
    bool wx_rec_valid;       // a reduction has written it since the switch went on
    bool in_mvn;   // the covariance pass reuses k_gram: keep it out of the k_gram stage timer
    int nev;
    struct { hipEvent_t a, b; int stage; } ev[256];
    // communicator of the row-sharded generation (sharded.hip): none, RCCL or caller-supplied collectives
    int comm_kind;            // 0 = none (world 1), 1 = RCCL, 2 = callbacks
    int comm_world, comm_rank;
    void* comm_nccl;          // ncclComm_t
    abc_comm_callbacks comm_cb;
    char* xbuf;               // exchange buffers of the sharded generation (winner lists, packed posterior rows), grown on demand
    size_t xbuf_bytes;
    double stage_ms[ABC_NSTAGE];
    double stage_host_ms[ABC_NSTAGE];
    long long stage_cnt[ABC_NSTAGE];
};

int abc_timing_flush(abc_ctx* ctx);
// Flags of the events that order the context's two streams: GPU-to-GPU dependencies on one device, so a device-scope release is
// enough (the default, system scope, also makes the writes visible to the host: more cache maintenance per record)
inline unsigned abc_xstream_event_flags() {
    return hipEventDisableTiming | hipEventReleaseToDevice;
}
// RAII marker: records an event pair around a stage when timing is on
struct StageTimer {
    abc_ctx* ctx; int slot;
    StageTimer(abc_ctx* c, int stage) : ctx(c), slot(-1) {
        if (!c->timing || stage < 0) return;
        if (c->timing == 2 && stage != ST_GRAM && stage != ST_KDE) return;
        // ring full: drain it (a stream synchronisation) unless an enclosing timer is still open -- then the sample is lost,
        // counted, and abc_timing_read says so instead of handing out a short sum
        if (c->nev >= 256) {
            if (c->timers_open == 0) (void)abc_timing_flush(c);
            if (c->nev >= 256) { c->timing_dropped++; return; }
        }
        c->timers_open++;
        slot = c->nev++;
        if (!c->ev[slot].a) { (void)hipEventCreate(&c->ev[slot].a); (void)hipEventCreate(&c->ev[slot].b); }
        c->ev[slot].stage = stage;
        (void)hipEventRecord(c->ev[slot].a, c->stream);
    }
    ~StageTimer() { if (slot >= 0) { (void)hipEventRecord(ctx->ev[slot].b, ctx->stream); ctx->timers_open--; } }
};

#define ABC_FAIL(ctx, code, ...)                                   \
    do {                                                           \
        snprintf((ctx)->err, sizeof((ctx)->err), __VA_ARGS__);     \
        return (code);                                             \
    } while (0)

#define ABC_HIP(ctx, call)                                                            \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess)                                                         \
            ABC_FAIL(ctx, ABC_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #call,   \
                     hipGetErrorString(e_));                                          \
    } while (0)

#define ABC_TRY(expr)                  \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != ABC_OK) return rc_; \
    } while (0)

// Scoped stream switch: the launchers queue on the context's stream, so work for another stream (side, cascade) is queued with
// that stream installed; the previous one is back when the scope ends, whichever way it is left
struct StreamScope {
    abc_ctx* ctx; hipStream_t prev;
    StreamScope(abc_ctx* c, hipStream_t s) : ctx(c), prev(c->stream) { c->stream = s; }
    ~StreamScope() { ctx->stream = prev; }
    StreamScope(const StreamScope&) = delete;
    StreamScope& operator=(const StreamScope&) = delete;
};

// ---- workspace ------------------------------------------------------------------------
int abc_ws_reserve(abc_ctx* ctx, size_t bytes);           // may reallocate; resets the arena
void* abc_ws_alloc(abc_ctx* ctx, size_t bytes);           // 256-B aligned bump; NULL if exhausted
int abc_pin_reserve(abc_ctx* ctx, size_t bytes);

static inline size_t abc_align(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- stats record layout (see abc_stats_len in the public header) ----------------------
struct StatsLayout {
    size_t C16;        // padded column count (multiple of 16)
    size_t off_n;      // 2 doubles: n_train, n_test
    size_t off_shift;  // C16
    size_t off_sum[2]; // C16 each
    size_t off_G[2];   // C16*C16 each, column-major, symmetric
    size_t len;
};
__host__ __device__ static inline StatsLayout stats_layout(size_t M, size_t P) {
    StatsLayout s;
    s.C16 = (M + P + 15) / 16 * 16;
    s.off_n = 0;
    s.off_shift = 2;
    s.off_sum[0] = s.off_shift + s.C16;
    s.off_sum[1] = s.off_sum[0] + s.C16;
    s.off_G[0] = s.off_sum[1] + s.C16;
    s.off_G[1] = s.off_G[0] + s.C16 * s.C16;
    s.len = s.off_G[1] + s.C16 * s.C16;
    return s;
}

// ---- model record layout ---------------------------------------------------------------
// [ ncomp, A, n_total, pad, mean[M+P], sd[M+P], zobs[M], obs_scores[A], R[M*A], Q[P*A], W[M*A],
//   Pl[M*A], H[A*A], press[A*P], per_response[P] ]
// H = R' (X'X of the z-scored validation rows) R: the second moments of the validation scores, a by-product of PRESS (round 5: the
// Wilcoxon reduction takes the scale of every test's paired differences from it, wilcoxon.hip)
struct ModelLayout {
    size_t off_hdr, off_mean, off_sd, off_zobs, off_oscore, off_R, off_Q, off_W, off_P, off_H, off_press,
        off_per, len;
};
__host__ __device__ static inline ModelLayout model_layout(size_t M, size_t P, size_t A) {
    ModelLayout m;
    m.off_hdr = 0;
    m.off_mean = 4;
    m.off_sd = m.off_mean + M + P;
    m.off_zobs = m.off_sd + M + P;
    m.off_oscore = m.off_zobs + M;
    m.off_R = m.off_oscore + A;
    m.off_Q = m.off_R + M * A;
    m.off_W = m.off_Q + P * A;
    m.off_P = m.off_W + M * A;
    m.off_H = m.off_P + M * A;
    m.off_press = m.off_H + A * A;
    m.off_per = m.off_press + A * P;
    m.len = m.off_per + P;
    return m;
}

// ---- stage launchers (each in its own .hip file) ---------------------------------------
int launch_stats_shift(abc_ctx*, const double* X, const double* Y, size_t n, size_t ldx, size_t ldy,
                       size_t M, size_t P, double* stats);
// n_set (0: n): the rows of the WHOLE set these n are a shard of -- the choice between the i8 and the fp64 kernel of wide sets is
// made from it, so that all ranks of a sharded generation and the unsharded run agree (abc_ctx_set_gram_mode)
bool abc_gram_takes_i8(const abc_ctx*, const double* X, const double* Y, size_t n, size_t ldx, size_t ldy, size_t M, size_t P,
                       uint64_t n_train_global, size_t n_set);     // the byte-limb statistics kernel for this set? (gram.hip)
int launch_stats_accumulate(abc_ctx*, const double* X, const double* Y, size_t n, size_t ldx,
                            size_t ldy, size_t M, size_t P, uint64_t row0, uint64_t n_train_global,
                            double* stats, size_t n_set = 0);
int launch_pls_model(abc_ctx*, const double* stats, const double* obs, size_t M, size_t P, size_t A,
                     int rule, double* model, hipEvent_t done = nullptr);
int launch_simple_model(abc_ctx*, const double* stats, const double* obs, size_t M, size_t P,
                        double* model);
int launch_project_distance(abc_ctx*, const double* X, size_t n, size_t ldx, size_t M, size_t P,
                            size_t A, const double* model, int simple, double* dist);
// scores of n rows (all A components) by the projection kernels: S[i + n k]; returns the rows taken (an even count, 0: not their shape)
size_t launch_project_scores(abc_ctx*, const double* X, size_t n, size_t ldx, size_t M, size_t P, size_t A, const double* model, double* S);
// the ranking's projection and the validation scores (rows from row_test on: S[i - row_test + sld k]) in one pass over X;
// 0: queued, 1: not a shape for it, nothing queued
int launch_project_distance_scores(abc_ctx*, const double* X, size_t n, size_t ldx, size_t M, size_t P, size_t A, const double* model,
                                   double* dist, double* S, size_t sld, size_t row_test, hipEvent_t done);
// the distances again from the scores of all rows that pass has left (S[i + sld k], row_test = 0): a repeat of the ranking on a
// lowered component count (model[0]) without a second pass over X
int launch_distance_from_scores(abc_ctx*, const double* S, size_t n, size_t sld, size_t M, size_t P, size_t A, const double* model, double* dist);
// batched ranking of B targets against one fitted model (targets.hip); any_excl: exclude is given and names a row for some target
size_t abc_targets_need(size_t N, size_t A, size_t B, size_t K, bool any_excl);
// keep (optional): where the ranking left the scores of every row (S[i + sld k], all A components) and the targets' scores
// (O[b KCO + k], 0 for k >= ncomp); both stay in the arena after the return, below the caller's next allocation
struct abc_tg_scores { const double* S; size_t sld; const double* O; int KCO; };
int launch_rank_targets(abc_ctx*, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M, size_t P,
                        const double* model, size_t A, const double* targets, size_t ldt, size_t B, const uint64_t* exclude,
                        bool any_excl, size_t K, uint64_t* idx, double* dist, double* post_mean, abc_tg_scores* keep = nullptr,
                        const double* om = nullptr);
// om (optional, here and below): the context's row importance weights (N, device): post_mean, the regression's weights and what
// follows from them take the RW instances of their kernels; idx and dist never depend on it
// the check of row weights (targets.hip): out4 (device) = bad entries, positive entries, sum, sum of squares
int launch_row_weights_check(abc_ctx*, const double* w_dev, size_t N, double* out4_dev);
// local-linear adjustment of the batched ranking (adjust.hip): the ranking of launch_rank_targets, then the regression of every
// target's K retained rows on their scores; out: device pointers (abc_adjust_out), dist may be NULL
size_t abc_adjust_need(size_t N, size_t A, size_t P, size_t B, size_t K, bool hcorr = false, size_t ridge = 0);
int launch_rank_targets_adjust(abc_ctx*, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M, size_t P,
                               const double* model, size_t A, const double* targets, size_t ldt, size_t B, const uint64_t* exclude,
                               bool any_excl, size_t K, int kernel, uint64_t* idx, double* dist, const abc_adjust_out* out,
                               struct abc_adj_keep* keep = nullptr, const struct AbcTf* tf = nullptr,
                               const struct AbcHc* hc = nullptr, const struct AbcRg* rg = nullptr, const double* om = nullptr);
// tf (optional, transf_dev.h): Y is already forward(Y) (launch_param_transf); theta and keep's readers carry the adjusted rows back
// hc (optional, adjust_dev.h): the heteroscedastic variance correction, its second fit written to hc->hcoef (B, or B x T on a path,
// slots laid out as coef); the *_need functions count its moment blocks with hcorr = true
// rg (optional, adjust_dev.h): the ridge adjustment, coef replaced by the fit of the penalty with the smallest leave-one-out PRESS,
// pick and press written to rg's buffers (slots as hc's); the *_need functions count its arena pieces with ridge = L
// tolerance path (adjust.hip): the ranking at K = path->Ks[T - 1], then the rejection mean and the regression at every tolerance;
// path: Ks in host memory, the outputs device pointers; dist may be NULL.  keep (optional): the fit is made whatever outputs path
// names, and keep receives what a reader of the adjusted rows needs, with coef B x T x (A + 1) x P and dist B x K_max
size_t abc_path_need(size_t N, size_t A, size_t P, size_t B, size_t K, size_t T, bool hcorr = false, size_t ridge = 0);
int launch_rank_targets_path(abc_ctx*, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M, size_t P,
                             const double* model, size_t A, const double* targets, size_t ldt, size_t B, const uint64_t* exclude,
                             bool any_excl, int kernel, uint64_t* idx, double* dist, const abc_path* path,
                             struct abc_adj_keep* keep = nullptr, const double* Yt = nullptr, const struct AbcTf* tf = nullptr,
                             const struct AbcHc* hc = nullptr, const struct AbcRg* rg = nullptr, const double* om = nullptr);
// Yt / tf (optional, both or neither): forward(Y) as N x P with ld = N, which the fit reads; post_mean stays the mean of the raw Y.
// launch_param_transf: the context's parameter transforms over a column-major n x P matrix (adjust.hip: k_tf_apply); tf NULL: a copy; in place is
// allowed; outside (optional, device): a forward pass adds the entries of transformed columns it found outside their domain
int launch_param_transf(abc_ctx*, const struct AbcTf* tf, const double* V, size_t ldv, size_t n, size_t P, int inverse, double* out,
                        size_t ldo, unsigned long long* outside);
// Box-Cox transform of the metrics (boxcox.hip).  Search: shift (M, or NULL) and grid (L) in device memory, out's members device
// pointers (lambda required); abc_box_cox_need: its arena pieces.  Apply: lambda (M) and shift (M, or NULL) in device memory; in
// place is allowed.  The callers have checked the sizes.
size_t abc_box_cox_need(size_t N, size_t M, size_t L);
int launch_box_cox_search(abc_ctx*, const double* X, size_t ldx, size_t N, size_t M, const double* shift, const double* grid, size_t L,
                          const abc_box_cox_out* out);
int launch_box_cox_apply(abc_ctx*, const double* X, size_t ldx, size_t n, size_t M, const double* lambda, const double* shift, double* out,
                         size_t ldo);
// weighted posterior quantiles and CDF (summary.hip).  abc_summary_need: workspace of launch_summary for B segment groups of P
// segments of K values.  SmValues: how the values and weights of segment (b, j) are made (method 0 / 1: the ranking's rows,
// method 2: V and w); sum: probs in host memory, truth / quant / cdf in device memory.
struct SmValues {
    int method;                  // 0 rejection, 1 loclinear, 2 generic
    const uint64_t* idx;         // B x K (methods 0 and 1)
    const double* Y;             // method 0: Y[i + ldy j]
    size_t ldy;
    const struct abc_adj_keep* adj;  // method 1
    int A;
    int kernel;
    const double* V;             // method 2: V[e + ldv j], w[e] (NULL: 1)
    size_t ldv;
    const double* w;
    const double* om;            // methods 0 and 1: the row importance weights (N, device; NULL: none), entry e weighs k_e om[idx[e]]
};
size_t abc_summary_need(size_t B, size_t K, size_t P);
int launch_summary(abc_ctx*, const SmValues& sv, size_t B, size_t K, size_t P, const abc_summary* sum);
// the summaries at every tolerance of a path (Ks: T ascending tolerances, host): sv describes the ranking at K_max = Ks[T - 1] (idx
// and, method 1, adj->dist with that row stride; adj->coef B x T x (A + 1) x P); quant B x T x nq x P, cdf B x T x P, truth B x P
size_t abc_path_summary_need(size_t B, const size_t* Ks, size_t T, size_t P, int method);
int launch_path_summary(abc_ctx*, const SmValues& sv, size_t B, const size_t* Ks, size_t T, size_t P, const abc_summary* sum);
// generic weights (device): ABC_ERR_INVALID when one is negative or non-finite or all are zero (synchronises)
int abc_summary_check_weights(abc_ctx*, const double* w, size_t K, const char* fn);
// weighted posterior densities and modes (density.hip) of the same segments: the quantiles it needs come from launch_summary.
// abc_density_need: workspace of launch_density (launch_summary's included); dn: every array in device memory; a given
// bandwidth that is not finite and positive is ABC_ERR_INVALID (checked on the device: synchronises)
size_t abc_density_need(size_t B, size_t K, size_t P, size_t G);
int launch_density(abc_ctx*, const SmValues& sv, size_t B, size_t K, size_t P, const abc_density* dn, const char* fn);
// the first half of launch_density, shared with the pair densities: the bandwidth check, the quantiles and k_dn_moments.  *segs:
// B x P records (density_dev.h) in the workspace; grid and bw_out of dn are written when given, its other outputs are not touched.
struct DnSeg;
size_t abc_density_segs_need(size_t B, size_t K, size_t P);
int launch_density_segs(abc_ctx*, const SmValues& sv, size_t B, size_t K, size_t P, const abc_density* dn, const DnSeg** segs,
                        const char* fn);
// joint posterior of the same segments (joint.hip): means, covariances, correlations, pair densities and joint modes.  npairs: the
// pairs of the request (jt->npairs, or P (P - 1) / 2 when jt->pairs is NULL); jt: pairs in host memory, every other array in device
// memory; a given bandwidth is checked as launch_density's
size_t abc_joint_pairs(const abc_joint* jt, size_t P);
size_t abc_joint_need(size_t B, size_t K, size_t P, size_t G, size_t npairs);
int launch_joint(abc_ctx*, const SmValues& sv, size_t B, size_t K, size_t P, const abc_joint* jt, const char* fn);
// posterior draws of the same segments (draws.hip): the weighted bootstrap, smoothed by the marginal densities' bandwidths on
// request (launch_density_segs's records).  dr: stream in host memory, every other array in device memory; a given bandwidth is
// checked as launch_density's
size_t abc_draws_need(size_t B, size_t K, size_t P, int smooth);
int launch_draws(abc_ctx*, const SmValues& sv, size_t B, size_t K, size_t P, const abc_draws* dr, const char* fn);
// posterior entropy of the same segments (entropy.hip): the k-nearest-neighbour estimate over a target's entries, whose weights are
// all equal (the entries refuse the rest).  en: scale in host memory, every other array in device memory
size_t abc_entropy_need(size_t B, size_t K, size_t P);
int launch_entropy(abc_ctx*, const SmValues& sv, size_t B, size_t K, size_t P, const abc_entropy* en, const char* fn);
// highest-density intervals of the same segments (summary.hip): the summary's sort and knots, then the shortest interval of every
// mass.  hd: mass in host memory, every other array in device memory
size_t abc_hpd_need(size_t B, size_t K, size_t P);
int launch_hpd(abc_ctx*, const SmValues& sv, size_t B, size_t K, size_t P, const abc_hpd* hd);
// ABC-GLM posterior (glm.hip) of B retained samples of K rows: the scores S[i + sld k] (n of them), the parameters Y[i + ldy j] and
// the row of entry e of target b, idx[b K + e] (NULL: e itself, B = 1); weights om[i] or w[e] (one of them at most, NULL: 1); the
// observed scores O[b KCO + k].  sv: the parameters' values and weights as launch_density_segs reads them (the bandwidths).
// nA >= n: the bound abc_glm_need was asked with (A of the model).  glm: every array in device memory, checked by the caller
// sum: NULL, or the exact quantiles and CDF of the marginal mixtures (the *_summary entries; abc_glm_need's sum says which)
size_t abc_glm_need(size_t B, size_t K, size_t P, size_t nA, size_t G, bool sum = false);
int launch_glm(abc_ctx*, const SmValues& sv, const double* S, size_t sld, const double* Y, size_t ldy, const uint64_t* idx,
               const double* om, const double* w, const double* O, int KCO, size_t B, size_t K, size_t P, size_t n, size_t nA,
               const abc_glm* glm, const abc_summary* sum, const char* fn);
int launch_select_smallest(abc_ctx*, const double* dist, size_t n, size_t K, uint64_t idx_base,
                           uint64_t* idx, double* dist_out, bool defer_check = false);
int abc_select_check(abc_ctx* ctx, int* failed);
// the same in two halves for a caller with its own synchronisation: queue the flag's copy into *slot (pinned), then, after the
// synchronisation, abc_select_check_done reads it
int abc_select_check_queue(abc_ctx* ctx, int* slot);
int abc_select_check_done(abc_ctx* ctx, const int* slot);
// the weight stage's plan and its column slices (abc_kde_slices; shared with the workspace sizing in api.hip)
#include "weights_plan.h"
// osrc (optional): for every output position the flat input position q * len + i it came from
int launch_merge_runs(abc_ctx* ctx, const double* key, const uint64_t* idx, int W, size_t len, double* okey, uint64_t* oidx,
                      uint64_t* osrc = nullptr);
int launch_sort_pairs(abc_ctx*, double* key, uint64_t* idx, size_t n);
// distributed radix select stages (state: 8 x int64, hist: 2048 x int32, all-reduced by the caller between hist and pick)
int launch_select_begin(abc_ctx*, uint64_t K, long long* state, int* hist);
int launch_select_hist(abc_ctx*, const double* dist, size_t n, const long long* state, int pass, int* hist);
int launch_select_pick(abc_ctx*, long long* state, int pass, int* hist, uint64_t K);
int launch_select_count(abc_ctx*, const double* dist, size_t n, const long long* state, long long* counts);
int launch_select_compact(abc_ctx*, const double* dist, size_t n, const long long* state, uint64_t n_less,
                          uint64_t ties_take, uint64_t idx_base, uint64_t* idx_out, double* dist_out);
int abc_sort_u64_bytes(abc_ctx*, unsigned long long* key0, unsigned long long* val0, unsigned long long* key1,
                       unsigned long long* val1, size_t n, int byte_lo, int byte_hi);
// Wilcoxon reduction of the per-response component counts (rule ABC_RULE_WILCOXON); test rows = [row_test, n).
// sh (row-sharded sets, sharded.hip): X / Y are THIS rank's rows; the counts of every level of the bounds cascade are all-reduced
// over the context's communicator, the keys of the tests the bounds leave undecided are all-gathered (wilcoxon.hip).  Returns
// ABC_INTERNAL_RETRY when the set is not one the cascade takes (abc_wx_cascade_applies) or a bin of its exact step outgrew LDS:
// the caller then gathers the validation rows and calls again without sh.
struct abc_wx_shard {
    size_t nv_total;          // validation rows of the whole set
    const double* nv_ranks;   // device: nv_ranks[q * nv_stride] = validation rows of rank q (the n_test word of its statistics record)
    size_t nv_stride;
};
bool abc_wx_cascade_applies(size_t nv_total, size_t P, size_t A);
// dec / changed_host (the fused generation's SPECULATIVE run, api.hip): with dec != NULL the cascade leaves the model record as the
// fit wrote it and puts its decision into dec (P per-response counts, then the largest); *changed_host = 0: the largest count is
// the fit's (everything ranked with it stands), 1: it differs (launch_wilcoxon_commit, rank again), 2: the reduction took a path
// that rewrote the model record itself (small sets, the sorted-path repeat): rank again.
int launch_wilcoxon(abc_ctx*, const double* X, const double* Y, size_t n, size_t ldx, size_t ldy, size_t M, size_t P,
                    size_t A, size_t row_test, double* model, const abc_wx_shard* sh = nullptr, double* dec = nullptr,
                    int* changed_host = nullptr, int stop_at_max = 0);
// stop_at_max (the generations: their caller only uses the LARGEST per-response count, AbcUtil.cpp:449): the cascade ends as soon as
// that is certain; the per-response counts it leaves are then upper ends for the responses it did not finish
int launch_wilcoxon_commit(abc_ctx*, double* model, size_t M, size_t P, size_t A, const double* dec, int with_hdr);
// the cascade in two halves, for a caller with work to queue between them (the fused generation: api.hip)
struct abc_wx_run;
// scores: the caller has a pass over X of its own to queue (the ranking's projection) and lets it write the validation scores
// too: fn(arg, &S, &sld) queues that pass, makes the context's (= the cascade's) stream wait for it, says where the validation rows'
// scores are (S[i + sld k], row i of the validation rows: the caller's own buffer -- round 6: the generation keeps the scores of ALL
// rows, so that a moved count repeats the distances from them instead of from X) and returns 0 -- or returns 1 without queueing
// anything, and the cascade scores the rows itself into a buffer of its own
struct abc_wx_scores_hook { int (*fn)(void* arg, double** S, size_t* sld); void* arg; };
int launch_wilcoxon_begin(abc_ctx*, const double* X, const double* Y, size_t n, size_t ldx, size_t ldy, size_t M, size_t P, size_t A,
                          size_t row_test, double* model, double* dec, int stop_at_max, abc_wx_run** out,
                          const abc_wx_scores_hook* scores = nullptr, int hold_level0 = 0, const abc_wx_shard* sh = nullptr);
// sh: the rows are a shard of a row-sharded set (the counts of every level are all-reduced over the context's communicator)
// hold_level0: begin stops in front of level 0's sweep; the caller queues it (on the cascade's stream) once its own launches are out
int launch_wilcoxon_level0(abc_ctx*, abc_wx_run* run);
int launch_wilcoxon_finish(abc_ctx*, abc_wx_run* run, int* changed_host);
void launch_wilcoxon_abandon(abc_ctx*, abc_wx_run* run, hipStream_t its_stream);
// collectives on the context's stream and the exchange buffer (sharded.hip)
int abc_comm_all_reduce(abc_ctx* ctx, void* buf, size_t count, int dtype);
int abc_comm_all_gather(abc_ctx* ctx, const void* send, void* recv, size_t bytes);
int abc_xbuf_reserve(abc_ctx* ctx, size_t bytes);
// sel_fail / sel_fail_pin (fused drivers): the bin selection's give-up flag is stored into the pinned status block by this
// kernel, and the proposals' give-up counter is snapshotted into its second slot.  done: an event bound to the kernel's OWN
// completion signal (hipExtLaunchKernelGGL's stop event) -- a hipEventRecord behind it is one more packet in the queue, and the
// next kernel waits for that packet: ~7 us of the main stream's critical path per record (rocprofv3 timeline)
int abc_giveups_ensure(abc_ctx* ctx);
int launch_gather_rows(abc_ctx*, const double* Y, size_t n_local, size_t ldy, size_t P,
                       const uint64_t* idx, size_t K, uint64_t idx_base, double* theta, size_t ldt,
                       const int* sel_fail = nullptr, int* sel_fail_pin = nullptr, hipEvent_t done = nullptr);
#define ABC_INTERNAL_RETRY (-2147483647)      // launch_resample: the caller's abort flag was set when the host looked (not an error code of the ABI)
int launch_doubled_variance(abc_ctx*, const double* theta, size_t K, size_t P, double* dv);
// K x P posterior moments computed once (Gram kernel) and shared by the doubled variance and the MVN factor
int launch_theta_stats(abc_ctx*, const double* theta, size_t K, size_t P, double** stats_out);
// everything that follows from the posterior's statistics record in ONE launch (mvn.hip: k_post_tail; P <= 64; fields optional)
struct abc_theta_fused {
    double* dv; double* L; int* spd; double* rows /* K x PP row-major, zero padded */; double* Lpad /* PP x PP */;
    // (fused drivers) the generation's status words straight into the pinned block, by the work-group that has the Cholesky status
    // anyway: the model header (component count; NULL: none) and the status -- no copy kernel behind the proposals then
    const double* model_hdr; double* hdr_pin; int* spd_pin;
};
int launch_post_tail(abc_ctx*, const double* theta, size_t K, size_t P, const double* stats, const abc_theta_fused* f);
int launch_dv_from_stats(abc_ctx*, const double* stats, size_t P, double* dv);
int launch_mvn_from_stats(abc_ctx*, const double* stats, size_t P, double* L, int* status_dev);
// the previous set's share of the weight stage (weights.hip: launch_weights_prev), prepared ahead of launch_weights_raw
struct abc_wprev {
    void* wc /* WConst */; double* b; double* hb; unsigned short* bt; unsigned* far_list;
    unsigned* tmin;        // KS_TOPN (tiles in the order of the rows' norm tops): the smallest top of every tile, f32 bits; else NULL
    size_t Kp, P, kn_max; int split, ready;
};
int launch_weights_prev(abc_ctx*, size_t P, size_t kn_max, const double* theta_prev, size_t Kp, const double* w_prev,
                        const double* dv_prev, abc_wprev* out, hipStream_t st);
int launch_weights_raw(abc_ctx*, const abc_prior* priors, const double* theta, size_t K, size_t P,
                       size_t k0, size_t kn, const double* theta_prev, size_t Kp,
                       const double* w_prev, const double* dv_prev, double* w_raw, const abc_wprev* prev = nullptr,
                       const double** sumsq_out = nullptr);
// sumsq_out (optional): when the call covers the whole set (k0 = 0, kn = K) the 64-row partials of the raw weights' sum of
// squares are computed by the same launch; *sumsq_out then points at them (device) for launch_normalize_l2's sumsq_parts, else NULL
// launch_weights_prev on the side stream (resample.hip); the caller makes its stream wait for ctx->ev_prev before the rest
int abc_weights_prev_early(abc_ctx* ctx, size_t P, size_t kn_max, const double* theta_prev, size_t Kp, const double* w_prev,
                           const double* dv_prev, abc_wprev* out);
int launch_fill(abc_ctx*, double* w, size_t K, double v, hipStream_t st = nullptr);     // st == NULL: the context's stream
int launch_normalize_l2(abc_ctx*, double* w, size_t K, double* host_mirror = nullptr, const double* sumsq_parts = nullptr);
// pinned scratch of the alias build over K weights: w | F | A | (pad) | E | the two index stacks (K + 1 entries each)
static inline size_t abc_alias_pin_bytes(size_t K) { return K * (sizeof(double) * 3 + sizeof(uint32_t) * 3) + 2 * sizeof(uint32_t) + 16; }
int launch_mvn_setup(abc_ctx*, const double* theta, size_t K, size_t P, double* L, int* status_host,
                     int* status_dev);
// while_host_builds (optional): called after the weights' copy to the host has been queued and before the host waits for it:
// GPU work launched there runs while the host builds the alias table
// uniform_weights: w is K copies of 1.0 / K (launch_fill): the table comes from abc_uniform_alias, no host round trip here
// raw_ready (optional): the n taus2 outputs of the draws, already queued on the side stream (abc_rng_streams_early)
int launch_resample(abc_ctx*, const abc_rng* rng, const double* w, size_t K, uint64_t i0, size_t n,
                    uint64_t* parent, int (*while_host_builds)(void*) = nullptr, void* hook_arg = nullptr,
                    bool uniform_weights = false, const uint32_t* raw_ready = nullptr, bool weights_on_host = false,
                    const volatile int* abort_flag = nullptr, bool parents_ready = false, int* alias_check_deferred = nullptr);
// alias_check_deferred (optional): with the table built on the device (ctx->alias_mode) nothing waits for the build's verdict
// here; *alias_check_deferred = 1 then tells the caller to read the pinned flag (ctx->status_pin->alias_fail) at its next
// synchronisation and, if it is set, to call launch_resample again with ctx->alias_mode = ABC_ALIAS_HOST.  NULL: this
// function synchronises and falls back by itself.
// parents_ready (uniform weights only): abc_rng_streams_early has drawn the parents on the side stream already
// abort_flag (pinned, optional): read right after the host has waited for the weights; non-zero -> nothing more is queued and
// ABC_INTERNAL_RETRY is returned (the weights belong to a placeholder selection: the caller repeats its generation)
// weights_on_host: the kernel that normalised w already stored them at the start of the context's pinned scratch
// (launch_normalize_l2's host_mirror, reserved with the size used here): nothing to copy
// Queues on the context's side stream everything of the proposals that depends on the rng state alone: the taus2 outputs
// i0 .. i0 + n - 1 of the resampling draws (-> *raw) and, if seeds != NULL, the simulator seeds = outputs seed_stream_offset +
// i0 + i.  The main stream waits for them in launch_resample (raw_ready).  Call before the first kernel of the generation.
int abc_rng_streams_early(abc_ctx* ctx, const abc_rng* rng, uint64_t i0, size_t n, uint64_t* seeds, uint64_t seed_stream_offset,
                          uint32_t** raw, uint64_t* parent_uniform = nullptr, size_t K_uniform = 0);
// parent_uniform (set 0): the weights will be K_uniform copies of 1 / K_uniform whatever the ranking says, their alias table is
// on the device already (abc_uniform_alias, called BEFORE the fork), so the parents are drawn here too, beside the ranking
int abc_rng_seeds_early(abc_ctx* ctx, const abc_rng* rng, uint64_t i0, size_t n, uint64_t* seeds, uint64_t seed_stream_offset);
int abc_side_fork(abc_ctx* ctx);      // records where on the main stream the side stream's work of this generation may start
// Alias table of K equal weights: gsl_ran_discrete_preproc on K copies of 1.0 / K (bit-identical to the table of the filled
// weight vector), built on the host on first use for this K and kept in HBM.  The fused drivers call it right after queueing
// the ranking kernels, so the host builds the table while the GPU ranks.
int abc_uniform_alias(abc_ctx* ctx, size_t K);
// what launch_perturb_prepare has already done: row-major posterior copy, seeds, the padded Cholesky factor
struct abc_perturb_prep { double* rows; int seeds_done; double* Lpad; };   // seeds_done may be preset by the caller
// multivariate / L_or_dv (optional): with them the factor is padded for the perturbation kernel as well
int launch_perturb_prepare(abc_ctx*, const abc_rng* rng, const double* theta, size_t K, size_t P, uint64_t i0, size_t n,
                           uint64_t* seeds, uint64_t seed_stream_offset, abc_perturb_prep* prep, int multivariate = 0,
                           const double* L_or_dv = nullptr);
// padded width of the row-major posterior copy the perturbation kernels read (and of their padded factor)
static inline int abc_perturb_pp(size_t P) {
    int PP = 2;
    while (PP < (int)P) PP *= 2;
    return (P > 64) ? (int)((P + 63) / 64 * 64) : PP;
}
int launch_perturb(abc_ctx*, const abc_rng* rng, const double* theta, size_t K, size_t P,
                   const abc_prior* priors, const uint64_t* parent, uint64_t i0, size_t n,
                   int multivariate, const double* L_or_dv, double* out, uint64_t* seeds,
                   uint64_t seed_stream_offset, const abc_perturb_prep* prep = nullptr);

// ---- the tail of a generation, shared by the fused and the sharded driver (resample.hip): from "the K winners' rows are in theta"
// to "the proposals are written".  The drivers keep their own conditions and call positions.
// The posterior's moments and what follows from them (doubled variance, proposal factor, the perturbation's row-major copy and
// padded factor, the status words into the pinned block) on the SIDE stream: allocates the factor (L_io or arena) and the
// perturbation's inputs, orders the side stream behind ev_theta (recorded here unless theta_ev_bound: the kernel that wrote theta
// carries it), queues launch_theta_stats + launch_post_tail there and records ev_moments.  who: prefix of the messages.
struct abc_side_moments { abc_theta_fused out; double* stats; double* L; };
int abc_moments_on_side(abc_ctx* ctx, const double* theta, size_t K, size_t P, bool multivariate, double* L_io, double* dv,
                        int* spd_dev, const double* model_hdr, bool theta_ev_bound, const char* who, abc_side_moments* m);
// AbcUtil.cpp:583 in front of launch_resample over Nn draws: *w_on_host says whether the normalised weights were mirrored into the
// pinned scratch (weights_on_host there)
int abc_normalize_for_resample(abc_ctx* ctx, double* w, size_t K, size_t Nn, const double* sumsq, bool* w_on_host);
// launch_resample's while_host_builds of both drivers: GPU work that does not need the alias table.  moments: the posterior's
// moments were deferred to here (theta_stats, dv, L, prep and the status words are then outputs); L == NULL: independent noise, or
// the factor is there already; i0 / seed_off: this caller's slice of the proposals and the length of the seed stream's first half
struct abc_prep_arg {
    abc_ctx* ctx; const abc_rng* rng; const double* theta; const double* theta_stats; size_t K, P, Nn;
    uint64_t i0, seed_off; uint64_t* seeds; abc_perturb_prep* prep; double* L; int* spd_dev; double* dv; bool moments;
    const double* model_hdr; double* hdr_pin; int* spd_pin;
};
int abc_prep_hook(void* prep_arg);
// the device build of the resampling table did not verify: the draws and the proposals of rows i0 .. i0 + Nn - 1 once more with the
// table from the host, from the rng of the generation's entry, then a synchronisation (the weights are final; only what depends
// on the table is repeated).  giveups_to_snapshot: the proposals' give-up counter goes back to the gather's snapshot first.
int abc_alias_repair(abc_ctx* ctx, const abc_rng* rng_entry, const double* w, size_t K, uint64_t i0, size_t Nn, uint64_t seed_off,
                     uint64_t* parent, const double* theta, size_t P, const abc_prior* priors, int multivariate, const double* L_or_dv,
                     double* next, abc_perturb_prep* prep, bool giveups_to_snapshot);

// reference-stream proposals (host loop, refstream_host.cpp): rng = state after the n resampling draws, advanced past all it consumes
int launch_perturb_reference(abc_ctx*, abc_rng* rng_after_draws, const double* theta, size_t K, size_t P, const abc_prior* priors,
                             const uint64_t* parent, size_t n, int multivariate, const double* L_or_dv, double* out,
                             uint64_t* seeds);

// [GSL] gsl_ran_discrete_preproc on the host (alias_host.cpp, a host-only translation unit built with the host compiler):
// scratch E: K doubles, smalls / bigs: K + 1 uint32 each
// knuth = false: without the final KNUTH_CONVENTION pass (k_alias_draw applies it when it reads the table)
void abc_alias_preproc(size_t K, const double* w, double* F, uint32_t* A, double* E, uint32_t* smalls, uint32_t* bigs, bool knuth = true);

// Walker alias table built on the device (alias_dev.hip): F without the KNUTH_CONVENTION map, as abc_alias_preproc(knuth = false);
// *fail_dev / *fail_pin (optional, pinned) = 1: the speculation did not verify (or the weights are outside its grid) -- the table
// must not be used, the caller builds it on the host
// verdict_src (optional): instead of a launch of its own that publishes the verdict, *verdict_src gets the device word that
// holds it; the caller's next kernel copies it to fail_dev / fail_pin (k_alias_draw does)
int launch_alias_build_dev(abc_ctx*, const double* w, size_t K, double* F, uint32_t* A, int* fail_dev, int* fail_pin,
                           const int** verdict_src = nullptr);
size_t abc_alias_dev_need(size_t K);       // arena bytes of one build
constexpr size_t ABC_ALIAS_DEV_MAX_K = (size_t)2 << 20;
// below this the ten launches of the device build (~90 us, latency-bound) lose to the host's round trip (K = 1e4: 26 us of host
// work + two PCIe hops); measured break-even between 1e4 and 1e5
constexpr size_t ABC_ALIAS_DEV_MIN_K = 20000;
constexpr size_t ABC_ALIAS_DEV_SMALL_K = 300000;   // up to here the build runs with two elements per thread, beyond with four (alias_dev.hip)

// arena bound shared by api.hip and sharded.hip
size_t abc_ws_need(size_t N, size_t M, size_t P, size_t A, size_t K, size_t Kp, size_t Nnext);
size_t abc_wx_need(size_t n_validation, size_t P, size_t A);     // arena of the Wilcoxon reduction (launch_wilcoxon)
int abc_timing_flush(abc_ctx* ctx);
void abc_comm_release(abc_ctx* ctx);     // sharded.hip: called by abc_ctx_destroy

// taus2 helpers shared by host code
void taus2_set(abc_rng* r, unsigned long seed);
uint32_t taus2_get(abc_rng* r);
void taus2_jump(abc_rng* r, uint64_t n);
