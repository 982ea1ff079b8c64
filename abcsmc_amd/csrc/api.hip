// C ABI of libabcsmc_hip.so (see include/abcsmc_hip.h for the contract and reference citations).
#include <math.h>
#include <stdlib.h>

#include <new>
#include <vector>

#include "abc_internal.h"
#include "adjust_dev.h"

// ---- workspace -------------------------------------------------------------------------------
int abc_ws_reserve(abc_ctx* ctx, size_t bytes) {
    ctx->ws_asked = bytes;
    ctx->ws_peak = 0;
    bytes = abc_align(bytes, 1 << 20);
    if (bytes > ctx->ws_bytes) {
        ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->ws) { ABC_HIP(ctx, hipFree(ctx->ws)); ctx->ws = nullptr; ctx->ws_bytes = 0; }
        ABC_HIP(ctx, hipMalloc((void**)&ctx->ws, bytes));
        ctx->ws_bytes = bytes;
    }
    ctx->ws_off = 0;
    // ABC_WS_POISON=<byte> (debugging): every entry point starts from a workspace filled with that byte (ff: NaNs and huge
    // integers), so that a kernel which reads a word nobody wrote in THIS call shows up in the tests instead of inheriting
    // whatever the previous call left there
    static const char* poison = abc_diag_env("ABC_WS_POISON");
    if (poison && ctx->ws) ABC_HIP(ctx, hipMemsetAsync(ctx->ws, (int)strtol(poison, nullptr, 16), ctx->ws_bytes, ctx->stream));
    return ABC_OK;
}
void* abc_ws_alloc(abc_ctx* ctx, size_t bytes) {
    const size_t off = abc_align(ctx->ws_off, 256);
    if (off + bytes > ctx->ws_bytes) return nullptr;
    ctx->ws_off = off + bytes;
    if (ctx->ws_off > ctx->ws_peak) ctx->ws_peak = ctx->ws_off;
    return ctx->ws + off;
}
int abc_pin_reserve(abc_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->pin_bytes) return ABC_OK;
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->pin) { ABC_HIP(ctx, hipHostFree(ctx->pin)); ctx->pin = nullptr; ctx->pin_bytes = 0; }
    bytes = abc_align(bytes, 1 << 16);
    ABC_HIP(ctx, hipHostMalloc((void**)&ctx->pin, bytes, hipHostMallocDefault));
    ctx->pin_bytes = bytes;
    return ABC_OK;
}

// generous upper bound of the arena needed by any single API call on these sizes
size_t abc_ws_need(size_t N, size_t M, size_t P, size_t A, size_t K, size_t Kp, size_t Nnext) {
    const size_t Call = (M + P + 15) / 16, C = Call > 6 ? 6 : Call;      // wider sets go through 96-column group pairs
    const size_t psz = (C * (C + 1) / 2) * 256 + 16 * C;
    size_t b = 0;
    b += 2 * 384 * psz * 8 * 2;                                   // gram partials (PLS stats + covariance)
    b += 4 * (stats_layout(M, P).len + model_layout(M, P, A ? A : 1).len) * 8;
    b += (2 * M * P + 2 * M * M + P + A * M + A * A + 2 * P * A + 64 + M * 40) * 8;
    b += (M * P + 3 * P * P + 2 * P + 8 * M + 2 * M * A + A + 64 + 2048) * 8 + 3 * 96 * 96 * 8 * 2;   // PLS work arrays beyond the LDS; group-pair records
    b += N * 8;                                                   // distances
    b += 4 * K * 8 + (N / 2048 + 2) * 8 + 2048 * 4 + 256 * (K / 2048 + 2) * 4 + 4096;   // select + sort
    b += 2 * (K + 1024) * 8 + 34 * 16384 * 4 + 4096;              // ... or the bin selection's pair buffer, counts and cursors
    b += 3 * N * 8 + 256 * (N / 2048 + 2) * 4;                    // full-sort case K == N
    const size_t PPw = P <= 64 ? 64 : (P + 63) / 64 * 64;         // padded row width of the row-major copies
    b += K * P * 8 + K * PPw * 8;                                 // theta, and its row-major copy for the perturb gather
    b += (K + Kp) * PPw * 8 + 1024 * 8 + 64 * PPw * 8 + 32768;    // weights: scaled copies of both sets, centre partials, constants
    b += (K + Kp + 512) * (9 * 32 + 8 + 12) + 8192;               // ... and their f16 limb tiles (<= 9 operands of 32 B a row), 1/2|a|^2 parts
    b += (K + 512) * 17 + 16384;                                   // far-row flags, list and fix-up sums
    b += (Kp + 64) * (8 + 4 + 4 + 1) + (Kp / 2048 + 2) * 256 * 4 + 4096;   // tiles in the order of the norm tops: keys, ranks, tops, tile info, bin counts
    if (K && Kp) b += ((size_t)64 << 20) + 64 * K + ((size_t)16 << 20);   // ... and the per-slice partial sums (abc_kde_slices)
    b += K * 8 + P * P * 8 + P * 8;
    b += Nnext * (8 + 8 + 4 + 4);                                 // parent, seeds, raw streams
    b += 2 * PPw * PPw * 8 + 4096;                                // padded Cholesky factor of the proposals, factorisation scratch
    if (K) b += abc_alias_dev_need(K);                            // the resampling table's device build (alias_dev.hip)
    b += 64 * 256;                                                // alignment slack
    return b + (4u << 20);
}

// ---- context ---------------------------------------------------------------------------------
extern "C" int abc_version(void) { return 102; }

extern "C" int abc_ctx_create(int device, abc_ctx** out) {
    if (!out) return ABC_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return ABC_ERR_HIP;
    if (hipSetDevice(device) != hipSuccess) return ABC_ERR_HIP;
    abc_ctx* ctx = new (std::nothrow) abc_ctx();
    if (!ctx) return ABC_ERR_NOMEM;
    memset(ctx, 0, sizeof(*ctx));
    ctx->device = device;
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return ABC_ERR_HIP; }
    if (hipHostMalloc((void**)&ctx->status_pin, sizeof(abc_status_block), hipHostMallocDefault) != hipSuccess) { (void)hipStreamDestroy(ctx->own_stream); delete ctx; return ABC_ERR_HIP; }
    ctx->stream = ctx->own_stream;
    ctx->wx_gather_rows = abc_diag_env("ABC_WX_GATHER") != nullptr;
    ctx->gram_mode = abc_diag_env("ABC_GRAM_FP64") ? ABC_GRAM_FP64 : (abc_diag_env("ABC_GRAM_I8") ? ABC_GRAM_I8 : ABC_GRAM_AUTO);      // (the diagnostic switch of round 4: the initial mode)
    *out = ctx;
    return ABC_OK;
}

extern "C" void abc_ctx_destroy(abc_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->ws) (void)hipFree(ctx->ws);
    if (ctx->pin) (void)hipHostFree(ctx->pin);
    if (ctx->status_pin) (void)hipHostFree(ctx->status_pin);
    if (ctx->alias_F) (void)hipFree(ctx->alias_F);       // alias_A lives in the same allocation
    if (ctx->ualias_F) (void)hipFree(ctx->ualias_F);
    if (ctx->ualias_pin) (void)hipHostFree(ctx->ualias_pin);
    if (ctx->jump_tab) (void)hipFree(ctx->jump_tab);
    if (ctx->kde_which) (void)hipFree(ctx->kde_which);
    if (ctx->giveups_dev) (void)hipFree(ctx->giveups_dev);
    if (ctx->alias_fail_dev) (void)hipFree(ctx->alias_fail_dev);
    if (ctx->tf_buf) (void)hipFree(ctx->tf_buf);
    if (ctx->tf_outside_dev) (void)hipFree(ctx->tf_outside_dev);
    if (ctx->hc_buf) (void)hipFree(ctx->hc_buf);
    if (ctx->hc_skipped_dev) (void)hipFree(ctx->hc_skipped_dev);
    if (ctx->rg_pick) (void)hipFree(ctx->rg_pick);
    if (ctx->rg_press) (void)hipFree(ctx->rg_press);
    if (ctx->rg_unscored_dev) (void)hipFree(ctx->rg_unscored_dev);
    if (ctx->rw_dev) (void)hipFree(ctx->rw_dev);
    if (ctx->wx_rec_dev) (void)hipFree(ctx->wx_rec_dev);
    abc_comm_release(ctx);
    if (ctx->xbuf) (void)hipFree(ctx->xbuf);
    if (ctx->ev_copy) (void)hipEventDestroy(ctx->ev_copy);
    if (ctx->ev_theta) { (void)hipEventDestroy(ctx->ev_theta); (void)hipEventDestroy(ctx->ev_moments); }
    if (ctx->wx_stream) { (void)hipStreamSynchronize(ctx->wx_stream); (void)hipStreamDestroy(ctx->wx_stream); (void)hipEventDestroy(ctx->ev_wx_fork); (void)hipEventDestroy(ctx->ev_wx_done); (void)hipEventDestroy(ctx->ev_wx_scores); }
    if (ctx->side) { (void)hipStreamSynchronize(ctx->side); (void)hipStreamDestroy(ctx->side); (void)hipEventDestroy(ctx->ev_fork); (void)hipEventDestroy(ctx->ev_side); if (ctx->ev_prev) (void)hipEventDestroy(ctx->ev_prev); }
    for (int i = 0; i < 256; i++) if (ctx->ev[i].a) { (void)hipEventDestroy(ctx->ev[i].a); (void)hipEventDestroy(ctx->ev[i].b); }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

extern "C" const char* abc_last_error(const abc_ctx* ctx) { return ctx ? ctx->err : "null context"; }

extern "C" int abc_ws_info(const abc_ctx* ctx, size_t* reserved, size_t* asked, size_t* peak) {
    if (!ctx) return ABC_ERR_INVALID;
    if (reserved) *reserved = ctx->ws_bytes;
    if (asked) *asked = ctx->ws_asked;
    if (peak) *peak = ctx->ws_peak;
    return ABC_OK;
}

extern "C" int abc_ctx_set_stream(abc_ctx* ctx, void* hip_stream) {
    if (!ctx) return ABC_ERR_INVALID;
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = (hipStream_t)hip_stream;
    return ABC_OK;
}

extern "C" int abc_ctx_use_own_stream(abc_ctx* ctx) {
    if (!ctx) return ABC_ERR_INVALID;
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = ctx->own_stream;
    return ABC_OK;
}

extern "C" int abc_ctx_set_kde_mode(abc_ctx* ctx, int mode) {
    if (!ctx) return ABC_ERR_INVALID;
    if (mode != ABC_KDE_AUTO && mode != ABC_KDE_FP64) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_kde_mode: unknown mode %d", mode);
    ctx->kde_mode = mode;
    return ABC_OK;
}

extern "C" int abc_ctx_set_gram_mode(abc_ctx* ctx, int mode) {
    if (!ctx) return ABC_ERR_INVALID;
    if (mode != ABC_GRAM_AUTO && mode != ABC_GRAM_FP64 && mode != ABC_GRAM_I8) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_gram_mode: unknown mode %d", mode);
    ctx->gram_mode = mode;
    return ABC_OK;
}

extern "C" int abc_ctx_set_weight_kernel(abc_ctx* ctx, int kernel) {
    if (!ctx) return ABC_ERR_INVALID;
    if (kernel != ABC_WEIGHT_GAUSSIAN && kernel != ABC_WEIGHT_EPANECHNIKOV)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_weight_kernel: unknown kernel %d", kernel);
    ctx->weight_kernel = kernel;
    return ABC_OK;
}

extern "C" int abc_ctx_set_noise_mode(abc_ctx* ctx, int mode) {
    if (!ctx) return ABC_ERR_INVALID;
    if (mode != ABC_NOISE_DEVICE && mode != ABC_NOISE_REFERENCE_STREAM)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_noise_mode: unknown mode %d", mode);
    ctx->noise_mode = mode;
    return ABC_OK;
}

extern "C" int abc_ctx_set_alias_mode(abc_ctx* ctx, int mode) {
    if (!ctx) return ABC_ERR_INVALID;
    if (mode != ABC_ALIAS_DEVICE && mode != ABC_ALIAS_HOST) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_alias_mode: unknown mode %d", mode);
    ctx->alias_mode = mode;
    return ABC_OK;
}

extern "C" int abc_alias_stats(abc_ctx* ctx, uint64_t* device_builds, uint64_t* host_fallbacks, int reset) {
    if (!ctx) return ABC_ERR_INVALID;
    if (device_builds) *device_builds = ctx->alias_dev_builds;
    if (host_fallbacks) *host_fallbacks = ctx->alias_dev_fallbacks;
    if (reset) { ctx->alias_dev_builds = 0; ctx->alias_dev_fallbacks = 0; }
    return ABC_OK;
}

extern "C" int abc_select_stats(abc_ctx* ctx, uint64_t* bin_selections, uint64_t* bin_giveups, int reset) {
    if (!ctx) return ABC_ERR_INVALID;
    if (bin_selections) *bin_selections = (uint64_t)ctx->sel_bin_selections;
    if (bin_giveups) *bin_giveups = (uint64_t)ctx->sel_bin_giveups;
    if (reset) { ctx->sel_bin_selections = 0; ctx->sel_bin_giveups = 0; }
    return ABC_OK;
}

extern "C" int abc_perturb_giveups(abc_ctx* ctx, uint64_t* count, int reset) {
    if (!ctx || !count) return ABC_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) ABC_FAIL(ctx, ABC_ERR_HIP, "hipSetDevice failed");
    unsigned long long dev = 0;
    if (ctx->giveups_dev) {
        ABC_HIP(ctx, hipMemcpyAsync(&dev, ctx->giveups_dev, sizeof(dev), hipMemcpyDeviceToHost, ctx->stream));
        if (reset) ABC_HIP(ctx, hipMemsetAsync(ctx->giveups_dev, 0, sizeof(dev), ctx->stream));
        ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    *count = (uint64_t)dev + (uint64_t)ctx->giveups_host;
    ctx->giveups_dev_known = reset ? 0ull : dev;
    ctx->giveups_seen = reset ? 0 : (unsigned long long)*count;
    if (reset) ctx->giveups_host = 0;
    return ABC_OK;
}

extern "C" int abc_generation_giveups(const abc_ctx* ctx, uint64_t* count) {
    if (!ctx || !count) return ABC_ERR_INVALID;
    *count = (uint64_t)ctx->giveups_last_call;
    return ABC_OK;
}

extern "C" int abc_generation_repeats(abc_ctx* ctx, uint64_t* ranking_repeats, uint64_t* generation_repeats, int reset) {
    if (!ctx) return ABC_ERR_INVALID;
    if (ranking_repeats) *ranking_repeats = (uint64_t)ctx->wx_moved_counts;
    if (generation_repeats) *generation_repeats = (uint64_t)ctx->generation_repeats;
    if (reset) { ctx->wx_moved_counts = 0; ctx->generation_repeats = 0; }
    return ABC_OK;
}

extern "C" int abc_kde_last_kernel(abc_ctx* ctx, int* which) {
    if (!ctx || !which) return ABC_ERR_INVALID;
    *which = ABC_KDE_RAN_NONE;
    if (!ctx->kde_which) return ABC_OK;
    ABC_HIP(ctx, hipMemcpyAsync(which, ctx->kde_which, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ABC_OK;
}

extern "C" int abc_ctx_set_wx_record(abc_ctx* ctx, int on) {
    if (!ctx) return ABC_ERR_INVALID;
    ctx->wx_record = on ? 1 : 0;
    ctx->wx_rec_valid = false;
    return ABC_OK;
}

extern "C" int abc_wx_last_record(abc_ctx* ctx, abc_wx_test_record* out, size_t cap, size_t* ntests, int* path) {
    if (!ctx || !ntests || !path || (cap && !out)) return ABC_ERR_INVALID;
    *ntests = 0;
    *path = ABC_WX_PATH_NONE;
    if (!ctx->wx_rec_dev || !ctx->wx_rec_valid) return ABC_OK;
    if (hipSetDevice(ctx->device) != hipSuccess) ABC_FAIL(ctx, ABC_ERR_HIP, "hipSetDevice failed");
    if (ctx->wx_stream) ABC_HIP(ctx, hipStreamSynchronize(ctx->wx_stream));
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int hdr[2] = {0, ABC_WX_PATH_NONE};
    ABC_HIP(ctx, hipMemcpy(hdr, ctx->wx_rec_dev, sizeof(hdr), hipMemcpyDeviceToHost));
    size_t n = hdr[0] > 0 ? (size_t)hdr[0] : 0;
    if (n > ctx->wx_rec_cap) n = ctx->wx_rec_cap;
    *ntests = n;
    *path = hdr[1];
    const size_t take = n < cap ? n : cap;
    if (take) ABC_HIP(ctx, hipMemcpy(out, ctx->wx_rec_dev + 256, take * sizeof(abc_wx_test_record), hipMemcpyDeviceToHost));
    return ABC_OK;
}

extern "C" int abc_ctx_synchronize(abc_ctx* ctx) {
    if (!ctx) return ABC_ERR_INVALID;
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ABC_OK;
}

static const char* const kStageNames[ABC_NSTAGE] = {
    "k_gram", "stats_reduce", "pls_model", "project_distance", "select", "sort_winners", "gather_dv", "k_kde",
    "weights_misc", "mvn_setup", "alias_host", "resample", "perturb", "collectives"};

extern "C" int abc_timing_enable(abc_ctx* ctx, int on) {
    if (!ctx) return ABC_ERR_INVALID;
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->timing = (on == 2) ? 2 : (on != 0);
    ctx->nev = 0;
    ctx->timers_open = 0;
    ctx->timing_dropped = 0;
    return ABC_OK;
}

int abc_timing_flush(abc_ctx* ctx) {
    if (!ctx->nev) return ABC_OK;
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < ctx->nev; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev[i].a, ctx->ev[i].b) == hipSuccess) {
            ctx->stage_ms[ctx->ev[i].stage] += ms;
            ctx->stage_cnt[ctx->ev[i].stage] += 1;
        }
    }
    ctx->nev = 0;
    return ABC_OK;
}

extern "C" int abc_timing_read(abc_ctx* ctx, const char** names, double* ms, double* host_ms, long long* count,
                               int max_stages, int reset) {
    if (!ctx) return ABC_ERR_INVALID;
    ABC_TRY(abc_timing_flush(ctx));
    if (ctx->timing_dropped) {
        const unsigned long long d = ctx->timing_dropped;
        ctx->timing_dropped = 0;
        ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_timing_read: %llu stage samples were lost (event ring full inside an open stage); the sums are short", d);
    }
    for (int i = 0; i < ABC_NSTAGE && i < max_stages; i++) {
        if (names) names[i] = kStageNames[i];
        if (ms) ms[i] = ctx->stage_ms[i];
        if (host_ms) host_ms[i] = ctx->stage_host_ms[i];
        if (count) count[i] = ctx->stage_cnt[i];
    }
    if (reset) for (int i = 0; i < ABC_NSTAGE; i++) { ctx->stage_ms[i] = 0; ctx->stage_host_ms[i] = 0; ctx->stage_cnt[i] = 0; }
    return ABC_NSTAGE;
}

// Event-bracket overhead: what an event pair around ONE kernel reports beyond that kernel's execution (packet
// processing before the dispatch, the end-of-kernel release before the closing marker).  b1 = bracket around one
// empty kernel, b2 = around two; b2 - b1 is the marginal cost of an empty kernel, so overhead = b1 - (b2 - b1).
__global__ void k_noop() {}
extern "C" int abc_timing_overhead(abc_ctx* ctx, int reps, double* overhead_ms) {
    if (!ctx || !overhead_ms || reps < 1) return ABC_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) ABC_FAIL(ctx, ABC_ERR_HIP, "hipSetDevice failed");
    hipEvent_t a, b;
    ABC_HIP(ctx, hipEventCreate(&a));
    ABC_HIP(ctx, hipEventCreate(&b));
    double acc[2] = {0, 0};
    for (int k = 0; k < 2; k++)
        for (int r = 0; r < reps + 2; r++) {
            hipLaunchKernelGGL(k_noop, dim3(256), dim3(256), 0, ctx->stream);      // the stream is busy, as in a step
            ABC_HIP(ctx, hipEventRecord(a, ctx->stream));
            for (int j = 0; j <= k; j++) hipLaunchKernelGGL(k_noop, dim3(256), dim3(256), 0, ctx->stream);
            ABC_HIP(ctx, hipEventRecord(b, ctx->stream));
            ABC_HIP(ctx, hipEventSynchronize(b));
            float ms = 0;
            ABC_HIP(ctx, hipEventElapsedTime(&ms, a, b));
            if (r >= 2) acc[k] += ms;                                              // two warm-up rounds
        }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    const double b1 = acc[0] / reps, b2 = acc[1] / reps;
    double ov = b1 - (b2 - b1);
    if (ov < 0) ov = 0;
    *overhead_ms = ov;
    return ABC_OK;
}

extern "C" void abc_rng_set(abc_rng* r, unsigned long seed) { taus2_set(r, seed); }
extern "C" uint32_t abc_rng_get(abc_rng* r) { return taus2_get(r); }
extern "C" void abc_rng_jump(abc_rng* r, uint64_t n) { taus2_jump(r, n); }

// Every public entry starts here.  With timing on, the event ring (256 pairs) is drained as soon as it is half full: no
// stage timer is open at an entry point, so every recorded pair is complete, and a long run of stage-level calls (the
// sharded driver opens ~30 timers per step and never reaches generation_core's flush) loses no sample.
#define CHECK_CTX(ctx)                         \
    do {                                       \
        if (!(ctx)) return ABC_ERR_INVALID;    \
        (ctx)->err[0] = 0;                     \
        if (hipSetDevice((ctx)->device) != hipSuccess) ABC_FAIL(ctx, ABC_ERR_HIP, "hipSetDevice failed"); \
        if ((ctx)->timing && (ctx)->nev > 128) ABC_TRY(abc_timing_flush(ctx)); \
    } while (0)

// ---- parameter transforms of the local-linear adjustment ---------------------------------------------------------------------
// the context's setting as the kernels take it (kind == NULL: nothing set)
static AbcTf ctx_tf(const abc_ctx* ctx) {
    AbcTf t{nullptr, nullptr, nullptr};
    if (ctx->tf_buf) {
        const double* lo = (const double*)ctx->tf_buf;
        t.lo = lo;
        t.hi = lo + ctx->tf_P;
        t.kind = (const int32_t*)(lo + 2 * ctx->tf_P);
    }
    return t;
}

extern "C" int abc_ctx_set_param_transf(abc_ctx* ctx, const abc_param_transf_t* tf) {
    if (!ctx) return ABC_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) ABC_FAIL(ctx, ABC_ERR_HIP, "hipSetDevice failed");
    bool any = false;
    if (tf && tf->P) {
        const size_t P = tf->P;
        if (P > 1024) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_param_transf: P = %zu parameters (at most 1024)", P);
        if (!tf->kind) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_param_transf: null argument (kind is required)");
        for (size_t j = 0; j < P; j++) {
            const int32_t k = tf->kind[j];
            if (k != ABC_TRANSF_NONE && k != ABC_TRANSF_LOG && k != ABC_TRANSF_LOGIT)
                ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_param_transf: kind[%zu] = %d (0 = none, 1 = log, 2 = logit)", j, (int)k);
            if (k == ABC_TRANSF_LOGIT) {
                if (!tf->lo || !tf->hi)
                    ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_param_transf: null bounds (lo and hi are required for logit, parameter %zu)", j);
                const double lo = tf->lo[j], hi = tf->hi[j];
                if (!isfinite(lo) || !isfinite(hi) || !(lo < hi))
                    ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_param_transf: bounds [%g, %g] of parameter %zu (finite, lo < hi)", lo, hi, j);
            }
            any = any || k != ABC_TRANSF_NONE;
        }
    }
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));                 // (queued kernels may still read the previous setting)
    if (ctx->tf_buf) { ABC_HIP(ctx, hipFree(ctx->tf_buf)); ctx->tf_buf = nullptr; ctx->tf_P = 0; }
    if (!any) return ABC_OK;
    const size_t P = tf->P;
    std::vector<double> h(2 * P + (P + 1) / 2, 0.0);                 // [lo | hi | kind]
    for (size_t j = 0; j < P; j++)
        if (tf->kind[j] == ABC_TRANSF_LOGIT) { h[j] = tf->lo[j]; h[P + j] = tf->hi[j]; }
    memcpy(h.data() + 2 * P, tf->kind, P * sizeof(int32_t));
    if (!ctx->tf_outside_dev) {
        ABC_HIP(ctx, hipMalloc((void**)&ctx->tf_outside_dev, sizeof(unsigned long long)));
        ABC_HIP(ctx, hipMemset(ctx->tf_outside_dev, 0, sizeof(unsigned long long)));
    }
    ABC_HIP(ctx, hipMalloc((void**)&ctx->tf_buf, h.size() * sizeof(double)));
    ABC_HIP(ctx, hipMemcpy(ctx->tf_buf, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->tf_P = P;
    return ABC_OK;
}

// ---- heteroscedastic variance correction of the local-linear adjustment ------------------------------------------------------

extern "C" int abc_ctx_set_adjust_hcorr(abc_ctx* ctx, int on) {
    CHECK_CTX(ctx);
    if (on != 0 && on != 1) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_adjust_hcorr: on = %d (0 or 1)", on);
    if (on && !ctx->hc_skipped_dev) {
        ABC_HIP(ctx, hipMalloc((void**)&ctx->hc_skipped_dev, sizeof(unsigned long long)));
        ABC_HIP(ctx, hipMemset(ctx->hc_skipped_dev, 0, sizeof(unsigned long long)));
    }
    ctx->hcorr = on;
    return ABC_OK;
}

// the context's record for a regressing call of `slots` fits under the setting (grown here, never while the setting is off); the
// counts are zeroed here and set by tg_run once every launch of the call has been queued, so a call that fails leaves no record
static int hcorr_record(abc_ctx* ctx, const char* fn, size_t slots, size_t A, size_t P, AbcHc* hc) {
    const size_t n = slots * (A + 1) * P;
    if (n > ctx->hc_cap) {
        ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->hc_buf) { ABC_HIP(ctx, hipFree(ctx->hc_buf)); ctx->hc_buf = nullptr; ctx->hc_cap = 0; }
        ctx->hc_slots = ctx->hc_a1 = ctx->hc_P = 0;
        if (hipMalloc((void**)&ctx->hc_buf, n * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            ctx->hc_buf = nullptr;
            ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: no memory for the variance correction's record (%zu doubles)", fn, n);
        }
        ctx->hc_cap = n;
    }
    ctx->hc_slots = ctx->hc_a1 = ctx->hc_P = 0;         // nothing recorded until the call has queued its fits (tg_run)
    hc->hcoef = ctx->hc_buf;
    hc->skipped = ctx->hc_skipped_dev;
    return ABC_OK;
}

extern "C" int abc_adjust_last_hcorr(abc_ctx* ctx, double* hcoef, size_t cap, size_t* slots, size_t* a1, size_t* P) {
    CHECK_CTX(ctx);
    if (!slots || !a1 || !P) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_adjust_last_hcorr: null argument (slots, a1 and P are required)");
    *slots = ctx->hc_slots;
    *a1 = ctx->hc_a1;
    *P = ctx->hc_P;
    size_t n = ctx->hc_slots * ctx->hc_a1 * ctx->hc_P;
    if (n > cap) n = cap;
    if (n && !hcoef) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_adjust_last_hcorr: null argument (hcoef with cap = %zu)", cap);
    if (n) ABC_HIP(ctx, hipMemcpyAsync(hcoef, ctx->hc_buf, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ABC_OK;
}

extern "C" int abc_adjust_hcorr_skipped(abc_ctx* ctx, uint64_t* count, int reset) {
    CHECK_CTX(ctx);
    if (!count) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_adjust_hcorr_skipped: null argument (count is required)");
    unsigned long long dev = 0;
    if (ctx->hc_skipped_dev) {
        ABC_HIP(ctx, hipMemcpyAsync(&dev, ctx->hc_skipped_dev, sizeof(dev), hipMemcpyDeviceToHost, ctx->stream));
        if (reset) ABC_HIP(ctx, hipMemsetAsync(ctx->hc_skipped_dev, 0, sizeof(dev), ctx->stream));
        ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    *count = (uint64_t)dev;
    return ABC_OK;
}

// ---- ridge adjustment with the penalty chosen by leave-one-out PRESS -------------------------------------------------------------

extern "C" int abc_ctx_set_adjust_ridge(abc_ctx* ctx, const double* lambda, size_t L) {
    CHECK_CTX(ctx);
    if (!lambda || L == 0) {
        ctx->rg_L = 0;
        return ABC_OK;
    }
    if (L > ABC_RIDGE_MAXL) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_adjust_ridge: L = %zu (at most %d)", L, (int)ABC_RIDGE_MAXL);
    for (size_t l = 0; l < L; l++) {
        if (!isfinite(lambda[l]) || lambda[l] < 0.0)
            ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_adjust_ridge: lambda[%zu] = %g (finite and >= 0)", l, lambda[l]);
        if (l && !(lambda[l] > lambda[l - 1]))
            ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_ctx_set_adjust_ridge: lambda[%zu] = %g after %g (strictly ascending)", l, lambda[l],
                     lambda[l - 1]);
    }
    if (!ctx->rg_unscored_dev) {
        ABC_HIP(ctx, hipMalloc((void**)&ctx->rg_unscored_dev, sizeof(unsigned long long)));
        ABC_HIP(ctx, hipMemset(ctx->rg_unscored_dev, 0, sizeof(unsigned long long)));
    }
    for (size_t l = 0; l < L; l++) ctx->rg_lambda[l] = lambda[l];
    ctx->rg_L = L;
    return ABC_OK;
}

// the context's record for a regressing call of `slots` fits under the setting (hcorr_record's rules)
static int ridge_record(abc_ctx* ctx, const char* fn, size_t slots, size_t P, AbcRg* rg) {
    const size_t np = slots * P, nq = slots * ctx->rg_L * P;
    if (np > ctx->rg_cap_pick || nq > ctx->rg_cap_press) {
        ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->rg_pick) { ABC_HIP(ctx, hipFree(ctx->rg_pick)); ctx->rg_pick = nullptr; ctx->rg_cap_pick = 0; }
        if (ctx->rg_press) { ABC_HIP(ctx, hipFree(ctx->rg_press)); ctx->rg_press = nullptr; ctx->rg_cap_press = 0; }
        ctx->rg_slots = ctx->rg_Lrec = ctx->rg_P = 0;
        if (hipMalloc((void**)&ctx->rg_pick, np * sizeof(int32_t)) != hipSuccess ||
            hipMalloc((void**)&ctx->rg_press, nq * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            if (ctx->rg_pick) (void)hipFree(ctx->rg_pick);
            ctx->rg_pick = nullptr;
            ctx->rg_press = nullptr;
            ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: no memory for the ridge adjustment's record (%zu picks)", fn, np);
        }
        ctx->rg_cap_pick = np;
        ctx->rg_cap_press = nq;
    }
    ctx->rg_slots = ctx->rg_Lrec = ctx->rg_P = 0;         // nothing recorded until the call has queued its fits (tg_run)
    for (size_t l = 0; l < ctx->rg_L; l++) rg->lambda[l] = ctx->rg_lambda[l];
    rg->L = (int)ctx->rg_L;
    rg->pick = ctx->rg_pick;
    rg->press = ctx->rg_press;
    rg->unscored = ctx->rg_unscored_dev;
    return ABC_OK;
}

extern "C" int abc_adjust_last_ridge(abc_ctx* ctx, int32_t* pick, size_t cap_pick, double* press, size_t cap_press, size_t* slots,
                                     size_t* L, size_t* P) {
    CHECK_CTX(ctx);
    if (!slots || !L || !P) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_adjust_last_ridge: null argument (slots, L and P are required)");
    *slots = ctx->rg_slots;
    *L = ctx->rg_Lrec;
    *P = ctx->rg_P;
    size_t np = ctx->rg_slots * ctx->rg_P, nq = np * ctx->rg_Lrec;
    if (np > cap_pick) np = cap_pick;
    if (nq > cap_press) nq = cap_press;
    if (np && !pick) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_adjust_last_ridge: null argument (pick with cap_pick = %zu)", cap_pick);
    if (nq && !press) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_adjust_last_ridge: null argument (press with cap_press = %zu)", cap_press);
    if (np) ABC_HIP(ctx, hipMemcpyAsync(pick, ctx->rg_pick, np * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (nq) ABC_HIP(ctx, hipMemcpyAsync(press, ctx->rg_press, nq * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ABC_OK;
}

extern "C" int abc_adjust_ridge_unscored(abc_ctx* ctx, uint64_t* count, int reset) {
    CHECK_CTX(ctx);
    if (!count) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_adjust_ridge_unscored: null argument (count is required)");
    unsigned long long dev = 0;
    if (ctx->rg_unscored_dev) {
        ABC_HIP(ctx, hipMemcpyAsync(&dev, ctx->rg_unscored_dev, sizeof(dev), hipMemcpyDeviceToHost, ctx->stream));
        if (reset) ABC_HIP(ctx, hipMemsetAsync(ctx->rg_unscored_dev, 0, sizeof(dev), ctx->stream));
        ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    *count = (uint64_t)dev;
    return ABC_OK;
}

// ---- row importance weights of the batched ranking ----------------------------------------------------------------------------

// both setters: a copy of the caller's N weights in a buffer of the context's own, checked by one kernel whose four numbers the
// host reads here; the setting changes only when the check passes
static int row_weights_set(abc_ctx* ctx, const char* fn, const double* w, size_t N, bool host) {
    if (!w || N == 0) {
        if (ctx->rw_dev) {
            ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            ABC_HIP(ctx, hipFree(ctx->rw_dev));
        }
        ctx->rw_dev = nullptr;
        ctx->rw_N = ctx->rw_pos = 0;
        ctx->rw_ess = 0.0;
        return ABC_OK;
    }
    double* buf = nullptr;                                      // the weights and, behind them, the check's four numbers
    if (hipMalloc((void**)&buf, (N + 4) * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: no memory for %zu row weights", fn, N);
    }
    double chk[4] = {0.0, 0.0, 0.0, 0.0};
    int rc = ABC_OK;
    if (hipMemcpyAsync(buf, w, N * sizeof(double), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
        rc = ABC_ERR_HIP;
    if (rc == ABC_OK) rc = launch_row_weights_check(ctx, buf, N, buf + N);
    if (rc == ABC_OK && (hipMemcpyAsync(chk, buf + N, sizeof(chk), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                         hipStreamSynchronize(ctx->stream) != hipSuccess))
        rc = ABC_ERR_HIP;
    if (rc != ABC_OK) {
        (void)hipGetLastError();
        (void)hipFree(buf);
        ABC_FAIL(ctx, rc, "%s: copying or checking the row weights failed", fn);
    }
    if (chk[0] > 0.0 || !(chk[1] > 0.0)) {
        (void)hipFree(buf);
        if (chk[0] > 0.0) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: %.0f of the %zu row weights are negative or not finite", fn, chk[0], N);
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: none of the %zu row weights is positive", fn, N);
    }
    if (!isfinite(chk[2]) || !isfinite(chk[3])) {               // every weighted sum of a call would overflow as these do
        (void)hipFree(buf);
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: the sum of the %zu row weights or of their squares is not finite (rescale them)", fn, N);
    }
    if (ctx->rw_dev) (void)hipFree(ctx->rw_dev);                // (the stream is idle: synchronised above)
    ctx->rw_dev = buf;
    ctx->rw_N = N;
    ctx->rw_pos = (size_t)chk[1];
    ctx->rw_ess = chk[2] * chk[2] / chk[3];
    return ABC_OK;
}

extern "C" int abc_ctx_set_row_weights(abc_ctx* ctx, const double* w, size_t N) {
    CHECK_CTX(ctx);
    return row_weights_set(ctx, "abc_ctx_set_row_weights", w, N, true);
}

extern "C" int abc_ctx_set_row_weights_dev(abc_ctx* ctx, const double* w_dev, size_t N) {
    CHECK_CTX(ctx);
    return row_weights_set(ctx, "abc_ctx_set_row_weights_dev", w_dev, N, false);
}

extern "C" int abc_row_weights_info(abc_ctx* ctx, size_t* N, size_t* positive, double* ess) {
    CHECK_CTX(ctx);
    if (N) *N = ctx->rw_N;
    if (positive) *positive = ctx->rw_pos;
    if (ess) *ess = ctx->rw_ess;
    return ABC_OK;
}

static int param_transf_check(abc_ctx* ctx, const char* fn, const double* V, size_t ldv, size_t n, size_t P, const double* out,
                              size_t ldo) {
    if (!V || !out) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (V and out are required)", fn);
    if (ldv < n) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: ldv %zu < n %zu", fn, ldv, n);
    if (ldo < n) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: ldo %zu < n %zu", fn, ldo, n);
    if (ctx->tf_buf && P != ctx->tf_P)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: P = %zu, but the parameter transforms were set for %zu parameters", fn, P, ctx->tf_P);
    return ABC_OK;
}

extern "C" int abc_param_transf_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t n, size_t P, int inverse, double* out,
                                    size_t ldo) {
    CHECK_CTX(ctx);
    ABC_TRY(param_transf_check(ctx, "abc_param_transf_dev", V, ldv, n, P, out, ldo));
    const AbcTf tf = ctx_tf(ctx);
    return launch_param_transf(ctx, &tf, V, ldv, n, P, inverse, out, ldo, ctx->tf_outside_dev);
}

extern "C" int abc_param_transf_outside(abc_ctx* ctx, uint64_t* count, int reset) {
    if (!ctx || !count) return ABC_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) ABC_FAIL(ctx, ABC_ERR_HIP, "hipSetDevice failed");
    unsigned long long dev = 0;
    if (ctx->tf_outside_dev) {
        ABC_HIP(ctx, hipMemcpyAsync(&dev, ctx->tf_outside_dev, sizeof(dev), hipMemcpyDeviceToHost, ctx->stream));
        if (reset) ABC_HIP(ctx, hipMemsetAsync(ctx->tf_outside_dev, 0, sizeof(dev), ctx->stream));
        ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    *count = (uint64_t)dev;
    return ABC_OK;
}

static size_t default_A(size_t M, size_t P, int max_comp) {
    return (max_comp > 0) ? (size_t)max_comp : (M < P ? M : P);
}

// ---- stage-level device entry points -----------------------------------------------------------
// Column-major arguments of the stage entry points: a leading dimension below the row count would make columns overlap, and a
// set without columns has no record.  The statistics also need a metric column: with M == 0 the record has no X'X block, and
// the column-group path (run_gram_grouped) that such a set would reach covers pairs of groups only, so it would leave the
// record unwritten.  Leading dimensions of an empty side (M == 0 / P == 0) are not looked at.
#define CHECK_COLS(ctx, fn, n, ldx, ldy, M, P)                                                                          \
    do {                                                                                                                \
        if ((M) + (P) == 0) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: no columns (M + P == 0)", fn);                         \
        if ((M) > 0 && (ldx) < (n)) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: ldx %zu < n %zu", fn, (size_t)(ldx), (size_t)(n)); \
        if ((P) > 0 && (ldy) < (n)) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: ldy %zu < n %zu", fn, (size_t)(ldy), (size_t)(n)); \
    } while (0)
#define CHECK_STATS_COLS(ctx, fn, n, ldx, ldy, M, P)                                                                    \
    do {                                                                                                                \
        CHECK_COLS(ctx, fn, n, ldx, ldy, M, P);                                                                         \
        if ((M) == 0) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: the statistics record needs at least one metric (M == 0)", fn); \
    } while (0)

// the chunk sort behind up to 2^18 winners carries an element's position in the top 16 bits of its index word (select.hip:
// k_sort_chunks): row indices idx_base .. idx_base + n - 1 must stay below 2^48, whichever selection path answers
#define CHECK_IDX48(ctx, fn, idx_base, n)                                                                               \
    do {                                                                                                                \
        const uint64_t lim48_ = (uint64_t)1 << 48;                                                                      \
        if ((uint64_t)(idx_base) > lim48_ || (uint64_t)(n) > lim48_ - (uint64_t)(idx_base))                             \
            ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: idx_base %llu + n %zu exceeds 2^48", fn,                            \
                     (unsigned long long)(idx_base), (size_t)(n));                                                      \
    } while (0)

extern "C" size_t abc_stats_len(size_t M, size_t P) { return stats_layout(M, P).len; }
extern "C" size_t abc_model_len(size_t M, size_t P, size_t A) { return model_layout(M, P, A).len; }

extern "C" int abc_stats_shift_dev(abc_ctx* ctx, const double* X, const double* Y, size_t n, size_t ldx, size_t ldy,
                                   size_t M, size_t P, double* stats) {
    CHECK_CTX(ctx);
    CHECK_STATS_COLS(ctx, "abc_stats_shift_dev", n, ldx, ldy, M, P);
    return launch_stats_shift(ctx, X, Y, n, ldx, ldy, M, P, stats);
}

extern "C" int abc_stats_accumulate_dev(abc_ctx* ctx, const double* X, const double* Y, size_t n, size_t ldx,
                                        size_t ldy, size_t M, size_t P, uint64_t row0, uint64_t n_train_global,
                                        double* stats) {
    CHECK_CTX(ctx);
    CHECK_STATS_COLS(ctx, "abc_stats_accumulate_dev", n, ldx, ldy, M, P);
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(0, M, P, 1, 0, 0, 0)));
    return launch_stats_accumulate(ctx, X, Y, n, ldx, ldy, M, P, row0, n_train_global, stats);
}

extern "C" int abc_pls_model_dev(abc_ctx* ctx, const double* stats, const double* obs, size_t M, size_t P, size_t A,
                                 int rule, double* model) {
    CHECK_CTX(ctx);
    if (rule != ABC_RULE_MIN_PRESS)
        ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "abc_pls_model_dev fits from statistics only: call abc_pls_wilcoxon_dev "
                 "afterwards for rule %d (needs the validation rows)", rule);
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(0, M, P, A, 0, 0, 0)));
    return launch_pls_model(ctx, stats, obs, M, P, A, rule, model);
}

extern "C" int abc_pls_wilcoxon_dev(abc_ctx* ctx, const double* X, const double* Y, size_t n, size_t ldx, size_t ldy,
                                    size_t M, size_t P, size_t A, size_t row_test, double* model) {
    CHECK_CTX(ctx);
    CHECK_COLS(ctx, "abc_pls_wilcoxon_dev", n, ldx, ldy, M, P);
    const size_t nt = row_test < n ? n - row_test : 0;
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(0, M, P, A, 0, 0, 0) + abc_wx_need(nt, P, A)));
    return launch_wilcoxon(ctx, X, Y, n, ldx, ldy, M, P, A, row_test, model);
}

extern "C" int abc_simple_model_dev(abc_ctx* ctx, const double* stats, const double* obs, size_t M, size_t P,
                                    double* model) {
    CHECK_CTX(ctx);
    return launch_simple_model(ctx, stats, obs, M, P, model);
}

extern "C" int abc_model_ncomp(abc_ctx* ctx, const double* model, size_t M, size_t P, size_t A, int32_t* ncomp) {
    CHECK_CTX(ctx);
    double hdr[4];
    ABC_HIP(ctx, hipMemcpyAsync(hdr, model, sizeof(hdr), hipMemcpyDeviceToHost, ctx->stream));
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ncomp) *ncomp = (int32_t)hdr[0];
    return ABC_OK;
}

extern "C" int abc_project_distance_dev(abc_ctx* ctx, const double* X, size_t n, size_t ldx, size_t M, size_t P,
                                        size_t A, const double* model, int simple, double* dist) {
    CHECK_CTX(ctx);
    CHECK_COLS(ctx, "abc_project_distance_dev", n, ldx, n, M, P);      // (X only: the ldy slot gets n, which always passes)
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(0, M, P, A, 0, 0, 0)));
    return launch_project_distance(ctx, X, n, ldx, M, P, A, model, simple, dist);
}

extern "C" int abc_select_smallest_dev(abc_ctx* ctx, const double* dist, size_t n, size_t K, uint64_t idx_base,
                                       uint64_t* idx, double* dist_out) {
    CHECK_CTX(ctx);
    CHECK_IDX48(ctx, "abc_select_smallest_dev", idx_base, n);
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(n, 1, 1, 1, K, 0, 0)));
    return launch_select_smallest(ctx, dist, n, K, idx_base, idx, dist_out);
}

extern "C" int abc_select_begin_dev(abc_ctx* ctx, uint64_t K, int64_t* state, int32_t* hist) {
    CHECK_CTX(ctx);
    return launch_select_begin(ctx, K, (long long*)state, (int*)hist);
}
extern "C" int abc_select_hist_dev(abc_ctx* ctx, const double* dist, size_t n, const int64_t* state, int pass,
                                   int32_t* hist) {
    CHECK_CTX(ctx);
    return launch_select_hist(ctx, dist, n, (const long long*)state, pass, (int*)hist);
}
extern "C" int abc_select_pick_dev(abc_ctx* ctx, int64_t* state, int pass, int32_t* hist, uint64_t K) {
    CHECK_CTX(ctx);
    return launch_select_pick(ctx, (long long*)state, pass, (int*)hist, K);
}
extern "C" int abc_select_count_dev(abc_ctx* ctx, const double* dist, size_t n, const int64_t* state, int64_t* counts) {
    CHECK_CTX(ctx);
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(n, 1, 1, 1, 0, 0, 0)));
    return launch_select_count(ctx, dist, n, (const long long*)state, (long long*)counts);
}
extern "C" int abc_select_compact_dev(abc_ctx* ctx, const double* dist, size_t n, const int64_t* state, uint64_t n_less,
                                      uint64_t ties_take, uint64_t idx_base, uint64_t* idx_out, double* dist_out) {
    CHECK_CTX(ctx);
    CHECK_IDX48(ctx, "abc_select_compact_dev", idx_base, n);
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(n, 1, 1, 1, n_less + ties_take, 0, 0)));
    return launch_select_compact(ctx, dist, n, (const long long*)state, n_less, ties_take, idx_base, idx_out, dist_out);
}

extern "C" int abc_sort_pairs_dev(abc_ctx* ctx, double* key, uint64_t* idx, size_t n) {
    CHECK_CTX(ctx);
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(n, 1, 1, 1, n, 0, 0)));
    return launch_sort_pairs(ctx, key, idx, n);
}

extern "C" int abc_merge_sorted_runs_dev(abc_ctx* ctx, const double* key, const uint64_t* idx, int n_runs, size_t run_len,
                                        double* key_out, uint64_t* idx_out) {
    CHECK_CTX(ctx);
    if (!key || !idx || !key_out || !idx_out || key == key_out || idx == idx_out)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "merge: null or aliased buffers");
    return launch_merge_runs(ctx, key, idx, n_runs, run_len, key_out, idx_out);
}

extern "C" int abc_gather_rows_dev(abc_ctx* ctx, const double* Y, size_t n_local, size_t ldy, size_t P,
                                   const uint64_t* idx, size_t K, uint64_t idx_base, double* theta, size_t ldt) {
    CHECK_CTX(ctx);
    if (P > 0 && ldy < n_local) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_gather_rows_dev: ldy %zu < n_local %zu", ldy, n_local);
    if (P > 0 && ldt < K) ABC_FAIL(ctx, ABC_ERR_INVALID, "abc_gather_rows_dev: ldt %zu < K %zu", ldt, K);
    return launch_gather_rows(ctx, Y, n_local, ldy, P, idx, K, idx_base, theta, ldt);
}

extern "C" int abc_doubled_variance_dev(abc_ctx* ctx, const double* theta, size_t K, size_t P, double* dv) {
    CHECK_CTX(ctx);
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(0, P, 0, 1, 0, 0, 0)));     // the moments go through the Gram kernel's partial records
    return launch_doubled_variance(ctx, theta, K, P, dv);
}

extern "C" int abc_weights_raw_dev(abc_ctx* ctx, const abc_prior* priors, const double* theta, size_t K, size_t P,
                                   size_t k0, size_t kn, const double* theta_prev, size_t Kp, const double* w_prev,
                                   const double* dv_prev, double* w_raw) {
    CHECK_CTX(ctx);
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(0, 1, P, 1, kn, Kp, 0)));
    return launch_weights_raw(ctx, priors, theta, K, P, k0, kn, theta_prev, Kp, w_prev, dv_prev, w_raw);
}

extern "C" int abc_normalize_l2_dev(abc_ctx* ctx, double* w, size_t K) {
    CHECK_CTX(ctx);
    ABC_TRY(abc_ws_reserve(ctx, (K / 64 + 2) * sizeof(double) + (1 << 20)));
    return launch_normalize_l2(ctx, w, K);
}

extern "C" int abc_setup_mvn_sampler_dev(abc_ctx* ctx, const double* theta, size_t K, size_t P, double* L) {
    CHECK_CTX(ctx);
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(0, P, 0, 1, 0, 0, 0)));
    int st = 0;
    ABC_TRY(launch_mvn_setup(ctx, theta, K, P, L, &st, nullptr));
    if (st) ABC_FAIL(ctx, ABC_ERR_NOT_SPD, "covariance of the selected particles is not positive definite");
    return ABC_OK;
}

extern "C" int abc_resample_dev(abc_ctx* ctx, const abc_rng* rng, const double* w, size_t K, uint64_t i0, size_t n,
                                uint64_t* parent) {
    CHECK_CTX(ctx);
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(0, 1, 1, 1, 0, 0, n) + abc_alias_dev_need(K)));
    return launch_resample(ctx, rng, w, K, i0, n, parent);
}

extern "C" int abc_perturb_dev(abc_ctx* ctx, const abc_rng* rng, const double* theta, size_t K, size_t P,
                               const abc_prior* priors, const uint64_t* parent, uint64_t i0, size_t n,
                               int multivariate, const double* L_or_dv, double* out, uint64_t* seeds,
                               uint64_t seed_stream_offset) {
    CHECK_CTX(ctx);
    if (ctx->noise_mode == ABC_NOISE_REFERENCE_STREAM)
        ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "abc_perturb_dev works on row slices; the reference stream is sequential over the whole "
                 "set (use abc_sample_*_predictive_priors or abc_generation_dev)");
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(0, 1, P, 1, K, 0, n)));
    return launch_perturb(ctx, rng, theta, K, P, priors, parent, i0, n, multivariate, L_or_dv, out, seeds,
                          seed_stream_offset);
}

// ---- fused generation (device-resident) ----------------------------------------------------------
// does NOT reserve/reset the arena: the caller has done so (lets host wrappers keep their staging
// buffers in the same arena)
// the status words of a generation (model header with the component count, Cholesky status, selection flag) stored by the GPU
// straight into the context's pinned, device-visible block
__global__ void k_status_words(const double* __restrict__ model_hdr, const int* __restrict__ spd, const int* __restrict__ fail,
                               const unsigned long long* __restrict__ giveups, double* __restrict__ hdr_out, int* __restrict__ spd_out,
                               int* __restrict__ fail_out, unsigned long long* __restrict__ giveups_out) {
    const int t = threadIdx.x;
    if (model_hdr && t < 4) hdr_out[t] = model_hdr[t];
    if (spd && t == 4) *spd_out = *spd;
    if (fail && t == 5) *fail_out = *fail;
    if (t == 6) *giveups_out = giveups ? giveups[0] : 0ull;
}

static int generation_core(abc_ctx* ctx, const abc_generation_cfg* cfg, const abc_generation_io* io, abc_rng* rng,
                           int32_t* ncomp_host, int simple, const double** model_out = nullptr) {
    const size_t N = cfg->N, M = cfg->M, P = cfg->P, K = cfg->K, Kp = cfg->Kp, Nn = cfg->Nnext;
    if (!N || !M || K > N) ABC_FAIL(ctx, ABC_ERR_INVALID, "generation: bad sizes N=%zu M=%zu K=%zu", N, M, K);
    const size_t ws_entry = ctx->ws_off;              // a failed bin selection (select.hip) repeats the call from here
    ctx->side_early_waited = false;
    ctx->giveups_last_call = 0;
    if (Nn) ABC_TRY(abc_giveups_ensure(ctx));         // (the gather snapshots the counter: it has to exist before the first proposals)
    abc_rng rng_entry;
    if (rng) rng_entry = *rng;
    if (!simple && !(0.0 < cfg->train_frac && cfg->train_frac <= 1.0))      // AbcUtil.cpp:428
        ABC_FAIL(ctx, ABC_ERR_INVALID, "training fraction %g outside (0,1]", cfg->train_frac);
    if (!simple && cfg->rule != ABC_RULE_MIN_PRESS && cfg->rule != ABC_RULE_WILCOXON)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "unknown component rule %d", cfg->rule);
    const size_t A = simple ? 0 : default_A(M, P, cfg->max_comp);
    const StatsLayout SL = stats_layout(M, P);
    const ModelLayout ML = model_layout(M, P, A);
    double* stats = (double*)abc_ws_alloc(ctx, SL.len * 8);
    double* model = (double*)abc_ws_alloc(ctx, ML.len * 8);
    double* dist = (double*)abc_ws_alloc(ctx, N * 8);
    int* spd_dev = (int*)abc_ws_alloc(ctx, sizeof(int));
    if (!stats || !model || !dist || !spd_dev) ABC_FAIL(ctx, ABC_ERR_NOMEM, "generation: workspace exhausted");
    if (model_out) *model_out = model;
    const uint64_t ntrain = simple ? N : (uint64_t)llround((double)N * cfg->train_frac);   // AbcUtil.cpp:438
    const double* Yp = io->Y ? io->Y : io->X;
    const size_t Pstat = io->Y ? P : 0;
    // first set: the weights will be 1/K whatever the ranking says, so their alias table is built (once per K, then kept) before
    // anything is queued, and the parents are drawn on the side stream beside the ranking
    const bool uniform_w = io->w && K && (Kp == 0 || !io->theta_prev);
    const bool early = io->w && Nn && K && rng && ctx->noise_mode != ABC_NOISE_REFERENCE_STREAM;
    uint64_t* parent_early = nullptr;
    if (uniform_w && Nn) {
        ABC_TRY(abc_uniform_alias(ctx, K));
        if (early) {
            parent_early = io->parent ? io->parent : (uint64_t*)abc_ws_alloc(ctx, Nn * 8);
            if (!parent_early) ABC_FAIL(ctx, ABC_ERR_NOMEM, "generation: workspace exhausted");
        }
    }
    // The side stream's work (taus2 streams, the previous set's share of the weight stage) depends on nothing this call queues:
    // it is forked at the call's START -- the record is the first packet of an idle queue, processed while the host prepares the
    // first launch -- and runs beside the Gram kernel; forked behind that kernel (rounds 2 and 3) the record sat between the
    // reduce and the fit and cost the critical path ~6 us (rocprofv3 timeline).  Its launches still follow the fit's.
    // ... except beside the BYTE-LIMB statistics kernel of wide sets (round 6): that one keeps a 512-thread work-group with 150-160 KB
    // of LDS on every CU, and every side-stream kernel resident beside it takes CUs away from it for as long as it runs -- the
    // previous set's prologue alone is 0.74 ms there at configs[3] (0.2 ms on an idle chip): 2.34 ms for the statistics pass against
    // 1.6 stand-alone.  Forked behind it the side stream's work runs beside the model fit and the projection instead: everything
    // but the pair sums 6.80 -> 6.57 ms at configs[3], 1.408 -> 1.387 at configs[4].
    const bool fork_late = !simple && abc_gram_takes_i8(ctx, io->X, Yp, N, N, N, M, Pstat, ntrain, N);
    ctx->side_forked = false;
    if (!fork_late) ABC_TRY(abc_side_fork(ctx));
    ABC_TRY(launch_stats_shift(ctx, io->X, Yp, N, N, N, M, Pstat, stats));
    ABC_TRY(launch_stats_accumulate(ctx, io->X, Yp, N, N, N, M, Pstat, 0, ntrain, stats));
    if (fork_late) ABC_TRY(abc_side_fork(ctx));
    // (the cascade's stream is forked behind the fit: where the generation will speculate -- the condition is restated below --
    // the fork's event rides on the fit kernel's completion signal)
    const bool wx_spec = !simple && cfg->rule == ABC_RULE_WILCOXON && io->w && K &&
                         abc_wx_cascade_applies(N > (size_t)ntrain ? N - (size_t)ntrain : 0, P, A);
    if (wx_spec && !ctx->wx_stream) {
        // (stream priorities were tried for it, highest and lowest: no effect on any config beyond the runs' spread)
        ABC_HIP(ctx, hipStreamCreateWithFlags(&ctx->wx_stream, hipStreamNonBlocking));
        ABC_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_wx_fork, abc_xstream_event_flags()));
        ABC_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_wx_done, abc_xstream_event_flags()));
        ABC_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_wx_scores, abc_xstream_event_flags()));
    }
    if (simple) ABC_TRY(launch_simple_model(ctx, stats, io->obs, M, Pstat, model));
    else ABC_TRY(launch_pls_model(ctx, stats, io->obs, M, P, A, cfg->rule, model, wx_spec ? ctx->ev_wx_fork : nullptr));
    // the taus2 streams of the proposals (draws, seeds) need the rng state only: on the side stream, forked behind the Gram
    // kernel (which wants the whole memory system) and running beside the reduce / model fit that leave the chip empty
    uint32_t* raw_early = nullptr;
    bool filled_early = false;
    if (early && uniform_w) {         // the uniform weights themselves (AbcUtil.cpp:543-544): nothing on the main stream reads them
        ABC_TRY(launch_fill(ctx, io->w, K, 1.0 / (double)K, ctx->side));
        filled_early = true;
    }
    // ... and so does everything the weight stage needs of the PREVIOUS set (scales, centre, scaled copy, limb tiles -- in the
    // order of the rows' norm tops where that saves the pair sums an MFMA).  Order on the side stream: the draws' taus2 outputs (pure
    // arithmetic: they run beside the Gram kernel without touching its memory system), the previous set's prologue (the pair sums
    // need it ~0.3 ms into the generation), THEN the seeds (an output nobody reads before the call returns): the moments' event,
    // which the main stream waits for in front of the resampling table, is recorded behind all of them on the same stream
    const bool weighted = io->w && K && Kp && io->theta_prev;
    const bool moments_side_possible = Nn && P <= 64 && K >= 2 && !uniform_w && ctx->side;
    const bool seeds_late = early && weighted && moments_side_possible;
    if (early) ABC_TRY(abc_rng_streams_early(ctx, rng, 0, Nn, seeds_late ? nullptr : io->seeds, Nn, &raw_early, parent_early, K));
    abc_wprev wprev;
    memset(&wprev, 0, sizeof(wprev));
    // (tried, round 6: the ranking's launches in front of the prologue's in this thread's order -- under rocprofv3 the selection's launches
    // arrive late behind the prologue's ten, 38 us of idle main stream; unprofiled the host is fast enough and the step is 11 us LONGER
    // that way, 0.609 against 0.597 ms outside the pair sums at configs[2]: the prologue then runs beside the selection instead of
    // beside the model fit's empty chip)
    if (weighted)
        ABC_TRY(abc_weights_prev_early(ctx, P, K, io->theta_prev, Kp, io->w_prev, io->dv_prev, &wprev));
    if (seeds_late) ABC_TRY(abc_rng_seeds_early(ctx, rng, 0, Nn, io->seeds, Nn));
    ctx->side_forked = false;
    // The Wilcoxon reduction of the component count goes BEHIND the side stream's launches in host order (round 5): the host looks
    // at the cascade's level counts between its launches, and whatever it has not queued by then waits for those looks -- queued
    // in front (rounds 1-4), the previous set's prologue and the taus2 streams started only after the reduction and the host's
    // ~90 us of enqueueing them showed as a bubble in front of the projection (rocprofv3 timeline, profiles/history/r05_timeline_*)
    // SPECULATION (round 5, second half): the ranking does not wait for the reduction.  The reduction can only LOWER the component
    // count of a response, and the count the distances use is the largest over the responses -- unchanged unless every response
    // that holds the maximum is reduced.  So projection, selection and gather are queued at once on the counts the fit wrote, the
    // cascade runs beside them on a stream of its own (it reads the model record, its decision goes to a buffer of its own), and
    // when the host has its result -- the ranking's kernels are long done by then -- either nothing has changed (the usual case:
    // the per-response counts are committed, the generation goes on) or the decision is committed and the three stages run again.
    // Whole generations on sets the cascade takes only (ranking-only calls and small sets: in stream order, as before).
    const bool wx_rule = !simple && cfg->rule == ABC_RULE_WILCOXON;
    // ROUND 6: the host LOOKS at the reduction in front of the weight stage again (round 5's first form), because the look has become
    // cheap: the cascade takes the LARGEST COUNT FIRST (wilcoxon.hip, k_wx_plan) -- level 0 over the tests of two to four responses
    // that hold it instead of all P (A - 1) --, so its verdict is there before the selection and the gather beside it have ended, and
    // a moved count costs the cascade's second half and the three ranking stages once more instead of the whole generation
    // (round 5's default queued everything up to the proposals on the fit's count first and repeated the generation).
    double* wx_dec = nullptr;
    abc_wx_run* wx_run = nullptr;
    struct WxGuard {          // an error return between the cascade's halves: its kernels still write into this call's arena
        abc_ctx* c; abc_wx_run** r;
        ~WxGuard() { if (*r) { launch_wilcoxon_abandon(c, *r, c->wx_stream); *r = nullptr; } }
    } wx_guard = {ctx, &wx_run};
    bool projected = false;                              // the ranking's projection queued by the cascade's first half (below)
    const double* scores_all = nullptr;                  // ... which has then left the scores of all rows (N x A, leading dimension N)
    if (wx_spec) {
        wx_dec = (double*)abc_ws_alloc(ctx, (P + 1) * 8);
        if (!wx_dec) ABC_FAIL(ctx, ABC_ERR_NOMEM, "generation: workspace exhausted");
        ABC_HIP(ctx, hipStreamWaitEvent(ctx->wx_stream, ctx->ev_wx_fork, 0));           // (the fit's completion: launch_pls_model above)
        // its first half -- plan, scores, the level-0 sweep and bounds -- is queued BEFORE the ranking (the host needs ~60 us to queue
        // the ranking's eight launches: the cascade started that much late behind them, rocprofv3 timeline)
        // ONE pass over X for both: the ranking's projection (main stream) also writes the validation rows' scores, all A
        // components, and the cascade's sweeps wait for it -- as two launches the validation half of X was read twice and the
        // second pass (51 us at configs[2]) ran beside the selection's kernels
        // (round 6: the pass leaves the scores of EVERY row, not only the validation half -- N x A doubles of this call's arena: should
        // the reduction lower the largest count, the distances are taken again from them, N x count x 8 bytes instead of X once more)
        struct ScoresArg { abc_ctx* ctx; hipStream_t main; const double* X; size_t N, M, P, A, ntrain; const double* model; double* dist; double* S_all; }
            sarg = {ctx, ctx->stream, io->X, N, M, P, A, (size_t)ntrain, model, dist, nullptr};
        if (!(N & 1)) sarg.S_all = (double*)abc_ws_alloc(ctx, N * A * 8);
        abc_wx_scores_hook hook = {
            [](void* a, double** S, size_t* sld) -> int {
                ScoresArg* q = (ScoresArg*)a;
                abc_ctx* c = q->ctx;
                hipStream_t wx = c->stream;
                double* S_half = nullptr;
                if (!q->S_all) {
                    S_half = (double*)abc_ws_alloc(c, (q->N - q->ntrain) * q->A * 8);
                    if (!S_half) { snprintf(c->err, sizeof(c->err), "generation: workspace exhausted"); return ABC_ERR_NOMEM; }
                }
                int rc;
                {
                    StreamScope on_main(c, q->main);
                    rc = q->S_all ? launch_project_distance_scores(c, q->X, q->N, q->N, q->M, q->P, q->A, q->model, q->dist, q->S_all, q->N, 0, c->ev_wx_scores)
                                  : launch_project_distance_scores(c, q->X, q->N, q->N, q->M, q->P, q->A, q->model, q->dist, S_half, q->N - q->ntrain, q->ntrain,
                                                                   c->ev_wx_scores);
                }
                if (rc == 0 && hipStreamWaitEvent(wx, c->ev_wx_scores, 0) != hipSuccess) rc = ABC_ERR_HIP;
                if (rc == 0) {
                    q->dist = nullptr;          // (taken)
                    *S = q->S_all ? q->S_all + q->ntrain : S_half;
                    *sld = q->S_all ? q->N : q->N - q->ntrain;
                } else if (rc == 1)
                    q->S_all = nullptr;         // (not a shape for the fused pass: no scores of all rows either)
                return rc;
            },
            &sarg};
        {
            StreamScope on_wx(ctx, ctx->wx_stream);
            // (level 0's sweep is held back until the selection and the gather are queued: the sweep cannot start before the projection
            // has ended anyway, and queued in front of them its three launches kept the selection from the main stream for ~65 us)
            ABC_TRY(launch_wilcoxon_begin(ctx, io->X, io->Y, N, N, N, M, P, A, (size_t)ntrain, model, wx_dec, /*stop_at_max=*/1, &wx_run, &hook,
                                          /*hold_level0=*/1));
        }
        projected = sarg.dist == nullptr;
        scores_all = projected ? sarg.S_all : nullptr;
    } else if (wx_rule)
        ABC_TRY(launch_wilcoxon(ctx, io->X, io->Y, N, N, N, M, P, A, (size_t)ntrain, model));
    if (!projected) ABC_TRY(launch_project_distance(ctx, io->X, N, N, M, simple ? Pstat : P, A, model, simple, dist));
    if (K == 0) return ABC_OK;
    ABC_TRY(launch_select_smallest(ctx, dist, N, K, 0, io->idx, io->dist, /*defer_check=*/io->w != nullptr));
    // (tried, round 6: level 0 of the cascade held BEHIND the selection where the gather is long enough to hide it -- at configs[3] the
    // sweep beside the selection's histogram pass stretches that from 45 to 164 us, and the 0.6 ms gather behind it has room for the
    // sweep: everything but the pair sums 6.60 -> 6.69 ms, the gather loses more than the histogram gains.  Not kept.)
    if (!simple && ncomp_host && !io->w) {
        double hdr[4];
        ABC_HIP(ctx, hipMemcpyAsync(hdr, model, sizeof(hdr), hipMemcpyDeviceToHost, ctx->stream));
        ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *ncomp_host = (int32_t)hdr[0];
    }
    if (!io->w) return ABC_OK;   // ranking only

    double* theta = io->theta ? io->theta : (double*)abc_ws_alloc(ctx, K * P * 8);
    if (!theta) ABC_FAIL(ctx, ABC_ERR_NOMEM, "generation: workspace exhausted");
    // (the gather is the first kernel behind the selection: it also stores the selection's give-up flag into the pinned block)
    int* pfail_early = &ctx->status_pin->gather_sel_fail;
    *pfail_early = 0;
    volatile unsigned* pgaveup = &ctx->status_pin->giveup_flag;       // raised by a proposal kernel that gives up (note_giveup)
    *pgaveup = 0u;
    // the status words the host reads at the generation's end (model header, Cholesky status): zeroed here, written by the
    // posterior's k_post_tail where that kernel runs -- the copy kernel behind the proposals is then not launched
    double* const hdr_pin = ctx->status_pin->model_hdr;
    int* const spd_pin = &ctx->status_pin->spd;
    hdr_pin[0] = 0.0; *spd_pin = 0;
    bool status_early = false;
    bool bins_deferred = ctx->sel_bins_ran && ctx->sel_fail_dev && !ctx->sel_force_radix;
    // The main stream needs what the side stream queued early (the previous set's tiles, the taus2 outputs) only behind the
    // gather, and those kernels ended long ago: the wait goes IN FRONT of the gather, where the event is certain to have fired
    // (a wait that still has to be resolved between the gather and the new set's tiles cost ~12 us of the critical path there)
    ctx->side_early_waited = false;
    if (wprev.ready) {
        ABC_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_prev, 0));
        ctx->side_early_waited = true;                 // (ev_prev was recorded behind ev_side on the same stream)
    }
    // (weighted generations hand the gathered rows to the side stream, for the posterior's moments: the event that orders the two
    // is the gather's own completion signal, not a record behind it)
    const bool defer_moments = Nn && P <= 64 && K >= 2;
    const bool moments_side_planned = defer_moments && !uniform_w && ctx->side && ctx->noise_mode != ABC_NOISE_REFERENCE_STREAM;
    if (moments_side_planned && !ctx->ev_theta) {
        ABC_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_theta, abc_xstream_event_flags()));
        ABC_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_moments, abc_xstream_event_flags()));
    }
    const bool theta_ev_bound = moments_side_planned;
    ABC_TRY(launch_gather_rows(ctx, io->Y, N, N, P, io->idx, K, 0, theta, K, bins_deferred ? ctx->sel_fail_dev : nullptr, pfail_early,
                               theta_ev_bound ? ctx->ev_theta : nullptr));
    if (wx_run) {                                        // level 0 of the cascade, behind the ranking's launches in host order
        StreamScope on_wx(ctx, ctx->wx_stream);
        ABC_TRY(launch_wilcoxon_level0(ctx, wx_run));
    }
    // Where the host looks at the cascade: HERE, in front of the weight stage (round 6; round 5's first form).  The verdict of the
    // cascade's first half -- the tests of a few responses that hold the largest count -- is there by the time the gather ends; a count
    // that stands costs nothing, a count that moved costs the cascade's second half and the ranking once more (distances from the
    // kept scores, selection, gather).
    bool wx_tail_pending = false;
    if (wx_spec) {
        // the reduction itself, on its own stream, while the ranking queued above runs (the host's looks at the cascade's level
        // counts happen here, beside GPU work that does not depend on them)
        int changed = 2, rc;
        {
            StreamScope on_wx(ctx, ctx->wx_stream);
            rc = launch_wilcoxon_finish(ctx, wx_run, &changed);
            wx_run = nullptr;
            if (rc == ABC_OK && hipEventRecord(ctx->ev_wx_done, ctx->wx_stream) != hipSuccess) rc = ABC_ERR_HIP;
        }
        if (rc == ABC_INTERNAL_RETRY) {          // a bin of its exact step outgrew LDS (massive ties): once more in stream order, on the sorted path
            ABC_HIP(ctx, hipStreamSynchronize(ctx->wx_stream));
            ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            rc = launch_wilcoxon(ctx, io->X, io->Y, N, N, N, M, P, A, (size_t)ntrain, model);
            changed = 2;
        }
        if (rc != ABC_OK) { if (!ctx->err[0]) snprintf(ctx->err, sizeof(ctx->err), "generation: the component rule's reduction failed"); return rc; }
        if (changed == 1) {                      // the counts AND the header, in front of the ranking's second run
            ABC_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_wx_done, 0));
            ABC_TRY(launch_wilcoxon_commit(ctx, model, M, P, A, wx_dec, 1));
        } else if (changed == 0) {
            // the per-response counts into the model record on the cascade's own stream: nothing this generation still queues reads
            // them (the largest count, which everything used, is the fit's); the host waits for that stream at the generation's end
            StreamScope on_wx(ctx, ctx->wx_stream);
            ABC_TRY(launch_wilcoxon_commit(ctx, model, M, P, A, wx_dec, 0));
            wx_tail_pending = true;
        }
        if (changed) {                           // the largest count moved: the ranking once more, with it
            ctx->wx_moved_counts++;
            // (the second selection's give-up flag goes to a word of its own in the pinned block: the first gather may still be
            // running -- resetting ITS word would need a wait for the stream here, ~15 us of idle GPU in front of the repeat)
            pfail_early = &ctx->status_pin->repeat_sel_fail;
            *pfail_early = 0;
            if (scores_all) ABC_TRY(launch_distance_from_scores(ctx, scores_all, N, N, M, P, A, model, dist));
            else ABC_TRY(launch_project_distance(ctx, io->X, N, N, M, P, A, model, 0, dist));
            ABC_TRY(launch_select_smallest(ctx, dist, N, K, 0, io->idx, io->dist, /*defer_check=*/true));
            bins_deferred = ctx->sel_bins_ran && ctx->sel_fail_dev && !ctx->sel_force_radix;
            ABC_TRY(launch_gather_rows(ctx, io->Y, N, N, P, io->idx, K, 0, theta, K, bins_deferred ? ctx->sel_fail_dev : nullptr, pfail_early,
                                       theta_ev_bound ? ctx->ev_theta : nullptr));
        }
    }
    // A failed bin selection (degenerate distances) leaves placeholder winners: everything downstream of it is repeated with
    // the radix select.  Weighted generations learn of it at the host's wait for the weights (launch_resample's abort flag),
    // before the alias table, the draws and the proposals of the placeholder are queued; set 0 has no host wait before its
    // end and finds out there.  Either way the proposals' give-up counter is put back to its snapshot.
    auto repeat_with_radix = [&]() -> int {
        ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->side) ABC_HIP(ctx, hipStreamSynchronize(ctx->side));
        if (ctx->wx_stream) ABC_HIP(ctx, hipStreamSynchronize(ctx->wx_stream));
        if (ctx->giveups_dev)
            ABC_HIP(ctx, hipMemcpyAsync(ctx->giveups_dev, ctx->giveups_dev + 1, sizeof(unsigned long long), hipMemcpyDeviceToDevice, ctx->stream));
        ctx->sel_bins_ran = false;
        ctx->ws_off = ws_entry;
        if (rng) *rng = rng_entry;
        ctx->generation_repeats++;
        const bool radix0 = ctx->sel_force_radix;      // (a repeat inside a repeat keeps the outer one's reason)
        ctx->sel_force_radix = true;
        const int rc = generation_core(ctx, cfg, io, rng, ncomp_host, simple, model_out);
        ctx->sel_force_radix = radix0;
        return rc;
    };
    double* dv = io->dv ? io->dv : (double*)abc_ws_alloc(ctx, P * 8);
    double* theta_stats = nullptr;        // moments of the posterior: shared by dv and the MVN factor
    // Weighted generations with proposals: the kernel density of the weights uses the PREVIOUS set's variance, so the new set's
    // moments (pilot shift, Gram, reduce, dv: 25 us of small launches) are not needed before the host's alias round trip --
    // they run in the GPU's idle time behind it (hook below) instead of in front of the pair sums.
    // (set 0 too: nothing in front of the proposals needs them, and up to 16 parameters ONE launch then delivers the moments,
    // the doubled variance, the proposal factor and the perturbation's row-major copy: k_theta_moments)
    if (defer_moments) {
    } else if (P <= 64 && K >= 2) {
        StageTimer tm(ctx, ST_GATHER_DV);
        ABC_TRY(launch_theta_stats(ctx, theta, K, P, &theta_stats));
        ABC_TRY(launch_dv_from_stats(ctx, theta_stats, P, dv));
    } else {
        ABC_TRY(launch_doubled_variance(ctx, theta, K, P, dv));
    }
    bool w_on_host = false;
    if (Kp == 0 || !io->theta_prev) {
        if (!filled_early) ABC_TRY(launch_fill(ctx, io->w, K, 1.0 / (double)K));                 // AbcUtil.cpp:543-544
    } else {
        if (wprev.ready && !ctx->side_early_waited) ABC_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_prev, 0));
        const double* sumsq = nullptr;       // the normalisation's sum of squares comes out of the weight stage's last kernel
        ABC_TRY(launch_weights_raw(ctx, io->priors, theta, K, P, 0, K, io->theta_prev, Kp, io->w_prev, io->dv_prev,
                                   io->w, &wprev, &sumsq));
        ABC_TRY(abc_normalize_for_resample(ctx, io->w, K, Nn, sumsq, &w_on_host));
    }
    // (queued BEHIND the weight stage's launches since round 5: with the ranking speculating beside the Wilcoxon cascade the host
    // arrives here late, and the side stream's four launches in front of them delayed the pair sums by their enqueue time)
    // The posterior's moments and what follows from them (doubled variance, proposal factor, the perturbation's row-major copy
    // and padded factor) need the gathered rows only: with the resampling table built on the device nothing waits for the host
    // any more, so they run on the SIDE stream from here on, beside the weight stage, and are long done when the proposals need
    // them (round 2 hid them behind the host's alias build).
    abc_side_moments side = {};
    bool moments_on_side = false, seeds_waited = false;
    // (set 0 has nothing to overlap them with: two cross-stream hand-overs for nothing, measured +35 us)
    if (moments_side_planned) {
        ABC_TRY(abc_moments_on_side(ctx, theta, K, P, cfg->multivariate != 0, io->L, dv, spd_dev, simple ? nullptr : model, theta_ev_bound,
                                    "generation", &side));
        theta_stats = side.stats;
        moments_on_side = status_early = true;
    }
    int spd = 0;
    bool have_spd = false;
    int alias_deferred = 0;
    uint64_t* parent_used = nullptr;
    double* L_used = nullptr;
    abc_perturb_prep prep_used = {nullptr, 0, nullptr};
    if (Nn) {
        uint64_t* parent = parent_early ? parent_early : (io->parent ? io->parent : (uint64_t*)abc_ws_alloc(ctx, Nn * 8));
        if (!parent) ABC_FAIL(ctx, ABC_ERR_NOMEM, "generation: workspace exhausted");
        double* L = nullptr;
        if (cfg->multivariate) {
            L = side.L ? side.L : (io->L ? io->L : (double*)abc_ws_alloc(ctx, P * P * 8));
            have_spd = true;
        }
        // (side.out: nulls unless the moments went to the side stream)
        abc_perturb_prep prep = {side.out.rows, (early && io->seeds) ? 1 : 0, side.out.Lpad};
        if (moments_on_side) { ABC_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_moments, 0)); seeds_waited = true; }   // (recorded behind the seeds)
        // (abc_prep_hook: what does not depend on the weights, beside the alias table's host round trip inside launch_resample)
        const bool hook_moments = defer_moments && !moments_on_side;
        abc_prep_arg pa = {ctx, rng, theta, theta_stats, K, P, Nn, 0, Nn, io->seeds, &prep, moments_on_side ? nullptr : L, spd_dev, dv,
                           hook_moments, nullptr, nullptr, nullptr};
        if (hook_moments) {
            pa.model_hdr = simple ? nullptr : model; pa.hdr_pin = hdr_pin; pa.spd_pin = L ? spd_pin : nullptr;
            status_early = true;
        }
        {
            const int rc = launch_resample(ctx, rng, io->w, K, 0, Nn, parent, abc_prep_hook, &pa, uniform_w, raw_early, w_on_host,
                                           bins_deferred ? pfail_early : nullptr, parent_early != nullptr,
                                           ctx->noise_mode == ABC_NOISE_REFERENCE_STREAM ? nullptr : &alias_deferred);
            if (rc == ABC_INTERNAL_RETRY) return repeat_with_radix();
            ABC_TRY(rc);
        }
        if (ctx->noise_mode == ABC_NOISE_REFERENCE_STREAM) {
            taus2_jump(rng, (uint64_t)Nn);   // the Nnext resampling draws; the host loop consumes the rest as the reference does
            ABC_TRY(launch_perturb_reference(ctx, rng, theta, K, P, io->priors, parent, Nn, cfg->multivariate,
                                             cfg->multivariate ? L : dv, io->next, io->seeds));
        } else {
            ABC_TRY(launch_perturb(ctx, rng, theta, K, P, io->priors, parent, 0, Nn, cfg->multivariate,
                                   cfg->multivariate ? L : dv, io->next, io->seeds, Nn, &prep));
            parent_used = parent; L_used = L; prep_used = prep;
            taus2_jump(rng, 2 * (uint64_t)Nn);   // Nnext resampling draws + Nnext seeds
        }
    }
    {
        // status words into the pinned block: model header (component count), Cholesky status, selection flag
        double* hdr = ctx->status_pin->model_hdr;
        int* pspd = &ctx->status_pin->spd;
        int* pfail = &ctx->status_pin->sel_fail;
        if (!status_early) { hdr[0] = 0.0; *pspd = 0; }
        *pfail = 0;
        if (seeds_late && !seeds_waited) ABC_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_side, 0));     // (never in practice: see below)
        // ONE tiny kernel stores the three words into the (device-visible) pinned block: three copies were three blit launches
        const int* fail_dev = (ctx->sel_bins_ran && ctx->sel_fail_dev) ? (const int*)ctx->sel_fail_dev : nullptr;
        unsigned long long* pgive = &ctx->status_pin->giveups;
        *pgive = 0;
        if (!status_early) {
            hipLaunchKernelGGL(k_status_words, dim3(1), dim3(64), 0, ctx->stream, simple ? (const double*)nullptr : (const double*)model,
                               have_spd ? (const int*)spd_dev : (const int*)nullptr, fail_dev, (const unsigned long long*)ctx->giveups_dev, hdr, pspd,
                               pfail, pgive);
            ABC_HIP(ctx, hipGetLastError());
        }
        ctx->side_early_waited = false;
        ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (wx_tail_pending) ABC_HIP(ctx, hipStreamSynchronize(ctx->wx_stream));
        if (status_early) {
            // header and Cholesky status came from k_post_tail, the selection's flag from the gather (bins_deferred), the proposals'
            // give-up counter is read only when a proposal kernel raised the flag word
            *pfail = fail_dev ? *(volatile int*)pfail_early : 0;
        } else {
            ctx->giveups_dev_known = *(volatile unsigned long long*)pgive;
        }
        if (ncomp_host) *ncomp_host = (int32_t)hdr[0];
        spd = *pspd;
        // the sampled-range bin selection gave up (degenerate distances, an atypical sample): everything downstream of it
        // worked on a placeholder; once more, from the top, with the radix select
        const int failed = abc_select_check_done(ctx, pfail);
        if (failed && !ctx->sel_force_radix) return repeat_with_radix();
        // the device build of the resampling table did not verify: the draws and the proposals once more, with the table from the
        // host (the weights are final; only what depends on the table is repeated)
        if (alias_deferred && *(volatile int*)&ctx->status_pin->alias_fail && parent_used) {
            ABC_TRY(abc_alias_repair(ctx, &rng_entry, io->w, K, 0, Nn, Nn, parent_used, theta, P, io->priors, cfg->multivariate,
                                     cfg->multivariate ? L_used : dv, io->next, &prep_used, /*giveups_to_snapshot=*/true));
        }
    }
    if (ctx->timing && ctx->nev > 128) ABC_TRY(abc_timing_flush(ctx));
    if (spd) ABC_FAIL(ctx, ABC_ERR_NOT_SPD, "covariance of the selected particles is not positive definite");
    // proposals the perturbation gave up on during THIS call (the reference never returns in that case, AbcUtil.cpp:132): the
    // outputs are complete -- such a row is its (valid) parent, or the prior mean in INDEPENDENT mode -- and the caller is told
    {
        if (status_early) {
            if (*pgaveup && ctx->giveups_dev) {           // (rare) a proposal kernel gave up: fetch the counter
                unsigned long long now = 0;
                ABC_HIP(ctx, hipMemcpyAsync(&now, ctx->giveups_dev, sizeof(now), hipMemcpyDeviceToHost, ctx->stream));
                ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
                ctx->giveups_dev_known = now;
            }
            *(volatile unsigned long long*)&ctx->status_pin->giveups = ctx->giveups_dev_known;
        }
        const unsigned long long gv = *(volatile unsigned long long*)&ctx->status_pin->giveups + ctx->giveups_host;
        const unsigned long long before = ctx->giveups_seen;
        ctx->giveups_seen = gv;
        // (status stays ABC_OK: a C caller's `if (rc)` must not read a finished generation as a failure; abc_generation_giveups)
        ctx->giveups_last_call = (Nn && gv > before) ? gv - before : 0ull;
    }
    return ABC_OK;
}

extern "C" int abc_generation_dev(abc_ctx* ctx, const abc_generation_cfg* cfg, const abc_generation_io* io, abc_rng* rng,
                                  int32_t* ncomp_host) {
    CHECK_CTX(ctx);
    if (!cfg || !io || !io->X || !io->obs || !io->idx) ABC_FAIL(ctx, ABC_ERR_INVALID, "generation: null argument");
    const size_t A = default_A(cfg->M, cfg->P, cfg->max_comp);
    size_t need = abc_ws_need(cfg->N, cfg->M, cfg->P, A, cfg->K, cfg->Kp, cfg->Nnext);
    if (cfg->rule == ABC_RULE_WILCOXON) need += abc_wx_need(cfg->N, cfg->P, A) + cfg->N * A * 8 + 4096;      // (+ the scores of all rows)
    ABC_TRY(abc_ws_reserve(ctx, need));
    return generation_core(ctx, cfg, io, rng, ncomp_host, 0);
}

// ---- host-pointer entry points ---------------------------------------------------------------------
namespace {
struct Stage {   // host<->device staging inside the arena
    abc_ctx* ctx;
    bool full = false;   // some allocation found the arena exhausted (and returned NULL)
    template <typename T>
    T* up(const T* h, size_t n) {
        T* d = dev<T>(n);
        if (d && h && n) (void)hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream);
        return d;
    }
    template <typename T>
    T* dev(size_t n) {
        T* d = (T*)abc_ws_alloc(ctx, n * sizeof(T));
        if (!d) full = true;
        return d;
    }
    template <typename T>
    void down(T* h, const T* d, size_t n) {
        if (h && d && n) (void)hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream);
    }
};
}  // namespace

static int ranking_host(abc_ctx* ctx, const double* X, const double* Y, const double* obs, size_t N, size_t M,
                        size_t P, double train_frac, int max_comp, int rule, size_t K, uint64_t* idx, double* dist,
                        int32_t* ncomp, double* R, double* mean, double* sd, int simple) {
    if (!X || !obs || !idx || (!simple && !Y)) ABC_FAIL(ctx, ABC_ERR_INVALID, "ranking: null argument");
    const size_t A = simple ? 0 : default_A(M, P, max_comp);
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(N, M, P, A, K, 0, 0) + (N * (M + P) + M + 2 * K) * 8 +
                                    ((!simple && rule == ABC_RULE_WILCOXON) ? abc_wx_need(N, P, A) : 0)));
    Stage s{ctx};
    abc_generation_io io;
    memset(&io, 0, sizeof(io));
    io.X = s.up(X, N * M);
    io.Y = simple ? nullptr : s.up(Y, N * P);
    io.obs = s.up(obs, M);
    io.idx = s.dev<uint64_t>(K);
    io.dist = s.dev<double>(K);
    if (!io.X || !io.obs || !io.idx || !io.dist) ABC_FAIL(ctx, ABC_ERR_NOMEM, "ranking: workspace exhausted");
    abc_generation_cfg cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.N = N; cfg.M = M; cfg.P = simple ? 0 : P; cfg.K = K; cfg.train_frac = train_frac;
    cfg.max_comp = max_comp; cfg.rule = rule;
    const double* model = nullptr;
    ABC_TRY(generation_core(ctx, &cfg, &io, nullptr, ncomp, simple, &model));
    s.down(idx, io.idx, K);
    s.down(dist, io.dist, K);
    if (R || mean || sd) {
        const ModelLayout ML = model_layout(M, simple ? 0 : P, A);
        if (R && !simple) s.down(R, model + ML.off_R, M * A);
        s.down(mean, model + ML.off_mean, M);
        s.down(sd, model + ML.off_sd, M);
    }
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}

extern "C" int abc_particle_ranking_pls(abc_ctx* ctx, const double* X, const double* Y, const double* obs, size_t N,
                                        size_t M, size_t P, double train_frac, int max_comp, int rule, size_t K,
                                        uint64_t* idx, double* dist, int32_t* ncomp, double* R, double* mean,
                                        double* sd) {
    CHECK_CTX(ctx);
    return ranking_host(ctx, X, Y, obs, N, M, P, train_frac, max_comp, rule, K, idx, dist, ncomp, R, mean, sd, 0);
}

extern "C" int abc_particle_ranking_simple(abc_ctx* ctx, const double* X, const double* obs, size_t N, size_t M,
                                           size_t K, uint64_t* idx, double* dist) {
    CHECK_CTX(ctx);
    return ranking_host(ctx, X, nullptr, obs, N, M, 0, 1.0, 0, 0, K, idx, dist, nullptr, nullptr, nullptr, nullptr, 1);
}

extern "C" int abc_calculate_doubled_variance(abc_ctx* ctx, const double* theta, size_t K, size_t P, double* dv) {
    CHECK_CTX(ctx);
    if (!theta || !dv) ABC_FAIL(ctx, ABC_ERR_INVALID, "doubled_variance: null argument");
    ABC_TRY(abc_ws_reserve(ctx, (K * P + P) * 8 + (1 << 20)));
    Stage s{ctx};
    double* dth = s.up(theta, K * P);
    double* ddv = s.dev<double>(P);
    ABC_TRY(launch_doubled_variance(ctx, dth, K, P, ddv));
    s.down(dv, ddv, P);
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ABC_OK;
}

extern "C" int abc_weight_predictive_prior_uniform(abc_ctx* ctx, size_t K, double* w) {
    CHECK_CTX(ctx);
    if (!w || !K) ABC_FAIL(ctx, ABC_ERR_INVALID, "weights: null argument");
    ABC_TRY(abc_ws_reserve(ctx, K * 8 + (1 << 20)));
    Stage s{ctx};
    double* dw = s.dev<double>(K);
    ABC_TRY(launch_fill(ctx, dw, K, 1.0 / (double)K));
    s.down(w, dw, K);
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ABC_OK;
}

extern "C" int abc_weight_predictive_prior(abc_ctx* ctx, const abc_prior* priors, const double* theta, size_t K,
                                           size_t P, const double* theta_prev, size_t Kp, const double* w_prev,
                                           const double* dv_prev, double* w) {
    CHECK_CTX(ctx);
    if (!priors || !theta || !theta_prev || !w_prev || !dv_prev || !w)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "weights: null argument");
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(0, 1, P, 1, K, Kp, 0) + ((K + Kp) * (P + 1) + 2 * P) * 8 + P * sizeof(abc_prior)));
    Stage s{ctx};
    abc_prior* dpr = s.up(priors, P);
    double* dth = s.up(theta, K * P);
    double* dtp = s.up(theta_prev, Kp * P);
    double* dwp = s.up(w_prev, Kp);
    double* ddv = s.up(dv_prev, P);
    double* dw = s.dev<double>(K);
    if (!dpr || !dth || !dtp || !dwp || !ddv || !dw) ABC_FAIL(ctx, ABC_ERR_NOMEM, "weights: workspace exhausted");
    ABC_TRY(launch_weights_raw(ctx, dpr, dth, K, P, 0, K, dtp, Kp, dwp, ddv, dw));
    ABC_TRY(launch_normalize_l2(ctx, dw, K));
    s.down(w, dw, K);
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ABC_OK;
}

extern "C" int abc_setup_mvn_sampler(abc_ctx* ctx, const double* theta, size_t K, size_t P, double* L) {
    CHECK_CTX(ctx);
    if (!theta || !L) ABC_FAIL(ctx, ABC_ERR_INVALID, "mvn: null argument");
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(0, P, 0, 1, 0, 0, 0) + (K * P + P * P) * 8));
    Stage s{ctx};
    double* dth = s.up(theta, K * P);
    double* dL = s.dev<double>(P * P);
    int st = 0;
    ABC_TRY(launch_mvn_setup(ctx, dth, K, P, dL, &st, nullptr));
    if (st) ABC_FAIL(ctx, ABC_ERR_NOT_SPD, "covariance of the selected particles is not positive definite");
    s.down(L, dL, P * P);
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ABC_OK;
}

extern "C" int abc_sample_posterior(abc_ctx* ctx, abc_rng* rng, const double* w, size_t K, size_t n, uint64_t* idx) {
    CHECK_CTX(ctx);
    if (!rng || !w || !idx) ABC_FAIL(ctx, ABC_ERR_INVALID, "sample_posterior: null argument");
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(0, 1, 1, 1, 0, 0, n) + K * 8 + n * 8 + abc_alias_dev_need(K)));
    Stage s{ctx};
    double* dw = s.up(w, K);
    uint64_t* dp = s.dev<uint64_t>(n);
    ABC_TRY(launch_resample(ctx, rng, dw, K, 0, n, dp));
    s.down(idx, dp, n);
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    taus2_jump(rng, n);
    return ABC_OK;
}

// the resampling table as this context builds it (for inspection / tests): F with GSL's KNUTH_CONVENTION applied
extern "C" int abc_alias_table(abc_ctx* ctx, const double* w, size_t K, double* F, uint64_t* A, int* on_device) {
    CHECK_CTX(ctx);
    if (!w || !F || !A || !K || K > 0xffffffffull) ABC_FAIL(ctx, ABC_ERR_INVALID, "alias table: null argument or K = %zu", K);
    if (on_device) *on_device = 0;
    std::vector<double> hF(K);
    std::vector<uint32_t> hA(K);
    bool done = false;
    if (ctx->alias_mode == ABC_ALIAS_DEVICE && K >= 2 && K <= ABC_ALIAS_DEV_MAX_K) {
        ABC_TRY(abc_ws_reserve(ctx, abc_alias_dev_need(K) + K * 20 + (1u << 20)));
        Stage s{ctx};
        double* dw = s.up(w, K);
        double* dF = s.dev<double>(K);
        uint32_t* dA = s.dev<uint32_t>(K);
        int* dfail = s.dev<int>(1);
        if (!dw || !dF || !dA || !dfail) ABC_FAIL(ctx, ABC_ERR_NOMEM, "alias table: workspace exhausted");
        ABC_TRY(launch_alias_build_dev(ctx, dw, K, dF, dA, dfail, nullptr));
        int fail = 0;
        ctx->alias_dev_builds++;
        s.down(hF.data(), (const double*)dF, K);
        s.down(hA.data(), (const uint32_t*)dA, K);
        s.down(&fail, (const int*)dfail, 1);
        ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (fail) ctx->alias_dev_fallbacks++; else done = true;
        if (done && on_device) *on_device = 1;
    }
    if (!done) {
        std::vector<double> E(K);
        std::vector<uint32_t> S(K + 1), B(K + 1);
        abc_alias_preproc(K, w, hF.data(), hA.data(), E.data(), S.data(), B.data(), /*knuth=*/false);
    }
    const double dK = (double)K;
    for (size_t k = 0; k < K; k++) { F[k] = (hF[k] + (double)k) / dK; A[k] = hA[k]; }      // KNUTH_CONVENTION, as k_alias_draw applies it
    return ABC_OK;
}

static int sample_host(abc_ctx* ctx, abc_rng* rng, size_t n, const double* w, const double* theta, size_t K, size_t P,
                       const abc_prior* priors, const double* L_or_dv, int multivariate, double* out, uint64_t* parent,
                       uint64_t* seeds) {
    if (!rng || !w || !theta || !priors || !L_or_dv || !out) ABC_FAIL(ctx, ABC_ERR_INVALID, "sample: null argument");
    ABC_TRY(abc_ws_reserve(ctx, abc_ws_need(0, 1, P, 1, K, 0, n) + (K * (P + 1) + P * P + n * (P + 2)) * 8 + P * sizeof(abc_prior)));
    Stage s{ctx};
    double* dw = s.up(w, K);
    double* dth = s.up(theta, K * P);
    abc_prior* dpr = s.up(priors, P);
    double* dl = s.up(L_or_dv, multivariate ? P * P : P);
    double* dout = s.dev<double>(n * P);
    uint64_t* dpar = s.dev<uint64_t>(n);
    uint64_t* dseed = seeds ? s.dev<uint64_t>(n) : nullptr;
    if (!dw || !dth || !dpr || !dl || !dout || !dpar) ABC_FAIL(ctx, ABC_ERR_NOMEM, "sample: workspace exhausted");
    ABC_TRY(launch_resample(ctx, rng, dw, K, 0, n, dpar));
    if (ctx->noise_mode == ABC_NOISE_REFERENCE_STREAM) {
        taus2_jump(rng, (uint64_t)n);
        ABC_TRY(launch_perturb_reference(ctx, rng, dth, K, P, dpr, dpar, n, multivariate, dl, dout, dseed));
    } else {
        ABC_TRY(launch_perturb(ctx, rng, dth, K, P, dpr, dpar, 0, n, multivariate, dl, dout, dseed, n));
        taus2_jump(rng, seeds ? 2 * (uint64_t)n : (uint64_t)n);
    }
    s.down(out, dout, n * P);
    s.down(parent, dpar, n);
    s.down(seeds, dseed, n);
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ABC_OK;
}

extern "C" int abc_sample_mvn_predictive_priors(abc_ctx* ctx, abc_rng* rng, size_t n, const double* w,
                                                const double* theta, size_t K, size_t P, const abc_prior* priors,
                                                const double* L, double* out, uint64_t* parent, uint64_t* seeds) {
    CHECK_CTX(ctx);
    return sample_host(ctx, rng, n, w, theta, K, P, priors, L, 1, out, parent, seeds);
}

extern "C" int abc_sample_predictive_priors(abc_ctx* ctx, abc_rng* rng, size_t n, const double* w, const double* theta,
                                            size_t K, size_t P, const abc_prior* priors, const double* dv, double* out,
                                            uint64_t* parent, uint64_t* seeds) {
    CHECK_CTX(ctx);
    return sample_host(ctx, rng, n, w, theta, K, P, priors, dv, 0, out, parent, seeds);
}

// ---- batched ranking of many observed targets against one fitted set (targets.hip), optionally followed by the local-linear
// adjustment (adjust.hip) or by a posterior product of every target's retained rows: the weighted quantiles and CDF (summary.hip),
// the densities and modes (density.hip), the joint moments and pair densities (joint.hip), the posterior draws (draws.hip), the
// posterior entropy (entropy.hip) or the highest-density intervals (summary.hip).  One pipeline (tg_*) behind the eighteen entry
// points of the family and one pair of paths (weighted_dev, weighted_host) behind the twelve abc_weighted_* entries, which
// compute the same products from given values; what differs between the products is in Product ----
static int summary_check(abc_ctx* ctx, const char* fn, const abc_summary* sum) {
    if (!sum) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (sum is required)", fn);
    if (sum->nq == 0 || sum->nq > 64) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: nq = %zu levels (1 to 64)", fn, sum->nq);
    if (!sum->probs) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (probs is required)", fn);
    for (size_t q = 0; q < sum->nq; q++)
        if (!(sum->probs[q] >= 0.0 && sum->probs[q] <= 1.0))
            ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: probs[%zu] = %g is not a level in [0, 1]", fn, q, sum->probs[q]);
    if (sum->cdf && !sum->truth) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: cdf requires truth", fn);
    return ABC_OK;
}

static int density_check(abc_ctx* ctx, const char* fn, const abc_density* den) {
    if (!den) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (den is required)", fn);
    if (den->G < 2 || den->G > 4096) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: G = %zu grid points (2 to 4096)", fn, den->G);
    if (!(den->cut >= 0.0) || !std::isfinite(den->cut)) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: cut = %g (finite, >= 0)", fn, den->cut);
    if (!(den->bw_scale > 0.0) || !std::isfinite(den->bw_scale))
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: bw_scale = %g (finite, > 0)", fn, den->bw_scale);
    if (!den->dens && !den->grid && !den->bw_out && !den->mode && !den->mode_dens)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: every output member of den is NULL", fn);
    return ABC_OK;
}

static int joint_check(abc_ctx* ctx, const char* fn, const abc_joint* jt, size_t P) {
    if (!jt) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (jt is required)", fn);
    if (jt->G < 2 || jt->G > 256) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: G = %zu grid points per axis (2 to 256)", fn, jt->G);
    if (!(jt->cut >= 0.0) || !std::isfinite(jt->cut)) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: cut = %g (finite, >= 0)", fn, jt->cut);
    if (!(jt->bw_scale > 0.0) || !std::isfinite(jt->bw_scale))
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: bw_scale = %g (finite, > 0)", fn, jt->bw_scale);
    if (jt->pairs) {
        if (jt->npairs == 0) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: pairs given with npairs == 0", fn);
        if (jt->npairs > ((size_t)1 << 22)) ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: npairs = %zu (at most 2^22)", fn, jt->npairs);
        for (size_t p = 0; p < jt->npairs; p++) {
            const int32_t i = jt->pairs[2 * p], j = jt->pairs[2 * p + 1];
            if (i < 0 || j < 0 || (size_t)i >= P || (size_t)j >= P || i == j)
                ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: pairs[%zu] = (%d, %d) is not a pair of two of the %zu parameters", fn, p, (int)i,
                         (int)j, P);
        }
    }
    if (!jt->mean && !jt->cov && !jt->corr && !jt->dens && !jt->grid && !jt->bw_out && !jt->mode && !jt->mode_dens)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: every output member of jt is NULL", fn);
    return ABC_OK;
}

static int draws_check(abc_ctx* ctx, const char* fn, const abc_draws* dr) {
    if (!dr) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (dr is required)", fn);
    if (dr->S == 0 || dr->S > ((size_t)1 << 24)) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: S = %zu draws per target (1 to 2^24)", fn, dr->S);
    if (dr->smooth != 0 && dr->smooth != 1)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: smooth %d (0 = weighted, 1 = smoothed bootstrap)", fn, dr->smooth);
    if (dr->smooth && (!(dr->bw_scale > 0.0) || !std::isfinite(dr->bw_scale)))
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: bw_scale = %g (finite, > 0)", fn, dr->bw_scale);
    if (!dr->draws && !dr->src && !dr->bw_out && !dr->ess) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: every output member of dr is NULL", fn);
    return ABC_OK;
}

static int entropy_check(abc_ctx* ctx, const char* fn, const abc_entropy* en, size_t P) {
    if (!en) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (en is required)", fn);
    if (en->k < 1 || en->k > 8) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: k = %d neighbours (1 to 8)", fn, en->k);
    if (!en->H && !en->knn && !en->zeros) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: every output member of en is NULL", fn);
    if (en->scale)
        for (size_t j = 0; j < P; j++)
            if (!(en->scale[j] > 0.0) || !std::isfinite(en->scale[j]))
                ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: scale[%zu] = %g (finite, > 0)", fn, j, en->scale[j]);
    return ABC_OK;
}

static int hpd_check(abc_ctx* ctx, const char* fn, const abc_hpd* hd) {
    if (!hd) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (hd is required)", fn);
    if (hd->nm == 0 || hd->nm > 16) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: nm = %zu masses (1 to 16)", fn, hd->nm);
    if (!hd->mass) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (mass is required)", fn);
    for (size_t i = 0; i < hd->nm; i++)
        if (!(hd->mass[i] > 0.0 && hd->mass[i] < 1.0))
            ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: mass[%zu] = %g is not a mass inside (0, 1)", fn, i, hd->mass[i]);
    if (!hd->lo && !hd->hi && !hd->plo && !hd->phi) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: every output member of hd is NULL", fn);
    return ABC_OK;
}

// an abc_summary's arrays for G groups of P segments, host (h) <-> arena: probs stay where they are, NULL members stay NULL
static abc_summary summary_stage(Stage& s, const abc_summary* h, size_t G, size_t P) {
    abc_summary d = *h;
    d.truth = h->truth ? s.up(h->truth, G * P) : nullptr;
    d.quant = h->quant ? s.dev<double>(G * h->nq * P) : nullptr;
    d.cdf = h->cdf ? s.dev<double>(G * P) : nullptr;
    return d;
}
static void summary_down(Stage& s, const abc_summary* h, const abc_summary& d, size_t G, size_t P) {
    s.down(h->quant, d.quant, G * h->nq * P);
    s.down(h->cdf, d.cdf, G * P);
}

// an abc_density's arrays for ns segments, host (h) <-> arena: NULL members stay NULL
static abc_density density_stage(Stage& s, const abc_density* h, size_t ns) {
    abc_density d = *h;
    d.bw = h->bw ? s.up(h->bw, ns) : nullptr;
    d.dens = h->dens ? s.dev<double>(ns * h->G) : nullptr;
    d.grid = h->grid ? s.dev<double>(ns * 2) : nullptr;
    d.bw_out = h->bw_out ? s.dev<double>(ns) : nullptr;
    d.mode = h->mode ? s.dev<double>(ns) : nullptr;
    d.mode_dens = h->mode_dens ? s.dev<double>(ns) : nullptr;
    return d;
}
static void density_down(Stage& s, const abc_density* h, const abc_density& d, size_t ns) {
    s.down(h->dens, d.dens, ns * h->G);
    s.down(h->grid, d.grid, ns * 2);
    s.down(h->bw_out, d.bw_out, ns);
    s.down(h->mode, d.mode, ns);
    s.down(h->mode_dens, d.mode_dens, ns);
}

// an abc_joint's arrays for B targets of P parameters, host (h) <-> arena: pairs stay where they are, NULL members stay NULL
static size_t joint_stage_bytes(const abc_joint* h, size_t B, size_t P) {
    const size_t np = abc_joint_pairs(h, P);
    return B * (P * (2 * P + 5) + np * ((h->dens ? h->G * h->G : 0) + 3)) * 8 + 40 * 256;
}
static abc_joint joint_stage(Stage& s, const abc_joint* h, size_t B, size_t P) {
    const size_t np = abc_joint_pairs(h, P);
    abc_joint d = *h;
    d.bw = h->bw ? s.up(h->bw, B * P) : nullptr;
    d.mean = h->mean ? s.dev<double>(B * P) : nullptr;
    d.cov = h->cov ? s.dev<double>(B * P * P) : nullptr;
    d.corr = h->corr ? s.dev<double>(B * P * P) : nullptr;
    d.dens = (h->dens && np) ? s.dev<double>(B * np * h->G * h->G) : nullptr;
    d.grid = h->grid ? s.dev<double>(B * P * 2) : nullptr;
    d.bw_out = h->bw_out ? s.dev<double>(B * P) : nullptr;
    d.mode = (h->mode && np) ? s.dev<double>(B * np * 2) : nullptr;
    d.mode_dens = (h->mode_dens && np) ? s.dev<double>(B * np) : nullptr;
    return d;
}
static void joint_down(Stage& s, const abc_joint* h, const abc_joint& d, size_t B, size_t P) {
    const size_t np = abc_joint_pairs(h, P);
    s.down(h->mean, d.mean, B * P);
    s.down(h->cov, d.cov, B * P * P);
    s.down(h->corr, d.corr, B * P * P);
    s.down(h->dens, d.dens, B * np * h->G * h->G);
    s.down(h->grid, d.grid, B * P * 2);
    s.down(h->bw_out, d.bw_out, B * P);
    s.down(h->mode, d.mode, B * np * 2);
    s.down(h->mode_dens, d.mode_dens, B * np);
}

// an abc_draws's arrays for B targets of P parameters, host (h) <-> arena: stream stays where it is, NULL members stay NULL
static abc_draws draws_stage(Stage& s, const abc_draws* h, size_t B, size_t P) {
    abc_draws d = *h;
    d.bw = (h->smooth && h->bw) ? s.up(h->bw, B * P) : nullptr;
    d.draws = h->draws ? s.dev<double>(B * h->S * P) : nullptr;
    d.src = h->src ? s.dev<uint64_t>(B * h->S) : nullptr;
    d.bw_out = h->bw_out ? s.dev<double>(B * P) : nullptr;
    d.ess = h->ess ? s.dev<double>(B) : nullptr;
    return d;
}
static void draws_down(Stage& s, const abc_draws* h, const abc_draws& d, size_t B, size_t P) {
    s.down(h->draws, d.draws, B * h->S * P);
    s.down(h->src, d.src, B * h->S);
    s.down(h->bw_out, d.bw_out, B * P);
    s.down(h->ess, d.ess, B);
}

// an abc_entropy's arrays for B targets of K entries, host (h) <-> arena: scale stays where it is, NULL members stay NULL
static abc_entropy entropy_stage(Stage& s, const abc_entropy* h, size_t B, size_t K) {
    abc_entropy d = *h;
    d.H = h->H ? s.dev<double>(B) : nullptr;
    d.knn = h->knn ? s.dev<double>(B * K) : nullptr;
    d.zeros = h->zeros ? s.dev<uint64_t>(B) : nullptr;
    return d;
}
static void entropy_down(Stage& s, const abc_entropy* h, const abc_entropy& d, size_t B, size_t K) {
    s.down(h->H, d.H, B);
    s.down(h->knn, d.knn, B * K);
    s.down(h->zeros, d.zeros, B);
}

// an abc_hpd's arrays for B targets of P segments, host (h) <-> arena: mass stays where it is, NULL members stay NULL
static abc_hpd hpd_stage(Stage& s, const abc_hpd* h, size_t B, size_t P) {
    abc_hpd d = *h;
    const size_t n = B * h->nm * P;
    d.lo = h->lo ? s.dev<double>(n) : nullptr;
    d.hi = h->hi ? s.dev<double>(n) : nullptr;
    d.plo = h->plo ? s.dev<double>(n) : nullptr;
    d.phi = h->phi ? s.dev<double>(n) : nullptr;
    return d;
}
static void hpd_down(Stage& s, const abc_hpd* h, const abc_hpd& d, size_t B, size_t P) {
    const size_t n = B * h->nm * P;
    s.down(h->lo, d.lo, n);
    s.down(h->hi, d.hi, n);
    s.down(h->plo, d.plo, n);
    s.down(h->phi, d.phi, n);
}

namespace {
// A posterior product: what is computed from the segments' values and weights, described by the caller's abc_summary, abc_density,
// abc_joint, abc_draws, abc_entropy or abc_hpd.  Every member below has one row per kind, and nothing else in this file tells the kinds
// apart: a new product adds its constructor and its six rows here (and a seventh where it has a demand of its own on the segments,
// as equal_weights()).
struct Product {
    enum Kind { NONE, SUMMARY, DENSITY, JOINT, DRAWS, ENTROPY, HPD } kind = NONE;
    union {
        const abc_summary* sum = nullptr;
        const abc_density* den;
        const abc_joint* jnt;
        const abc_draws* drw;
        const abc_entropy* ent;
        const abc_hpd* hpd;
    };
    union { abc_summary sum; abc_density den; abc_joint jnt; abc_draws drw; abc_entropy ent; abc_hpd hpd; } staged;      // stage()'s copy of the descriptor
    Product() {}
    explicit Product(const abc_summary* s) : kind(SUMMARY), sum(s) {}
    explicit Product(const abc_density* d) : kind(DENSITY), den(d) {}
    explicit Product(const abc_joint* j) : kind(JOINT), jnt(j) {}
    explicit Product(const abc_draws* d) : kind(DRAWS), drw(d) {}
    explicit Product(const abc_entropy* e) : kind(ENTROPY), ent(e) {}
    explicit Product(const abc_hpd* h) : kind(HPD), hpd(h) {}

    // the descriptor's own argument checks (a NULL descriptor among them)
    int check(abc_ctx* ctx, const char* fn, size_t P) const {
        switch (kind) {
        case SUMMARY: return summary_check(ctx, fn, sum);
        case DENSITY: return density_check(ctx, fn, den);
        case JOINT: return joint_check(ctx, fn, jnt, P);
        case DRAWS: return draws_check(ctx, fn, drw);
        case ENTROPY: return entropy_check(ctx, fn, ent, P);
        case HPD: return hpd_check(ctx, fn, hpd);
        default: return ABC_OK;
        }
    }
    // workspace of launch() for B groups of P segments of K values; checked descriptors only, as everything below
    size_t need(size_t B, size_t K, size_t P) const {
        switch (kind) {
        case SUMMARY: return abc_summary_need(B, K, P);
        case DENSITY: return abc_density_need(B, K, P, den->G);
        case JOINT: return abc_joint_need(B, K, P, jnt->G, abc_joint_pairs(jnt, P));
        case DRAWS: return abc_draws_need(B, K, P, drw->smooth);
        case ENTROPY: return abc_entropy_need(B, K, P);
        case HPD: return abc_hpd_need(B, K, P);
        default: return 0;
        }
    }
    // arena bytes of stage(): what the host entries reserve beyond need()
    size_t stage_bytes(size_t B, size_t K, size_t P) const {
        switch (kind) {
        case SUMMARY: return B * P * (sum->nq + 2) * 8 + 16 * 256;         // truth, quant, cdf
        case DENSITY: return B * P * (den->G + 6) * 8 + 32 * 256;          // bw, dens, grid, bw_out, mode, mode_dens
        case JOINT: return joint_stage_bytes(jnt, B, P);
        case DRAWS: return B * (drw->S * (P + 1) + 2 * P + 1) * 8 + 20 * 256;  // draws, src, bw, bw_out, ess
        case ENTROPY: return B * (K + 2) * 8 + 12 * 256;                   // H, knn, zeros
        case HPD: return B * P * hpd->nm * 4 * 8 + 16 * 256;               // lo, hi, plo, phi
        default: return 0;
        }
    }
    // A host descriptor's arrays in the arena (inputs uploaded, NULL members stay NULL): the product on those copies.  It points
    // into this object, which has to outlive it.
    Product stage(Stage& s, size_t B, size_t K, size_t P) {
        switch (kind) {
        case SUMMARY: staged.sum = summary_stage(s, sum, B, P); return Product(&staged.sum);
        case DENSITY: staged.den = density_stage(s, den, B * P); return Product(&staged.den);
        case JOINT: staged.jnt = joint_stage(s, jnt, B, P); return Product(&staged.jnt);
        case DRAWS: staged.drw = draws_stage(s, drw, B, P); return Product(&staged.drw);
        case ENTROPY: staged.ent = entropy_stage(s, ent, B, K); return Product(&staged.ent);
        case HPD: staged.hpd = hpd_stage(s, hpd, B, P); return Product(&staged.hpd);
        default: return Product();
        }
    }
    // stage()'s outputs back into the host descriptor's arrays
    void down(Stage& s, size_t B, size_t K, size_t P) const {
        switch (kind) {
        case SUMMARY: summary_down(s, sum, staged.sum, B, P); break;
        case DENSITY: density_down(s, den, staged.den, B * P); break;
        case JOINT: joint_down(s, jnt, staged.jnt, B, P); break;
        case DRAWS: draws_down(s, drw, staged.drw, B, P); break;
        case ENTROPY: entropy_down(s, ent, staged.ent, B, K); break;
        case HPD: hpd_down(s, hpd, staged.hpd, B, P); break;
        default: break;
        }
    }
    // device descriptor, the workspace reserved
    int launch(abc_ctx* ctx, const SmValues& sv, size_t B, size_t K, size_t P, const char* fn) const {
        switch (kind) {
        case SUMMARY: return launch_summary(ctx, sv, B, K, P, sum);
        case DENSITY: return launch_density(ctx, sv, B, K, P, den, fn);
        case JOINT: return launch_joint(ctx, sv, B, K, P, jnt, fn);
        case DRAWS: return launch_draws(ctx, sv, B, K, P, drw, fn);
        case ENTROPY: return launch_entropy(ctx, sv, B, K, P, ent, fn);
        case HPD: return launch_hpd(ctx, sv, B, K, P, hpd);
        default: return ABC_OK;
        }
    }
    // the product is of an unweighted sample: the entries refuse segments whose weights are not all equal
    bool equal_weights() const { return kind == ENTROPY; }
};

// what follows the ranking: nothing, the adjustment, a posterior product, the tolerance path, the ABC-GLM posterior (glm.hip)
enum { TG_PLAIN, TG_ADJUST, TG_PRODUCT, TG_PATH, TG_GLM };
struct TgRequest {                             // (members in the order of the entries' arguments)
    int kind;
    const double* X;  size_t ldx;
    const double* Y;  size_t ldy;
    size_t N, M, P;
    const double* model;  size_t A;
    const double* targets;  size_t ldt, B;
    const uint64_t* exclude;
    size_t K;                                  // TG_PATH: set by tg_check to the largest tolerance
    uint64_t* idx;                             // optional for TG_PRODUCT and a path with summaries
    double* dist;                              // optional
    double* post_mean = nullptr;               // TG_PLAIN only, optional
    int method = 0, kernel = 0;                // method: TG_PRODUCT only (of which values the segments are)
    const abc_adjust_out* adj = nullptr;       // TG_ADJUST: required, any member may be NULL; TG_PRODUCT: optional, method 1 only
    Product prod;                              // TG_PRODUCT; TG_PATH: none or the summaries (method: of those)
    bool any_excl = false;                     // exclude names a row for some target: set by tg_check
    const abc_path* path = nullptr;            // TG_PATH only: required; Ks in host memory
    const abc_glm* glm = nullptr;              // TG_GLM only: required
    bool glm_summary = false;                  // TG_GLM: a *_summary entry; glm_sum is then required and every output of glm optional
    const abc_summary* glm_sum = nullptr;
    int* glm_nc = nullptr;                     // TG_GLM, optional: receives the model's ncomp once the run has read it (host)
    bool segments() const { return kind == TG_PRODUCT; }      // the rows' values are read after the ranking
    bool regress() const { return kind == TG_ADJUST || (segments() && method == ABC_POSTERIOR_LOCLINEAR); }
    bool path_summary() const { return kind == TG_PATH && prod.kind == Product::SUMMARY; }      // prod: the summaries at every tolerance
    // the call fits the regression, so the context's parameter transforms (if any) apply to it
    bool fits() const {
        if (kind == TG_PATH) return path && (path->coef || path->rank || path->status || (path_summary() && method == ABC_POSTERIOR_LOCLINEAR));
        return regress();
    }
};
}  // namespace

// the descriptor of an ABC-GLM request, its limits and the context's settings it refuses (A: 0 where the caller has none)
// (summary: a *_summary entry, whose sum is required; every level strictly inside (0, 1), the mixture's quantile at 0 or 1 being infinite)
static int glm_check(abc_ctx* ctx, const char* fn, const abc_glm* m, size_t P, size_t A, bool summary = false,
                     const abc_summary* sum = nullptr) {
    if (!m) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (glm is required)", fn);
    if (ctx->tf_buf) ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: parameter transforms are set on the context, and ABC-GLM is not an adjustment", fn);
    if (ctx->hcorr) ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: the variance correction is set on the context, and ABC-GLM is not an adjustment", fn);
    if (ctx->rg_L) ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: ridge is set on the context, and ABC-GLM is not an adjustment", fn);
    if (P == 0 || P > ABC_GLM_MAX) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: P = %zu parameters (1 to %d)", fn, P, ABC_GLM_MAX);
    if (A > 64) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: A = %zu components (at most 64)", fn, A);
    if (m->G < 2 || m->G > 4096) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: G = %zu grid points (2 to 4096)", fn, m->G);
    if (!(m->cut >= 0.0) || !std::isfinite(m->cut)) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: cut = %g (finite, >= 0)", fn, m->cut);
    if (!(m->bw_scale > 0.0) || !std::isfinite(m->bw_scale))
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: bw_scale = %g (finite, > 0)", fn, m->bw_scale);
    const bool none = !m->dens && !m->lo_x && !m->step && !m->mode && !m->mode_dens && !m->mean && !m->var && !m->ess && !m->log_md &&
                      !m->C && !m->c0 && !m->sigma_s && !m->T && !m->peaks && !m->c && !m->status;
    if (!summary) {
        if (none) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: every output member of glm is NULL", fn);
        return ABC_OK;
    }
    if (!sum) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (sum is required)", fn);
    if (sum->quant) {
        if (sum->nq == 0 || sum->nq > 64) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: nq = %zu levels (1 to 64)", fn, sum->nq);
        if (!sum->probs) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (probs is required)", fn);
        for (size_t q = 0; q < sum->nq; q++)
            if (!(sum->probs[q] > 0.0 && sum->probs[q] < 1.0))
                ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: probs[%zu] = %g is not a level strictly inside (0, 1)", fn, q, sum->probs[q]);
    }
    if (sum->cdf && !sum->truth) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: cdf requires truth", fn);
    if (none && !sum->quant && !sum->cdf)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: quant and cdf of sum and every output member of glm are NULL", fn);
    return ABC_OK;
}
// the model's ncomp of a device model record (synchronises), within ABC-GLM's limit
static int glm_ncomp(abc_ctx* ctx, const char* fn, const double* model, size_t A, size_t* n) {
    double hdr = 0.0;
    ABC_HIP(ctx, hipMemcpyAsync(&hdr, model, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n = hdr < 0.0 ? 0 : (hdr > (double)A ? A : (size_t)hdr);      // the ranking's tg_ncomp
    if (*n == 0 || *n > ABC_GLM_MAX) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: the model has %zu components (1 to %d)", fn, *n, ABC_GLM_MAX);
    return ABC_OK;
}
// an abc_glm's arrays for B targets, host (h) <-> arena: NULL members stay NULL; C, c0 and sigma_s with room for nA components
static size_t glm_stage_bytes(const abc_glm* h, size_t B, size_t K, size_t P, size_t nA) {
    if (nA > ABC_GLM_MAX) nA = ABC_GLM_MAX;
    return B * (P * (h->G + 8) + 2 + nA * (P + 1 + nA) + P * P + K * (P + 1) + 1) * 8 + 40 * 256;
}
static abc_glm glm_stage(Stage& s, const abc_glm* h, size_t B, size_t K, size_t P, size_t nA) {
    if (nA > ABC_GLM_MAX) nA = ABC_GLM_MAX;
    abc_glm d = *h;
    d.bw = h->bw ? s.up(h->bw, B * P) : nullptr;
    d.dens = h->dens ? s.dev<double>(B * P * h->G) : nullptr;
    d.lo_x = h->lo_x ? s.dev<double>(B * P) : nullptr;
    d.step = h->step ? s.dev<double>(B * P) : nullptr;
    d.mode = h->mode ? s.dev<double>(B * P) : nullptr;
    d.mode_dens = h->mode_dens ? s.dev<double>(B * P) : nullptr;
    d.mean = h->mean ? s.dev<double>(B * P) : nullptr;
    d.var = h->var ? s.dev<double>(B * P) : nullptr;
    d.ess = h->ess ? s.dev<double>(B) : nullptr;
    d.log_md = h->log_md ? s.dev<double>(B) : nullptr;
    d.C = h->C ? s.dev<double>(B * nA * P) : nullptr;
    d.c0 = h->c0 ? s.dev<double>(B * nA) : nullptr;
    d.sigma_s = h->sigma_s ? s.dev<double>(B * nA * nA) : nullptr;
    d.T = h->T ? s.dev<double>(B * P * P) : nullptr;
    d.peaks = h->peaks ? s.dev<double>(B * K * P) : nullptr;
    d.c = h->c ? s.dev<double>(B * K) : nullptr;
    d.status = h->status ? s.dev<int32_t>(B) : nullptr;
    return d;
}
static void glm_down(Stage& s, const abc_glm* h, const abc_glm& d, size_t B, size_t K, size_t P, size_t n) {
    s.down(h->dens, d.dens, B * P * h->G);
    s.down(h->lo_x, d.lo_x, B * P);
    s.down(h->step, d.step, B * P);
    s.down(h->mode, d.mode, B * P);
    s.down(h->mode_dens, d.mode_dens, B * P);
    s.down(h->mean, d.mean, B * P);
    s.down(h->var, d.var, B * P);
    s.down(h->ess, d.ess, B);
    s.down(h->log_md, d.log_md, B);
    s.down(h->C, d.C, B * n * P);
    s.down(h->c0, d.c0, B * n);
    s.down(h->sigma_s, d.sigma_s, B * n * n);
    s.down(h->T, d.T, B * P * P);
    s.down(h->peaks, d.peaks, B * K * P);
    s.down(h->c, d.c, B * K);
    s.down(h->status, d.status, B);
}

// the abc_summary of a *_summary entry of ABC-GLM for B targets, host (h) <-> arena: quant only with levels (nq is not read without)
static abc_summary glm_summary_stage(Stage& s, const abc_summary* h, size_t B, size_t P) {
    abc_summary d = *h;
    d.truth = h->truth ? s.up(h->truth, B * P) : nullptr;
    d.quant = h->quant ? s.dev<double>(B * h->nq * P) : nullptr;
    d.cdf = h->cdf ? s.dev<double>(B * P) : nullptr;
    return d;
}
static void glm_summary_down(Stage& s, const abc_summary* h, const abc_summary& d, size_t B, size_t P) {
    if (h->quant) s.down(h->quant, d.quant, B * h->nq * P);
    s.down(h->cdf, d.cdf, B * P);
}

// the tolerance list of a path request
static int path_check(abc_ctx* ctx, const char* fn, const abc_path* path) {
    if (!path) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (path is required)", fn);
    if (!path->Ks) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (path->Ks is required)", fn);
    if (path->T == 0 || path->T > 16) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: T = %zu tolerances (1 to 16)", fn, path->T);
    if (path->Ks[0] == 0) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: Ks[0] == 0", fn);
    for (size_t t = 1; t < path->T; t++)
        if (path->Ks[t] <= path->Ks[t - 1])
            ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: Ks[%zu] = %zu after Ks[%zu] = %zu (strictly ascending)", fn, t, path->Ks[t], t - 1,
                     path->Ks[t - 1]);
    return ABC_OK;
}

// Argument checks of the family; sets r.any_excl (and r.K of a path).  host: the arrays are in host memory and the model is fitted by the call
// (which needs Y); otherwise exclude is brought to the host here, after every check that does not need it.
static int tg_check(abc_ctx* ctx, const char* fn, TgRequest& r, bool host) {
    const bool plain = r.kind == TG_PLAIN, summary = r.segments();
    if (r.kind == TG_PATH) {
        ABC_TRY(path_check(ctx, fn, r.path));
        r.K = r.path->Ks[r.path->T - 1];
    }
    const size_t N = r.N, B = r.B, K = r.K;
    if (ctx->rw_N && N != ctx->rw_N)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: N = %zu, but the row weights were set for %zu rows", fn, N, ctx->rw_N);
    if (ctx->tf_buf && r.fits() && r.P != ctx->tf_P)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: P = %zu, but the parameter transforms were set for %zu parameters", fn, r.P, ctx->tf_P);
    if (!r.X) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (X is required)", fn);
    if (!r.targets) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (targets is required)", fn);
    if (!r.idx && !summary && !r.path_summary() && r.kind != TG_GLM)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (idx is required)", fn);
    if (!r.Y && (host || !plain)) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (Y is required)", fn);
    if (!r.Y && r.post_mean && r.P) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: post_mean needs Y", fn);
    if (!host) {
        if (!r.model) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (model is required)", fn);
        if (r.A == 0) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: A == 0", fn);
        if (r.ldx < N) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: ldx %zu < N %zu", fn, r.ldx, N);
        if (r.ldt < B) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: ldt %zu < B %zu", fn, r.ldt, B);
    }
    if ((summary || r.path_summary()) && r.method != ABC_POSTERIOR_REJECTION && r.method != ABC_POSTERIOR_LOCLINEAR)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: method %d (0 = rejection, 1 = loclinear)", fn, r.method);
    if (r.kind == TG_ADJUST && !r.adj) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (out is required)", fn);
    if (!plain && r.kernel != ABC_KERNEL_EPANECHNIKOV && r.kernel != ABC_KERNEL_RECTANGULAR)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: kernel %d (0 = Epanechnikov, 1 = rectangular)", fn, r.kernel);
    if ((!plain || r.post_mean) && r.P && r.ldy < N) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: ldy %zu < N %zu", fn, r.ldy, N);
    if (r.kind == TG_GLM) ABC_TRY(glm_check(ctx, fn, r.glm, r.P, r.A, r.glm_summary, r.glm_sum));
    if (!plain) {     // the adjustment's limits, for both of a product's methods too
        if (r.A > 64) ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: A = %zu components (at most 64)", fn, r.A);
        if (r.P > 1024) ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: P = %zu parameters (at most 1024)", fn, r.P);
    }
    ABC_TRY(r.prod.check(ctx, fn, r.P));
    if (summary && r.prod.equal_weights()) {     // (an estimator for an unweighted sample: ignoring weights would give a wrong number)
        if (ctx->rw_N)
            ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: row importance weights are set on the context, and the estimate is for entries of equal weight", fn);
        if (r.method == ABC_POSTERIOR_LOCLINEAR && r.kernel != ABC_KERNEL_RECTANGULAR)
            ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: the Epanechnikov kernel weights the entries, and the estimate is for entries of equal weight (pass the rectangular kernel)", fn);
    }
    if (r.path_summary() && !r.prod.sum->quant && !r.prod.sum->cdf)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: quant and cdf of sum are both NULL", fn);
    if (B == 0) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: no targets (B == 0)", fn);
    if (K == 0) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: K == 0", fn);
    if (r.M == 0) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: no metrics (M == 0)", fn);
    if (K > N) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: K = %zu > N = %zu", fn, K, N);
    if (N >= ((size_t)1 << 32)) ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: N = %zu rows (at most 2^32 - 1)", fn, N);
    std::vector<uint64_t> copy;
    const uint64_t* ex = r.exclude;
    if (ex && !host) {
        copy.resize(B);
        ABC_HIP(ctx, hipMemcpyAsync(copy.data(), r.exclude, B * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ex = copy.data();
    }
    r.any_excl = false;
    if (ex)
        for (size_t b = 0; b < B; b++) {
            if (ex[b] == UINT64_MAX) continue;
            if (ex[b] >= N) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: exclude[%zu] = %llu is not a row (N = %zu)", fn, b,
                                     (unsigned long long)ex[b], N);
            r.any_excl = true;
        }
    if (r.any_excl && K > N - 1) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: K = %zu > N - 1 = %zu with an excluded row", fn, K, N - 1);
    return ABC_OK;
}

// Arena bytes of a checked request: what tg_run takes and, for the host entries (host: the fit under `rule`, every array staged),
// what tg_host takes around it.  The device entries get the model from the caller, so their ranking needs no fit workspace.
static size_t tg_need(const abc_ctx* ctx, const TgRequest& r, bool host, int rule) {
    const size_t N = r.N, M = r.M, P = r.P, A = r.A, B = r.B, K = r.K;
    size_t b = abc_targets_need(N, A, B, K, r.any_excl);
    if (ctx->tf_buf && r.fits()) b += N * P * 8 + 256;                                      // forward(Y)
    const bool hc = ctx->hcorr && r.fits();
    const size_t rg = r.fits() ? ctx->rg_L : 0;
    if (r.regress()) b += abc_adjust_need(N, A, P, B, K, hc, rg);
    if (r.kind == TG_PATH) b += abc_path_need(N, A, P, B, K, r.path->T, hc, rg);
    if (r.segments()) b += 2 * B * K * 8 + 16 * 256;                                         // (tg_run's own idx and dist)
    if (r.kind == TG_GLM) b += 2 * B * K * 8 + 16 * 256 + abc_glm_need(B, K, P, A, r.glm->G, r.glm_summary);
    // (under row importance weights the rejection path's summaries take the loclinear path's route, one tolerance at a time)
    if (r.path_summary())
        b += abc_path_summary_need(B, r.path->Ks, r.path->T, P, ctx->rw_N ? 1 : r.method) + (r.idx ? 0 : B * K * 8 + 256);
    else b += r.prod.need(B, K, P);
    if (!host) return b + abc_ws_need(N, 1, 1, 1, K + 1, 0, 0);
    b += abc_ws_need(N, M, P, A, K + 1, 0, 0) + (rule == ABC_RULE_WILCOXON ? abc_wx_need(N, P, A) : 0);
    b += (N * (M + P) + M + 4) * 8;                                               // X, Y, the zero observation and its one idx, dist
    b += (B * M + B + 2 * B * K) * 8 + 8 * 256;                                   // targets, exclude, idx, dist
    if (r.kind == TG_PLAIN) b += B * P * 8;                                       // post_mean
    else if (r.kind == TG_PATH) b += B * r.path->T * ((A + 2) * P + 2) * 8 + 8 * 256;      // abc_path: post_mean, coef, rank + status, h
    else if (r.kind != TG_GLM) b += (B * K * P + B * K + B * (A + 1) * P + B) * 8 + 8 * 256;      // abc_adjust_out: theta, weight, coef, rank + status
    if (r.path_summary()) return b + B * P * (r.path->T * (r.prod.sum->nq + 1) + 1) * 8 + 16 * 256;     // truth, quant, cdf
    if (r.kind == TG_GLM) b += glm_stage_bytes(r.glm, B, K, P, A);
    if (r.kind == TG_GLM && r.glm_summary) b += B * P * (r.glm_sum->quant ? r.glm_sum->nq + 2 : 2) * 8 + 4 * 256;      // truth, quant, cdf
    return b + r.prod.stage_bytes(B, K, P);
}

// the values a product of the request reads: the retained rows ix of its Y (raw: the transforms are in adj), adjusted under adj
static SmValues tg_values(const TgRequest& r, const uint64_t* ix, const abc_adj_keep* adj, const double* om) {
    SmValues sv = {};
    sv.method = r.method;
    sv.idx = ix;
    sv.Y = r.Y;
    sv.ldy = r.ldy;
    sv.adj = adj;
    sv.A = (int)r.A;
    sv.kernel = r.kernel;
    sv.om = om;
    return sv;
}

// The ranking or (regress) the ranking with the adjustment, then the product if one is asked for; device pointers, the workspace reserved.
static int tg_run_queued(abc_ctx* ctx, const char* fn, const TgRequest& r, const AbcHc* hc, const AbcRg* rg) {
    const size_t B = r.B, K = r.K;
    const bool summary = r.segments();
    const double* om = ctx->rw_N ? ctx->rw_dev : nullptr;      // the row importance weights (tg_check: rw_N == N)
    uint64_t* ix = r.idx;
    double* d = r.dist;
    if (summary) {     // every product reads both
        if (!ix) ix = (uint64_t*)abc_ws_alloc(ctx, B * K * 8);
        if (!d) d = (double*)abc_ws_alloc(ctx, B * K * 8);
        if (!ix || !d) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    }
    // parameter transforms: forward(Y) once per call (N x P, ld = N), which the regression reads as its Y; everything that reads raw
    // values (method 0, the path's post_mean) keeps r.Y
    const AbcTf tf = ctx_tf(ctx);
    double* Yt = nullptr;
    if (tf.kind && r.fits() && r.P) {
        Yt = (double*)abc_ws_alloc(ctx, r.N * r.P * 8);
        if (!Yt) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
        ABC_TRY(launch_param_transf(ctx, &tf, r.Y, r.ldy, r.N, r.P, 0, Yt, r.N, ctx->tf_outside_dev));
    }
    if (r.kind == TG_GLM) {     // the ranking with its scores kept, the model's ncomp, the GLM on the retained rows
        if (!ix) ix = (uint64_t*)abc_ws_alloc(ctx, B * K * 8);
        if (!d) d = (double*)abc_ws_alloc(ctx, B * K * 8);
        if (!ix || !d) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
        size_t n = 0;
        ABC_TRY(glm_ncomp(ctx, fn, r.model, r.A, &n));      // (before the ranking: a model beyond the limit runs nothing)
        if (r.glm_nc) *r.glm_nc = (int)n;
        abc_tg_scores sc;
        ABC_TRY(launch_rank_targets(ctx, r.X, r.ldx, r.Y, r.ldy, r.N, r.M, r.P, r.model, r.A, r.targets, r.ldt, B, r.exclude,
                                    r.any_excl, K, ix, d, nullptr, &sc));
        return launch_glm(ctx, tg_values(r, ix, nullptr, om), sc.S, sc.sld, r.Y, r.ldy, ix, om, nullptr, sc.O, sc.KCO, B, K, r.P, n,
                          r.A, r.glm, r.glm_summary ? r.glm_sum : nullptr, fn);
    }
    if (r.kind == TG_PATH) {
        const bool ps = r.path_summary(), lin = ps && r.method == ABC_POSTERIOR_LOCLINEAR;
        if (ps && !ix) {
            ix = (uint64_t*)abc_ws_alloc(ctx, B * K * 8);
            if (!ix) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
        }
        abc_adj_keep pk;
        ABC_TRY(launch_rank_targets_path(ctx, r.X, r.ldx, r.Y, r.ldy, r.N, r.M, r.P, r.model, r.A, r.targets, r.ldt, B, r.exclude,
                                         r.any_excl, r.kernel, ix, d, r.path, lin ? &pk : nullptr, Yt, Yt ? &tf : nullptr, hc, rg, om));
        if (!ps) return ABC_OK;
        return launch_path_summary(ctx, tg_values(r, ix, lin ? &pk : nullptr, om), B, r.path->Ks, r.path->T, r.P, r.prod.sum);
    }
    abc_adj_keep keep;
    if (!r.regress()) {     // (post_mean: of the plain ranking only)
        ABC_TRY(launch_rank_targets(ctx, r.X, r.ldx, r.Y, r.ldy, r.N, r.M, r.P, r.model, r.A, r.targets, r.ldt, B, r.exclude,
                                    r.any_excl, K, ix, d, r.post_mean, nullptr, om));
    } else {                // (without keep nothing is regressed when every member of adj is NULL)
        abc_adjust_out od = {};
        if (r.adj) od = *r.adj;
        ABC_TRY(launch_rank_targets_adjust(ctx, r.X, r.ldx, Yt ? Yt : r.Y, Yt ? r.N : r.ldy, r.N, r.M, r.P, r.model, r.A, r.targets, r.ldt,
                                           B, r.exclude, r.any_excl, K, r.kernel, ix, d, &od, summary ? &keep : nullptr,
                                           Yt ? &tf : nullptr, hc, rg, om));
    }
    if (!summary) return ABC_OK;
    return r.prod.launch(ctx, tg_values(r, ix, r.regress() ? &keep : nullptr, om), B, K, r.P, fn);
}

// tg_run_queued under the variance correction and the ridge adjustment: the call's second fits, picks and PRESS go to the context's
// records, which name them only after everything has been queued without an error
static int tg_run(abc_ctx* ctx, const char* fn, const TgRequest& r) {
    AbcHc hcd = {nullptr, nullptr};
    const bool hcon = ctx->hcorr && r.fits() && r.P;
    const size_t slots = r.kind == TG_PATH ? r.B * r.path->T : r.B;
    if (hcon) ABC_TRY(hcorr_record(ctx, fn, slots, r.A, r.P, &hcd));
    AbcRg rgd = {};
    const bool rgon = ctx->rg_L && r.fits() && r.P;
    if (rgon) ABC_TRY(ridge_record(ctx, fn, slots, r.P, &rgd));
    ABC_TRY(tg_run_queued(ctx, fn, r, hcon ? &hcd : nullptr, rgon ? &rgd : nullptr));
    if (rgon) {
        ctx->rg_slots = slots;
        ctx->rg_Lrec = ctx->rg_L;
        ctx->rg_P = r.P;
    }
    if (hcon) {
        ctx->hc_slots = slots;
        ctx->hc_a1 = r.A + 1;
        ctx->hc_P = r.P;
    }
    return ABC_OK;
}

static int tg_dev(abc_ctx* ctx, const char* fn, TgRequest r) {
    ABC_TRY(tg_check(ctx, fn, r, false));
    ABC_TRY(abc_ws_reserve(ctx, tg_need(ctx, r, false, 0)));
    return tg_run(ctx, fn, r);
}

// The host entries: h holds host pointers.  Upload, one fit, the request on the arena's copies, downloads, synchronise.
static int tg_host(abc_ctx* ctx, const char* fn, TgRequest h, double train_frac, int max_comp, int rule, int32_t* ncomp) {
    const size_t N = h.N, M = h.M, P = h.P, B = h.B;
    const size_t A = h.A = default_A(M, P, max_comp);
    ABC_TRY(tg_check(ctx, fn, h, true));
    const size_t K = h.K;                                   // (a path's: set by the check)
    ABC_TRY(abc_ws_reserve(ctx, tg_need(ctx, h, true, rule)));
    Stage s{ctx};
    // the fit: the single-target ranking's own path (generation_core) on an all-zero observation, whose scores are not used
    abc_generation_io io;
    memset(&io, 0, sizeof(io));
    io.X = s.up(h.X, N * M);
    io.Y = s.up(h.Y, N * P);
    double* zobs = s.dev<double>(M);
    io.obs = zobs;
    io.idx = s.dev<uint64_t>(1);
    io.dist = s.dev<double>(1);
    if (s.full) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    ABC_HIP(ctx, hipMemsetAsync(zobs, 0, M * sizeof(double), ctx->stream));
    abc_generation_cfg cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.N = N; cfg.M = M; cfg.P = P; cfg.K = 1; cfg.train_frac = train_frac;
    cfg.max_comp = max_comp; cfg.rule = rule;
    ABC_TRY(generation_core(ctx, &cfg, &io, nullptr, ncomp, 0, &h.model));
    // the request on device copies: every output the caller gave, in the arena
    TgRequest r = h;
    r.X = io.X; r.Y = io.Y;
    r.targets = s.up(h.targets, B * M);
    r.exclude = h.exclude ? s.up(h.exclude, B) : nullptr;
    r.idx = h.idx ? s.dev<uint64_t>(B * K) : nullptr;
    r.dist = h.dist ? s.dev<double>(B * K) : nullptr;
    r.post_mean = (h.post_mean && P) ? s.dev<double>(B * P) : nullptr;
    const abc_adjust_out* ah = h.regress() ? h.adj : nullptr;
    abc_adjust_out od = {};
    if (ah) {     // (theta and coef one element longer, as the adjustment's own buffers)
        od.theta = ah->theta ? s.dev<double>(B * K * P + 1) : nullptr;
        od.weight = ah->weight ? s.dev<double>(B * K) : nullptr;
        od.coef = ah->coef ? s.dev<double>(B * (A + 1) * P + 1) : nullptr;
        od.rank = ah->rank ? s.dev<int32_t>(B) : nullptr;
        od.status = ah->status ? s.dev<int32_t>(B) : nullptr;
    }
    r.adj = ah ? &od : nullptr;
    abc_path pd = {};
    if (h.kind == TG_PATH) {     // (coef one element longer, as the adjustment's own buffer)
        const size_t T = h.path->T;
        pd = *h.path;
        pd.post_mean = (h.path->post_mean && P) ? s.dev<double>(B * T * P) : nullptr;
        pd.coef = h.path->coef ? s.dev<double>(B * T * (A + 1) * P + 1) : nullptr;
        pd.rank = h.path->rank ? s.dev<int32_t>(B * T) : nullptr;
        pd.status = h.path->status ? s.dev<int32_t>(B * T) : nullptr;
        pd.h = h.path->h ? s.dev<double>(B * T) : nullptr;
        r.path = &pd;
    }
    abc_summary psd = {};
    if (h.path_summary()) {     // (truth per target, the outputs per target and tolerance)
        const abc_summary* sh = h.prod.sum;
        const size_t T = h.path->T;
        psd = *sh;
        psd.truth = sh->truth ? s.up(sh->truth, B * P) : nullptr;
        psd.quant = sh->quant ? s.dev<double>(B * T * sh->nq * P) : nullptr;
        psd.cdf = sh->cdf ? s.dev<double>(B * T * P) : nullptr;
        r.prod = Product(&psd);
    } else {
        r.prod = h.prod.stage(s, B, K, P);
    }
    abc_glm gd = {};
    int gnc = 0;
    if (h.kind == TG_GLM) {
        gd = glm_stage(s, h.glm, B, K, P, A);
        r.glm = &gd;
        r.glm_nc = &gnc;
    }
    abc_summary gsd = {};
    if (h.kind == TG_GLM && h.glm_summary) {
        gsd = glm_summary_stage(s, h.glm_sum, B, P);
        r.glm_sum = &gsd;
    }
    if (s.full) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    ABC_TRY(tg_run(ctx, fn, r));
    if (h.kind == TG_GLM) glm_down(s, h.glm, gd, B, K, P, (size_t)gnc);
    if (h.kind == TG_GLM && h.glm_summary) glm_summary_down(s, h.glm_sum, gsd, B, P);
    s.down(h.idx, r.idx, B * K);
    s.down(h.dist, r.dist, B * K);
    s.down(h.post_mean, r.post_mean, B * P);
    if (ah) {
        s.down(ah->theta, od.theta, B * K * P);
        s.down(ah->weight, od.weight, B * K);
        s.down(ah->coef, od.coef, B * (A + 1) * P);
        s.down(ah->rank, od.rank, B);
        s.down(ah->status, od.status, B);
    }
    if (h.kind == TG_PATH) {
        const size_t T = h.path->T;
        s.down(h.path->post_mean, pd.post_mean, B * T * P);
        s.down(h.path->coef, pd.coef, B * T * (A + 1) * P);
        s.down(h.path->rank, pd.rank, B * T);
        s.down(h.path->status, pd.status, B * T);
        s.down(h.path->h, pd.h, B * T);
    }
    if (h.path_summary()) {
        s.down(h.prod.sum->quant, psd.quant, B * h.path->T * h.prod.sum->nq * P);
        s.down(h.prod.sum->cdf, psd.cdf, B * h.path->T * P);
    } else {
        h.prod.down(s, B, K, P);
    }
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}

extern "C" int abc_rank_targets_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                                    size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                    const uint64_t* exclude, size_t K, uint64_t* idx, double* dist, double* post_mean) {
    CHECK_CTX(ctx);
    const TgRequest r{TG_PLAIN, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, K, idx, dist, post_mean};
    return tg_dev(ctx, "abc_rank_targets_dev", r);
}

extern "C" int abc_particle_ranking_pls_targets(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                                const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                                const uint64_t* exclude, size_t K, uint64_t* idx, double* dist, double* post_mean,
                                                int32_t* ncomp) {
    CHECK_CTX(ctx);
    const TgRequest h{TG_PLAIN, X, N, Y, N, N, M, P, nullptr, 0, targets, B, B, exclude, K, idx, dist, post_mean};
    return tg_host(ctx, "abc_particle_ranking_pls_targets", h, train_frac, max_comp, rule, ncomp);
}

extern "C" int abc_rank_targets_adjust_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                                           size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                           const uint64_t* exclude, size_t K, int kernel, uint64_t* idx, double* dist,
                                           const abc_adjust_out* out) {
    CHECK_CTX(ctx);
    const TgRequest r{TG_ADJUST, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, K, idx, dist, nullptr, 0, kernel, out};
    return tg_dev(ctx, "abc_rank_targets_adjust_dev", r);
}

extern "C" int abc_particle_ranking_pls_targets_adjust(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                                       const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                                       const uint64_t* exclude, size_t K, int kernel, uint64_t* idx, double* dist,
                                                       const abc_adjust_out* out, int32_t* ncomp) {
    CHECK_CTX(ctx);
    const TgRequest h{TG_ADJUST, X, N, Y, N, N, M, P, nullptr, 0, targets, B, B, exclude, K, idx, dist, nullptr, 0, kernel, out};
    return tg_host(ctx, "abc_particle_ranking_pls_targets_adjust", h, train_frac, max_comp, rule, ncomp);
}

extern "C" int abc_rank_targets_path_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                                         size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                         const uint64_t* exclude, int kernel, uint64_t* idx, double* dist, const abc_path* path) {
    CHECK_CTX(ctx);
    TgRequest r{TG_PATH, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, 0, idx, dist, nullptr, 0, kernel};
    r.path = path;
    return tg_dev(ctx, "abc_rank_targets_path_dev", r);
}

extern "C" int abc_particle_ranking_pls_targets_path(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                                     const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                                     const uint64_t* exclude, int kernel, uint64_t* idx, double* dist,
                                                     const abc_path* path, int32_t* ncomp) {
    CHECK_CTX(ctx);
    TgRequest h{TG_PATH, X, N, Y, N, N, M, P, nullptr, 0, targets, B, B, exclude, 0, idx, dist, nullptr, 0, kernel};
    h.path = path;
    return tg_host(ctx, "abc_particle_ranking_pls_targets_path", h, train_frac, max_comp, rule, ncomp);
}

extern "C" int abc_rank_targets_path_summary_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N,
                                                 size_t M, size_t P, const double* model, size_t A, const double* targets, size_t ldt,
                                                 size_t B, const uint64_t* exclude, int method, int kernel, uint64_t* idx, double* dist,
                                                 const abc_path* path, const abc_summary* sum) {
    CHECK_CTX(ctx);
    TgRequest r{TG_PATH, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, 0, idx, dist, nullptr, method, kernel, nullptr,
                Product(sum)};
    r.path = path;
    return tg_dev(ctx, "abc_rank_targets_path_summary_dev", r);
}

extern "C" int abc_particle_ranking_pls_targets_path_summary(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M,
                                                             size_t P, const double* targets, size_t B, double train_frac,
                                                             int max_comp, int rule, const uint64_t* exclude, int method, int kernel,
                                                             uint64_t* idx, double* dist, const abc_path* path,
                                                             const abc_summary* sum, int32_t* ncomp) {
    CHECK_CTX(ctx);
    TgRequest h{TG_PATH, X, N, Y, N, N, M, P, nullptr, 0, targets, B, B, exclude, 0, idx, dist, nullptr, method, kernel, nullptr,
                Product(sum)};
    h.path = path;
    return tg_host(ctx, "abc_particle_ranking_pls_targets_path_summary", h, train_frac, max_comp, rule, ncomp);
}

extern "C" int abc_rank_targets_summary_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                                            size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                            const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx, double* dist,
                                            const abc_adjust_out* adj, const abc_summary* sum) {
    CHECK_CTX(ctx);
    const TgRequest r{TG_PRODUCT, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, K, idx, dist, nullptr, method, kernel,
                      adj, Product(sum)};
    return tg_dev(ctx, "abc_rank_targets_summary_dev", r);
}

extern "C" int abc_particle_ranking_pls_targets_summary(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                                        const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                                        const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx,
                                                        double* dist, const abc_adjust_out* adj, const abc_summary* sum, int32_t* ncomp) {
    CHECK_CTX(ctx);
    const TgRequest h{TG_PRODUCT, X, N, Y, N, N, M, P, nullptr, 0, targets, B, B, exclude, K, idx, dist, nullptr, method, kernel,
                      adj, Product(sum)};
    return tg_host(ctx, "abc_particle_ranking_pls_targets_summary", h, train_frac, max_comp, rule, ncomp);
}

extern "C" int abc_rank_targets_density_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                                            size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                            const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx, double* dist,
                                            const abc_adjust_out* adj, const abc_density* den) {
    CHECK_CTX(ctx);
    const TgRequest r{TG_PRODUCT, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, K, idx, dist, nullptr, method, kernel,
                      adj, Product(den)};
    return tg_dev(ctx, "abc_rank_targets_density_dev", r);
}

extern "C" int abc_particle_ranking_pls_targets_density(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                                        const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                                        const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx,
                                                        double* dist, const abc_adjust_out* adj, const abc_density* den, int32_t* ncomp) {
    CHECK_CTX(ctx);
    const TgRequest h{TG_PRODUCT, X, N, Y, N, N, M, P, nullptr, 0, targets, B, B, exclude, K, idx, dist, nullptr, method, kernel,
                      adj, Product(den)};
    return tg_host(ctx, "abc_particle_ranking_pls_targets_density", h, train_frac, max_comp, rule, ncomp);
}

extern "C" int abc_rank_targets_joint_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                                          size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                          const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx, double* dist,
                                          const abc_adjust_out* adj, const abc_joint* jt) {
    CHECK_CTX(ctx);
    const TgRequest r{TG_PRODUCT, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, K, idx, dist, nullptr, method, kernel,
                      adj, Product(jt)};
    return tg_dev(ctx, "abc_rank_targets_joint_dev", r);
}

extern "C" int abc_particle_ranking_pls_targets_joint(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                                      const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                                      const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx,
                                                      double* dist, const abc_adjust_out* adj, const abc_joint* jt, int32_t* ncomp) {
    CHECK_CTX(ctx);
    const TgRequest h{TG_PRODUCT, X, N, Y, N, N, M, P, nullptr, 0, targets, B, B, exclude, K, idx, dist, nullptr, method, kernel,
                      adj, Product(jt)};
    return tg_host(ctx, "abc_particle_ranking_pls_targets_joint", h, train_frac, max_comp, rule, ncomp);
}

extern "C" int abc_rank_targets_draws_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                                          size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                          const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx, double* dist,
                                          const abc_adjust_out* adj, const abc_draws* dr) {
    CHECK_CTX(ctx);
    const TgRequest r{TG_PRODUCT, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, K, idx, dist, nullptr, method, kernel,
                      adj, Product(dr)};
    return tg_dev(ctx, "abc_rank_targets_draws_dev", r);
}

extern "C" int abc_rank_targets_entropy_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M,
                                            size_t P, const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                            const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx, double* dist,
                                            const abc_adjust_out* adj, const abc_entropy* en) {
    CHECK_CTX(ctx);
    const TgRequest r{TG_PRODUCT, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, K, idx, dist, nullptr, method, kernel,
                      adj, Product(en)};
    return tg_dev(ctx, "abc_rank_targets_entropy_dev", r);
}

extern "C" int abc_particle_ranking_pls_targets_entropy(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                                        const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                                        const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx,
                                                        double* dist, const abc_adjust_out* adj, const abc_entropy* en, int32_t* ncomp) {
    CHECK_CTX(ctx);
    const TgRequest h{TG_PRODUCT, X, N, Y, N, N, M, P, nullptr, 0, targets, B, B, exclude, K, idx, dist, nullptr, method, kernel,
                      adj, Product(en)};
    return tg_host(ctx, "abc_particle_ranking_pls_targets_entropy", h, train_frac, max_comp, rule, ncomp);
}

extern "C" int abc_rank_targets_hpd_dev(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M, size_t P,
                                        const double* model, size_t A, const double* targets, size_t ldt, size_t B,
                                        const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx, double* dist,
                                        const abc_adjust_out* adj, const abc_hpd* hd) {
    CHECK_CTX(ctx);
    const TgRequest r{TG_PRODUCT, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, K, idx, dist, nullptr, method, kernel,
                      adj, Product(hd)};
    return tg_dev(ctx, "abc_rank_targets_hpd_dev", r);
}

extern "C" int abc_particle_ranking_pls_targets_hpd(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                                    const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                                    const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx,
                                                    double* dist, const abc_adjust_out* adj, const abc_hpd* hd, int32_t* ncomp) {
    CHECK_CTX(ctx);
    const TgRequest h{TG_PRODUCT, X, N, Y, N, N, M, P, nullptr, 0, targets, B, B, exclude, K, idx, dist, nullptr, method, kernel,
                      adj, Product(hd)};
    return tg_host(ctx, "abc_particle_ranking_pls_targets_hpd", h, train_frac, max_comp, rule, ncomp);
}

extern "C" int abc_particle_ranking_pls_targets_draws(abc_ctx* ctx, const double* X, const double* Y, size_t N, size_t M, size_t P,
                                                      const double* targets, size_t B, double train_frac, int max_comp, int rule,
                                                      const uint64_t* exclude, size_t K, int method, int kernel, uint64_t* idx,
                                                      double* dist, const abc_adjust_out* adj, const abc_draws* dr, int32_t* ncomp) {
    CHECK_CTX(ctx);
    const TgRequest h{TG_PRODUCT, X, N, Y, N, N, M, P, nullptr, 0, targets, B, B, exclude, K, idx, dist, nullptr, method, kernel,
                      adj, Product(dr)};
    return tg_host(ctx, "abc_particle_ranking_pls_targets_draws", h, train_frac, max_comp, rule, ncomp);
}

// ---- ABC-GLM posterior of the batched ranking (glm.hip): the descriptor first, the call is a method of the request ----
static TgRequest glm_request(const abc_glm* glm, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M, size_t P,
                             const double* model, size_t A, const double* targets, size_t ldt, size_t B, const uint64_t* exclude,
                             size_t K, uint64_t* idx, double* dist) {
    TgRequest r{TG_GLM, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, K, idx, dist};
    r.glm = glm;
    return r;
}

extern "C" int abc_glm_rank_targets_dev(const abc_glm* glm, abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy,
                                        size_t N, size_t M, size_t P, const double* model, size_t A, const double* targets, size_t ldt,
                                        size_t B, const uint64_t* exclude, size_t K, uint64_t* idx, double* dist) {
    CHECK_CTX(ctx);
    return tg_dev(ctx, "abc_glm_rank_targets_dev",
                  glm_request(glm, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, K, idx, dist));
}

extern "C" int abc_glm_particle_ranking_pls_targets(const abc_glm* glm, abc_ctx* ctx, const double* X, const double* Y, size_t N,
                                                    size_t M, size_t P, const double* targets, size_t B, double train_frac,
                                                    int max_comp, int rule, const uint64_t* exclude, size_t K, uint64_t* idx,
                                                    double* dist, int32_t* ncomp) {
    CHECK_CTX(ctx);
    return tg_host(ctx, "abc_glm_particle_ranking_pls_targets",
                   glm_request(glm, X, N, Y, N, N, M, P, nullptr, 0, targets, B, B, exclude, K, idx, dist), train_frac, max_comp, rule,
                   ncomp);
}

// the same with the exact quantiles and CDF of the marginal mixtures: the summary's descriptor second, every output of glm optional
extern "C" int abc_glm_rank_targets_summary_dev(const abc_glm* glm, const abc_summary* sum, abc_ctx* ctx, const double* X, size_t ldx,
                                                const double* Y, size_t ldy, size_t N, size_t M, size_t P, const double* model, size_t A,
                                                const double* targets, size_t ldt, size_t B, const uint64_t* exclude, size_t K,
                                                uint64_t* idx, double* dist) {
    CHECK_CTX(ctx);
    TgRequest r = glm_request(glm, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, K, idx, dist);
    r.glm_summary = true;
    r.glm_sum = sum;
    return tg_dev(ctx, "abc_glm_rank_targets_summary_dev", r);
}

extern "C" int abc_glm_particle_ranking_pls_targets_summary(const abc_glm* glm, const abc_summary* sum, abc_ctx* ctx, const double* X,
                                                            const double* Y, size_t N, size_t M, size_t P, const double* targets,
                                                            size_t B, double train_frac, int max_comp, int rule,
                                                            const uint64_t* exclude, size_t K, uint64_t* idx, double* dist,
                                                            int32_t* ncomp) {
    CHECK_CTX(ctx);
    TgRequest r = glm_request(glm, X, N, Y, N, N, M, P, nullptr, 0, targets, B, B, exclude, K, idx, dist);
    r.glm_summary = true;
    r.glm_sum = sum;
    return tg_host(ctx, "abc_glm_particle_ranking_pls_targets_summary", r, train_frac, max_comp, rule, ncomp);
}

// the generic form: any retained sample with any statistics, B = 1
static int glm_weighted_check(abc_ctx* ctx, const char* fn, const abc_glm* glm, const double* theta, size_t ldv, const double* stats,
                              size_t lds, size_t K, size_t P, size_t n, const double* obs, bool summary = false,
                              const abc_summary* sum = nullptr) {
    ABC_TRY(glm_check(ctx, fn, glm, P, 0, summary, sum));
    if (!theta) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (theta is required)", fn);
    if (!stats) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (stats is required)", fn);
    if (!obs) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (obs is required)", fn);
    if (K == 0) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: K == 0", fn);
    if (n == 0 || n > ABC_GLM_MAX) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: n = %zu statistics (1 to %d)", fn, n, ABC_GLM_MAX);
    if (ldv < K) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: ldv %zu < K %zu", fn, ldv, K);
    if (lds < K) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: lds %zu < K %zu", fn, lds, K);
    if (K >= ((size_t)1 << 32)) ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: K = %zu rows (at most 2^32 - 1)", fn, K);
    return ABC_OK;
}

static SmValues weighted_values(const double* V, size_t ldv, const double* w);

extern "C" int abc_glm_weighted_dev(const abc_glm* glm, abc_ctx* ctx, const double* theta, size_t ldv, const double* stats, size_t lds,
                                    size_t K, size_t P, size_t n, const double* obs, const double* w) {
    CHECK_CTX(ctx);
    const char* fn = "abc_glm_weighted_dev";
    ABC_TRY(glm_weighted_check(ctx, fn, glm, theta, ldv, stats, lds, K, P, n, obs));
    ABC_TRY(abc_ws_reserve(ctx, abc_glm_need(1, K, P, n, glm->G) + 16 * 256));
    if (w) ABC_TRY(abc_summary_check_weights(ctx, w, K, fn));
    return launch_glm(ctx, weighted_values(theta, ldv, w), stats, lds, theta, ldv, nullptr, nullptr, w, obs, (int)n, 1, K, P, n, n, glm,
                      nullptr, fn);
}

extern "C" int abc_glm_weighted_summary_dev(const abc_glm* glm, const abc_summary* sum, abc_ctx* ctx, const double* theta, size_t ldv,
                                            const double* stats, size_t lds, size_t K, size_t P, size_t n, const double* obs,
                                            const double* w) {
    CHECK_CTX(ctx);
    const char* fn = "abc_glm_weighted_summary_dev";
    ABC_TRY(glm_weighted_check(ctx, fn, glm, theta, ldv, stats, lds, K, P, n, obs, true, sum));
    ABC_TRY(abc_ws_reserve(ctx, abc_glm_need(1, K, P, n, glm->G, true) + 16 * 256));
    if (w) ABC_TRY(abc_summary_check_weights(ctx, w, K, fn));
    return launch_glm(ctx, weighted_values(theta, ldv, w), stats, lds, theta, ldv, nullptr, nullptr, w, obs, (int)n, 1, K, P, n, n, glm,
                      sum, fn);
}

extern "C" int abc_glm_weighted(const abc_glm* glm, abc_ctx* ctx, const double* theta, const double* stats, size_t K, size_t P, size_t n,
                                const double* obs, const double* w) {
    CHECK_CTX(ctx);
    const char* fn = "abc_glm_weighted";
    ABC_TRY(glm_weighted_check(ctx, fn, glm, theta, K, stats, K, K, P, n, obs));
    ABC_TRY(abc_ws_reserve(ctx, abc_glm_need(1, K, P, n, glm->G) + (K * (P + n + 1) + n) * 8 + glm_stage_bytes(glm, 1, K, P, n) + 16 * 256));
    Stage s{ctx};
    const double* th_d = s.up(theta, K * P);
    const double* st_d = s.up(stats, K * n);
    const double* ob_d = s.up(obs, n);
    const double* w_d = w ? s.up(w, K) : nullptr;
    const abc_glm d = glm_stage(s, glm, 1, K, P, n);
    if (s.full) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    if (w_d) ABC_TRY(abc_summary_check_weights(ctx, w_d, K, fn));
    ABC_TRY(launch_glm(ctx, weighted_values(th_d, K, w_d), st_d, K, th_d, K, nullptr, nullptr, w_d, ob_d, (int)n, 1, K, P, n, n, &d, nullptr,
                       fn));
    glm_down(s, glm, d, 1, K, P, n);
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}

extern "C" int abc_glm_weighted_summary(const abc_glm* glm, const abc_summary* sum, abc_ctx* ctx, const double* theta, const double* stats,
                                        size_t K, size_t P, size_t n, const double* obs, const double* w) {
    CHECK_CTX(ctx);
    const char* fn = "abc_glm_weighted_summary";
    ABC_TRY(glm_weighted_check(ctx, fn, glm, theta, K, stats, K, K, P, n, obs, true, sum));
    ABC_TRY(abc_ws_reserve(ctx, abc_glm_need(1, K, P, n, glm->G, true) + (K * (P + n + 1) + n) * 8 + glm_stage_bytes(glm, 1, K, P, n) +
                                    P * (sum->quant ? sum->nq + 2 : 2) * 8 + 20 * 256));
    Stage s{ctx};
    const double* th_d = s.up(theta, K * P);
    const double* st_d = s.up(stats, K * n);
    const double* ob_d = s.up(obs, n);
    const double* w_d = w ? s.up(w, K) : nullptr;
    const abc_glm d = glm_stage(s, glm, 1, K, P, n);
    const abc_summary sd = glm_summary_stage(s, sum, 1, P);
    if (s.full) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    if (w_d) ABC_TRY(abc_summary_check_weights(ctx, w_d, K, fn));
    ABC_TRY(launch_glm(ctx, weighted_values(th_d, K, w_d), st_d, K, th_d, K, nullptr, nullptr, w_d, ob_d, (int)n, 1, K, P, n, n, &d, &sd, fn));
    glm_down(s, glm, d, 1, K, P, n);
    glm_summary_down(s, sum, sd, 1, P);
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}

// ---- the same products of P given columns of K values (V[e + ldv j], weights w or NULL): one segment group ----
static int weighted_values_check(abc_ctx* ctx, const char* fn, const double* V, size_t ldv, size_t K, size_t P) {
    if (!V) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (V is required)", fn);
    if (K == 0) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: K == 0", fn);
    if (P == 0) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: P == 0", fn);
    if (ldv < K) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: ldv %zu < K %zu", fn, ldv, K);
    if (P > 1024) ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: P = %zu parameters (at most 1024)", fn, P);
    if (K >= ((size_t)1 << 32)) ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: K = %zu values (at most 2^32 - 1)", fn, K);
    return ABC_OK;
}

static SmValues weighted_values(const double* V, size_t ldv, const double* w) {
    SmValues sv = {};
    sv.method = 2;
    sv.V = V;
    sv.ldv = ldv;
    sv.w = w;
    return sv;
}

// a product of an unweighted sample takes no weights
static int weighted_equal_check(abc_ctx* ctx, const char* fn, const double* w, const Product& p) {
    if (w && p.equal_weights())
        ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: weights w are given, and the estimate is for entries of equal weight (pass w = NULL)", fn);
    return ABC_OK;
}

// device pointers (p's arrays too)
static int weighted_dev(abc_ctx* ctx, const char* fn, const double* V, size_t ldv, size_t K, size_t P, const double* w,
                        const Product& p) {
    ABC_TRY(weighted_values_check(ctx, fn, V, ldv, K, P));
    ABC_TRY(p.check(ctx, fn, P));
    ABC_TRY(weighted_equal_check(ctx, fn, w, p));
    ABC_TRY(abc_ws_reserve(ctx, p.need(1, K, P) + 16 * 256));
    if (w) ABC_TRY(abc_summary_check_weights(ctx, w, K, fn));
    return p.launch(ctx, weighted_values(V, ldv, w), 1, K, P, fn);
}

// host pointers: upload, the product on the arena's copies, downloads, synchronise
static int weighted_host(abc_ctx* ctx, const char* fn, const double* V, size_t K, size_t P, const double* w, Product p) {
    ABC_TRY(weighted_values_check(ctx, fn, V, K, K, P));
    ABC_TRY(p.check(ctx, fn, P));
    ABC_TRY(weighted_equal_check(ctx, fn, w, p));
    ABC_TRY(abc_ws_reserve(ctx, p.need(1, K, P) + (K * P + K) * 8 + p.stage_bytes(1, K, P) + 16 * 256));
    Stage s{ctx};
    const double* V_d = s.up(V, K * P);
    const double* w_d = w ? s.up(w, K) : nullptr;
    const Product d = p.stage(s, 1, K, P);
    if (s.full) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    if (w_d) ABC_TRY(abc_summary_check_weights(ctx, w_d, K, fn));
    ABC_TRY(d.launch(ctx, weighted_values(V_d, K, w_d), 1, K, P, fn));
    p.down(s, 1, K, P);
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}

extern "C" int abc_weighted_summary_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t K, size_t P, const double* w,
                                        const abc_summary* sum) {
    CHECK_CTX(ctx);
    return weighted_dev(ctx, "abc_weighted_summary_dev", V, ldv, K, P, w, Product(sum));
}

extern "C" int abc_weighted_summary(abc_ctx* ctx, const double* V, size_t K, size_t P, const double* w, const abc_summary* sum) {
    CHECK_CTX(ctx);
    return weighted_host(ctx, "abc_weighted_summary", V, K, P, w, Product(sum));
}

extern "C" int abc_weighted_density_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t K, size_t P, const double* w,
                                        const abc_density* den) {
    CHECK_CTX(ctx);
    return weighted_dev(ctx, "abc_weighted_density_dev", V, ldv, K, P, w, Product(den));
}

extern "C" int abc_weighted_density(abc_ctx* ctx, const double* V, size_t K, size_t P, const double* w, const abc_density* den) {
    CHECK_CTX(ctx);
    return weighted_host(ctx, "abc_weighted_density", V, K, P, w, Product(den));
}

extern "C" int abc_weighted_joint_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t K, size_t P, const double* w,
                                      const abc_joint* jt) {
    CHECK_CTX(ctx);
    return weighted_dev(ctx, "abc_weighted_joint_dev", V, ldv, K, P, w, Product(jt));
}

extern "C" int abc_weighted_joint(abc_ctx* ctx, const double* V, size_t K, size_t P, const double* w, const abc_joint* jt) {
    CHECK_CTX(ctx);
    return weighted_host(ctx, "abc_weighted_joint", V, K, P, w, Product(jt));
}

extern "C" int abc_weighted_draws_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t K, size_t P, const double* w,
                                      const abc_draws* dr) {
    CHECK_CTX(ctx);
    return weighted_dev(ctx, "abc_weighted_draws_dev", V, ldv, K, P, w, Product(dr));
}

extern "C" int abc_weighted_draws(abc_ctx* ctx, const double* V, size_t K, size_t P, const double* w, const abc_draws* dr) {
    CHECK_CTX(ctx);
    return weighted_host(ctx, "abc_weighted_draws", V, K, P, w, Product(dr));
}

extern "C" int abc_weighted_entropy_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t K, size_t P, const double* w,
                                        const abc_entropy* en) {
    CHECK_CTX(ctx);
    return weighted_dev(ctx, "abc_weighted_entropy_dev", V, ldv, K, P, w, Product(en));
}

extern "C" int abc_weighted_entropy(abc_ctx* ctx, const double* V, size_t K, size_t P, const double* w, const abc_entropy* en) {
    CHECK_CTX(ctx);
    return weighted_host(ctx, "abc_weighted_entropy", V, K, P, w, Product(en));
}

extern "C" int abc_weighted_hpd_dev(abc_ctx* ctx, const double* V, size_t ldv, size_t K, size_t P, const double* w, const abc_hpd* hd) {
    CHECK_CTX(ctx);
    return weighted_dev(ctx, "abc_weighted_hpd_dev", V, ldv, K, P, w, Product(hd));
}

extern "C" int abc_weighted_hpd(abc_ctx* ctx, const double* V, size_t K, size_t P, const double* w, const abc_hpd* hd) {
    CHECK_CTX(ctx);
    return weighted_host(ctx, "abc_weighted_hpd", V, K, P, w, Product(hd));
}

extern "C" int abc_param_transf(abc_ctx* ctx, const double* V, size_t n, size_t P, int inverse, double* out) {
    CHECK_CTX(ctx);
    ABC_TRY(param_transf_check(ctx, "abc_param_transf", V, n, n, P, out, n));
    if (n == 0 || P == 0) return ABC_OK;
    ABC_TRY(abc_ws_reserve(ctx, n * P * 8 + 4 * 256));
    Stage s{ctx};
    const double* V_d = s.up(V, n * P);
    if (s.full) ABC_FAIL(ctx, ABC_ERR_NOMEM, "abc_param_transf: workspace exhausted");
    const AbcTf tf = ctx_tf(ctx);
    ABC_TRY(launch_param_transf(ctx, &tf, V_d, n, n, P, inverse, (double*)V_d, n, ctx->tf_outside_dev));
    s.down(out, V_d, n * P);
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}

// ---- Box-Cox transform of the metrics (boxcox.hip) ---------------------------------------------------------------------------------
extern "C" int abc_box_cox_grid(float lambda_min, float lambda_max, float step, double* grid, size_t cap, size_t* L) {
    if (!L) return ABC_ERR_INVALID;
    *L = 0;
    const double lo = (double)lambda_min, hi = (double)lambda_max, st = (double)step;
    if (!isfinite(lo) || !isfinite(hi) || !isfinite(st) || !(st > 0.0)) return ABC_ERR_INVALID;
    size_t n = 0;
    for (double lam = lo; lam <= hi; lam += st) {            // the reference's loop (AbcUtil.cpp:93) with its float arguments widened
        if (n == ABC_BOX_COX_MAXL) return ABC_ERR_INVALID;
        if (grid && n < cap) grid[n] = lam;
        n++;
    }
    if (n == 0) return ABC_ERR_INVALID;
    *L = n;
    return (grid && cap < n) ? ABC_ERR_INVALID : ABC_OK;
}

static int box_cox_check(abc_ctx* ctx, const char* fn, const char* rows_name, size_t ldx, size_t rows, size_t M, const double* shift) {
    if (rows == 0 || M == 0) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: %s = %zu, M = %zu (both must be positive)", fn, rows_name, rows, M);
    if (ldx < rows) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: ldx %zu < %s %zu", fn, ldx, rows_name, rows);
    if (rows >= ((size_t)1 << 32)) ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: %s = %zu, 2^32 rows or more are not supported", fn, rows_name, rows);
    if (shift)
        for (size_t j = 0; j < M; ++j)
            if (!isfinite(shift[j])) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: shift[%zu] is not finite", fn, j);
    return ABC_OK;
}

static int box_cox_search_check(abc_ctx* ctx, const char* fn, const double* X, size_t ldx, size_t N, size_t M, const double* shift,
                                const double* grid, size_t L, const abc_box_cox_out* out) {
    if (!X || !grid || !out || !out->lambda)
        ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (X, grid, out and out->lambda are required)", fn);
    if (L < 1 || L > ABC_BOX_COX_MAXL) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: L = %zu is outside 1..%d", fn, L, (int)ABC_BOX_COX_MAXL);
    ABC_TRY(box_cox_check(ctx, fn, "N", ldx, N, M, shift));
    for (size_t k = 0; k < L; ++k)
        if (!isfinite(grid[k])) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: grid[%zu] is not finite", fn, k);
    return ABC_OK;
}

static int box_cox_apply_check(abc_ctx* ctx, const char* fn, const double* X, size_t ldx, size_t n, size_t M, const double* lambda,
                               const double* shift, const double* out, size_t ldo) {
    if (!X || !lambda || !out) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: null argument (X, lambda and out are required)", fn);
    ABC_TRY(box_cox_check(ctx, fn, "n", ldx, n, M, shift));
    if (ldo < n) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: ldo %zu < n %zu", fn, ldo, n);
    for (size_t j = 0; j < M; ++j)
        if (!isfinite(lambda[j])) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: lambda[%zu] is not finite", fn, j);
    return ABC_OK;
}

extern "C" int abc_optimize_box_cox_dev(abc_ctx* ctx, const double* X, size_t ldx, size_t N, size_t M, const double* shift,
                                        const double* grid, size_t L, const abc_box_cox_out* out) {
    CHECK_CTX(ctx);
    ABC_TRY(box_cox_search_check(ctx, "abc_optimize_box_cox_dev", X, ldx, N, M, shift, grid, L, out));
    ABC_TRY(abc_ws_reserve(ctx, abc_box_cox_need(N, M, L) + (L + M) * 8 + 4 * 256));
    Stage s{ctx};
    const double* grid_d = s.up(grid, L);
    const double* shift_d = shift ? s.up(shift, M) : nullptr;
    if (s.full) ABC_FAIL(ctx, ABC_ERR_NOMEM, "abc_optimize_box_cox_dev: workspace exhausted");
    const int rc = launch_box_cox_search(ctx, X, ldx, N, M, shift_d, grid_d, L, out);
    if (rc == ABC_ERR_NOMEM) ABC_FAIL(ctx, ABC_ERR_NOMEM, "abc_optimize_box_cox_dev: workspace exhausted");
    ABC_TRY(rc);
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}

extern "C" int abc_optimize_box_cox(abc_ctx* ctx, const double* X, size_t N, size_t M, const double* shift, const double* grid, size_t L,
                                    const abc_box_cox_out* out) {
    CHECK_CTX(ctx);
    ABC_TRY(box_cox_search_check(ctx, "abc_optimize_box_cox", X, N, N, M, shift, grid, L, out));
    ABC_TRY(abc_ws_reserve(ctx, abc_box_cox_need(N, M, L) + (N * M + L + 4 * M + M * L) * 8 + 10 * 256));
    Stage s{ctx};
    const double* X_d = s.up(X, N * M);
    const double* grid_d = s.up(grid, L);
    const double* shift_d = shift ? s.up(shift, M) : nullptr;
    abc_box_cox_out d;
    d.lambda = s.dev<double>(M);
    d.best_skew = out->best_skew ? s.dev<double>(M) : nullptr;
    d.skew = out->skew ? s.dev<double>(M * L) : nullptr;
    d.pick = out->pick ? s.dev<int32_t>(M) : nullptr;
    d.status = out->status ? s.dev<int32_t>(M) : nullptr;
    if (s.full) ABC_FAIL(ctx, ABC_ERR_NOMEM, "abc_optimize_box_cox: workspace exhausted");
    const int rc = launch_box_cox_search(ctx, X_d, N, N, M, shift_d, grid_d, L, &d);
    if (rc == ABC_ERR_NOMEM) ABC_FAIL(ctx, ABC_ERR_NOMEM, "abc_optimize_box_cox: workspace exhausted");
    ABC_TRY(rc);
    s.down(out->lambda, (const double*)d.lambda, M);
    s.down(out->best_skew, (const double*)d.best_skew, M);
    s.down(out->skew, (const double*)d.skew, M * L);
    s.down(out->pick, (const int32_t*)d.pick, M);
    s.down(out->status, (const int32_t*)d.status, M);
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}

extern "C" int abc_box_cox_dev(abc_ctx* ctx, const double* X, size_t ldx, size_t n, size_t M, const double* lambda, const double* shift,
                               double* out, size_t ldo) {
    CHECK_CTX(ctx);
    ABC_TRY(box_cox_apply_check(ctx, "abc_box_cox_dev", X, ldx, n, M, lambda, shift, out, ldo));
    ABC_TRY(abc_ws_reserve(ctx, 2 * M * 8 + 4 * 256));
    Stage s{ctx};
    const double* lambda_d = s.up(lambda, M);
    const double* shift_d = shift ? s.up(shift, M) : nullptr;
    if (s.full) ABC_FAIL(ctx, ABC_ERR_NOMEM, "abc_box_cox_dev: workspace exhausted");
    return launch_box_cox_apply(ctx, X, ldx, n, M, lambda_d, shift_d, out, ldo);
}

extern "C" int abc_box_cox(abc_ctx* ctx, const double* X, size_t n, size_t M, const double* lambda, const double* shift, double* out) {
    CHECK_CTX(ctx);
    ABC_TRY(box_cox_apply_check(ctx, "abc_box_cox", X, n, n, M, lambda, shift, out, n));
    ABC_TRY(abc_ws_reserve(ctx, (n * M + 2 * M) * 8 + 6 * 256));
    Stage s{ctx};
    const double* X_d = s.up(X, n * M);
    const double* lambda_d = s.up(lambda, M);
    const double* shift_d = shift ? s.up(shift, M) : nullptr;
    if (s.full) ABC_FAIL(ctx, ABC_ERR_NOMEM, "abc_box_cox: workspace exhausted");
    ABC_TRY(launch_box_cox_apply(ctx, X_d, n, n, M, lambda_d, shift_d, (double*)X_d, n));
    s.down(out, X_d, n * M);
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}

extern "C" int abc_targets_fallbacks(abc_ctx* ctx, uint64_t* count, int reset) {
    if (!ctx || !count) return ABC_ERR_INVALID;
    *count = (uint64_t)ctx->targets_fallbacks;
    if (reset) ctx->targets_fallbacks = 0;
    return ABC_OK;
}
