// AbcUtilHip.hpp -- C++ host facade with the reference's own signatures for the hot path
// (/root/reference/include/AbcSmc/AbcUtil.h:78-172), header-only over the C ABI (include/abcsmc_hip.h).
//
// Drop-in intent: a translation unit that used `ABC::particle_ranking_PLS(...)` etc. from AbcUtil.h includes
// this header instead and links libabcsmc_hip.so.  Eigen and GSL are not required: Mat2D / Row / Col are the
// minimal column-major containers below (Eigen's default storage order, so `Eigen::Map` over `.data()` is a
// zero-copy view either way), `gsl_rng*` becomes `ABC::RNG*` (taus2, bit-compatible stream), and the
// `vector<const Parameter*>` argument keeps its meaning through the three concrete priors of Priors.h:46-110.
// Errors: the reference asserts / exits / lets GSL abort; here every failure throws ABC::HipError.
#ifndef ABCSMC_AMD_ABCUTILHIP_HPP
#define ABCSMC_AMD_ABCUTILHIP_HPP

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/abcsmc_hip.h"

namespace ABC {

typedef double float_type;
typedef std::vector<float_type> Row;
typedef std::vector<float_type> Col;

struct Mat2D {                                   // column-major, like Eigen::Matrix<double,Dynamic,Dynamic>
    size_t r, c;
    std::vector<float_type> v;
    Mat2D() : r(0), c(0) {}
    Mat2D(size_t rows_, size_t cols_) : r(rows_), c(cols_), v(rows_ * cols_, 0.0) {}
    size_t rows() const { return r; }
    size_t cols() const { return c; }
    float_type& operator()(size_t i, size_t j) { return v[i + r * j]; }
    float_type operator()(size_t i, size_t j) const { return v[i + r * j]; }
    const float_type* data() const { return v.data(); }
    float_type* data() { return v.data(); }
};

struct HipError : std::runtime_error {
    int code;
    HipError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// ---- RNG: stands in for `const gsl_rng*` of type gsl_rng_taus2 (examples/include/examples.h:10) ----------
struct RNG {
    mutable abc_rng state;
    explicit RNG(unsigned long seed = 0) { abc_rng_set(&state, seed); }
};
inline void rng_set(const RNG* r, unsigned long seed) { abc_rng_set(&r->state, seed); }     // gsl_rng_set
inline unsigned long rng_get(const RNG* r) { return abc_rng_get(&r->state); }                // gsl_rng_get
// the three GSL draws Priors.h uses for set 0 (host side, one-off per fit): gsl_rng_uniform = get / 2^32;
// gsl_rng_uniform_pos redraws a zero; gsl_rng_uniform_int rejects above n * (0xffffffff / n); gsl_ran_gaussian is the
// polar Box-Muller on uniform_pos draws mapped to (-1, 1) [published GSL 2.x algorithms; GSL itself is not in this image]
inline double rng_uniform(const RNG* r) { return abc_rng_get(&r->state) / 4294967296.0; }
inline double rng_uniform_pos(const RNG* r) {
    double x;
    do { x = rng_uniform(r); } while (x == 0.0);
    return x;
}
inline unsigned long rng_uniform_int(const RNG* r, unsigned long n) {
    const unsigned long scale = 0xffffffffUL / n;
    unsigned long k;
    do { k = abc_rng_get(&r->state) / scale; } while (k >= n);
    return k;
}
inline double ran_gaussian(const RNG* r, double sigma) {
    double x, y, r2;
    do {
        x = -1.0 + 2.0 * rng_uniform_pos(r);      // gauss.c: gsl_rng_uniform_pos, a zero output is drawn again
        y = -1.0 + 2.0 * rng_uniform_pos(r);
        r2 = x * x + y * y;
    } while (r2 > 1.0 || r2 == 0.0);
    return sigma * y * std::sqrt(-2.0 * std::log(r2) / r2);
}

// ---- ParRNG (ParRNG.h:19-81): the RNG handed to Parameter::sample, plus the odometer over PSEUDO states and
// the cursor over POSTERIOR rows.  One pseudo parameter advances per unlock(); a parameter at its last state
// wraps to 0 and lets the next one advance.
struct Parameter;
struct ParRNG {
    ParRNG(const RNG* rng, const std::vector<const Parameter*>& mpars, size_t posterior_size);
    const RNG* rng() const { return rng_; }
    void unlock() { lock_ = false; }
    size_t pseudo(const Parameter* p) {
        std::pair<size_t, size_t>* st = nullptr;
        for (auto& e : pseudo_) if (e.first == p) st = &e.second;
        if (!st) throw std::logic_error("ParRNG::pseudo: parameter was not registered");
        const size_t ret = st->first;
        if (!lock_) {
            if (st->first < st->second) { st->first++; lock_ = true; } else { st->first = 0; }
        }
        return ret;
    }
    size_t posterior() {
        const size_t ret = post_idx_;
        if (!lock_) post_idx_ = (post_idx_ < post_max_) ? post_idx_ + 1 : 0;
        return ret;
    }

   private:
    const RNG* rng_;
    std::vector<std::pair<const Parameter*, std::pair<size_t, size_t>>> pseudo_;   // (state, last state)
    bool lock_ = false;
    size_t post_idx_ = 0, post_max_;
};
typedef ParRNG PRNG;

// ---- parameters (Parameter.h:36-87, Priors.h:9-110, IndexedPars.h:9-55) ------------------------------------
// The device evaluates likelihood / recast / valid / noise from the POD (`pod()`); the host keeps the names and
// the set-0 `sample`.  The two-argument constructors (no names) are a convenience the reference does not have.
struct Parameter {
    Parameter(const std::string& s = "", const std::string& ss = "", size_t states = 0)
        : name(s), short_name(ss), state_size_(states) {}
    virtual ~Parameter() {}
    std::string get_name() const { return name; }
    std::string get_short_name() const { return short_name; }
    virtual abc_prior pod() const = 0;
    virtual float_type sample(PRNG& prng) const = 0;
    virtual float_type likelihood(float_type pval) const = 0;
    virtual float_type recast(float_type pval) const = 0;
    virtual float_type get_mean() const { return std::nan(""); }
    virtual float_type get_sd() const { return std::nan(""); }
    virtual bool isPosterior() const { return false; }
    bool valid(float_type pval) const { return likelihood(pval) != 0.0; }
    // Parameter.h:52-77 / Priors.h:19-43: recast(N(mu, sigma)) from the shared taus2 stream until it is valid, at most MAX_ATTEMPTS
    // times; then the prior's mean, with the reference's message on stderr (host side: one value at a time, as upstream)
    float_type noise(const RNG* rng, const float_type mu, const float_type sigma, const size_t MAX_ATTEMPTS = 1000) const {
        size_t attempts = 1;
        float_type dev = recast(ran_gaussian(rng, sigma) + mu);
        while (!valid(dev) && (attempts++ < MAX_ATTEMPTS)) dev = recast(ran_gaussian(rng, sigma) + mu);
        if (!valid(dev)) {
            std::fprintf(stderr, "ERROR: failed to draw valid noise from prior %s - returning mean value.\n", get_name().c_str());
            return get_mean();
        }
        return dev;
    }
    size_t state_size() const { return state_size_; }

   private:
    std::string name, short_name;
    size_t state_size_;
};
inline ParRNG::ParRNG(const RNG* rng, const std::vector<const Parameter*>& mpars, size_t posterior_size)
    : rng_(rng), post_max_(posterior_size - 1) {
    for (const Parameter* p : mpars)
        if (!p->isPosterior() && p->state_size() != 0) pseudo_.push_back({p, {0, p->state_size() - 1}});
}

struct GaussianPrior : Parameter {
    float_type mean, sd;
    GaussianPrior(const std::string& nm, const std::string& snm, float_type mn, float_type s)
        : Parameter(nm, snm), mean(mn), sd(s) {}
    GaussianPrior(float_type mn, float_type s) : mean(mn), sd(s) {}
    abc_prior pod() const override { return abc_prior{ABC_PRIOR_GAUSS, 0, mean, sd}; }
    float_type sample(PRNG& prng) const override { return ran_gaussian(prng.rng(), sd) + mean; }
    float_type likelihood(float_type pval) const override {
        const float_type u = (pval - mean) / std::fabs(sd);
        return (1.0 / (std::sqrt(2.0 * M_PI) * std::fabs(sd))) * std::exp(-u * u / 2.0);
    }
    float_type recast(float_type pval) const override { return pval; }
    float_type get_mean() const override { return mean; }
    float_type get_sd() const override { return sd; }
};
struct DiscreteUniformPrior : Parameter {
    long minval, maxval;
    DiscreteUniformPrior(const std::string& nm, const std::string& snm, long mn, long mx)
        : Parameter(nm, snm), minval(mn), maxval(mx) {}
    DiscreteUniformPrior(long mn, long mx) : minval(mn), maxval(mx) {}
    abc_prior pod() const override { return abc_prior{ABC_PRIOR_UNIF_INT, 0, (double)minval, (double)maxval}; }
    float_type sample(PRNG& prng) const override {
        return (float_type)((long)rng_uniform_int(prng.rng(), (unsigned long)(maxval - minval + 1)) + minval);
    }
    float_type likelihood(float_type pval) const override {
        return (pval == recast(pval) && minval <= pval && pval <= maxval) ? 1.0 / (maxval - minval + 1) : 0.0;
    }
    float_type recast(float_type pval) const override { return std::round(pval); }
    float_type get_mean() const override { return (float_type)(maxval + minval) / 2.0; }
    float_type get_sd() const override { return (float_type)(maxval - minval) / std::sqrt(12.0); }
};
struct ContinuousUniformPrior : Parameter {
    float_type minval, maxval;
    ContinuousUniformPrior(const std::string& nm, const std::string& snm, float_type mn, float_type mx)
        : Parameter(nm, snm), minval(mn), maxval(mx) {}
    ContinuousUniformPrior(float_type mn, float_type mx) : minval(mn), maxval(mx) {}
    abc_prior pod() const override { return abc_prior{ABC_PRIOR_UNIF_REAL, 0, minval, maxval}; }
    float_type sample(PRNG& prng) const override { return rng_uniform(prng.rng()) * (maxval - minval) + minval; }
    float_type likelihood(float_type pval) const override {
        return (minval <= pval && pval <= maxval) ? 1.0 / (maxval - minval) : 0.0;
    }
    float_type recast(float_type pval) const override { return pval; }
    float_type get_mean() const override { return (maxval + minval) / 2.0; }
    float_type get_sd() const override { return (maxval - minval) / std::sqrt(12.0); }
};
// PSEUDO / POSTERIOR parameters only occur in projection mode (one set, no weights, no perturbation): asking them
// for a density is an error upstream too (IndexedPars.h:20-28)
struct IndexedPar : Parameter {
    IndexedPar(const std::string& s, const std::string& ss, size_t size) : Parameter(s, ss, size) {
        if (size == 0) throw std::invalid_argument("IndexedPar: empty state set");
    }
    abc_prior pod() const override { throw std::logic_error("IndexedPar " + get_name() + " has no prior density"); }
    float_type likelihood(float_type) const override { throw std::logic_error("likelihood asked of IndexedPar " + get_name()); }
    float_type recast(float_type) const override { throw std::logic_error("recast asked of IndexedPar " + get_name()); }
};
struct PseudoPar : IndexedPar {
    std::vector<float_type> states;
    PseudoPar(const std::string& s, const std::string& ss, const std::vector<float_type>& vals)
        : IndexedPar(s, ss, vals.size()), states(vals) {}
    float_type sample(PRNG& prng) const override { return states[prng.pseudo(this)]; }
};
struct PosteriorPar : IndexedPar {
    PosteriorPar(const std::string& s, const std::string& ss, size_t size) : IndexedPar(s, ss, size) {}
    float_type sample(PRNG& prng) const override { return (float_type)prng.posterior(); }
    bool isPosterior() const override { return true; }
};

// ---- context (one per host thread, device 0 unless set before first use) -------------------------------
inline int& default_device() { static int d = 0; return d; }
inline abc_ctx* context() {
    static thread_local abc_ctx* ctx = nullptr;
    if (!ctx) {
        const int rc = abc_ctx_create(default_device(), &ctx);
        if (rc != ABC_OK) throw HipError(rc, "abc_ctx_create failed: no usable MI355X (there is no CPU fallback)");
    }
    return ctx;
}
inline void check(int rc) { if (rc != ABC_OK) throw HipError(rc, abc_last_error(context())); }
// Proposals from the reference's own sequential taus2 stream (abc_ctx_set_noise_mode): values, seeds and the final RNG state
// of sample_*_predictive_priors then equal a CPU run of the reference bit for bit; default off (device Philox stream).
inline void set_reference_stream(bool on) { check(abc_ctx_set_noise_mode(context(), on ? ABC_NOISE_REFERENCE_STREAM : ABC_NOISE_DEVICE)); }
inline uint64_t perturb_giveups(bool reset = false) {
    uint64_t n = 0;
    check(abc_perturb_giveups(context(), &n, reset ? 1 : 0));
    return n;
}
// What the speculation on the component count has cost this context (abc_generation_repeats): whole generations under the Wilcoxon
// rule rank on the count the fit wrote while the reduction runs beside them; .first = how often the reduction lowered the largest
// count and the ranking was repeated, .second = how often a generation started over (degenerate selection, a cascade that gave up)
inline std::pair<uint64_t, uint64_t> generation_repeats(bool reset = false) {
    uint64_t r = 0, g = 0;
    check(abc_generation_repeats(context(), &r, &g, reset ? 1 : 0));
    return {r, g};
}
// How many PLS components particle_ranking_PLS keeps (AbcUtil.cpp:447-449: `PLS::optimal_num_components(em).maxCoeff()`; the PLS
// library is not in the reference tree).  SURVEY A.2, the only specification of it at hand, describes upstream as: per response
// the component count of least PRESS, REDUCED to the smallest count whose validation errors a two-sided Wilcoxon signed-rank
// test (alpha = 0.1) cannot tell from it.  That is the drop-in default here (ABC_RULE_WILCOXON); ABC_RULE_MIN_PRESS keeps the
// plain argmin (about 1 ms less per million particles; never fewer components).  `max_components` = 0 means min(#metrics,
// #parameters), the unverifiable default of `PLS::Model plsm(X, Y)` (AbcUtil.cpp:443).
inline int& component_rule_ref() { static int r = ABC_RULE_WILCOXON; return r; }
inline int& max_components_ref() { static int a = 0; return a; }
inline void set_component_rule(int rule) {
    if (rule != ABC_RULE_MIN_PRESS && rule != ABC_RULE_WILCOXON) throw HipError(ABC_ERR_INVALID, "set_component_rule: unknown rule");
    component_rule_ref() = rule;
}
inline int component_rule() { return component_rule_ref(); }
inline void set_max_components(int a) { max_components_ref() = a < 0 ? 0 : a; }
inline std::vector<abc_prior> to_pod(const std::vector<const Parameter*>& pars) {
    std::vector<abc_prior> p;
    for (const Parameter* q : pars) p.push_back(q->pod());
    return p;
}

// ---- several GPUs of one node (include/abcsmc_hip.h, "Multi-GPU"; the reference has no multi-device path) ----------
// use_devices({0, 1, ...}) joins the listed GPUs with RCCL communicators (abc_ctx_create_multi); rank_and_weight() then
// runs the rank + truncate + doubled variance + weights of one finished set (AbcSmc.cpp:634-664, 1041-1066) with the set's
// rows sharded over them (abc_generation_multi).  Without it every call below runs on the one default device.
inline std::vector<abc_ctx*>& multi_contexts() { static std::vector<abc_ctx*> v; return v; }
inline void use_devices(const std::vector<int>& devices) {
    for (abc_ctx* c : multi_contexts()) abc_ctx_destroy(c);
    multi_contexts().clear();
    if (devices.empty()) return;
    std::vector<abc_ctx*> v(devices.size(), nullptr);
    const int rc = abc_ctx_create_multi(devices.data(), (int)devices.size(), v.data());
    if (rc != ABC_OK) throw HipError(rc, "abc_ctx_create_multi failed (RCCL not loadable, or a listed GPU is not usable)");
    multi_contexts() = v;
}
inline bool multi_device() { return !multi_contexts().empty(); }
struct RankedSet {
    std::vector<size_t> idx;      // the K best particles, ascending distance
    Row dist;                     // their distances
    Mat2D theta;                  // their parameter rows (K x P)
    Row weights, doubled_variance;
    int ncomp = 0;
};
inline RankedSet rank_and_weight(const Mat2D& X, const Mat2D& Y, const Row& obs, float_type training_fraction, size_t K,
                                 const std::vector<const Parameter*>& mpars, const Mat2D* prev_params = nullptr,
                                 const Row* prev_weights = nullptr, const Row* prev_doubled_variance = nullptr,
                                 int rule = -1 /* -1: component_rule() */, int max_components = -1 /* -1: the process-wide setting */) {
    if (!multi_device()) throw HipError(ABC_ERR_INVALID, "rank_and_weight: call use_devices() first");
    const size_t N = X.rows(), M = X.cols(), P = Y.cols();
    RankedSet out;
    std::vector<uint64_t> idx(K);
    out.dist.assign(K, 0.0); out.theta = Mat2D(K, P); out.weights.assign(K, 0.0); out.doubled_variance.assign(P, 0.0);
    const std::vector<abc_prior> pr = to_pod(mpars);
    abc_generation_cfg cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.N = N; cfg.M = M; cfg.P = P; cfg.K = K; cfg.Kp = prev_params ? prev_params->rows() : 0; cfg.Nnext = 0;
    cfg.train_frac = training_fraction; cfg.max_comp = max_components < 0 ? max_components_ref() : max_components;
    cfg.rule = rule < 0 ? component_rule() : rule; cfg.multivariate = 0;
    abc_generation_io io;
    memset(&io, 0, sizeof(io));
    io.X = X.data(); io.Y = Y.data(); io.obs = obs.data(); io.priors = pr.data();
    if (prev_params) { io.theta_prev = prev_params->data(); io.w_prev = prev_weights->data(); io.dv_prev = prev_doubled_variance->data(); }
    io.idx = idx.data(); io.dist = out.dist.data(); io.theta = out.theta.data(); io.w = out.weights.data();
    io.dv = out.doubled_variance.data();
    abc_rng unused = {0, 0, 0};
    int32_t nc = 0;
    const int rc = abc_generation_multi(multi_contexts().data(), (int)multi_contexts().size(), &cfg, &io, &unused, &nc);
    if (rc != ABC_OK) throw HipError(rc, abc_last_error(multi_contexts()[0]));
    out.idx.assign(idx.begin(), idx.end());
    out.ncomp = nc;
    return out;
}

// ---- AbcUtil.h:144-153 ----------------------------------------------------------------------------------
// (rule / max_components: what an AbcSmc object was configured with -- the process-wide set_component_rule / set_max_components are
// only the defaults of the four-argument form the reference has)
inline std::vector<size_t> particle_ranking_PLS(const Mat2D& X_orig, const Mat2D& Y_orig, const Row& target_values,
                                                const float_type training_fraction, int rule, int max_components) {
    if (!((0 < training_fraction) && (training_fraction <= 1))) throw HipError(ABC_ERR_INVALID, "training_fraction");
    const size_t N = X_orig.rows();
    std::vector<uint64_t> idx(N);
    check(abc_particle_ranking_pls(context(), X_orig.data(), Y_orig.data(), target_values.data(), N, X_orig.cols(),
                                   Y_orig.cols(), training_fraction, max_components, rule, N, idx.data(), nullptr,
                                   nullptr, nullptr, nullptr, nullptr));
    return std::vector<size_t>(idx.begin(), idx.end());
}
inline std::vector<size_t> particle_ranking_PLS(const Mat2D& X_orig, const Mat2D& Y_orig, const Row& target_values,
                                                const float_type training_fraction) {
    return particle_ranking_PLS(X_orig, Y_orig, target_values, training_fraction, component_rule(), max_components_ref());
}
// Many observed targets against one set (abc_particle_ranking_pls_targets): targets is B x M, one target per row.  One fit shared by
// all targets; returns, per target, the K best rows in ascending distance -- the first K of particle_ranking_PLS for that target.
inline std::vector<std::vector<size_t>> particle_ranking_PLS_targets(const Mat2D& X, const Mat2D& Y, const Mat2D& targets,
                                                                    const float_type train_frac, size_t K) {
    if (!((0 < train_frac) && (train_frac <= 1))) throw HipError(ABC_ERR_INVALID, "training_fraction");
    const size_t B = targets.rows();
    std::vector<uint64_t> idx(B * K);
    check(abc_particle_ranking_pls_targets(context(), X.data(), Y.data(), X.rows(), X.cols(), Y.cols(), targets.data(), B, train_frac,
                                           max_components_ref(), component_rule(), nullptr, K, idx.data(), nullptr, nullptr, nullptr));
    std::vector<std::vector<size_t>> out(B);
    for (size_t b = 0; b < B; b++) out[b].assign(idx.begin() + b * K, idx.begin() + (b + 1) * K);
    return out;
}
// The same ranking followed by the local-linear regression adjustment of every target's K rows on their PLS scores
// (abc_particle_ranking_pls_targets_adjust; kernel 0 Epanechnikov, 1 rectangular).  Per target: the rows, the adjusted parameter
// rows (K x P) and the coefficients ((A + 1) x P: row 0 = alpha, the adjusted posterior mean; row 1 + k = beta_k).
struct TargetAdjustment {
    std::vector<size_t> idx;
    Mat2D theta;
    Mat2D coef;
    int rank = 0, status = 0;
};
inline std::vector<TargetAdjustment> particle_ranking_PLS_targets_adjust(const Mat2D& X, const Mat2D& Y, const Mat2D& targets,
                                                                        const float_type train_frac, size_t K, int kernel = 0) {
    if (!((0 < train_frac) && (train_frac <= 1))) throw HipError(ABC_ERR_INVALID, "training_fraction");
    const size_t B = targets.rows(), P = Y.cols(), M = X.cols();
    const int mc = max_components_ref();
    const size_t A = mc > 0 ? (size_t)mc : (M < P ? M : P);
    std::vector<uint64_t> idx(B * K);
    std::vector<double> th(B * K * P), cf(B * (A + 1) * P);
    std::vector<int32_t> rank(B), status(B);
    abc_adjust_out out = {th.data(), nullptr, cf.data(), rank.data(), status.data()};
    check(abc_particle_ranking_pls_targets_adjust(context(), X.data(), Y.data(), X.rows(), M, P, targets.data(), B, train_frac, mc,
                                                  component_rule(), nullptr, K, kernel, idx.data(), nullptr, &out, nullptr));
    std::vector<TargetAdjustment> res(B);
    for (size_t b = 0; b < B; b++) {
        TargetAdjustment& r = res[b];
        r.idx.assign(idx.begin() + b * K, idx.begin() + (b + 1) * K);
        r.theta = Mat2D(K, P);
        for (size_t e = 0; e < K; e++)
            for (size_t j = 0; j < P; j++) r.theta(e, j) = th[(b * K + e) * P + j];
        r.coef = Mat2D(A + 1, P);
        for (size_t k = 0; k <= A; k++)
            for (size_t j = 0; j < P; j++) r.coef(k, j) = cf[(b * (A + 1) + k) * P + j];
        r.rank = rank[b];
        r.status = status[b];
    }
    return res;
}
// Parameter transforms of the local-linear adjustment (abc_ctx_set_param_transf; the definition is in the header): kinds holds
// ABC_TRANSF_NONE / ABC_TRANSF_LOG / ABC_TRANSF_LOGIT per parameter, lo / hi the bounds of the LOGIT entries (may be empty when
// there is none).  The setting stays in the process's context until it is cleared: every call above and below that regresses then
// fits on the transformed scale and returns adjusted rows carried back into the support.
inline void set_param_transf(const std::vector<int>& kinds, const std::vector<double>& lo = {}, const std::vector<double>& hi = {}) {
    if ((!lo.empty() && lo.size() != kinds.size()) || (!hi.empty() && hi.size() != kinds.size()))
        throw HipError(ABC_ERR_INVALID, "set_param_transf: lo and hi need one entry per parameter");
    const std::vector<int32_t> k(kinds.begin(), kinds.end());
    const abc_param_transf_t tf = {k.size(), k.data(), lo.empty() ? nullptr : lo.data(), hi.empty() ? nullptr : hi.data()};
    check(abc_ctx_set_param_transf(context(), &tf));
}
inline void clear_param_transf() { check(abc_ctx_set_param_transf(context(), nullptr)); }
// the context's transforms over the columns of V (rows x P), forward or (inverse) back; with nothing set a copy
inline Mat2D param_transf(const Mat2D& V, bool inverse = false) {
    Mat2D out(V.rows(), V.cols());
    check(abc_param_transf(context(), V.data(), V.rows(), V.cols(), inverse ? 1 : 0, out.data()));
    return out;
}

// Box-Cox transform of the metrics (AbcUtil.h:60-62, AbcUtil.cpp:89-109; the definition is in the C header).  The reference's two
// signatures over one column, the same search over every column of a table, and the transform itself.  A column with an entry
// <= 0 returns lambda = 1 (the reference would return lambda_min).  Transform the table AND the observed metrics with the same
// lambda (and shift), then hand both to any ranking call.
inline Row optimize_box_cox(const Mat2D& data, const float lambda_min = -5, const float lambda_max = 5, const float step = 0.1f,
                            const Row& shift = {}) {
    if (!shift.empty() && shift.size() != data.cols()) throw HipError(ABC_ERR_INVALID, "optimize_box_cox: shift needs one entry per column");
    double grid[ABC_BOX_COX_MAXL];
    size_t L = 0;
    if (abc_box_cox_grid(lambda_min, lambda_max, step, grid, ABC_BOX_COX_MAXL, &L) != ABC_OK)
        throw HipError(ABC_ERR_INVALID, "optimize_box_cox: the grid needs finite bounds, a step > 0 and 1 to 512 values");
    Row lambda(data.cols());
    abc_box_cox_out out = {lambda.data(), nullptr, nullptr, nullptr, nullptr};
    check(abc_optimize_box_cox(context(), data.data(), data.rows(), data.cols(), shift.empty() ? nullptr : shift.data(), grid, L, &out));
    return lambda;
}
inline float_type optimize_box_cox(const Col& data, const float lambda_min, const float lambda_max, const float step) {
    Mat2D one(data.size(), 1);
    std::copy(data.begin(), data.end(), one.data());
    return optimize_box_cox(one, lambda_min, lambda_max, step)[0];
}
inline float_type optimize_box_cox(const Col& data) { return optimize_box_cox(data, -5, 5, 0.1f); }
// y = ((x + shift)^lambda - 1) / lambda per column (lambda == 0: log(x + shift)); shift empty: zeros
inline Mat2D box_cox(const Mat2D& data, const Row& lambda, const Row& shift = {}) {
    if (lambda.size() != data.cols() || (!shift.empty() && shift.size() != data.cols()))
        throw HipError(ABC_ERR_INVALID, "box_cox: lambda and shift need one entry per column");
    Mat2D out(data.rows(), data.cols());
    check(abc_box_cox(context(), data.data(), data.rows(), data.cols(), lambda.data(), shift.empty() ? nullptr : shift.data(), out.data()));
    return out;
}

// Heteroscedastic variance correction of the local-linear adjustment (abc_ctx_set_adjust_hcorr; the definition is in the header):
// on, every call that regresses rescales the residuals of its adjusted rows by a fitted model of the residual variance.
inline void set_adjust_hcorr(bool on) { check(abc_ctx_set_adjust_hcorr(context(), on ? 1 : 0)); }

// Ridge adjustment with the penalty chosen by leave-one-out PRESS (abc_ctx_set_adjust_ridge; the definition is in the header):
// every call that regresses then returns, per parameter, the ridge fit of the penalty of `lambda` (strictly ascending, at most
// ABC_RIDGE_MAXL entries) with the smallest PRESS.  An empty list turns the setting off.
inline void set_adjust_ridge(const std::vector<double>& lambda) {
    check(abc_ctx_set_adjust_ridge(context(), lambda.empty() ? nullptr : lambda.data(), lambda.size()));
}

// Row importance weights of the batched ranking (abc_ctx_set_row_weights; the definition is in the header): one finite weight
// >= 0 per row of the table (at least one positive), copied by the context.  While set, every particle_ranking_PLS_targets* call
// on a table of that many rows weighs entry e of a target by its kernel weight times w[idx[e]]; the ranking itself does not
// change.  weight_predictive_prior's output for the N rows of a generation is accepted as is.
inline void set_row_weights(const std::vector<double>& w) {
    if (w.empty()) throw HipError(ABC_ERR_INVALID, "set_row_weights: no weights (clear_row_weights turns the setting off)");
    check(abc_ctx_set_row_weights(context(), w.data(), w.size()));
}
inline void clear_row_weights() { check(abc_ctx_set_row_weights(context(), nullptr, 0)); }

// hcoef of the last regressing call made under the correction (abc_adjust_last_hcorr), slot after slot: (slots * (A + 1)) x P,
// row s (A + 1) the log residual variance at the observation of slot s (NaN: skipped), the A rows after it its slopes
inline Mat2D last_hcorr() {
    size_t slots = 0, a1 = 0, P = 0;
    check(abc_adjust_last_hcorr(context(), nullptr, 0, &slots, &a1, &P));
    std::vector<double> buf(slots * a1 * P);
    if (!buf.empty()) check(abc_adjust_last_hcorr(context(), buf.data(), buf.size(), &slots, &a1, &P));
    Mat2D out(slots * a1, P);
    for (size_t r = 0; r < slots * a1; r++)
        for (size_t j = 0; j < P; j++) out(r, j) = buf[r * P + j];
    return out;
}
// Tolerance path (abc_particle_ranking_pls_targets_path): ONE ranking at K_max = Ks.back(), then the rejection mean and the
// local-linear fit at every tolerance of the strictly ascending list Ks (at most 16), each from the first Ks[t] rows only.  Per
// target: the K_max rows, post_mean (T x P), alpha (T x P: the adjusted posterior means), the bandwidths h, rank and status (T).
struct TargetPath {
    std::vector<size_t> idx;
    Mat2D post_mean, alpha;
    std::vector<double> h;
    std::vector<int> rank, status;
};
inline std::vector<TargetPath> particle_ranking_PLS_targets_path(const Mat2D& X, const Mat2D& Y, const Mat2D& targets,
                                                                const float_type train_frac, const std::vector<size_t>& Ks,
                                                                int kernel = 0) {
    if (!((0 < train_frac) && (train_frac <= 1))) throw HipError(ABC_ERR_INVALID, "training_fraction");
    const size_t B = targets.rows(), P = Y.cols(), M = X.cols(), T = Ks.size(), K = T ? Ks.back() : 0;
    const int mc = max_components_ref();
    const size_t A = mc > 0 ? (size_t)mc : (M < P ? M : P);
    std::vector<uint64_t> idx(B * K);
    std::vector<double> pm(B * T * P), cf(B * T * (A + 1) * P), h(B * T);
    std::vector<int32_t> rank(B * T), status(B * T);
    abc_path path = {Ks.data(), T, pm.data(), cf.data(), rank.data(), status.data(), h.data()};
    check(abc_particle_ranking_pls_targets_path(context(), X.data(), Y.data(), X.rows(), M, P, targets.data(), B, train_frac, mc,
                                                component_rule(), nullptr, kernel, idx.data(), nullptr, &path, nullptr));
    std::vector<TargetPath> res(B);
    for (size_t b = 0; b < B; b++) {
        TargetPath& r = res[b];
        r.idx.assign(idx.begin() + b * K, idx.begin() + (b + 1) * K);
        r.post_mean = Mat2D(T, P);
        r.alpha = Mat2D(T, P);
        for (size_t t = 0; t < T; t++)
            for (size_t j = 0; j < P; j++) {
                r.post_mean(t, j) = pm[(b * T + t) * P + j];
                r.alpha(t, j) = cf[(b * T + t) * (A + 1) * P + j];
            }
        r.h.assign(h.begin() + b * T, h.begin() + (b + 1) * T);
        r.rank.assign(rank.begin() + b * T, rank.begin() + (b + 1) * T);
        r.status.assign(status.begin() + b * T, status.begin() + (b + 1) * T);
    }
    return res;
}
// The same ranking followed by weighted posterior quantiles of every target's K rows and, with truth (B x P), the posterior CDF at
// the truth (abc_particle_ranking_pls_targets_summary; method 0 rejection, 1 loclinear with kernel 0 Epanechnikov / 1 rectangular).
// Per target: quant (nq x P, row q = level probs[q]) and cdf (P; empty without truth).
struct TargetSummary {
    Mat2D quant;
    std::vector<double> cdf;
};
inline std::vector<TargetSummary> particle_ranking_PLS_targets_summary(const Mat2D& X, const Mat2D& Y, const Mat2D& targets,
                                                                       const float_type train_frac, size_t K,
                                                                       const std::vector<double>& probs, const Mat2D* truth = nullptr,
                                                                       int method = 0, int kernel = 0) {
    if (!((0 < train_frac) && (train_frac <= 1))) throw HipError(ABC_ERR_INVALID, "training_fraction");
    const size_t B = targets.rows(), P = Y.cols(), M = X.cols(), nq = probs.size();
    if (truth && (truth->rows() != B || truth->cols() != P)) throw HipError(ABC_ERR_INVALID, "truth must be B x P");
    std::vector<double> tr, q(B * nq * P), cdf(truth ? B * P : 0);
    if (truth) {
        tr.resize(B * P);
        for (size_t b = 0; b < B; b++)
            for (size_t j = 0; j < P; j++) tr[b * P + j] = (*truth)(b, j);
    }
    abc_summary sum = {probs.data(), nq, truth ? tr.data() : nullptr, q.data(), truth ? cdf.data() : nullptr};
    check(abc_particle_ranking_pls_targets_summary(context(), X.data(), Y.data(), X.rows(), M, P, targets.data(), B, train_frac,
                                                   max_components_ref(), component_rule(), nullptr, K, method, kernel, nullptr, nullptr,
                                                   nullptr, &sum, nullptr));
    std::vector<TargetSummary> res(B);
    for (size_t b = 0; b < B; b++) {
        res[b].quant = Mat2D(nq, P);
        for (size_t k = 0; k < nq; k++)
            for (size_t j = 0; j < P; j++) res[b].quant(k, j) = q[(b * nq + k) * P + j];
        if (truth) res[b].cdf.assign(cdf.begin() + b * P, cdf.begin() + (b + 1) * P);
    }
    return res;
}
// The tolerance path with the summaries at every tolerance (abc_particle_ranking_pls_targets_path_summary): one ranking at
// K_max = Ks.back(), the path's outputs, and the quantiles and CDF of particle_ranking_PLS_targets_summary at every Ks[t] (bit for
// bit under method 0, from one sort per target and parameter).  Per target: the TargetPath fields, quant (T x nq x P: row t * nq + q
// = level probs[q] at tolerance t) and cdf (T x P; 0 x 0 without truth).
struct TargetPathSummary : TargetPath {
    Mat2D quant, cdf;
};
inline std::vector<TargetPathSummary> particle_ranking_PLS_targets_path_summary(const Mat2D& X, const Mat2D& Y, const Mat2D& targets,
                                                                                const float_type train_frac,
                                                                                const std::vector<size_t>& Ks,
                                                                                const std::vector<double>& probs,
                                                                                const Mat2D* truth = nullptr, int method = 0,
                                                                                int kernel = 0) {
    if (!((0 < train_frac) && (train_frac <= 1))) throw HipError(ABC_ERR_INVALID, "training_fraction");
    const size_t B = targets.rows(), P = Y.cols(), M = X.cols(), T = Ks.size(), K = T ? Ks.back() : 0, nq = probs.size();
    if (truth && (truth->rows() != B || truth->cols() != P)) throw HipError(ABC_ERR_INVALID, "truth must be B x P");
    const int mc = max_components_ref();
    const size_t A = mc > 0 ? (size_t)mc : (M < P ? M : P);
    std::vector<uint64_t> idx(B * K);
    std::vector<double> pm(B * T * P), cf(B * T * (A + 1) * P), h(B * T), tr, q(B * T * nq * P), cdf(truth ? B * T * P : 0);
    std::vector<int32_t> rank(B * T), status(B * T);
    if (truth) {
        tr.resize(B * P);
        for (size_t b = 0; b < B; b++)
            for (size_t j = 0; j < P; j++) tr[b * P + j] = (*truth)(b, j);
    }
    abc_path path = {Ks.data(), T, pm.data(), cf.data(), rank.data(), status.data(), h.data()};
    abc_summary sum = {probs.data(), nq, truth ? tr.data() : nullptr, q.data(), truth ? cdf.data() : nullptr};
    check(abc_particle_ranking_pls_targets_path_summary(context(), X.data(), Y.data(), X.rows(), M, P, targets.data(), B, train_frac, mc,
                                                        component_rule(), nullptr, method, kernel, idx.data(), nullptr, &path, &sum,
                                                        nullptr));
    std::vector<TargetPathSummary> res(B);
    for (size_t b = 0; b < B; b++) {
        TargetPathSummary& r = res[b];
        r.idx.assign(idx.begin() + b * K, idx.begin() + (b + 1) * K);
        r.post_mean = Mat2D(T, P);
        r.alpha = Mat2D(T, P);
        r.quant = Mat2D(T * nq, P);
        if (truth) r.cdf = Mat2D(T, P);
        for (size_t t = 0; t < T; t++)
            for (size_t j = 0; j < P; j++) {
                r.post_mean(t, j) = pm[(b * T + t) * P + j];
                r.alpha(t, j) = cf[(b * T + t) * (A + 1) * P + j];
                if (truth) r.cdf(t, j) = cdf[(b * T + t) * P + j];
                for (size_t k = 0; k < nq; k++) r.quant(t * nq + k, j) = q[((b * T + t) * nq + k) * P + j];
            }
        r.h.assign(h.begin() + b * T, h.begin() + (b + 1) * T);
        r.rank.assign(rank.begin() + b * T, rank.begin() + (b + 1) * T);
        r.status.assign(status.begin() + b * T, status.begin() + (b + 1) * T);
    }
    return res;
}
// Weighted quantiles of every column of values (K x P; weights: K entries, or empty for equal weights, which gives NumPy's
// "hazen" / R's type 5): nq x P, row q = level probs[q] (abc_weighted_summary).
inline Mat2D weighted_quantiles(const Mat2D& values, const std::vector<double>& weights, const std::vector<double>& probs) {
    const size_t K = values.rows(), P = values.cols(), nq = probs.size();
    if (!weights.empty() && weights.size() != K) throw HipError(ABC_ERR_INVALID, "weights needs one entry per row");
    std::vector<double> q(nq * P);
    abc_summary sum = {probs.data(), nq, nullptr, q.data(), nullptr};
    check(abc_weighted_summary(context(), values.data(), K, P, weights.empty() ? nullptr : weights.data(), &sum));
    Mat2D out(nq, P);
    for (size_t k = 0; k < nq; k++)
        for (size_t j = 0; j < P; j++) out(k, j) = q[k * P + j];
    return out;
}
// The same ranking followed by the weighted Gaussian kernel density of every (target, parameter) on G grid points and the mode
// taken from it (abc_particle_ranking_pls_targets_density: R's density() with bw.nrd0; bw_scale is R's adjust).  Per target:
// dens (P x G), lo_x / step / bw / mode / mode_dens (P each); the grid points are x_g = fma(g, step, lo_x).
struct TargetDensity {
    Mat2D dens;
    std::vector<double> lo_x, step, bw, mode, mode_dens;
};
namespace detail {
inline TargetDensity target_density(const double* dens, const double* grid, const double* bw, const double* mode,
                                    const double* mode_dens, size_t P, size_t G) {
    TargetDensity r;
    r.dens = Mat2D(P, G);
    r.lo_x.resize(P);
    r.step.resize(P);
    for (size_t j = 0; j < P; j++) {
        for (size_t g = 0; g < G; g++) r.dens(j, g) = dens[j * G + g];
        r.lo_x[j] = grid[2 * j];
        r.step[j] = grid[2 * j + 1];
    }
    r.bw.assign(bw, bw + P);
    r.mode.assign(mode, mode + P);
    r.mode_dens.assign(mode_dens, mode_dens + P);
    return r;
}
}  // namespace detail
inline std::vector<TargetDensity> particle_ranking_PLS_targets_density(const Mat2D& X, const Mat2D& Y, const Mat2D& targets,
                                                                       const float_type train_frac, size_t K, size_t G = 512,
                                                                       double cut = 3.0, double bw_scale = 1.0, int method = 0,
                                                                       int kernel = 0) {
    if (!((0 < train_frac) && (train_frac <= 1))) throw HipError(ABC_ERR_INVALID, "training_fraction");
    const size_t B = targets.rows(), P = Y.cols(), M = X.cols(), ns = B * P;
    std::vector<double> dens(ns * G), grid(ns * 2), bw(ns), mode(ns), md(ns);
    abc_density den = {G, cut, bw_scale, nullptr, dens.data(), grid.data(), bw.data(), mode.data(), md.data()};
    check(abc_particle_ranking_pls_targets_density(context(), X.data(), Y.data(), X.rows(), M, P, targets.data(), B, train_frac,
                                                   max_components_ref(), component_rule(), nullptr, K, method, kernel, nullptr, nullptr,
                                                   nullptr, &den, nullptr));
    std::vector<TargetDensity> res(B);
    for (size_t b = 0; b < B; b++)
        res[b] = detail::target_density(dens.data() + b * P * G, grid.data() + b * P * 2, bw.data() + b * P, mode.data() + b * P,
                                        md.data() + b * P, P, G);
    return res;
}
// The weighted kernel density and mode of every column of values (K x P; weights: K entries, or empty for equal weights)
// (abc_weighted_density).
inline TargetDensity weighted_density(const Mat2D& values, const std::vector<double>& weights, size_t G = 512, double cut = 3.0,
                                      double bw_scale = 1.0) {
    const size_t K = values.rows(), P = values.cols();
    if (!weights.empty() && weights.size() != K) throw HipError(ABC_ERR_INVALID, "weights needs one entry per row");
    std::vector<double> dens(P * G), grid(P * 2), bw(P), mode(P), md(P);
    abc_density den = {G, cut, bw_scale, nullptr, dens.data(), grid.data(), bw.data(), mode.data(), md.data()};
    check(abc_weighted_density(context(), values.data(), K, P, weights.empty() ? nullptr : weights.data(), &den));
    return detail::target_density(dens.data(), grid.data(), bw.data(), mode.data(), md.data(), P, G);
}
// The same ranking followed by the joint posterior of every target (abc_particle_ranking_pls_targets_joint): weighted means,
// covariance and correlation matrices of the P parameters, and for every pair of parameters (pairs: (i, j) with i != j; empty: all
// i < j) the product-Gaussian kernel density on a G x G grid, dens[p](g, g') with g along parameter i, and its mode.  Per
// target: mean / lo_x / step / bw (P each), cov and corr (P x P), dens (one G x G matrix per pair), mode_x / mode_y / mode_dens
// (one per pair).  The densities take B * npairs * G * G doubles on the host and in the context's workspace; with dens = false
// they are neither computed into memory nor returned (TargetJoint::dens stays empty) and the moments and modes are the same bits.
struct TargetJoint {
    std::vector<double> mean, lo_x, step, bw;
    Mat2D cov, corr;
    std::vector<std::pair<int, int>> pairs;
    std::vector<Mat2D> dens;
    std::vector<double> mode_x, mode_y, mode_dens;
};
namespace detail {
struct JointBuffers {
    size_t P, G, np;
    std::vector<int32_t> pairs;
    std::vector<double> mean, cov, corr, dens, grid, bw, mode, md;
    bool with_dens;
    JointBuffers(size_t B, size_t P_, size_t G_, const std::vector<std::pair<int, int>>& given, bool dens_)
        : P(P_), G(G_), with_dens(dens_) {
        for (const auto& p : given) {
            pairs.push_back(p.first);
            pairs.push_back(p.second);
        }
        np = given.empty() ? P * (P - 1) / 2 : given.size();
        mean.resize(B * P); cov.resize(B * P * P); corr.resize(B * P * P);
        if (with_dens) dens.resize(B * np * G * G);
        grid.resize(B * P * 2); bw.resize(B * P); mode.resize(B * np * 2); md.resize(B * np);
    }
    abc_joint arg(double cut, double bw_scale) {
        return {G, cut, bw_scale, nullptr, pairs.empty() ? nullptr : pairs.data(), pairs.size() / 2, mean.data(), cov.data(),
                corr.data(), with_dens ? dens.data() : nullptr, grid.data(), bw.data(), mode.data(), md.data()};
    }
    TargetJoint target(size_t b) const {
        TargetJoint r;
        r.mean.assign(mean.begin() + b * P, mean.begin() + (b + 1) * P);
        r.bw.assign(bw.begin() + b * P, bw.begin() + (b + 1) * P);
        r.lo_x.resize(P);
        r.step.resize(P);
        r.cov = Mat2D(P, P);
        r.corr = Mat2D(P, P);
        for (size_t i = 0; i < P; i++) {
            r.lo_x[i] = grid[(b * P + i) * 2];
            r.step[i] = grid[(b * P + i) * 2 + 1];
            for (size_t j = 0; j < P; j++) {
                r.cov(i, j) = cov[(b * P + i) * P + j];
                r.corr(i, j) = corr[(b * P + i) * P + j];
            }
        }
        if (pairs.empty()) {
            for (size_t i = 0; i < P; i++)
                for (size_t j = i + 1; j < P; j++) r.pairs.emplace_back((int)i, (int)j);
        } else {
            for (size_t p = 0; p < np; p++) r.pairs.emplace_back(pairs[2 * p], pairs[2 * p + 1]);
        }
        for (size_t p = 0; p < np; p++) {
            if (with_dens) {
                const double* f = dens.data() + (b * np + p) * G * G;
                Mat2D d(G, G);
                for (size_t g = 0; g < G; g++)
                    for (size_t g2 = 0; g2 < G; g2++) d(g, g2) = f[g * G + g2];
                r.dens.push_back(d);
            }
            r.mode_x.push_back(mode[(b * np + p) * 2]);
            r.mode_y.push_back(mode[(b * np + p) * 2 + 1]);
            r.mode_dens.push_back(md[b * np + p]);
        }
        return r;
    }
};
}  // namespace detail
inline std::vector<TargetJoint> particle_ranking_PLS_targets_joint(const Mat2D& X, const Mat2D& Y, const Mat2D& targets,
                                                                   const float_type train_frac, size_t K, size_t G = 64,
                                                                   const std::vector<std::pair<int, int>>& pairs = {},
                                                                   double cut = 3.0, double bw_scale = 1.0, int method = 0,
                                                                   int kernel = 0, bool dens = true) {
    if (!((0 < train_frac) && (train_frac <= 1))) throw HipError(ABC_ERR_INVALID, "training_fraction");
    const size_t B = targets.rows(), P = Y.cols(), M = X.cols();
    detail::JointBuffers buf(B, P, G, pairs, dens);
    abc_joint jt = buf.arg(cut, bw_scale);
    check(abc_particle_ranking_pls_targets_joint(context(), X.data(), Y.data(), X.rows(), M, P, targets.data(), B, train_frac,
                                                 max_components_ref(), component_rule(), nullptr, K, method, kernel, nullptr, nullptr,
                                                 nullptr, &jt, nullptr));
    std::vector<TargetJoint> res;
    for (size_t b = 0; b < B; b++) res.push_back(buf.target(b));
    return res;
}
// The joint posterior of the columns of values (K x P; weights: K entries, or empty for equal weights) (abc_weighted_joint).
inline TargetJoint weighted_joint(const Mat2D& values, const std::vector<double>& weights, size_t G = 64,
                                  const std::vector<std::pair<int, int>>& pairs = {}, double cut = 3.0, double bw_scale = 1.0,
                                  bool dens = true) {
    const size_t K = values.rows(), P = values.cols();
    if (!weights.empty() && weights.size() != K) throw HipError(ABC_ERR_INVALID, "weights needs one entry per row");
    detail::JointBuffers buf(1, P, G, pairs, dens);
    abc_joint jt = buf.arg(cut, bw_scale);
    check(abc_weighted_joint(context(), values.data(), K, P, weights.empty() ? nullptr : weights.data(), &jt));
    return buf.target(0);
}
// The same ranking followed by S posterior draws of every target, made on the device (abc_particle_ranking_pls_targets_draws): rows
// of the target's K retained rows resampled with their weights, as they are (smooth = false, the weighted bootstrap) or with h_j z_j
// added to parameter j (smooth = true, the smoothed bootstrap with the marginal densities' bandwidths).  seed keys the Philox stream
// of the draws (no RNG object is advanced); target b takes stream id b.  Nothing is clipped to prior bounds.  Per target: draws
// (S x P), src (S: the position in 0..K-1 of the row a draw came from), bw (P; NaN without smoothing) and ess = W^2 / sum w^2.
struct TargetDraws {
    Mat2D draws;
    std::vector<size_t> src;
    std::vector<double> bw;
    double ess;
};
namespace detail {
inline TargetDraws target_draws(const double* draws, const uint64_t* src, const double* bw, double ess, size_t S, size_t P) {
    TargetDraws r;
    r.draws = Mat2D(S, P);
    for (size_t s = 0; s < S; s++)
        for (size_t j = 0; j < P; j++) r.draws(s, j) = draws[s * P + j];
    r.src.assign(src, src + S);
    r.bw.assign(bw, bw + P);
    r.ess = ess;
    return r;
}
}  // namespace detail
inline std::vector<TargetDraws> particle_ranking_PLS_targets_draws(const Mat2D& X, const Mat2D& Y, const Mat2D& targets,
                                                                   const float_type train_frac, size_t K, size_t S,
                                                                   bool smooth = false, uint64_t seed = 0, int method = 0,
                                                                   int kernel = 0, double bw_scale = 1.0) {
    if (!((0 < train_frac) && (train_frac <= 1))) throw HipError(ABC_ERR_INVALID, "training_fraction");
    const size_t B = targets.rows(), P = Y.cols(), M = X.cols();
    std::vector<double> draws(B * S * P), bw(B * P), ess(B);
    std::vector<uint64_t> src(B * S);
    abc_draws dr = {S, smooth ? 1 : 0, bw_scale, nullptr, seed, nullptr, draws.data(), src.data(), bw.data(), ess.data()};
    check(abc_particle_ranking_pls_targets_draws(context(), X.data(), Y.data(), X.rows(), M, P, targets.data(), B, train_frac,
                                                 max_components_ref(), component_rule(), nullptr, K, method, kernel, nullptr, nullptr,
                                                 nullptr, &dr, nullptr));
    std::vector<TargetDraws> res(B);
    for (size_t b = 0; b < B; b++)
        res[b] = detail::target_draws(draws.data() + b * S * P, src.data() + b * S, bw.data() + b * P, ess[b], S, P);
    return res;
}
// S draws of the rows of values (K x P; weights: K entries, or empty for equal weights) (abc_weighted_draws); stream id 0.
inline TargetDraws weighted_draws(const Mat2D& values, const std::vector<double>& weights, size_t S, bool smooth = false,
                                  uint64_t seed = 0, double bw_scale = 1.0) {
    const size_t K = values.rows(), P = values.cols();
    if (!weights.empty() && weights.size() != K) throw HipError(ABC_ERR_INVALID, "weights needs one entry per row");
    std::vector<double> draws(S * P), bw(P);
    std::vector<uint64_t> src(S);
    double ess = 0.0;
    abc_draws dr = {S, smooth ? 1 : 0, bw_scale, nullptr, seed, nullptr, draws.data(), src.data(), bw.data(), &ess};
    check(abc_weighted_draws(context(), values.data(), K, P, weights.empty() ? nullptr : weights.data(), &dr));
    return detail::target_draws(draws.data(), src.data(), bw.data(), ess, S, P);
}
// The same ranking followed by the k-nearest-neighbour entropy of every target's posterior in all P parameters at once
// (abc_particle_ranking_pls_targets_entropy; the definition is in the header): the lower, the more concentrated.  k: 1..8; scale:
// empty, or P positive values the parameters are divided by.  The estimate is for entries of equal weight: method 1 needs the
// rectangular kernel (1, the default here).  Per target: H (NaN when K <= k or a value is not finite, -inf when zeros > 0), knn
// (K: each entry's distance to its k-th nearest neighbour) and zeros (entries with k or more exact duplicates).
struct TargetEntropy {
    double H;
    std::vector<double> knn;
    size_t zeros;
};
inline std::vector<TargetEntropy> particle_ranking_PLS_targets_entropy(const Mat2D& X, const Mat2D& Y, const Mat2D& targets,
                                                                       const float_type train_frac, size_t K, int k = 4,
                                                                       const std::vector<double>& scale = {}, int method = 0,
                                                                       int kernel = 1) {
    if (!((0 < train_frac) && (train_frac <= 1))) throw HipError(ABC_ERR_INVALID, "training_fraction");
    const size_t B = targets.rows(), P = Y.cols(), M = X.cols();
    if (!scale.empty() && scale.size() != P) throw HipError(ABC_ERR_INVALID, "scale needs one entry per parameter");
    std::vector<double> H(B), knn(B * K);
    std::vector<uint64_t> zeros(B);
    abc_entropy en = {k, scale.empty() ? nullptr : scale.data(), H.data(), knn.data(), zeros.data()};
    check(abc_particle_ranking_pls_targets_entropy(context(), X.data(), Y.data(), X.rows(), M, P, targets.data(), B, train_frac,
                                                   max_components_ref(), component_rule(), nullptr, K, method, kernel, nullptr,
                                                   nullptr, nullptr, &en, nullptr));
    std::vector<TargetEntropy> res(B);
    for (size_t b = 0; b < B; b++)
        res[b] = TargetEntropy{H[b], std::vector<double>(knn.begin() + b * K, knn.begin() + (b + 1) * K), (size_t)zeros[b]};
    return res;
}
// The k-nearest-neighbour entropy of the rows of values (K x P) as one unweighted sample (abc_weighted_entropy).
inline TargetEntropy knn_entropy(const Mat2D& values, int k = 4, const std::vector<double>& scale = {}) {
    const size_t K = values.rows(), P = values.cols();
    if (!scale.empty() && scale.size() != P) throw HipError(ABC_ERR_INVALID, "scale needs one entry per parameter");
    TargetEntropy r{0.0, std::vector<double>(K), 0};
    uint64_t zeros = 0;
    abc_entropy en = {k, scale.empty() ? nullptr : scale.data(), &r.H, r.knn.data(), &zeros};
    check(abc_weighted_entropy(context(), values.data(), K, P, nullptr, &en));
    r.zeros = (size_t)zeros;
    return r;
}
// The same ranking followed by the highest-density interval of every target's posterior in every parameter: the shortest interval
// that holds each mass (abc_particle_ranking_pls_targets_hpd; the definition is in the header; method and kernel as
// particle_ranking_PLS_targets_summary).  Per target: lo, hi (nm x P, row m = mass[m]) and the probabilities plo, phi of the two
// ends, so that (lo, hi) are the summary's quantiles at (plo, phi).
struct TargetHpd {
    Mat2D lo, hi, plo, phi;
};
namespace detail {
inline TargetHpd target_hpd(const double* lo, const double* hi, const double* plo, const double* phi, size_t nm, size_t P) {
    TargetHpd r{Mat2D(nm, P), Mat2D(nm, P), Mat2D(nm, P), Mat2D(nm, P)};
    for (size_t k = 0; k < nm; k++)
        for (size_t j = 0; j < P; j++) {
            r.lo(k, j) = lo[k * P + j];
            r.hi(k, j) = hi[k * P + j];
            r.plo(k, j) = plo[k * P + j];
            r.phi(k, j) = phi[k * P + j];
        }
    return r;
}
}  // namespace detail
inline std::vector<TargetHpd> particle_ranking_PLS_targets_hpd(const Mat2D& X, const Mat2D& Y, const Mat2D& targets,
                                                               const float_type train_frac, size_t K,
                                                               const std::vector<double>& mass = {0.5, 0.95}, int method = 0,
                                                               int kernel = 0) {
    if (!((0 < train_frac) && (train_frac <= 1))) throw HipError(ABC_ERR_INVALID, "training_fraction");
    const size_t B = targets.rows(), P = Y.cols(), M = X.cols(), nm = mass.size(), n = B * nm * P;
    std::vector<double> lo(n), hi(n), plo(n), phi(n);
    abc_hpd hd = {mass.data(), nm, lo.data(), hi.data(), plo.data(), phi.data()};
    check(abc_particle_ranking_pls_targets_hpd(context(), X.data(), Y.data(), X.rows(), M, P, targets.data(), B, train_frac,
                                               max_components_ref(), component_rule(), nullptr, K, method, kernel, nullptr, nullptr,
                                               nullptr, &hd, nullptr));
    std::vector<TargetHpd> res(B);
    for (size_t b = 0; b < B; b++)
        res[b] = detail::target_hpd(lo.data() + b * nm * P, hi.data() + b * nm * P, plo.data() + b * nm * P, phi.data() + b * nm * P,
                                    nm, P);
    return res;
}
// The highest-density intervals of every column of values (K x P) with the given weights (empty: equal) (abc_weighted_hpd).
inline TargetHpd weighted_hpd(const Mat2D& values, const std::vector<double>& weights = {}, const std::vector<double>& mass = {0.95}) {
    const size_t K = values.rows(), P = values.cols(), nm = mass.size(), n = nm * P;
    if (!weights.empty() && weights.size() != K) throw HipError(ABC_ERR_INVALID, "weights needs one entry per row");
    std::vector<double> lo(n), hi(n), plo(n), phi(n);
    abc_hpd hd = {mass.data(), nm, lo.data(), hi.data(), plo.data(), phi.data()};
    check(abc_weighted_hpd(context(), values.data(), K, P, weights.empty() ? nullptr : weights.data(), &hd));
    return detail::target_hpd(lo.data(), hi.data(), plo.data(), phi.data(), nm, P);
}
// The same ranking followed by the ABC-GLM posterior of every target (abc_glm_particle_ranking_pls_targets; Leuenberger & Wegmann
// 2010; the definition is in the header).  Per target: mean, var, mode, mode_dens, lo_x, step (P), dens (P x G, row j at
// x_g = fma(g, step[j], lo_x[j])), ess, log_md (the evidence) and status (0: fitted; otherwise everything else is NaN).
struct TargetGlm {
    Row mean, var, mode, mode_dens, lo_x, step;
    Mat2D dens;
    double ess, log_md;
    int32_t status;
};
namespace detail {
struct GlmBuffers {
    size_t P, G;
    std::vector<double> mean, var, mode, mode_dens, lo_x, step, dens, ess, log_md;
    std::vector<int32_t> status;
    GlmBuffers(size_t B, size_t P_, size_t G_)
        : P(P_), G(G_), mean(B * P_), var(B * P_), mode(B * P_), mode_dens(B * P_), lo_x(B * P_), step(B * P_), dens(B * P_ * G_),
          ess(B), log_md(B), status(B) {}
    abc_glm descriptor(double cut, double bw_scale) {
        abc_glm g = {};
        g.G = G; g.cut = cut; g.bw_scale = bw_scale;
        g.dens = dens.data(); g.lo_x = lo_x.data(); g.step = step.data(); g.mode = mode.data(); g.mode_dens = mode_dens.data();
        g.mean = mean.data(); g.var = var.data(); g.ess = ess.data(); g.log_md = log_md.data(); g.status = status.data();
        return g;
    }
    TargetGlm target(size_t b) const {
        TargetGlm r{Row(P), Row(P), Row(P), Row(P), Row(P), Row(P), Mat2D(P, G), ess[b], log_md[b], status[b]};
        for (size_t j = 0; j < P; j++) {
            r.mean[j] = mean[b * P + j]; r.var[j] = var[b * P + j]; r.mode[j] = mode[b * P + j];
            r.mode_dens[j] = mode_dens[b * P + j]; r.lo_x[j] = lo_x[b * P + j]; r.step[j] = step[b * P + j];
            for (size_t g = 0; g < G; g++) r.dens(j, g) = dens[(b * P + j) * G + g];
        }
        return r;
    }
};
}  // namespace detail
inline std::vector<TargetGlm> particle_ranking_PLS_targets_glm(const Mat2D& X, const Mat2D& Y, const Mat2D& targets,
                                                               const float_type train_frac, size_t K, size_t G = 512,
                                                               double cut = 3.0, double bw_scale = 1.0) {
    if (!((0 < train_frac) && (train_frac <= 1))) throw HipError(ABC_ERR_INVALID, "training_fraction");
    const size_t B = targets.rows(), P = Y.cols(), M = X.cols();
    detail::GlmBuffers buf(B, P, G);
    const abc_glm g = buf.descriptor(cut, bw_scale);
    check(abc_glm_particle_ranking_pls_targets(&g, context(), X.data(), Y.data(), X.rows(), M, P, targets.data(), B, train_frac,
                                               max_components_ref(), component_rule(), nullptr, K, nullptr, nullptr, nullptr));
    std::vector<TargetGlm> res(B);
    for (size_t b = 0; b < B; b++) res[b] = buf.target(b);
    return res;
}
// The ABC-GLM posterior of any retained sample: theta (K x P), stats (K x n), obs (n), weights (empty: equal) (abc_glm_weighted).
inline TargetGlm weighted_glm(const Mat2D& theta, const Mat2D& stats, const Row& obs, const std::vector<double>& weights = {},
                              size_t G = 512, double cut = 3.0, double bw_scale = 1.0) {
    const size_t K = theta.rows(), P = theta.cols(), n = stats.cols();
    if (stats.rows() != K || obs.size() != n) throw HipError(ABC_ERR_INVALID, "stats needs one row per row of theta, obs one entry per statistic");
    if (!weights.empty() && weights.size() != K) throw HipError(ABC_ERR_INVALID, "weights needs one entry per row");
    detail::GlmBuffers buf(1, P, G);
    const abc_glm g = buf.descriptor(cut, bw_scale);
    check(abc_glm_weighted(&g, context(), theta.data(), stats.data(), K, P, n, obs.data(), weights.empty() ? nullptr : weights.data()));
    return buf.target(0);
}
// The same two with the exact quantiles of the marginal mixtures at the levels probs (each strictly inside (0, 1)) and their CDF at a
// truth (abc_glm_particle_ranking_pls_targets_summary, abc_glm_weighted_summary): quant (nq x P), cdf (P; empty without a truth).
// truth: one row per target (B x P), or no rows; the generic form takes one row or an empty one.
struct TargetGlmSummary {
    TargetGlm glm;
    Mat2D quant;
    Row cdf;
};
namespace detail {
inline TargetGlmSummary glm_summary_target(const GlmBuffers& buf, size_t b, const std::vector<double>& quant, const std::vector<double>& cdf,
                                           size_t nq) {
    TargetGlmSummary r{buf.target(b), Mat2D(nq, buf.P), Row(cdf.empty() ? 0 : buf.P)};
    for (size_t q = 0; q < nq; q++)
        for (size_t j = 0; j < buf.P; j++) r.quant(q, j) = quant[(b * nq + q) * buf.P + j];
    for (size_t j = 0; j < r.cdf.size(); j++) r.cdf[j] = cdf[b * buf.P + j];
    return r;
}
}  // namespace detail
inline std::vector<TargetGlmSummary> particle_ranking_PLS_targets_glm_summary(const Mat2D& X, const Mat2D& Y, const Mat2D& targets,
                                                                              const float_type train_frac, size_t K,
                                                                              const std::vector<double>& probs, const Mat2D& truth = Mat2D(0, 0),
                                                                              size_t G = 512, double cut = 3.0, double bw_scale = 1.0) {
    if (!((0 < train_frac) && (train_frac <= 1))) throw HipError(ABC_ERR_INVALID, "training_fraction");
    const size_t B = targets.rows(), P = Y.cols(), M = X.cols(), nq = probs.size();
    const bool tr = truth.rows() != 0;
    if (tr && (truth.rows() != B || truth.cols() != P)) throw HipError(ABC_ERR_INVALID, "truth needs one row of P values per target");
    detail::GlmBuffers buf(B, P, G);
    const abc_glm g = buf.descriptor(cut, bw_scale);
    std::vector<double> tv(tr ? B * P : 0), quant(B * nq * P), cdf(tr ? B * P : 0);
    for (size_t b = 0; tr && b < B; b++)
        for (size_t j = 0; j < P; j++) tv[b * P + j] = truth(b, j);
    const abc_summary sm = {probs.data(), nq, tr ? tv.data() : nullptr, nq ? quant.data() : nullptr, tr ? cdf.data() : nullptr};
    check(abc_glm_particle_ranking_pls_targets_summary(&g, &sm, context(), X.data(), Y.data(), X.rows(), M, P, targets.data(), B, train_frac,
                                                       max_components_ref(), component_rule(), nullptr, K, nullptr, nullptr, nullptr));
    std::vector<TargetGlmSummary> res;
    for (size_t b = 0; b < B; b++) res.push_back(detail::glm_summary_target(buf, b, quant, cdf, nq));
    return res;
}
inline TargetGlmSummary weighted_glm_summary(const Mat2D& theta, const Mat2D& stats, const Row& obs, const std::vector<double>& probs,
                                             const Row& truth = Row(0), const std::vector<double>& weights = {}, size_t G = 512,
                                             double cut = 3.0, double bw_scale = 1.0) {
    const size_t K = theta.rows(), P = theta.cols(), n = stats.cols(), nq = probs.size();
    if (stats.rows() != K || obs.size() != n) throw HipError(ABC_ERR_INVALID, "stats needs one row per row of theta, obs one entry per statistic");
    if (!weights.empty() && weights.size() != K) throw HipError(ABC_ERR_INVALID, "weights needs one entry per row");
    const bool tr = truth.size() != 0;
    if (tr && truth.size() != P) throw HipError(ABC_ERR_INVALID, "truth needs one value per parameter");
    detail::GlmBuffers buf(1, P, G);
    const abc_glm g = buf.descriptor(cut, bw_scale);
    std::vector<double> quant(nq * P), cdf(tr ? P : 0);
    const abc_summary sm = {probs.data(), nq, tr ? truth.data() : nullptr, nq ? quant.data() : nullptr, tr ? cdf.data() : nullptr};
    check(abc_glm_weighted_summary(&g, &sm, context(), theta.data(), stats.data(), K, P, n, obs.data(),
                                   weights.empty() ? nullptr : weights.data()));
    return detail::glm_summary_target(buf, 0, quant, cdf, nq);
}
inline std::vector<size_t> particle_ranking_simple(const Mat2D& X_orig, const Mat2D& /* Y_orig */,
                                                   const Row& target_values) {
    const size_t N = X_orig.rows();
    std::vector<uint64_t> idx(N);
    check(abc_particle_ranking_simple(context(), X_orig.data(), target_values.data(), N, X_orig.cols(), N, idx.data(),
                                      nullptr));
    return std::vector<size_t>(idx.begin(), idx.end());
}

// ---- AbcUtil.h:155-170 ----------------------------------------------------------------------------------
inline Row calculate_doubled_variance(const Mat2D& params) {
    Row dv(params.cols());
    check(abc_calculate_doubled_variance(context(), params.data(), params.rows(), params.cols(), dv.data()));
    return dv;
}
inline Row weight_predictive_prior(const std::vector<const Parameter*>& /* mpars */, const Mat2D& params) {
    Row w(params.rows());
    check(abc_weight_predictive_prior_uniform(context(), params.rows(), w.data()));
    return w;
}
inline Row weight_predictive_prior(const std::vector<const Parameter*>& mpars, const Mat2D& params,
                                   const Mat2D& prev_params, const Row& prev_weights,
                                   const Row& prev_doubled_variance) {
    Row w(params.rows());
    const std::vector<abc_prior> pr = to_pod(mpars);
    check(abc_weight_predictive_prior(context(), pr.data(), params.data(), params.rows(), params.cols(),
                                      prev_params.data(), prev_params.rows(), prev_weights.data(),
                                      prev_doubled_variance.data(), w.data()));
    return w;
}

// ---- AbcUtil.h:78, 110-137 ------------------------------------------------------------------------------
// setup_mvn_sampler returns an owning gsl_matrix* in the reference (freed by the caller, AbcSmc.cpp:492,502);
// here a value: P x P, lower triangle + diagonal = L.
inline Mat2D setup_mvn_sampler(const Mat2D& params) {
    Mat2D L(params.cols(), params.cols());
    check(abc_setup_mvn_sampler(context(), params.data(), params.rows(), params.cols(), L.data()));
    return L;
}
inline std::vector<size_t> gsl_rng_nonuniform_int(const RNG* rng, const size_t num_samples, const Col& weights) {
    std::vector<uint64_t> idx(num_samples);
    check(abc_sample_posterior(context(), &rng->state, weights.data(), weights.size(), num_samples, idx.data()));
    return std::vector<size_t>(idx.begin(), idx.end());
}
inline Mat2D sample_posterior(const RNG* rng, const size_t num_samples, const Col& weights, const Mat2D& posterior) {
    const std::vector<size_t> rows = gsl_rng_nonuniform_int(rng, num_samples, weights);
    Mat2D out(num_samples, posterior.cols());
    for (size_t j = 0; j < posterior.cols(); j++)
        for (size_t i = 0; i < num_samples; i++) out(i, j) = posterior(rows[i], j);
    return out;
}
// `seeds` (optional, not in the reference signature): the per-particle simulator seeds AbcSmc.cpp:535 draws with
// gsl_rng_get after the proposals; when asked for they are produced by the same call and the stream advances
// past them (DESIGN.md "Declared deviations": the Gaussian noise does not consume the taus2 stream).
inline Mat2D sample_mvn_predictive_priors(const RNG* rng, const size_t num_samples, const Col& weights,
                                          const Mat2D& parameter_prior, const std::vector<const Parameter*>& pars,
                                          const Mat2D& L, std::vector<unsigned long>* seeds = nullptr) {
    Mat2D out(num_samples, parameter_prior.cols());
    const std::vector<abc_prior> pr = to_pod(pars);
    std::vector<uint64_t> sd(seeds ? num_samples : 0);
    check(abc_sample_mvn_predictive_priors(context(), &rng->state, num_samples, weights.data(), parameter_prior.data(),
                                           parameter_prior.rows(), parameter_prior.cols(), pr.data(), L.data(),
                                           out.data(), nullptr, seeds ? sd.data() : nullptr));
    if (seeds) seeds->assign(sd.begin(), sd.end());
    return out;
}
inline Mat2D sample_predictive_priors(const RNG* rng, const size_t num_samples, const Col& weights,
                                      const Mat2D& parameter_prior, const std::vector<const Parameter*>& pars,
                                      const Row& doubled_variance, std::vector<unsigned long>* seeds = nullptr) {
    Mat2D out(num_samples, parameter_prior.cols());
    const std::vector<abc_prior> pr = to_pod(pars);
    std::vector<uint64_t> sd(seeds ? num_samples : 0);
    check(abc_sample_predictive_priors(context(), &rng->state, num_samples, weights.data(), parameter_prior.data(),
                                       parameter_prior.rows(), parameter_prior.cols(), pr.data(),
                                       doubled_variance.data(), out.data(), nullptr, seeds ? sd.data() : nullptr));
    if (seeds) seeds->assign(sd.begin(), sd.end());
    return out;
}

// ---- AbcUtil.h:80-91: the per-row samplers behind sample_predictive_priors / sample_mvn_predictive_priors ------------------------
// The reference only calls them from those two (AbcUtil.cpp:386, 401); a drop-in header carries every declaration of
// AbcUtil.h:78-172, so here they are, with the reference's semantics on the reference's stream: ONE row from the shared taus2
// stream on the host (the device path draws whole sets: abc_sample_*).  Bit for bit the oracle's rows (tests/test_gpu_parity.py).
// AbcUtil.cpp:145-158: per coordinate Parameter::noise (<= 1000 tries, then the prior's mean)
inline Row gsl_ran_trunc_normal(const RNG* rng, const std::vector<const Parameter*> _model_pars, const Row& mu,
                                const Row& sigma_squared) {
    Row res(sigma_squared.size(), 0.0);
    for (size_t parIdx = 0; parIdx < sigma_squared.size(); parIdx++)
        res[parIdx] = _model_pars[parIdx]->noise(rng, mu[parIdx], std::sqrt(sigma_squared[parIdx]));
    return res;
}
// AbcUtil.cpp:122-143: x = mu + L z (z iid N(0,1) in coordinate order: gsl_ran_multivariate_gaussian), every coordinate recast,
// the whole draw again unless all are valid.  L: P x P, the lower triangle + diagonal of setup_mvn_sampler's factor.  The
// reference retries without bound; here ABC_MVN_MAX_TRIES draws, then HipError (the device path falls back to the parent and
// counts it, abc_perturb_giveups)
constexpr size_t ABC_MVN_MAX_TRIES = 16384;
inline Row gsl_ran_trunc_mv_normal(const RNG* rng, const std::vector<const Parameter*> _model_pars, const Row& mu, const Mat2D& L) {
    const size_t npar = _model_pars.size();
    Row par_values(npar, 0.0), z(npar, 0.0);
    for (size_t tries = 0; tries < ABC_MVN_MAX_TRIES; tries++) {
        bool success = true;
        for (size_t i = 0; i < npar; i++) z[i] = ran_gaussian(rng, 1.0);                     // gsl_ran_ugaussian
        for (size_t parIdx = 0; success && (parIdx < npar); parIdx++) {
            double x = 0.0;                                                                  // dtrmv, lower, non-unit: row parIdx of L times z
            for (size_t k = 0; k <= parIdx; k++) x += L(parIdx, k) * z[k];
            par_values[parIdx] = _model_pars[parIdx]->recast(x + mu[parIdx]);
            success = _model_pars[parIdx]->valid(par_values[parIdx]);
        }
        if (success) return par_values;
    }
    throw HipError(ABC_ERR_INVALID, "gsl_ran_trunc_mv_normal: no valid draw in 16384 tries");
}

// AbcUtil.cpp:320-324 (host helper kept for completeness; the device fuses it into the projection)
inline Col euclidean(const Mat2D& sims, const Row& ref) {
    Col d(sims.rows());
    for (size_t i = 0; i < sims.rows(); i++) {
        double s = 0;
        for (size_t k = 0; k < sims.cols(); k++) { const double t = sims(i, k) - ref[k]; s = std::fma(t, t, s); }
        d[i] = std::sqrt(s);
    }
    return d;
}

// ---- host-side helpers of the shell (one-off or O(K) work; not on the per-generation device path) --------
// AbcUtil.cpp:490-526: set 0 (and projection mode): every non-posterior parameter is sampled in order, then the
// posterior cursor; the posterior columns are filled from the looked-up rows afterwards.
inline Mat2D sample_priors(const RNG* rng, const size_t num_samples, const Mat2D& posterior,
                           const std::vector<const Parameter*>& mpars, std::vector<size_t>& post_ranks) {
    ParRNG par_rng(rng, mpars, posterior.rows());
    Mat2D par_samples(num_samples, mpars.size());
    std::vector<size_t> nonpost, post;
    for (size_t j = 0; j < mpars.size(); j++) (mpars[j]->isPosterior() ? post : nonpost).push_back(j);
    if (post.size() != posterior.cols()) throw std::invalid_argument("sample_priors: posterior columns != POSTERIOR parameters");
    if (!post.empty()) post_ranks.resize(num_samples);
    for (size_t i = 0; i < num_samples; i++) {
        par_rng.unlock();
        for (size_t j : nonpost) par_samples(i, j) = mpars[j]->sample(par_rng);
        if (!post.empty()) post_ranks[i] = (size_t)mpars[post[0]]->sample(par_rng);
    }
    for (size_t c = 0; c < post.size(); c++)
        for (size_t i = 0; i < num_samples; i++) par_samples(i, post[c]) = posterior(post_ranks[i], c);
    return par_samples;
}
inline Mat2D select_rows(const Mat2D& m, const std::vector<size_t>& rows) {     // Eigen's m(rows, all)
    Mat2D out(rows.size(), m.cols());
    for (size_t j = 0; j < m.cols(); j++)
        for (size_t i = 0; i < rows.size(); i++) out(i, j) = m(rows[i], j);
    return out;
}
inline Row col_means(const Mat2D& m) {
    Row mu(m.cols(), 0.0);
    for (size_t j = 0; j < m.cols(); j++) {
        double s = 0;
        for (size_t i = 0; i < m.rows(); i++) s += m(i, j);
        mu[j] = m.rows() ? s / (double)m.rows() : 0.0;
    }
    return mu;
}
inline float_type median(Col data) {                                            // AbcUtil.cpp:46-62
    if (data.empty()) throw std::invalid_argument("median of an empty column");
    std::sort(data.begin(), data.end());
    const size_t n = data.size();
    return (n % 2 == 0) ? (data[n / 2 - 1] + data[n / 2]) / 2 : data[n / 2];
}
inline float_type calculate_nrmse(const Mat2D& posterior_mets, const Row& observed) {   // AbcUtil.cpp:326-345
    const Row sim = col_means(posterior_mets);
    double acc = 0;
    for (size_t i = 0; i < sim.size(); i++) {
        double expected = (std::fabs(observed[i]) + std::fabs(sim[i])) / 2.0;
        if (sim[i] == observed[i]) expected = 1;
        const double d = (sim[i] - observed[i]) / expected;
        acc += d * d;
    }
    return std::sqrt(acc / (double)sim.size());
}
inline float_type logistic(float_type t) { return 1.0 / (1.0 + std::exp(-t)); }

}  // namespace ABC
#endif
