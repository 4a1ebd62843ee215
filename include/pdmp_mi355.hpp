// pdmp_mi355.hpp -- C++17 host-side mirror of the reference's sampler entry points on top of the C ABI (pdmp_mi355.h).
//
// The reference is Julia; its boundary is the method signatures
//     spdmp (∇ϕ, t0, x0, θ0, T, c, F::Union{ZigZag,FactBoomerang}, args...; factor=1.8, adapt=false, adaptscale=false, seed)
//                                                   -> Ξ::FactTrace, (t, x, θ), (acc, num), c      (src/sfact.jl:162-163,211,214)
//     pdmp  (∇ϕ, ...same...)  = spdmp(..., All(), ...)                                              (src/sfact.jl:236)
//     pdmp  (∇ϕ!, t0, x0, θ0, T, c, Flow::Union{BouncyParticle,Boomerang}; adapt, factor=2.0)
//                                                   -> Ξ::PDMPTrace, (t, x, θ), (acc, num), c      (src/not_fact_samplers.jl:117,146)
//     sspdmp(∇ϕ, t0, x0, θ0, T, c, F::ZigZag, κ, args...; reversible, strong_upperbounds, factor=1.5, adapt)
//                                                                                                  (src/ss_fact.jl:159-160,217)
//     stickyzz(u0, target, StickyFlow(F::ZigZag), StickyUpperBounds(G, G1, Γ, c; adapt, strong, multiplier), barriers, EndTime(T))
//                                                   -> Ξ, t′, (t, x, θ), (acc, num)                 (src/stickyzz.jl:176-218)
// Same names, argument order, keyword meaning (struct Options), return shape (struct Result) and error behaviour (the
// reference's `error("Tuning parameter `c` too small.")`, src/sfact.jl:124, becomes std::runtime_error with that text).
// Differences forced by the C ABI: `∇ϕ, args...` is an enumerated target (GaussianTarget, LogisticTarget, DiffusionBridge, PrecisionCholesky); coordinates are
// 0-based; one call runs ONE chain (pass nchains > 1 through pdmp::Ensemble directly for ensembles).
// Header-only; link with -lpdmp_mi355.  There is no CPU fallback: without a gfx950 device every call throws.
#ifndef PDMP_MI355_HPP
#define PDMP_MI355_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <type_traits>
#include <string>
#include <utility>
#include <vector>

#include "pdmp_mi355.h"

namespace pdmp {

struct Error : std::runtime_error {
    pdmp_status code;
    Error(pdmp_status c, const std::string& what) : std::runtime_error(what), code(c) {}
};
inline void check(pdmp_status st) {
    if (st != PDMP_OK) throw Error(st, pdmp_last_error());
}

// SparseMatrixCSC{Float64,Int64}, 0-based (SparseArrays layout, src/common.jl:17-20)
struct SparseCSC {
    int64_t n = 0;
    std::vector<int64_t> colptr, rowval;
    std::vector<double> nzval;
};

// ZigZag(Γ, μ, σ=ones; ρ=0, λref=0)  src/types.jl:19-27
struct ZigZag {
    SparseCSC Gamma;
    std::vector<double> mu, sigma;
    double lambda_ref = 0.0, rho = 0.0;
};
// FactBoomerang(Γ, μ, λ, σ=diag(Γ)^-1/2; ρ=0)  src/types.jl:71-79
struct FactBoomerang {
    SparseCSC Gamma;
    std::vector<double> mu, sigma;
    double lambda_ref = 0.1, rho = 0.0;
};
// BouncyParticle(Γ, μ, λ, ρ, U, L)  src/types.jl:35-45.  L is the mass factor the reference's short constructor computes as
// cholesky(Symmetric(Γ)).L (:43): LOWER triangular CSC with a stored diagonal; leave it empty (n == 0) only for Γ = I -- the engine refuses a
// general Γ without its factor (PDMP_ERR_UNSUPPORTED) instead of running with a silent L = I.
// BouncyParticle(missing, missing, λ, ρ, U, L) of the speed-recorded driver (src/not_fact_samplers.jl:336-384): Gamma empty (n == 0), L empty
// (identity) or the factor, U empty or the diagonal of a PDiagMat metric ([d] > 0; not together with L).
struct BouncyParticle {
    SparseCSC Gamma;
    std::vector<double> mu;
    double lambda_ref = 1.0, rho = 0.0;
    SparseCSC L;
    std::vector<double> U;
};
// LocalBound(c), src/types.jl:122-124: selects the speed-recorded pdmp below
struct LocalBound {
    double c = 1.0;
};
// Boomerang(Γ, μ, λ; ρ=0)  src/types.jl:59-66: Γ enters through its factor L only (empty: identity)
struct Boomerang {
    std::vector<double> mu;
    double lambda_ref = 1.0, rho = 0.0;
    SparseCSC L;
};
// ∇ϕ(x, i, Γ) = idot(Γ, i, x) [- idot(Γ, i, μ)]  (scripts/gaussianrandomfield.jl:25)
struct GaussianTarget {
    SparseCSC Gamma;
    std::vector<double> mu;  // empty: no shift
};
// ∇ϕmoving(t, x, θ, i, t′, F, A, At, μ, y, ny, k), SelfMoving()  (scripts/logistic.jl:78-95,107,167)
struct LogisticTarget {
    int64_t n = 0;  // observations
    SparseCSC A, At;
    std::vector<double> y, ny, mu;
    double gamma0 = 0.01;
    int64_t k_sub = 10;
};
// dϕ, ∇ϕ! of a Bayesian logistic regression for the speed-recorded pdmp (turing/lr.jl:105-139, tilde/lr.jl:55-98):
// ϕ(x) = Σ_i [m_i log(1 + e^{η_i}) − y_i η_i] + (γ0/2)‖x‖², η = A x.  A is n x d (A.n = d columns), At its transpose (At.n = n columns),
// y successes, m trials (empty: ones); pdmp_ensemble_set_target_bps_logistic
struct LogisticRegression {
    int64_t n = 0;  // observations
    SparseCSC A, At;
    std::vector<double> y, m;
    double gamma0 = 0.0;
};
// ∇ϕmoving(t, ξ, θ, i, t′, F, L, T), SelfMoving() (research/diffusion_bridge/faberschauder.jl:128-145, diffbridge.jl:32-33): the bridge of
// dX = b(X) ds + dW on [0, T], b(x) = −βx + α sin(ωx), in the Faber-Schauder basis up to level L: d = (2 << L) + 1 coefficients, the first and
// the last being the fixed end points u/√T and v/√T (θ0 = 0 and c = 0 there).  The flow is ZigZag(I, 0); pdmp_ensemble_set_target_diffusion_bridge
struct DiffusionBridge {
    int32_t L = 7;
    double T = 2.0, alpha = 1.5, beta = 0.1, omega = 6.283185307179586;
    int64_t d() const { return ((int64_t)2 << L) + 1; }
    // dotψ(ξ, s, L, T), faberschauder.jl:16-24: the bridge at time 0 <= s < T of the coefficients ξ
    double path(const std::vector<double>& xi, double s) const {
        const double sT = std::sqrt(T);
        double r = s / sT * xi.back() + sT * (1 - s / T) * xi.front();
        for (int lev = 0; lev <= L; ++lev) {
            const double p2 = (double)((int64_t)1 << (L - lev));
            const int64_t j = (int64_t)std::floor(s / T * p2) * ((int64_t)2 << lev) + ((int64_t)1 << lev);
            r += xi[(size_t)j] * ((sT * 0.5 - std::fabs(std::fmod(s * p2, T) / sT - sT * 0.5)) / std::sqrt(p2));
        }
        return r;
    }
};
// ∇ϕ(u, i, YY, (𝕀, 𝕁), N) of casestudies/precision/precision.jl:42-53 (gamma0 = 0) and research/newsticky/precision/precision4.jl:82-93: N
// observations Y_k ~ N(0, (L Lᵀ)⁻¹) through YY = Σ Y_k Y_kᵀ ([n x n] row-major, symmetric); the d = n(n+1)/2 coordinates are the lower triangle
// of L packed column by column.  For sspdmp with a diagonal ZigZag(Γ̂, μ̂); n <= 64.  pdmp_ensemble_set_target_precision_cholesky
struct PrecisionCholesky {
    int32_t n = 0;
    std::vector<double> YY;
    double N = 1.0, gamma0 = 0.0;
    int64_t d() const { return (int64_t)n * (n + 1) / 2; }
    // transform / backform of the script (:11-18): the coordinate of L[r, c], r >= c (0-based)
    int64_t index(int64_t r, int64_t c) const { return c * n - c * (c - 1) / 2 + (r - c); }
    std::vector<double> unpack(const std::vector<double>& u) const {  // backform(u, 𝕀): L, [n x n] row-major
        std::vector<double> L((size_t)n * (size_t)n, 0.0);
        for (int64_t c = 0; c < n; ++c)
            for (int64_t r = c; r < n; ++r) L[(size_t)(r * n + c)] = u[(size_t)index(r, c)];
        return L;
    }
};

struct Options {  // the reference's keyword arguments
    double factor = 1.8;
    bool adapt = false;
    bool adaptscale = false;
    bool local_bound = false;  // c is LocalBound(c): spdmp(∇ϕ, t0, x0, θ0, T, C::LocalBound, F, args...), src/local.jl:95-149; for the
                               // non-factorised pdmp: src/not_fact_samplers.jl:29-31,65-71
    bool subsample = false;    // pdmp(∇ϕ!, ...; subsample) of the non-factorised samplers, src/not_fact_samplers.jl:53,90
    bool oscn = false;         // pdmp(dϕ, ∇ϕ!, ..., c::LocalBound, flow::BouncyParticle; oscn): the orthogonal-subspace Crank-Nicolson bounce, src/oscn.jl
    bool tracked = false;      // engine-only: tracked-gradient evaluation of spdmp (pdmp_ensemble_set_gradient_tracking), the engine's fast
                               // path (2.5 x the default's rate on C3).  NOT the reference's arithmetic: floats to ~1e-13 instead of bit for
                               // bit; indices / counters / bounds identical until such a difference flips a test -- measured 3 of 4096
                               // chains by T = 20 on the 128 x 128 lattice (6e-10 per proposal).  false: the reference's evaluation order
    uint64_t seed = 0x5EED0000ull;
    int device = 0;
    int64_t trace_capacity = 0;  // 0: sized from d and T, refilled on demand
    // sspdmp only
    bool reversible = false, strong_upperbounds = false;
    // the optional argument G of spdmp(∇ϕ, t0, x0, θ0, T, c, G, F, ...) / sspdmp(..., c, G, F, κ, ...) (src/sfact.jl:162, src/ss_fact.jl:159):
    // column patterns = the G[i] (values unused); empty = Matched().  G ⊇ G1 or the call throws (the reference's @assert, src/sfact.jl:177)
    SparseCSC G;
    // stickyzz only, engine-only: consume every slice of the trace on the device before its buffer is recycled (pdmp_ensemble_barrier_consume_begin)
    // and fill Result::consumed -- mean, the path on the grid t0 + k·consume_dt (consume_points rows reserved; 0: no grid) and the barrier
    // occupation.  The consumers follow the path the chain travelled: a coordinate that starts on the barrier of its θ0 starts with θ = 0
    bool consume = false;
    double consume_dt = 0.0;
    int64_t consume_points = 0;
    bool consume_only = false;  // ... and copy no event to the host: Result::trace.events stays empty (the Python mirror's trace=False)
    // pdmp on a BouncyParticle (event-recorded) or a Boomerang, engine-only: with consume and a pair list -- the Python mirror's
    // consume=dict(cov=(pi, pj), center=c) -- every slice also adds to the exact path integrals S_k = ∫ (x_i − c_i)(x_j − c_j) dt of the pairs
    // (cov_pi[k], cov_pj[k]) and J_i = ∫ (x_i − c_i) dt (pdmp_ensemble_bps_consume_pairs; a Boomerang's pieces are arcs:
    // pdmp_ensemble_bps_consume_arc_pairs), returned in Result::pairs.  cov_center: empty = 0
    std::vector<int64_t> cov_pi, cov_pj;
    std::vector<double> cov_center;
    // ... and with consume and hist_bins > 0 -- the Python mirror's consume=dict(hist=dict(coords=..., lo=..., hi=..., bins=B)) -- every slice also
    // adds to the exact marginal histograms of the path: the time each coordinate of hist_coords (empty: all) spends in each of hist_bins bins
    // of its own range [hist_lo, hist_hi) (one entry per listed coordinate, or one for all), returned in Result::hist
    // (pdmp_ensemble_bps_consume_hist; a Boomerang's pieces are arcs: pdmp_ensemble_bps_consume_arc_hist)
    std::vector<int64_t> hist_coords;
    std::vector<double> hist_lo, hist_hi;
    int64_t hist_bins = 0;
};

// What Options::consume with hist_bins > 0 returns: per listed coordinate s the row H [s * (bins + 2) + k] -- slot 0 the time below lo, slots
// 1..bins the bins, slot bins + 1 the time at or above hi --, the time at rest Z [s], the edges [s * (bins + 1) + k] = e_k as the device computes
// them, and the last event time T.  quantile(s, q): the piecewise-linear CDF of the row inverted at q, as trace.histogram_quantiles in Python
struct Histogram {
    std::vector<int64_t> coords;
    std::vector<double> H, Z, edges;
    int64_t bins = 0;
    double T = 0.0;
    double quantile(size_t s, double q) const {  // (NaN where the requested mass lies in an outer slot, or in a row without mass)
        const double* row = H.data() + s * (size_t)(bins + 2);
        const double* e = edges.data() + s * (size_t)(bins + 1);
        std::vector<double> inner((size_t)bins + 1);  // the CDF at the edges e_0 .. e_bins, summed in slot order
        double acc = 0.0;
        for (int64_t k = 0; k <= bins; ++k) inner[(size_t)k] = acc = acc + row[k];
        const double total = acc + row[bins + 1], mass = q * total;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        if (!(total > 0.0) || !(inner[(size_t)bins] > inner[0]) || !(inner[0] <= mass && mass <= inner[(size_t)bins])) return nan;
        size_t k = 0;
        while (inner[k] < mass) ++k;  // the bin k − 1 with inner[k − 1] < mass <= inner[k]
        return k == 0 ? e[0] : e[k - 1] + (e[k] - e[k - 1]) * ((mass - inner[k - 1]) / (inner[k] - inner[k - 1]));
    }
};

// What Options::consume with a pair list returns: S [npairs] in the order of the list, J [d], and the last event time T; with L = T − t0
// cov_ij = S_ij / L − (J_i / L)(J_j / L) and mean_i = J_i / L + c_i
struct PairIntegrals {
    std::vector<double> S, J;
    double T = 0.0;
};

// What the device consumers of a stickyzz run return (Options::consume): mean(Ξ) [d] and the last event time T; the rows of
// collect(discretize(Ξ, dt)) [npoints x d], row k at t0 + k dt; per coordinate the time it sat frozen on its lower / upper barrier over [t0, T]
// and the hits of each, raw sums (1 − (frozen_lo + frozen_hi) / (T − t0) is sspdmp2's posterior inclusion probability)
struct BarrierConsumed {
    std::vector<double> mean, grid_x, frozen_lo, frozen_hi;
    std::vector<uint64_t> hits_lo, hits_hi;
    double T = 0.0;
    int64_t npoints = 0;
};

// StickyBarriers(x, rule, κ), src/stickyzz.jl:19-25: the lower and the upper barrier of one coordinate -- levels (∓Inf: none on that side), the
// rule each applies to the restored speed at thaw time (PDMP_BARRIER_STICKY keeps it, _REFLECT negates it, _REVERSIBLE flips its sign by a
// coin) and thaw rates κ (+Inf: an instantaneous wall).  Barrier{} is StickyBarriers(): no barrier at all.
struct Barrier {
    double lo = -std::numeric_limits<double>::infinity(), hi = std::numeric_limits<double>::infinity();
    int rule_lo = PDMP_BARRIER_REFLECT, rule_hi = PDMP_BARRIER_REFLECT;
    double kappa_lo = std::numeric_limits<double>::infinity(), kappa_hi = std::numeric_limits<double>::infinity();
};

using Event = pdmp_event;  // (t, i, x, θ), src/trace.jl:38; i 0-based

struct FactTrace {  // FactTrace(F, t0, x0, θ0, events), src/trace.jl:7-13
    double t0 = 0.0;
    std::vector<double> x0, theta0;
    std::vector<Event> events;
};
struct PDMPTrace {  // PDMPTrace(F, t0, x0, θ0, events), src/trace.jl:20-27; events (t, copy(x), copy(θ))
    double t0 = 0.0;
    int64_t d = 0;
    std::vector<double> x0, theta0;
    std::vector<double> t, x, theta;  // [n], [n x d], [n x d]
};

template <class Trace>
struct Result {  // Ξ, (t, x, θ), (acc, num), c
    Trace trace;
    std::vector<double> t, x, theta;  // factorised samplers: t is the vector of per-coordinate clocks (src/sfact.jl:210-211)
    std::vector<int64_t> acc;         // per coordinate (spdmp) or one entry (BPS, sticky: scalar acc)
    int64_t num = 0;
    std::vector<double> c;
    std::vector<double> sigma;  // tuned F.σ when adaptscale (the reference mutates F.σ in place)
    // stickyzz: t′ of the last event, and per coordinate whether it ended frozen (v == 0 && v_old != 0) and its saved speed v_old
    double t_prime = 0.0;
    std::vector<uint8_t> frozen;
    std::vector<double> theta_saved;
    BarrierConsumed consumed;  // stickyzz with Options::consume
    PairIntegrals pairs;       // pdmp on a BouncyParticle / Boomerang with Options::consume and cov_pi, cov_pj
    Histogram hist;            // ... with Options::consume and hist_bins > 0
};

// RAII handle on pdmp_ensemble
class Ensemble {
  public:
    Ensemble(int64_t nchains, int64_t d, int sampler, const Options& o, int64_t trace_capacity) : nchains_(nchains), d_(d) {
        pdmp_config cfg{};
        cfg.struct_size = sizeof cfg;
        cfg.device = o.device;
        cfg.sampler = sampler;
        cfg.adapt = o.adapt ? 1 : 0;
        cfg.factor = o.factor;
        cfg.nchains = nchains;
        cfg.d = d;
        cfg.trace_capacity = trace_capacity;
        check(pdmp_ensemble_create(&cfg, &h_));
    }
    ~Ensemble() {
        if (h_) pdmp_ensemble_destroy(h_);
    }
    Ensemble(const Ensemble&) = delete;
    Ensemble& operator=(const Ensemble&) = delete;
    pdmp_ensemble* get() const { return h_; }
    int64_t nchains() const { return nchains_; }
    int64_t d() const { return d_; }

    // sspdmp(…, Flow::Union{BouncyParticle, Boomerang}, κ; strong_upperbounds) (src/ss_not_fact.jl:182-201): after set_flow_bps /
    // set_flow_boomerang, before set_state_bps; events then carry the free mask (pdmp_ensemble_bps_trace_free_copy)
    void set_bps_sticky(const std::vector<double>& kappa, bool strong_upperbounds = false) {
        if ((int64_t)kappa.size() != d_) throw std::invalid_argument("set_bps_sticky: kappa needs d entries");
        check(pdmp_ensemble_set_bps_sticky(h_, kappa.data(), strong_upperbounds ? 1 : 0));
    }

    // the device trace consumers of a barrier ensemble (stickyzz): after set_state and before the first run; then pdmp_ensemble_consume after
    // every slice.  occupation: [n x d] each, any output may be nullptr
    void barrier_consume_begin(double grid_dt = 0.0, int64_t grid_points = 0) { check(pdmp_ensemble_barrier_consume_begin(h_, grid_dt, grid_points)); }
    void refresh_consume_begin(double grid_dt = 0.0, int64_t grid_points = 0) { check(pdmp_ensemble_refresh_consume_begin(h_, grid_dt, grid_points)); }
    void barrier_consume_occupation(int64_t chain_first, int64_t n, std::vector<double>* frozen_lo, std::vector<double>* frozen_hi,
                                    std::vector<uint64_t>* hits_lo, std::vector<uint64_t>* hits_hi, std::vector<double>* T_last = nullptr) const {
        const size_t nd = (size_t)(n * d_);
        if (frozen_lo) frozen_lo->resize(nd);
        if (frozen_hi) frozen_hi->resize(nd);
        if (hits_lo) hits_lo->resize(nd);
        if (hits_hi) hits_hi->resize(nd);
        if (T_last) T_last->resize((size_t)n);
        check(pdmp_ensemble_barrier_consume_occupation(h_, chain_first, n, frozen_lo ? frozen_lo->data() : nullptr, frozen_hi ? frozen_hi->data() : nullptr,
                                                       hits_lo ? hits_lo->data() : nullptr, hits_hi ? hits_hi->data() : nullptr,
                                                       T_last ? T_last->data() : nullptr));
    }

    std::vector<pdmp_chain_counters> counters() const {
        std::vector<pdmp_chain_counters> c((size_t)nchains_);
        check(pdmp_ensemble_counters(h_, c.data()));
        return c;
    }
    // run to T; drains the trace of chain 0..nchains-1 into `sink(chain, events)` whenever the buffer fills
    template <class Sink>
    std::vector<pdmp_chain_counters> run_and_drain(double T, Sink&& sink) {
        for (;;) {
            check(pdmp_ensemble_run(h_, T, PDMP_RUN_REFERENCE_TAIL, nullptr));
            check(pdmp_ensemble_sync(h_));
            auto cnt = counters();
            for (const auto& k : cnt)
                if (k.status == PDMP_CHAIN_BOUND_VIOLATED) throw std::runtime_error("Tuning parameter `c` too small.");
            sink(cnt);
            bool full = false;
            for (const auto& k : cnt) full = full || k.status == PDMP_CHAIN_TRACE_FULL || k.status == PDMP_CHAIN_PAUSED;  // (both resume with the next run)
            if (!full) return cnt;
        }
    }

  private:
    pdmp_ensemble* h_ = nullptr;
    int64_t nchains_, d_;
};

namespace detail {
inline const double* opt(const std::vector<double>& v) { return v.empty() ? nullptr : v.data(); }
inline int64_t default_capacity(int64_t d, double t0, double T) {
    const double span = std::max(T - t0, 1.0);
    return (int64_t)std::min(std::max(1024.0, 2.0 * (double)d * span), (double)(1 << 22));
}
inline void set_target(Ensemble& e, const GaussianTarget& g) {
    check(pdmp_ensemble_set_target_gaussian_csc(e.get(), g.Gamma.colptr.data(), g.Gamma.rowval.data(), g.Gamma.nzval.data(),
                                                opt(g.mu)));
}
inline void set_target(Ensemble& e, const LogisticTarget& g) {
    check(pdmp_ensemble_set_target_logistic(e.get(), g.n, g.A.colptr.data(), g.A.rowval.data(), g.A.nzval.data(),
                                            g.At.colptr.data(), g.At.rowval.data(), g.At.nzval.data(), g.y.data(), g.ny.data(),
                                            g.mu.data(), g.gamma0, g.k_sub));
}
inline void set_target(Ensemble& e, const LogisticRegression& g) {
    const std::vector<double> ones(g.m.empty() ? (size_t)g.n : 0, 1.0);
    check(pdmp_ensemble_set_target_bps_logistic(e.get(), g.n, g.A.colptr.data(), g.A.rowval.data(), g.A.nzval.data(), g.At.colptr.data(),
                                                g.At.rowval.data(), g.At.nzval.data(), g.y.data(), g.m.empty() ? ones.data() : g.m.data(),
                                                g.gamma0));
}
inline void set_target(Ensemble& e, const DiffusionBridge& g) {
    check(pdmp_ensemble_set_target_diffusion_bridge(e.get(), g.L, g.T, g.alpha, g.beta, g.omega));
}
inline void set_target(Ensemble& e, const PrecisionCholesky& g) {
    if (g.YY.size() != (size_t)g.n * (size_t)g.n) throw std::invalid_argument("PrecisionCholesky: YY must hold n x n entries");
    check(pdmp_ensemble_set_target_precision_cholesky(e.get(), g.n, g.YY.data(), g.N, g.gamma0));
}
inline void set_flow(Ensemble& e, const ZigZag& F) {
    check(pdmp_ensemble_set_flow_zigzag(e.get(), F.Gamma.colptr.data(), F.Gamma.rowval.data(), F.Gamma.nzval.data(), opt(F.mu),
                                        opt(F.sigma), F.lambda_ref, F.rho));
}
inline void set_flow(Ensemble& e, const FactBoomerang& F) {
    check(pdmp_ensemble_set_flow_factboomerang(e.get(), F.Gamma.colptr.data(), F.Gamma.rowval.data(), F.Gamma.nzval.data(),
                                               opt(F.mu), opt(F.sigma), F.lambda_ref, F.rho));
}

template <class Target, class Flow>
Result<FactTrace> factorised(int sampler, const Target& target, double t0, const std::vector<double>& x0,
                             const std::vector<double>& theta0, double T, const std::vector<double>& c, const Flow& F,
                             const std::vector<double>* kappa, const Options& o, const std::vector<Barrier>* barriers = nullptr) {
    const int64_t d = (int64_t)x0.size();
    const int64_t cap = o.trace_capacity > 0 ? o.trace_capacity : default_capacity(d, t0, T);
    Ensemble e(1, d, sampler, o, cap);
    set_flow(e, F);
    if (o.G.n > 0) check(pdmp_ensemble_set_neighbourhood(e.get(), o.G.colptr.data(), o.G.rowval.data()));
    set_target(e, target);
    if (kappa) check(pdmp_ensemble_set_sticky(e.get(), kappa->data(), o.reversible ? 1 : 0, o.strong_upperbounds ? 1 : 0));
    if (barriers) {
        if ((int64_t)barriers->size() != d) throw std::invalid_argument("stickyzz: one Barrier per coordinate");
        std::vector<double> lo, hi, kl, kh;
        std::vector<int32_t> rl, rh;
        for (const Barrier& b : *barriers) {
            lo.push_back(b.lo);
            hi.push_back(b.hi);
            rl.push_back(b.rule_lo);
            rh.push_back(b.rule_hi);
            kl.push_back(b.kappa_lo);
            kh.push_back(b.kappa_hi);
        }
        check(pdmp_ensemble_set_barriers(e.get(), lo.data(), hi.data(), rl.data(), rh.data(), kl.data(), kh.data(), o.strong_upperbounds ? 1 : 0));
    }
    if (o.adaptscale) check(pdmp_ensemble_set_adaptscale(e.get(), 1));
    if (o.local_bound) check(pdmp_ensemble_set_local_bound(e.get(), 1));
    if (o.tracked) check(pdmp_ensemble_set_gradient_tracking(e.get(), 1));
    const uint64_t seed = o.seed;
    check(pdmp_ensemble_set_state(e.get(), t0, x0.data(), theta0.data(), c.data(), &seed));
    const bool consume = o.consume;
    if (consume && !barriers) throw std::invalid_argument("Options::consume is an option of stickyzz");
    if (consume) e.barrier_consume_begin(o.consume_dt, o.consume_points);
    Result<FactTrace> R;
    R.trace.t0 = t0;
    R.trace.x0 = x0;
    R.trace.theta0 = theta0;
    auto cnt = e.run_and_drain(T, [&](const std::vector<pdmp_chain_counters>& k) {
        if (consume) check(pdmp_ensemble_consume(e.get()));  // (every slice, before its buffer is recycled)
        const int64_t m = (int64_t)k[0].ntrace;
        if (m > 0 && !(consume && o.consume_only)) {
            const size_t old = R.trace.events.size();
            R.trace.events.resize(old + (size_t)m);
            check(pdmp_ensemble_trace_copy(e.get(), 0, 0, m, R.trace.events.data() + old));
        }
        check(pdmp_ensemble_trace_reset(e.get()));
    });
    // (the reference would go on to evaluate N/0: the affine bound let a diagonal of L run into 0 -- a tuning failure like `c` too small)
    if (std::is_same<Target, PrecisionCholesky>::value && cnt[0].status == PDMP_CHAIN_STALLED)
        throw std::runtime_error("PrecisionCholesky: the chain stalled: a diagonal coordinate L[c, c] reached 0 (or a coordinate was started at x = 0 "
                                 "with theta = 0); the bound c is too small for the -N/L[c, c] term");
    R.t.resize((size_t)d);
    R.x.resize((size_t)d);
    R.theta.resize((size_t)d);
    R.acc.resize((size_t)d);
    R.c.resize((size_t)d);
    check(pdmp_ensemble_final_state(e.get(), 0, 1, R.t.data(), R.x.data(), R.theta.data(), R.acc.data(), R.c.data()));
    if (!o.adapt) R.c = c;
    if (kappa) R.acc.assign(1, (int64_t)cnt[0].nacc);  // sticky: scalar acc, src/ss_fact.jl:175
    if (barriers) {  // Ξ, t′, u, acc, src/stickyzz.jl:217
        R.acc.assign(1, (int64_t)cnt[0].nacc);
        R.t_prime = cnt[0].t_last;
        R.frozen.resize((size_t)d);
        R.theta_saved.resize((size_t)d);
        check(pdmp_ensemble_final_barrier(e.get(), 0, 1, R.frozen.data(), R.theta_saved.data()));
    }
    if (consume) {
        BarrierConsumed& C = R.consumed;
        C.mean.resize((size_t)d);
        check(pdmp_ensemble_consume_mean(e.get(), 0, 1, C.mean.data(), &C.T));
        e.barrier_consume_occupation(0, 1, &C.frozen_lo, &C.frozen_hi, &C.hits_lo, &C.hits_hi);
        if (o.consume_points > 0) {
            check(pdmp_ensemble_consume_discretized(e.get(), 0, 0, 0, nullptr, &C.npoints, nullptr));
            if (C.npoints > o.consume_points) throw std::runtime_error("stickyzz: the trace runs past the grid of Options::consume_points");
            C.grid_x.resize((size_t)(C.npoints * d));
            check(pdmp_ensemble_consume_discretized(e.get(), 0, 0, C.npoints, C.grid_x.data(), nullptr, nullptr));
        }
    }
    R.num = (int64_t)cnt[0].num;
    if (o.adaptscale) {
        R.sigma.resize((size_t)d);
        check(pdmp_ensemble_final_sigma(e.get(), 0, 1, R.sigma.data()));
    }
    return R;
}

inline Result<PDMPTrace> not_factorised(Ensemble& e, double t0, const std::vector<double>& x0, const std::vector<double>& theta0,
                                        double T, double c, const Options& o, bool arcs = false) {
    const int64_t d = (int64_t)x0.size();
    const uint64_t seed = o.seed;
    check(pdmp_ensemble_set_state_bps(e.get(), t0, x0.data(), theta0.data(), c, &seed));
    const bool pairs = o.consume && !o.cov_pi.empty();
    if (pairs) {
        if (o.cov_pi.size() != o.cov_pj.size()) throw std::invalid_argument("Options::cov_pi and cov_pj have one entry per pair");
        if (!o.cov_center.empty() && (int64_t)o.cov_center.size() != d) throw std::invalid_argument("Options::cov_center needs d entries");
        check(pdmp_ensemble_bps_consume_begin(e.get(), 0.0, 0));
        check((arcs ? pdmp_ensemble_bps_consume_arc_pairs : pdmp_ensemble_bps_consume_pairs)(e.get(), (int64_t)o.cov_pi.size(), o.cov_pi.data(),
                                                                                            o.cov_pj.data(), opt(o.cov_center)));
    }
    const bool hist = o.consume && o.hist_bins > 0;
    Histogram hg;
    if (hist) {
        hg.coords = o.hist_coords;
        if (hg.coords.empty())
            for (int64_t k = 0; k < d; ++k) hg.coords.push_back(k);
        const size_t m = hg.coords.size();
        if ((o.hist_lo.size() != m && o.hist_lo.size() != 1) || (o.hist_hi.size() != m && o.hist_hi.size() != 1))
            throw std::invalid_argument("Options::hist_lo and hist_hi have one entry per listed coordinate, or one for all");
        std::vector<double> lo(m), hi(m);
        for (size_t s = 0; s < m; ++s) {
            lo[s] = o.hist_lo[o.hist_lo.size() == 1 ? 0 : s];
            hi[s] = o.hist_hi[o.hist_hi.size() == 1 ? 0 : s];
        }
        if (!pairs) check(pdmp_ensemble_bps_consume_begin(e.get(), 0.0, 0));
        check((arcs ? pdmp_ensemble_bps_consume_arc_hist : pdmp_ensemble_bps_consume_hist)(e.get(), (int64_t)m, hg.coords.data(), lo.data(), hi.data(),
                                                                                          o.hist_bins));
        hg.bins = o.hist_bins;
        hg.edges.resize(m * (size_t)(o.hist_bins + 1));
        for (size_t s = 0; s < m; ++s) {  // (the contract's edges: e_0 = lo, e_k = lo + w·k, e_bins = hi)
            double* const ed = hg.edges.data() + s * (size_t)(o.hist_bins + 1);
            const double w = (hi[s] - lo[s]) / (double)o.hist_bins;
            for (int64_t k = 0; k <= o.hist_bins; ++k) ed[k] = k == 0 ? lo[s] : (k == o.hist_bins ? hi[s] : lo[s] + w * (double)k);
        }
    }
    Result<PDMPTrace> R;
    R.trace.t0 = t0;
    R.trace.d = d;
    R.trace.x0 = x0;
    R.trace.theta0 = theta0;
    auto cnt = e.run_and_drain(T, [&](const std::vector<pdmp_chain_counters>& k) {
        if (pairs || hist) check(pdmp_ensemble_bps_consume(e.get()));  // (every slice, before its buffer is recycled)
        const int64_t m = (int64_t)k[0].ntrace;
        if (m > 0 && !((pairs || hist) && o.consume_only)) {
            const size_t old = R.trace.t.size();
            R.trace.t.resize(old + (size_t)m);
            R.trace.x.resize((old + (size_t)m) * (size_t)d);
            R.trace.theta.resize((old + (size_t)m) * (size_t)d);
            check(pdmp_ensemble_bps_trace_copy(e.get(), 0, 0, m, R.trace.t.data() + old, R.trace.x.data() + old * (size_t)d,
                                               R.trace.theta.data() + old * (size_t)d));
        }
        check(pdmp_ensemble_trace_reset(e.get()));
    });
    R.t.resize(1);
    R.x.resize((size_t)d);
    R.theta.resize((size_t)d);
    R.c.resize(1);
    check(pdmp_ensemble_bps_final_state(e.get(), 0, 1, R.t.data(), R.x.data(), R.theta.data(), R.c.data()));
    R.acc.assign(1, (int64_t)cnt[0].nacc);
    R.num = (int64_t)cnt[0].num;
    if (pairs) {
        R.pairs.S.resize(o.cov_pi.size());
        R.pairs.J.resize((size_t)d);
        check(pdmp_ensemble_bps_consume_pair_integrals(e.get(), 0, 1, R.pairs.S.data(), R.pairs.J.data(), &R.pairs.T, nullptr));
    }
    if (hist) {
        hg.H.resize(hg.coords.size() * (size_t)(hg.bins + 2));
        hg.Z.resize(hg.coords.size());
        check(pdmp_ensemble_bps_consume_histogram(e.get(), 0, 1, 0, hg.H.data(), hg.Z.data(), &hg.T, nullptr));
        R.hist = std::move(hg);
    }
    return R;
}
}  // namespace detail

// spdmp(∇ϕ, t0, x0, θ0, T, c, F, args...; factor, adapt, adaptscale, seed)  -- src/sfact.jl:162-212,214
template <class Target, class Flow>
Result<FactTrace> spdmp(const Target& target, double t0, const std::vector<double>& x0, const std::vector<double>& theta0,
                        double T, const std::vector<double>& c, const Flow& F, const Options& o = {}) {
    return detail::factorised(PDMP_SAMPLER_ZIGZAG_LOCAL, target, t0, x0, theta0, T, c, F, nullptr, o);
}
// pdmp(∇ϕ, t0, x0, θ0, T, c, F, args...) = spdmp(..., All(), ...)  -- src/sfact.jl:236
template <class Target, class Flow>
Result<FactTrace> pdmp(const Target& target, double t0, const std::vector<double>& x0, const std::vector<double>& theta0,
                       double T, const std::vector<double>& c, const Flow& F, const Options& o = {}) {
    return detail::factorised(PDMP_SAMPLER_ZIGZAG_ALL, target, t0, x0, theta0, T, c, F, nullptr, o);
}
// parallel_spdmp(partition, ∇ϕ, t0, x0, θ0, T, c, G, F::ZigZag; factor, adapt, Δ)  -- src/parallel.jl:104-175: the chain on `nt` wavefronts,
// one per chunk of d / nt coordinates.  F.Gamma is the bounding Γ written on G's pattern (explicit zeros where it has no entry) and g1_mask
// marks its own structural entries (empty: all of them); the result's events are sorted by time (:167), acc holds the scalar of the reference.
template <class Target>
Result<FactTrace> parallel_spdmp(int nt, const Target& target, double t0, const std::vector<double>& x0, const std::vector<double>& theta0,
                                 double T, const std::vector<double>& c, const ZigZag& F, const std::vector<uint8_t>& g1_mask,
                                 double Delta = 0.1, const Options& o = {}) {
    const int64_t d = (int64_t)x0.size();
    const int64_t cap = o.trace_capacity > 0 ? o.trace_capacity : 2 * detail::default_capacity(d, t0, T);
    Ensemble e(1, d, PDMP_SAMPLER_ZIGZAG_LOCAL, o, cap);
    detail::set_flow(e, F);
    detail::set_target(e, target);
    const uint64_t seed = o.seed;
    check(pdmp_ensemble_set_state(e.get(), t0, x0.data(), theta0.data(), c.data(), &seed));
    check(pdmp_ensemble_run_partitioned(e.get(), T, nt, Delta, g1_mask.empty() ? nullptr : g1_mask.data(), (int64_t)g1_mask.size(), nullptr));
    const auto cnt = e.counters();
    if (cnt[0].status == PDMP_CHAIN_BOUND_VIOLATED) throw std::runtime_error("Tuning parameter `c` too small.");
    if (cnt[0].status == PDMP_CHAIN_TRACE_FULL) throw std::runtime_error("trace_capacity too small for a partitioned run (it is not resumable)");
    Result<FactTrace> R;
    R.trace.t0 = t0;
    R.trace.x0 = x0;
    R.trace.theta0 = theta0;
    R.trace.events.resize((size_t)cnt[0].ntrace);
    if (cnt[0].ntrace > 0) check(pdmp_ensemble_trace_copy(e.get(), 0, 0, (int64_t)cnt[0].ntrace, R.trace.events.data()));
    std::stable_sort(R.trace.events.begin(), R.trace.events.end(), [](const pdmp_event& a, const pdmp_event& b) { return a.t < b.t; });
    R.t.resize((size_t)d);
    R.x.resize((size_t)d);
    R.theta.resize((size_t)d);
    R.c.resize((size_t)d);
    std::vector<int64_t> acc_vec((size_t)d);
    check(pdmp_ensemble_final_state(e.get(), 0, 1, R.t.data(), R.x.data(), R.theta.data(), acc_vec.data(), R.c.data()));
    if (!o.adapt) R.c = c;
    R.acc.assign(1, (int64_t)cnt[0].nacc);
    R.num = (int64_t)cnt[0].num;
    return R;
}
// sspdmp(∇ϕ, t0, x0, θ0, T, c, F::ZigZag, κ, args...; reversible, strong_upperbounds, factor=1.5, adapt)  -- src/ss_fact.jl:159-217
template <class Target>
Result<FactTrace> sspdmp(const Target& target, double t0, const std::vector<double>& x0, const std::vector<double>& theta0,
                         double T, const std::vector<double>& c, const ZigZag& F, const std::vector<double>& kappa,
                         Options o = {}) {
    if (o.factor == 1.8) o.factor = 1.5;
    return detail::factorised(PDMP_SAMPLER_STICKY_ZIGZAG, target, t0, x0, theta0, T, c, F, &kappa, o);
}
// stickyzz (src/stickyzz.jl:176-218) in the call shape of the other samplers, G = G1 = the pattern of F.Γ: barriers holds one Barrier per
// coordinate; Options::strong_upperbounds, adapt and factor (multiplier, 1.5) are StickyUpperBounds' keywords.  The result's t_prime, frozen and
// theta_saved are filled; acc is the scalar of AcceptanceDiagnostics.
template <class Target>
Result<FactTrace> stickyzz(const Target& target, double t0, const std::vector<double>& x0, const std::vector<double>& theta0, double T,
                           const std::vector<double>& c, const ZigZag& F, const std::vector<Barrier>& barriers, Options o = {}) {
    if (o.factor == 1.8) o.factor = 1.5;
    return detail::factorised(PDMP_SAMPLER_BARRIER_ZIGZAG, target, t0, x0, theta0, T, c, F, nullptr, o, &barriers);
}
// pdmp(∇ϕ!, t0, x0, θ0, T, c, B::BouncyParticle; adapt, factor=2.0) with ∇ϕ!(y, x) = B.Γ(x − B.μ)  -- src/not_fact_samplers.jl:117-147
inline Result<PDMPTrace> pdmp(double t0, const std::vector<double>& x0, const std::vector<double>& theta0, double T, double c,
                              const BouncyParticle& B, Options o = {}) {
    if (o.factor == 1.8) o.factor = 2.0;
    const int64_t d = (int64_t)x0.size();
    const int64_t cap = o.trace_capacity > 0 ? o.trace_capacity : std::max<int64_t>(256, (int64_t)(64 * std::max(T - t0, 1.0)));
    Ensemble e(1, d, PDMP_SAMPLER_BPS, o, cap);
    check(pdmp_ensemble_set_flow_bps(e.get(), B.Gamma.colptr.data(), B.Gamma.rowval.data(), B.Gamma.nzval.data(),
                                     detail::opt(B.mu), B.lambda_ref, B.rho));
    if (B.L.n > 0) check(pdmp_ensemble_set_mass_cholesky(e.get(), B.L.colptr.data(), B.L.rowval.data(), B.L.nzval.data()));
    if (o.local_bound || o.subsample) check(pdmp_ensemble_set_bps_options(e.get(), o.local_bound ? 1 : 0, o.subsample ? 1 : 0));
    return detail::not_factorised(e, t0, x0, theta0, T, c, o);
}
// pdmp(∇ϕ!, t0, x0, θ0, T, c, B::BouncyParticle; ...) with a target of its own, ∇ϕ!(y, x) = Γt(x − μt): ab(…GlobalBound…) keeps B.Γ, B.μ
// (src/not_fact_samplers.jl:26-28), gradient / rate / reflection use the target's (:122)
inline Result<PDMPTrace> pdmp(const GaussianTarget& target, double t0, const std::vector<double>& x0, const std::vector<double>& theta0,
                              double T, double c, const BouncyParticle& B, Options o = {}) {
    if (o.factor == 1.8) o.factor = 2.0;
    const int64_t d = (int64_t)x0.size();
    const int64_t cap = o.trace_capacity > 0 ? o.trace_capacity : std::max<int64_t>(256, (int64_t)(64 * std::max(T - t0, 1.0)));
    Ensemble e(1, d, PDMP_SAMPLER_BPS, o, cap);
    check(pdmp_ensemble_set_flow_bps(e.get(), B.Gamma.colptr.data(), B.Gamma.rowval.data(), B.Gamma.nzval.data(),
                                     detail::opt(B.mu), B.lambda_ref, B.rho));
    check(pdmp_ensemble_set_target_gaussian_csc(e.get(), target.Gamma.colptr.data(), target.Gamma.rowval.data(),
                                                target.Gamma.nzval.data(), detail::opt(target.mu)));
    if (B.L.n > 0) check(pdmp_ensemble_set_mass_cholesky(e.get(), B.L.colptr.data(), B.L.rowval.data(), B.L.nzval.data()));
    if (o.local_bound || o.subsample) check(pdmp_ensemble_set_bps_options(e.get(), o.local_bound ? 1 : 0, o.subsample ? 1 : 0));
    return detail::not_factorised(e, t0, x0, theta0, T, c, o);
}
// pdmp(∇ϕ!, t0, x0, θ0, T, c, B::Boomerang; ...) with ∇ϕ!(y, x) = Γt(x − μt)  -- test/maintest.jl:139-154
inline Result<PDMPTrace> pdmp(const GaussianTarget& target, double t0, const std::vector<double>& x0,
                              const std::vector<double>& theta0, double T, double c, const Boomerang& B, Options o = {}) {
    if (o.factor == 1.8) o.factor = 2.0;
    const int64_t d = (int64_t)x0.size();
    const int64_t cap = o.trace_capacity > 0 ? o.trace_capacity : std::max<int64_t>(256, (int64_t)(64 * std::max(T - t0, 1.0)));
    Ensemble e(1, d, PDMP_SAMPLER_BPS, o, cap);
    check(pdmp_ensemble_set_flow_boomerang(e.get(), target.Gamma.colptr.data(), target.Gamma.rowval.data(),
                                           target.Gamma.nzval.data(), detail::opt(target.mu), detail::opt(B.mu), B.lambda_ref,
                                           B.rho));
    if (B.L.n > 0) {
        check(pdmp_ensemble_set_mass_cholesky(e.get(), B.L.colptr.data(), B.L.rowval.data(), B.L.nzval.data()));
    } else {  // (an empty L is this struct's "identity": the ABI wants it spelled out for a Boomerang)
        std::vector<int64_t> cp((size_t)d + 1), rv((size_t)d);
        std::vector<double> nz((size_t)d, 1.0);
        for (int64_t k = 0; k < d; ++k) cp[(size_t)k] = rv[(size_t)k] = k;
        cp[(size_t)d] = d;
        check(pdmp_ensemble_set_mass_cholesky(e.get(), cp.data(), rv.data(), nz.data()));
    }
    if (o.subsample) check(pdmp_ensemble_set_bps_options(e.get(), 0, 1));
    return detail::not_factorised(e, t0, x0, theta0, T, c, o, true);  // (the pair list and the histograms of Options::consume take arcs about B.mu)
}

// pdmp(dϕ, ∇ϕ!, t0, x0, θ0, T, c::LocalBound, flow::BouncyParticle; oscn, adapt, factor=2.0)  -- src/not_fact_samplers.jl:336-384, the
// speed-recorded Bouncy Particle: dϕ = (θ'Γt(x−μt), θ'Γtθ) and ∇ϕ! = Γt(x−μt) of the Gaussian target, or those of a LogisticRegression;
// B.Gamma is empty.  The trace holds one record per 1/λref of speed-time and does not begin with (t0, x0, θ0).  T is an end time (the last
// record has t >= T); the overload taking an int64_t is the reference's `T::Int`, a number of samples.
namespace detail {
template <class Target>
inline Result<PDMPTrace> modern(const Target& target, double t0, const std::vector<double>& x0, const std::vector<double>& theta0,
                                double T, int64_t nsamples, LocalBound c, const BouncyParticle& B, Options o) {
    if (o.factor == 1.8) o.factor = 2.0;
    if (B.Gamma.n != 0) throw std::invalid_argument("pdmp(..., c::LocalBound, B): the speed-recorded driver takes BouncyParticle(missing, missing, ...): B.Gamma must be empty");
    const int64_t d = (int64_t)x0.size();
    if (!B.U.empty() && (int64_t)B.U.size() != d) throw std::invalid_argument("BouncyParticle::U needs d entries");
    const int64_t want = nsamples > 0 ? nsamples : (int64_t)(4 * B.lambda_ref * std::max(T - t0, 1.0));
    const int64_t cap = o.trace_capacity > 0 ? o.trace_capacity : std::max<int64_t>(64, want);
    Ensemble e(1, d, PDMP_SAMPLER_BPS, o, cap);
    check(pdmp_ensemble_set_flow_bps_modern(e.get(), B.lambda_ref, B.rho, opt(B.U), o.oscn ? 1 : 0));
    set_target(e, target);
    if (B.L.n > 0) check(pdmp_ensemble_set_mass_cholesky(e.get(), B.L.colptr.data(), B.L.rowval.data(), B.L.nzval.data()));
    if (nsamples > 0) {  // (set_state_bps comes first inside not_factorised: the limit is set on the flow, which keeps it)
        check(pdmp_ensemble_set_bps_record_limit(e.get(), nsamples));
    }
    return not_factorised(e, t0, x0, theta0, T, c.c, o);
}
}  // namespace detail
inline Result<PDMPTrace> pdmp(const GaussianTarget& target, double t0, const std::vector<double>& x0, const std::vector<double>& theta0,
                              double T, LocalBound c, const BouncyParticle& B, Options o = {}) {
    return detail::modern(target, t0, x0, theta0, T, 0, c, B, o);
}
inline Result<PDMPTrace> pdmp(const GaussianTarget& target, double t0, const std::vector<double>& x0, const std::vector<double>& theta0,
                              int64_t nsamples, LocalBound c, const BouncyParticle& B, Options o = {}) {
    if (nsamples <= 0) throw std::invalid_argument("pdmp(..., T::Int, ...): a positive number of samples");
    return detail::modern(target, t0, x0, theta0, std::numeric_limits<double>::infinity(), nsamples, c, B, o);
}

inline Result<PDMPTrace> pdmp(const LogisticRegression& target, double t0, const std::vector<double>& x0, const std::vector<double>& theta0,
                              double T, LocalBound c, const BouncyParticle& B, Options o = {}) {
    return detail::modern(target, t0, x0, theta0, T, 0, c, B, o);
}
inline Result<PDMPTrace> pdmp(const LogisticRegression& target, double t0, const std::vector<double>& x0, const std::vector<double>& theta0,
                              int64_t nsamples, LocalBound c, const BouncyParticle& B, Options o = {}) {
    if (nsamples <= 0) throw std::invalid_argument("pdmp(..., T::Int, ...): a positive number of samples");
    return detail::modern(target, t0, x0, theta0, std::numeric_limits<double>::infinity(), nsamples, c, B, o);
}

// ---- the one-dimensional samplers: pdmp(∇ϕ, x, θ, T, c, Flow::Union{ZigZag1d, Boomerang1d}; adapt, factor = 2.0) -> Ξ, acc/num
// (src/zigzagboom1d.jl:34-67).  ∇ϕ(x) = (x − μ)/σ² + noise (rand() − 0.5) (test/test1d.jl:9-10).
struct ZigZag1d {};
struct Boomerang1d {
    double Sigma = 1.0, mu = 0.0, lambda_ref = 1.0;  // Boomerang1d(Σ, μ, λ), src/types.jl:89-100
};
struct GaussianTarget1d {
    double mu = 0.0, sigma2 = 1.0, noise = 0.0;
};
struct Result1d {
    std::vector<pdmp_event1d> trace;  // Ξ: (t, x, θ), the first entry (0, x0, θ0)
    double acceptance;                // acc/num
    double c;                         // the tuning parameter after adaptation
};
namespace detail {
inline std::vector<Result1d> run_1d(pdmp_1d_config cfg, const std::vector<double>& x0, const std::vector<double>& theta0, double T, double c,
                                    const Options& o) {
    const size_t n = x0.size();
    cfg.struct_size = (uint32_t)sizeof(pdmp_1d_config);
    cfg.device = o.device;
    cfg.adapt = o.adapt ? 1 : 0;
    cfg.factor = (o.factor == 1.8) ? 2.0 : o.factor;  // (the 1-d driver's default, :34)
    cfg.nchains = (int64_t)n;
    cfg.trace_capacity = o.trace_capacity > 0 ? o.trace_capacity : 4096;
    std::vector<pdmp_1d_state> st(n);
    std::vector<uint64_t> seeds(n);
    for (size_t k = 0; k < n; ++k) {
        st[k] = pdmp_1d_state{};
        st[k].x = x0[k];
        st[k].theta = theta0[k];
        st[k].c = c;
        seeds[k] = o.seed + k;
    }
    std::vector<pdmp_event1d> ev(n * (size_t)cfg.trace_capacity);
    std::vector<int64_t> nev(n);
    std::vector<Result1d> out(n);
    for (;;) {
        check(pdmp_1d_run(&cfg, st.data(), seeds.data(), T, ev.data(), nev.data()));
        bool again = false;
        for (size_t k = 0; k < n; ++k) {
            out[k].trace.insert(out[k].trace.end(), ev.begin() + (ptrdiff_t)(k * (size_t)cfg.trace_capacity),
                                ev.begin() + (ptrdiff_t)(k * (size_t)cfg.trace_capacity + (size_t)nev[k]));
            if (st[k].status == PDMP_CHAIN_BOUND_VIOLATED) throw std::runtime_error("Tuning parameter `c` too small.");  // :55
            again = again || st[k].status == PDMP_CHAIN_TRACE_FULL || st[k].status == PDMP_CHAIN_PAUSED;
        }
        if (!again) break;
    }
    for (size_t k = 0; k < n; ++k) {
        out[k].acceptance = st[k].num ? (double)st[k].acc / (double)st[k].num : 0.0;
        out[k].c = st[k].c;
    }
    return out;
}
}  // namespace detail
inline std::vector<Result1d> pdmp(const GaussianTarget1d& g, const std::vector<double>& x0, const std::vector<double>& theta0, double T, double c,
                                  const ZigZag1d&, const Options& o = {}) {
    pdmp_1d_config cfg{};
    cfg.flow = PDMP_1D_ZIGZAG;
    cfg.mu = g.mu, cfg.sigma2 = g.sigma2, cfg.noise = g.noise;
    cfg.b_sigma = 1.0, cfg.b_mu = 0.0, cfg.b_lambda = 1.0;
    return detail::run_1d(cfg, x0, theta0, T, c, o);
}
inline std::vector<Result1d> pdmp(const GaussianTarget1d& g, const std::vector<double>& x0, const std::vector<double>& theta0, double T, double c,
                                  const Boomerang1d& B, const Options& o = {}) {
    pdmp_1d_config cfg{};
    cfg.flow = PDMP_1D_BOOMERANG;
    cfg.mu = g.mu, cfg.sigma2 = g.sigma2, cfg.noise = g.noise;
    cfg.b_sigma = B.Sigma, cfg.b_mu = B.mu, cfg.b_lambda = B.lambda_ref;
    return detail::run_1d(cfg, x0, theta0, T, c, o);
}

}  // namespace pdmp

#endif  // PDMP_MI355_HPP
