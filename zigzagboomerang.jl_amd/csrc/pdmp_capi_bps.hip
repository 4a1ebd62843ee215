// pdmp_capi_bps.hip -- the Bouncy Particle family (BouncyParticle, Boomerang, their sticky and speed-recorded forms): flow, options, state, reads.
#include <algorithm>
#include <cmath>

#include "pdmp_ensemble.hpp"

pdmp::BpsModernParams bps_modern_params(const pdmp_ensemble* e) {
    pdmp::BpsModernParams q{};
    q.u_diag = e->bps.udiag ? e->b_udiag.p : nullptr;
    q.su_diag = e->bps.udiag ? e->b_sudiag.p : nullptr;
    q.mstate = e->b_mstate.p;
    q.record_limit = e->bps.record_limit;
    q.count_limit = e->dbg_count_limit ? e->dbg_count_limit : pdmp::PDMP_LAUNCH_COUNT_LIMIT;
    q.oscn = e->bps.oscn;
    return q;
}

pdmp::BpsLogitParams bps_logit_params(const pdmp_ensemble* e) {
    pdmp::BpsLogitParams g{};
    g.A_colptr = e->bl_Acp.p;
    g.A_rowval = e->bl_Arv.p;
    g.A_nzval = e->bl_Anz.p;
    g.At_colptr = e->bl_Atcp.p;
    g.At_rowval = e->bl_Atrv.p;
    g.At_nzval = e->bl_Atnz.p;
    g.y = e->bl_y.p;
    g.m = e->bl_m.p;
    g.eta = e->bl_eta.p;
    g.n = e->bl_n;
    g.gamma0 = e->bl_gamma0;
    return g;
}

static void fill_bps_ext(const pdmp_ensemble* e, pdmp::BpsRunParams& B) {
    B.local_bound = e->bps.local_bound;
    B.subsample = e->bps.subsample;
    B.ext = (e->bps.mass_tables || e->bps.local_bound || e->bps.subsample || e->bps.own_target) ? 1 : 0;
    if (e->bps.own_target) {
        B.t_colptr = e->bt_colptr.p;
        B.t_rowval = e->bt_rowval.p;
        B.t_nzval = e->bt_nzval.p;
        B.t_mu = e->bt_mu.p;
        B.ident = 0;  // (the gradient-free register layout belongs to the isotropic TARGET)
    }
    if (e->bps.mass_tables) {
        B.Lcp = e->m_Lcp.p;
        B.Lrv = e->m_Lrv.p;
        B.Lnz = e->m_Lnz.p;
        B.Ucp = e->m_Ucp.p;
        B.Urv = e->m_Urv.p;
        B.Unz = e->m_Unz.p;
    }
}

pdmp::BpsRunParams bps_run_params(const pdmp_ensemble* e, double T, int flags) {
    pdmp::BpsRunParams B{};
    B.colptr = e->b_colptr.p;
    B.rowval = e->b_rowval.p;
    B.nzval = e->b_nzval.p;
    B.mu = e->b_mu.p;
    B.mu_flow = e->b_mu_flow.p;
    B.flow_kind = e->bps.flow_kind;
    B.ident = e->bps.ident ? 1 : 0;
    B.x = e->b_x.p;
    B.th = e->b_th.p;
    B.scal = e->b_scal.p;
    B.hdr = e->d_hdr.p;
    B.ev_t = e->b_ev_t.p;
    B.ev_x = e->b_ev_x.p;
    B.ev_th = e->b_ev_th.p;
    B.d = e->cfg.d;
    B.trace_cap = e->cfg.trace_capacity;
    B.T = T;
    B.factor = e->cfg.factor;
    B.lambda_ref = e->bps.lambda;
    B.rho = e->bps.rho;
    B.flags = flags;
    B.adapt = e->cfg.adapt;
    fill_bps_ext(e, B);
    return B;
}

pdmp::BpsStickyParams bps_sticky_params(const pdmp_ensemble* e) {
    pdmp::BpsStickyParams q{};
    q.kappa = e->b_kappa.p;
    q.thf = e->b_thf.p;
    q.tfrez = e->b_tfrez.p;
    q.fmask = e->b_fmask.p;
    q.ev_f = e->b_ev_f.p;
    q.strong_upperbounds = e->bps.strong;
    return q;
}

pdmp::BpsMomParams bps_moments_params(const pdmp_ensemble* e) {
    pdmp::BpsMomParams m{};
    m.mom = e->bps.mom;
    m.J1 = e->bps.mom >= 1 ? e->b_j1.p : nullptr;
    m.J2 = e->bps.mom >= 2 ? e->b_j2.p : nullptr;
    return m;
}

static pdmp_status set_flow_nf(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                               const double* mu, double lambda_ref, double rho, int kind, const double* mu_flow) {
    if (!e || !colptr || !rowval || !nzval) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS) return fail(PDMP_ERR_INVALID, "ensemble was not created with PDMP_SAMPLER_BPS");
    if (!(lambda_ref > 0)) return fail(PDMP_ERR_INVALID, "BouncyParticle needs a strictly positive refreshment rate");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d;
    PDMP_TRY(check_csc("flow matrix", colptr, rowval, d, d));
    const int64_t nnz = colptr[d];
    bool diag = (nnz == d);
    for (int64_t i = 0; diag && i < d; ++i) diag = colptr[i + 1] - colptr[i] == 1 && rowval[colptr[i]] == i;
    bool ident = diag && kind == 0;
    for (int64_t i = 0; ident && i < d; ++i) ident = (nzval[i] == 1.0) && (!mu || mu[i] == 0.0);
    bool gI = diag;
    for (int64_t i = 0; gI && i < d; ++i) gI = (nzval[i] == 1.0);
    e->bps = BpsOptions{};
    e->bps.flow_kind = kind;
    e->bps.diag = diag;
    e->bps.ident = ident;
    e->bps.gamma_is_I = gI;
    e->bps.lambda = lambda_ref;
    e->bps.rho = rho;
    PDMP_TRY(e->b_colptr.upload(std::vector<int64_t>(colptr, colptr + d + 1)));
    PDMP_TRY(e->b_rowval.upload(std::vector<int64_t>(rowval, rowval + nnz)));
    PDMP_TRY(e->b_nzval.upload(std::vector<double>(nzval, nzval + nnz)));
    std::vector<double> muv(d, 0.0);
    if (mu) muv.assign(mu, mu + d);
    PDMP_TRY(e->b_mu.upload(muv));
    std::vector<double> mfv(d, 0.0);
    if (mu_flow) mfv.assign(mu_flow, mu_flow + d);
    PDMP_TRY(e->b_mu_flow.upload(mfv));
    e->has_flow = true;
    e->has_target = true;
    e->has_state = false;
    return PDMP_OK;
}

// The moments of chains [chain_first, chain_first + n) at T into b_jT (and b_jT2 with `two`), rows 0..n-1 -- after checking that T lies
// on the stretch of every chain's path its state describes: t <= T <= min(tp, tau_ref) (no event between the chain's clock and T), the
// chain neither BOUND_VIOLATED nor STALLED.
pdmp_status bps_moments_at(pdmp_ensemble* e, double T, int64_t chain_first, int64_t n, bool two) {
    const int64_t d = e->cfg.d, nch = e->cfg.nchains;
    std::vector<double> sc((size_t)(n * 8));
    std::vector<pdmp::DevChain> h((size_t)n);
    if (n > 0) {
        HIP_TRY(hipMemcpy(sc.data(), e->b_scal.p + chain_first * 8, sc.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(h.data(), e->d_hdr.p + chain_first, h.size() * sizeof(pdmp::DevChain), hipMemcpyDeviceToHost));
    }
    for (int64_t k = 0; k < n; ++k) {
        const long long ch = (long long)(chain_first + k);
        const uint32_t cs = h[(size_t)k].c.status;
        if (cs != PDMP_CHAIN_OK && cs != PDMP_CHAIN_TRACE_FULL)
            return fail(PDMP_ERR_INVALID, "chain %lld: status %u (bound violated / stalled): its path moments are not defined", ch, cs);
        const double t = sc[(size_t)(k * 8)], next = std::min(sc[(size_t)(k * 8 + 3)], sc[(size_t)(k * 8 + 4)]);
        if (!(t <= T))
            return fail(PDMP_ERR_INVALID, "chain %lld: T = %.17g lies before the chain's clock %.17g (a reference-tail run passes T)", ch, T, t);
        if (!(T <= next))
            return fail(PDMP_ERR_INVALID, "chain %lld: T = %.17g lies past the chain's next event at %.17g (run to T with PDMP_RUN_STOP_BEFORE)",
                        ch, T, next);
    }
    if (e->b_jT.n != (size_t)(nch * d)) PDMP_TRY(e->b_jT.alloc((size_t)(nch * d)));
    if (two && e->b_jT2.n != (size_t)(nch * d)) PDMP_TRY(e->b_jT2.alloc((size_t)(nch * d)));
    pdmp::BpsRunParams B{};
    B.x = e->b_x.p;
    B.th = e->b_th.p;
    B.scal = e->b_scal.p;
    B.mu_flow = e->b_mu_flow.p;
    B.flow_kind = e->bps.flow_kind;
    B.d = d;
    LAUNCH_TRY("bps_moments_tail", pdmp::launch_bps_moments_tail(B, bps_moments_params(e), chain_first, n, T, e->b_jT.p, two ? e->b_jT2.p : nullptr, e->stream));
    return PDMP_OK;
}

pdmp_status init_state_bps(pdmp_ensemble* e, double t0, const double* x0, const double* theta0, double c, const uint64_t* seeds) {
    if (!e || !x0 || !theta0 || !seeds) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_bps first");
    if (e->bps.sticky) {
        // sticky_pdmp_inner! (src/ss_not_fact.jl:104-179) has no LocalBound, subsample or path-moment form here, and never reads a BouncyParticle's L
        if (e->cfg.d > 64 * pdmp::BPS_STICKY_WORDS)
            return fail(PDMP_ERR_UNSUPPORTED, "sticky BouncyParticle / Boomerang keeps d <= 1024 coordinates in registers: got %lld", (long long)e->cfg.d);
        if (e->bps.local_bound) return fail(PDMP_ERR_UNSUPPORTED, "set_bps_sticky: not together with local_bound (set_bps_options)");
        if (e->bps.subsample) return fail(PDMP_ERR_UNSUPPORTED, "set_bps_sticky: not together with subsample (set_bps_options)");
        if (e->bps.mom >= 1) return fail(PDMP_ERR_UNSUPPORTED, "set_bps_sticky: not together with set_bps_moments(order >= 1)");
        if (e->bps.flow_kind == 1 && e->bps.mass_tables)
            return fail(PDMP_ERR_UNSUPPORTED, "set_bps_sticky: a Boomerang with a general mass factor L (set_mass_cholesky) is not implemented: identity only");
    }
    if (e->bps.logit && (!e->bps.modern || e->bps.sticky))
        return fail(PDMP_ERR_UNSUPPORTED, "set_target_bps_logistic: the logistic-regression target belongs to the speed-recorded driver "
                    "(pdmp_ensemble_set_flow_bps_modern), not to %s", e->bps.sticky ? "a sticky ensemble (set_bps_sticky)"
                    : e->bps.flow_kind == 1 ? "a Boomerang (set_flow_boomerang)" : "the event-recorded set_flow_bps");
    if (e->bps.modern) {
        // the speed-recorded driver always bounds locally and always subsamples; its options are its own
        if (!e->bps.own_target && !e->bps.logit)
            return fail(PDMP_ERR_INVALID, "set_flow_bps_modern: the flow has no Γ of its own, pdmp_ensemble_set_target_gaussian_csc or "
                        "pdmp_ensemble_set_target_bps_logistic must follow it");
        if (e->cfg.d > 1024)
            return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern keeps d <= 1024 coordinates in registers: got d = %lld", (long long)e->cfg.d);
        if (e->bps.mom >= 1) return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: not together with set_bps_moments(order >= 1)");
        if (e->bps.sticky) return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: not together with set_bps_sticky");
        if (e->bps.subsample) return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: not together with subsample (set_bps_options): this driver always subsamples");
        if (e->bps.local_bound) return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: not together with local_bound (set_bps_options): this driver always bounds locally");
        if (e->bps.oscn && e->bps.udiag) return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: oscn with u_diag is not defined (src/not_fact_samplers.jl:267 asserts L == I)");
        if (e->bps.oscn && e->bps.mass_tables)
            return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: oscn with a mass factor (set_mass_cholesky) that is not the identity (src/not_fact_samplers.jl:267)");
        if (e->bps.udiag && e->bps.has_mass) return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: u_diag together with a mass factor (set_mass_cholesky): one metric only");
        if (!(c > 0) || !std::isfinite(c)) return fail(PDMP_ERR_INVALID, "LocalBound(c) needs a finite c > 0 (the bound expires after 2√d/c/V): got %g", c);
        if (e->bps.logit && pdmp::bps_logit_lds_bytes(e->cfg.d, e->bl_n) > pdmp::BPS_LOGIT_LDS_MAX)
            return fail(PDMP_ERR_UNSUPPORTED, "set_target_bps_logistic keeps η and ζ of n = %lld observations in LDS beside the [d] staging buffer: "
                        "8 d + 16 n = %zu bytes, the limit is %zu", (long long)e->bl_n, pdmp::bps_logit_lds_bytes(e->cfg.d, e->bl_n), pdmp::BPS_LOGIT_LDS_MAX);
    }
    if (!e->bps.modern && !e->bps.sticky && e->bps.flow_kind == 0 && !e->bps.gamma_is_I && !e->bps.has_mass)
        return fail(PDMP_ERR_UNSUPPORTED,
                    "BouncyParticle(Γ ≠ I) carries the mass factor L = cholesky(Symmetric(Γ)).L (src/types.jl:43): pass it with "
                    "pdmp_ensemble_set_mass_cholesky (an identity factor selects the identity mass explicitly)");
    if (e->bps.flow_kind == 1 && !e->bps.has_mass)
        return fail(PDMP_ERR_UNSUPPORTED,
                    "Boomerang(Γ, μ, λ) carries L = cholesky(Symmetric(Γ)).L (src/types.jl:66) and this library never sees the flow's Γ: "
                    "pass the factor with pdmp_ensemble_set_mass_cholesky (an identity factor selects the identity mass explicitly)");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d, n = e->cfg.nchains, cap = e->cfg.trace_capacity;
    // (arrays of the right size are kept: a second set_state -- set_state_bps's placement probes among them -- writes into the same memory)
    if (e->b_x.n != (size_t)(n * d)) PDMP_TRY(e->b_x.alloc((size_t)(n * d)));
    if (e->b_th.n != (size_t)(n * d)) PDMP_TRY(e->b_th.alloc((size_t)(n * d)));
    if (e->b_scal.n != (size_t)(n * 8)) PDMP_TRY(e->b_scal.alloc((size_t)(n * 8)));
    if (e->d_hdr.n != (size_t)n) PDMP_TRY(e->d_hdr.alloc((size_t)n));
    if (cap > 0) {
        if (e->b_ev_t.n != (size_t)(n * cap)) PDMP_TRY(e->b_ev_t.alloc((size_t)(n * cap)));
        if (e->b_ev_x.n != (size_t)(n * cap * d)) PDMP_TRY(e->b_ev_x.alloc((size_t)(n * cap * d)));
        if (e->b_ev_th.n != (size_t)(n * cap * d)) PDMP_TRY(e->b_ev_th.alloc((size_t)(n * cap * d)));
    }
    HIP_TRY(hipMemcpy(e->b_x.p, x0, (size_t)(n * d) * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->b_th.p, theta0, (size_t)(n * d) * sizeof(double), hipMemcpyHostToDevice));
    DevBuf<uint64_t> sseed;
    PDMP_TRY(sseed.alloc((size_t)n));
    HIP_TRY(hipMemcpy(sseed.p, seeds, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
    const pdmp::BpsRunParams B = bps_run_params(e, t0, 0);  // (the init kernel reads the tables and the state arrays of the event loop's block)
    // the moments start at t0 (also after set_state_bps's placement probes, which run launches in between)
    if (e->bps.mom >= 1) HIP_TRY(hipMemsetAsync(e->b_j1.p, 0, (size_t)(n * d) * sizeof(double), e->stream));
    if (e->bps.mom >= 2) HIP_TRY(hipMemsetAsync(e->b_j2.p, 0, (size_t)(n * d) * sizeof(double), e->stream));
    if (e->bps.modern) {
        if (e->b_mstate.n != (size_t)(n * 4)) PDMP_TRY(e->b_mstate.alloc((size_t)(n * 4)));
        if (e->bps.logit) {
            if (e->bl_eta.n != (size_t)(n * e->bl_n)) PDMP_TRY(e->bl_eta.alloc((size_t)(n * e->bl_n)));
            LAUNCH_TRY_CODE("bps_logit_init", pdmp::launch_bps_logit_init(B, bps_modern_params(e), bps_logit_params(e), n, sseed.p, t0, c, e->stream));
        } else {
            LAUNCH_TRY_CODE("bps_modern_init", pdmp::launch_bps_modern_init(B, bps_modern_params(e), n, sseed.p, t0, c, e->stream));
        }
    } else if (e->bps.sticky) {
        const size_t W = (size_t)pdmp::BPS_STICKY_WORDS;
        if (e->b_thf.n != (size_t)(n * d)) PDMP_TRY(e->b_thf.alloc((size_t)(n * d)));
        if (e->b_tfrez.n != (size_t)(n * d)) PDMP_TRY(e->b_tfrez.alloc((size_t)(n * d)));
        if (e->b_fmask.n != (size_t)n * W) PDMP_TRY(e->b_fmask.alloc((size_t)n * W));
        if (cap > 0) {
            if (e->b_ev_f.n != (size_t)(n * cap) * W) PDMP_TRY(e->b_ev_f.alloc((size_t)(n * cap) * W));
            HIP_TRY(hipMemsetAsync(e->b_ev_f.p, 0, e->b_ev_f.n * sizeof(uint64_t), e->stream));  // (words past the last slot stay 0)
        }
        LAUNCH_TRY_CODE("bps_sticky_init", pdmp::launch_bps_sticky_init(B, bps_sticky_params(e), n, sseed.p, t0, c, e->stream));
    } else {
        LAUNCH_TRY_CODE("bps_init", pdmp::launch_bps_init(B, n, sseed.p, t0, c, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->has_state = true;
    e->ran = false;
    e->timed = false;
    e->t0_state = t0;  // (pdmp_ensemble_bps_consume_begin's grid starts here)
    e->bc_on = false;
    e->bcn_on = false;
    e->bpr_on = false;
    e->bhs_on = e->bhs_arc = false;
    e->trace_appended = false;
    return PDMP_OK;
}

// `rows` free masks from the device (bit e & 63 of word e >> 6) -> one byte per coordinate, [rows x d]
static pdmp_status copy_free_masks(const uint64_t* dev_words, int64_t rows, int64_t d, uint8_t* f) {
    const int64_t W = pdmp::BPS_STICKY_WORDS;
    std::vector<uint64_t> w((size_t)(rows * W));
    HIP_TRY(hipMemcpy(w.data(), dev_words, w.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < rows; ++k)
        for (int64_t i = 0; i < d; ++i) f[k * d + i] = (uint8_t)((w[(size_t)(k * W + (i >> 6))] >> (i & 63)) & 1ull);
    return PDMP_OK;
}

extern "C" {

pdmp_status pdmp_ensemble_set_flow_bps(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                                       const double* mu, double lambda_ref, double rho) {
    return set_flow_nf(e, colptr, rowval, nzval, mu, lambda_ref, rho, 0, nullptr);
}

pdmp_status pdmp_ensemble_set_flow_boomerang(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval,
                                             const double* nzval, const double* mu_target, const double* mu_flow,
                                             double lambda_ref, double rho) {
    return set_flow_nf(e, colptr, rowval, nzval, mu_target, lambda_ref, rho, 1, mu_flow);
}

// pdmp(dϕ, ∇ϕ!, t0, x0, θ0, T, c::LocalBound, flow::BouncyParticle; oscn, adapt, factor), src/not_fact_samplers.jl:336-384: the flow carries
// no Γ of its own (BouncyParticle(missing, missing, λref, ρ, U, L)); the target follows with pdmp_ensemble_set_target_gaussian_csc.
pdmp_status pdmp_ensemble_set_flow_bps_modern(pdmp_ensemble* e, double lambda_ref, double rho, const double* u_diag, int oscn) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS) return fail(PDMP_ERR_INVALID, "ensemble was not created with PDMP_SAMPLER_BPS");
    if (e->has_state) return fail(PDMP_ERR_INVALID, "set_flow_bps_modern goes before set_state_bps");
    if (!(lambda_ref > 0) || !std::isfinite(lambda_ref)) return fail(PDMP_ERR_INVALID, "BouncyParticle needs a strictly positive refreshment rate");
    if (!(std::fabs(rho) <= 1.0)) return fail(PDMP_ERR_INVALID, "rho = %g: the refreshment's autocorrelation lies in [-1, 1]", rho);
    const int64_t d = e->cfg.d;
    if (u_diag)
        for (int64_t i = 0; i < d; ++i)
            if (!(u_diag[i] > 0) || !std::isfinite(u_diag[i])) return fail(PDMP_ERR_INVALID, "u_diag[%lld] must be positive and finite", (long long)i);
    HIP_TRY(hipSetDevice(e->cfg.device));
    e->bps = BpsOptions{};
    e->bps.lambda = lambda_ref;
    e->bps.rho = rho;
    e->b_colptr.release();
    e->b_rowval.release();
    e->b_nzval.release();
    e->b_mu.release();
    e->b_mu_flow.release();
    if (u_diag) {
        std::vector<double> u(u_diag, u_diag + d), su((size_t)d);
        for (int64_t i = 0; i < d; ++i) su[(size_t)i] = std::sqrt(u[(size_t)i]);
        PDMP_TRY(e->b_udiag.upload(u));
        PDMP_TRY(e->b_sudiag.upload(su));
    }
    e->bps.modern = true;
    e->bps.udiag = u_diag != nullptr;
    e->bps.oscn = oscn ? 1 : 0;
    e->has_flow = true;
    e->has_target = false;
    e->has_state = false;
    return PDMP_OK;
}

// dϕ and ∇ϕ! of a Bayesian logistic regression for the speed-recorded driver (pdmp_bps_logit.inc): takes the place of set_target_gaussian_csc.
pdmp_status pdmp_ensemble_set_target_bps_logistic(pdmp_ensemble* e, int64_t n, const int64_t* A_colptr, const int64_t* A_rowval, const double* A_nzval,
                                                  const int64_t* At_colptr, const int64_t* At_rowval, const double* At_nzval, const double* y,
                                                  const double* m, double gamma0) {
    if (!e || !A_colptr || !A_rowval || !A_nzval || !At_colptr || !At_rowval || !At_nzval || !y || !m) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS) return fail(PDMP_ERR_INVALID, "set_target_bps_logistic: the ensemble was not created with PDMP_SAMPLER_BPS");
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_target_bps_logistic follows pdmp_ensemble_set_flow_bps_modern");
    if (e->has_state) return fail(PDMP_ERR_INVALID, "set_target_bps_logistic goes before set_state_bps");
    if (n <= 0) return fail(PDMP_ERR_INVALID, "set_target_bps_logistic: n = %lld observations, need n > 0", (long long)n);
    if (!(gamma0 >= 0) || !std::isfinite(gamma0)) return fail(PDMP_ERR_INVALID, "set_target_bps_logistic: gamma0 = %g, the prior precision is finite and >= 0", gamma0);
    const int64_t d = e->cfg.d;
    PDMP_TRY(check_csc("design A", A_colptr, A_rowval, n, d));
    PDMP_TRY(check_csc("design At", At_colptr, At_rowval, d, n));
    const int64_t nnz = A_colptr[d];
    if (At_colptr[n] != nnz) return fail(PDMP_ERR_INVALID, "A / At are inconsistent: nnz %lld and %lld", (long long)nnz, (long long)At_colptr[n]);
    {  // At is the transpose PATTERN of A: column by column of A, the next unread entry of At's column `row` is this coordinate
        std::vector<int64_t> next(At_colptr, At_colptr + n);
        for (int64_t j = 0; j < d; ++j)
            for (int64_t p = A_colptr[j]; p < A_colptr[j + 1]; ++p) {
                const int64_t r = A_rowval[p];
                if (next[(size_t)r] >= At_colptr[r + 1] || At_rowval[next[(size_t)r]] != j)
                    return fail(PDMP_ERR_INVALID, "A / At are inconsistent: At is not the transpose pattern of A at A[%lld, %lld]", (long long)r, (long long)j);
                next[(size_t)r]++;
            }
    }
    for (int64_t i = 0; i < n; ++i) {
        if (!std::isfinite(m[i]) || !(m[i] >= 0)) return fail(PDMP_ERR_INVALID, "m[%lld] = %g: trial counts are finite and >= 0", (long long)i, m[i]);
        if (!std::isfinite(y[i]) || !(y[i] >= 0) || !(y[i] <= m[i]))
            return fail(PDMP_ERR_INVALID, "y[%lld] = %g: successes are finite and lie in [0, m] (m = %g)", (long long)i, y[i], m[i]);
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    PDMP_TRY(e->bl_Acp.upload(std::vector<int64_t>(A_colptr, A_colptr + d + 1)));
    PDMP_TRY(e->bl_Arv.upload(std::vector<int64_t>(A_rowval, A_rowval + nnz)));
    PDMP_TRY(e->bl_Anz.upload(std::vector<double>(A_nzval, A_nzval + nnz)));
    PDMP_TRY(e->bl_Atcp.upload(std::vector<int64_t>(At_colptr, At_colptr + n + 1)));
    PDMP_TRY(e->bl_Atrv.upload(std::vector<int64_t>(At_rowval, At_rowval + nnz)));
    PDMP_TRY(e->bl_Atnz.upload(std::vector<double>(At_nzval, At_nzval + nnz)));
    PDMP_TRY(e->bl_y.upload(std::vector<double>(y, y + n)));
    PDMP_TRY(e->bl_m.upload(std::vector<double>(m, m + n)));
    e->bl_n = n;
    e->bl_gamma0 = gamma0;
    e->bps.logit = true;
    e->bps.own_target = false;  // (the later of the two target calls wins)
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_bps_record_limit(pdmp_ensemble* e, int64_t n) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->bps.modern)
        return fail(PDMP_ERR_INVALID, "set_bps_record_limit: pdmp_ensemble_set_flow_bps_modern first (PDMP_SAMPLER_BPS)");
    if (n < 0) return fail(PDMP_ERR_INVALID, "record limit %lld: 0 (no limit) or a positive number of records", (long long)n);
    e->bps.record_limit = n;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_mass_cholesky(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval,
                                            const double* nzval) {
    if (!e || !colptr || !rowval || !nzval) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->has_flow)
        return fail(PDMP_ERR_INVALID, "set_flow_bps / set_flow_boomerang first (PDMP_SAMPLER_BPS)");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d;
    PDMP_TRY(check_csc("mass factor", colptr, rowval, d, d, true));
    const int64_t nnz = colptr[d];
    if (nnz >= ((int64_t)1 << 31)) return fail(PDMP_ERR_INVALID, "mass factor: bad number of entries");
    bool identity = (nnz == d);
    for (int64_t j = 0; j < d; ++j) {
        const double djj = nzval[colptr[j]];
        if (!(djj != 0.0) || djj != djj) return fail(PDMP_ERR_INVALID, "mass factor: zero or NaN diagonal at %lld", (long long)j);
        if (djj != 1.0) identity = false;
    }
    e->bps.has_mass = true;
    e->bps.mass_tables = false;
    e->has_state = false;
    if (identity) return PDMP_OK;  // L = I: x / 1.0 and no off-diagonal updates -- the identity-mass kernels are bit-identical
    std::vector<int32_t> lcp(colptr, colptr + d + 1), lrv(rowval, rowval + nnz), ucp(d + 2, 0), urv((size_t)nnz);
    std::vector<double> lnz(nzval, nzval + nnz), unz((size_t)nnz);
    for (int64_t p = 0; p < nnz; ++p) ucp[(size_t)rowval[p] + 2]++;
    for (int64_t j = 0; j < d; ++j) ucp[(size_t)j + 2] += ucp[(size_t)j + 1];
    for (int64_t j = 0; j < d; ++j)
        for (int64_t p = colptr[j]; p < colptr[j + 1]; ++p) {
            const int32_t q = ucp[(size_t)rowval[p] + 1]++;
            urv[(size_t)q] = (int32_t)j;
            unz[(size_t)q] = nzval[p];
        }
    ucp.pop_back();
    PDMP_TRY(e->m_Lcp.upload(lcp));
    PDMP_TRY(e->m_Lrv.upload(lrv));
    PDMP_TRY(e->m_Lnz.upload(lnz));
    PDMP_TRY(e->m_Ucp.upload(ucp));
    PDMP_TRY(e->m_Urv.upload(urv));
    PDMP_TRY(e->m_Unz.upload(unz));
    e->bps.mass_tables = true;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_bps_options(pdmp_ensemble* e, int local_bound, int subsample) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->has_flow)
        return fail(PDMP_ERR_INVALID, "set_flow_bps / set_flow_boomerang first (PDMP_SAMPLER_BPS)");
    if (local_bound && e->bps.flow_kind != 0)
        return fail(PDMP_ERR_UNSUPPORTED, "c::LocalBound is defined for BouncyParticle only (src/not_fact_samplers.jl:29-31)");
    e->bps.local_bound = local_bound ? 1 : 0;
    e->bps.subsample = subsample ? 1 : 0;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_bps_moments(pdmp_ensemble* e, int order) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->has_flow)
        return fail(PDMP_ERR_INVALID, "set_flow_bps / set_flow_boomerang first (PDMP_SAMPLER_BPS)");
    if (order < 0 || order > 2) return fail(PDMP_ERR_INVALID, "moments order %d: 0 (off), 1 (∫x dt) or 2 (∫x dt and ∫x² dt)", order);
    if (e->has_state) return fail(PDMP_ERR_INVALID, "set_bps_moments goes before set_state_bps");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const size_t nd = (size_t)(e->cfg.nchains * e->cfg.d);
    if (order >= 1) {
        if (e->b_j1.n != nd) PDMP_TRY(e->b_j1.alloc(nd));
    } else {
        e->b_j1.release();
    }
    if (order >= 2) {
        if (e->b_j2.n != nd) PDMP_TRY(e->b_j2.alloc(nd));
    } else {
        e->b_j2.release();
    }
    e->bps.mom = order;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_bps_sticky(pdmp_ensemble* e, const double* kappa, int strong_upperbounds) {
    if (!e || !kappa) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->has_flow)
        return fail(PDMP_ERR_INVALID, "set_flow_bps / set_flow_boomerang first (PDMP_SAMPLER_BPS)");
    if (e->has_state) return fail(PDMP_ERR_INVALID, "set_bps_sticky goes before set_state_bps");
    const int64_t d = e->cfg.d;
    for (int64_t i = 0; i < d; ++i)
        if (!(kappa[i] > 0) || !std::isfinite(kappa[i])) return fail(PDMP_ERR_INVALID, "kappa[%lld] must be positive and finite", (long long)i);
    HIP_TRY(hipSetDevice(e->cfg.device));
    PDMP_TRY(e->b_kappa.upload(std::vector<double>(kappa, kappa + d)));
    e->bps.sticky = true;
    e->bps.strong = strong_upperbounds ? 1 : 0;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_bps_moments(pdmp_ensemble* e, double T, int64_t chain_first, int64_t n, double* j1, double* j2) {
    if (!e || !j1) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || e->bps.mom < 1)
        return fail(PDMP_ERR_INVALID, "no path moments: a BPS ensemble with pdmp_ensemble_set_bps_moments(order >= 1)");
    if (j2 && e->bps.mom < 2) return fail(PDMP_ERR_INVALID, "∫x² dt needs moments of order 2 (this ensemble keeps order %d)", e->bps.mom);
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "no state");
    PDMP_TRY(check_chain_range(e, chain_first, n));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    pdmp_status st = bps_moments_at(e, T, chain_first, n, j2 != nullptr);
    if (st != PDMP_OK || n == 0) return st;
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t cnt = (size_t)(n * e->cfg.d);
    HIP_TRY(hipMemcpy(j1, e->b_jT.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
    if (j2) HIP_TRY(hipMemcpy(j2, e->b_jT2.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_state_bps(pdmp_ensemble* e, double t0, const double* x0, const double* theta0, double c,
                                        const uint64_t* seeds) {
    return init_state_bps_tuned(e, t0, x0, theta0, c, seeds);
}

pdmp_status pdmp_ensemble_bps_trace_copy(pdmp_ensemble* e, int64_t chain, int64_t first, int64_t count, double* t, double* x,
                                         double* theta) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    const int64_t cap = e->cfg.trace_capacity, d = e->cfg.d;
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || cap <= 0) return fail(PDMP_ERR_INVALID, "no BPS trace buffer");
    PDMP_TRY(check_trace_range(e, chain, first, count));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    if (count == 0) return PDMP_OK;
    const int64_t slot = chain * cap + first;
    if (t) HIP_TRY(hipMemcpy(t, e->b_ev_t.p + slot, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    if (x) HIP_TRY(hipMemcpy(x, e->b_ev_x.p + slot * d, (size_t)(count * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (theta)
        HIP_TRY(hipMemcpy(theta, e->b_ev_th.p + slot * d, (size_t)(count * d) * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_bps_final_state(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* t, double* x,
                                          double* theta, double* c) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->has_state) return fail(PDMP_ERR_INVALID, "no BPS state");
    PDMP_TRY(check_chain_range(e, chain_first, n));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d;
    if (n == 0) return PDMP_OK;
    if (x) HIP_TRY(hipMemcpy(x, e->b_x.p + chain_first * d, (size_t)(n * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (theta)
        HIP_TRY(hipMemcpy(theta, e->b_th.p + chain_first * d, (size_t)(n * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (t || c) {
        std::vector<double> sc((size_t)n * 8);
        HIP_TRY(hipMemcpy(sc.data(), e->b_scal.p + chain_first * 8, sc.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < n; ++k) {
            if (t) t[k] = sc[k * 8 + 0];
            if (c) c[k] = sc[k * 8 + 5];
        }
    }
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_bps_trace_free_copy(pdmp_ensemble* e, int64_t chain, int64_t first, int64_t count, uint8_t* f) {
    if (!e || !f) return fail(PDMP_ERR_INVALID, "null argument");
    const int64_t cap = e->cfg.trace_capacity, d = e->cfg.d, W = pdmp::BPS_STICKY_WORDS;
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->bps.sticky || !e->has_state || cap <= 0)
        return fail(PDMP_ERR_INVALID, "no sticky BPS trace buffer (pdmp_ensemble_set_bps_sticky, trace_capacity > 0, set_state_bps)");
    PDMP_TRY(check_trace_range(e, chain, first, count));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    if (count == 0) return PDMP_OK;
    return copy_free_masks(e->b_ev_f.p + (chain * cap + first) * W, count, d, f);
}

pdmp_status pdmp_ensemble_bps_final_sticky(pdmp_ensemble* e, int64_t chain_first, int64_t n, uint8_t* f, double* theta_f) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->bps.sticky || !e->has_state) return fail(PDMP_ERR_INVALID, "no sticky BPS state");
    PDMP_TRY(check_chain_range(e, chain_first, n));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d, W = pdmp::BPS_STICKY_WORDS;
    if (n == 0) return PDMP_OK;
    if (f) PDMP_TRY(copy_free_masks(e->b_fmask.p + chain_first * W, n, d, f));
    if (theta_f) HIP_TRY(hipMemcpy(theta_f, e->b_thf.p + chain_first * d, (size_t)(n * d) * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}
}  // extern "C"
