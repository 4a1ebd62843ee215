// pdmp_capi_stats.hip -- what is computed from a run on the device: batch means, ESS sums, path integrals, the trace consumers.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pdmp_ensemble.hpp"

static pdmp_status ess_ready(pdmp_ensemble* e) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler == PDMP_SAMPLER_BPS && e->bps.mom < 1)
        return fail(PDMP_ERR_INVALID, "path integrals are kept by the factorised samplers only");  // (and by a BPS ensemble with moments on)
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "no state");
    if (e->cfg.sampler == PDMP_SAMPLER_BPS) return PDMP_OK;
    if (e->target_kind == TARGET_BRIDGE)  // (zz_bridge_run_kernel moves coefficients without accumulating ∫ξ dt: no number rather than a wrong one)
        return fail(PDMP_ERR_UNSUPPORTED, "the diffusion-bridge target keeps no path integrals: batch means, ESS sums and path integrals come from the "
                                          "trace consumers (pdmp_ensemble_consume_*) or the returned trace");
    if (e->target_kind == TARGET_PRECISION)  // (zz_precision_run_kernel moves a column without accumulating ∫x dt)
        return fail(PDMP_ERR_UNSUPPORTED, "the precision-cholesky target keeps no path integrals: batch means, ESS sums and path integrals come from the "
                                          "trace consumers (pdmp_ensemble_consume_*) or the returned trace");
    if (!e->keep_integrals) return fail(PDMP_ERR_INVALID, "the path integrals were switched off (pdmp_ensemble_set_path_integrals)");
    if (e->flow_kind != 0)
        return fail(PDMP_ERR_UNSUPPORTED, "path integrals assume the linear flow of the ZigZag (FactBoomerang rotates between events)");
    return PDMP_OK;
}

// The factorised counterpart of bps_moments_at's rule.  J_i(T) = I_i + dt (x_i + θ_i dt / 2), dt = T - t_i, is the integral of the sampled path
// only where no event of the chain lies between a coordinate's clock and T: every chain PDMP_CHAIN_OK (a chain that stopped short of the
// horizon -- TRACE_FULL, PAUSED, BOUND_VIOLATED, STALLED -- would be extrapolated through events it has not sampled yet), T not before the
// latest proposal the chain has processed (a reference-tail run passes its horizon: the coordinate that reflected there would be extrapolated
// backwards with its new velocity) and T not beyond the horizon of the last run (t0 before the first).  Without a refresh clock the
// proposals come off the queue in time order and the header's t_last, the time of the last one, is the latest; with one they do not
// (src/sfact.jl:84-85 re-bounds at stale clocks), t_last may lie below an earlier proposal, and the only T known to be at or past all of
// them is the horizon of a run that stopped before it.  With t0 != 0 the first proposals lie before t0 (the reference draws the first
// queue times without adding t0): t_last <= T holds for them as it must.  One copy of the chain headers per read; nothing on the hot path.
static pdmp_status fact_integrals_at(pdmp_ensemble* e, double T) {
    const int64_t n = e->cfg.nchains;
    if (!(T <= e->run_T))
        return fail(PDMP_ERR_INVALID, "T = %.17g lies past the horizon %.17g of the last run (t0 before the first): the path is not sampled there "
                                      "(run to T with PDMP_RUN_STOP_BEFORE)", T, e->run_T);
    if (e->lambda_ref > 0 && T != e->run_T)
        return fail(PDMP_ERR_INVALID, "T = %.17g is not the horizon %.17g of the last run: with a refresh clock the proposals are not processed in "
                                      "time order and the path integrals are read at the end of a PDMP_RUN_STOP_BEFORE run only", T, e->run_T);
    std::vector<pdmp::DevChain> h((size_t)n);
    HIP_TRY(hipMemcpy(h.data(), e->d_hdr.p, h.size() * sizeof(pdmp::DevChain), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < n; ++k) {
        const uint32_t cs = h[(size_t)k].c.status;
        const double tl = h[(size_t)k].c.t_last;
        if (cs != PDMP_CHAIN_OK)
            return fail(PDMP_ERR_INVALID, "chain %lld: status %u at t = %.17g (trace full / paused / bound violated / stalled): it has not reached "
                                          "T = %.17g, its path integrals are not defined there (drain and run again)", (long long)k, cs, tl, T);
        if (!(tl <= T))
            return fail(PDMP_ERR_INVALID, "chain %lld: T = %.17g lies before the chain's last proposal at %.17g (a reference-tail run passes T; "
                                          "run to T with PDMP_RUN_STOP_BEFORE)", (long long)k, T, tl);
    }
    return PDMP_OK;
}

// one step (mode 0 begin, 1 batch, 2 end) of the ESS sums over [Ta, Tb]; J: where a BPS ensemble's moments at Tb lie (the factorised samplers read their records)
static int launch_ess(pdmp_ensemble* e, const double* J, int mode, double Ta, double Tb) {
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    return e->cfg.sampler == PDMP_SAMPLER_BPS ? pdmp::launch_dense_ess(J, e->d_jprev.p, e->d_jstart.p, d, n, mode, Ta, Tb, e->d_essacc.p, e->stream)
                                              : pdmp::launch_zz_ess(e->d_rec.p, e->track ? 128 : 64, e->d_jprev.p, e->d_jstart.p, d, n, mode, Ta, Tb, e->d_essacc.p, e->stream);
}

// consume_mean / consume_inclusion: one [n x d] reduction of the cursors of chains [chain_first, chain_first + n) and the chains' last event times;
// `launch` fills the two device buffers it is given
template <class Launch>
static pdmp_status consume_reduce(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* out, double* T_last, const char* name, Launch launch) {
    if (!e || !out) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->consuming) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_consume_begin first");
    if (chain_first < 0 || n <= 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "chain range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));  // (asynchronous consumers run on a second stream)
    const int64_t d = e->cfg.d;
    DevBuf<double> bm, bt;
    PDMP_TRY(bm.alloc((size_t)(n * d)));
    PDMP_TRY(bt.alloc((size_t)n));
    LAUNCH_TRY(name, launch(bm.p, bt.p));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out, bm.p, (size_t)(n * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (T_last) HIP_TRY(hipMemcpy(T_last, bt.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

constexpr uint64_t COND_MAX_ROW_BYTES = 1ull << 38;  // 256 GiB: the device's memory, about

// what both families check of the (p, n, max_hits) of a conditional trace: the support of n comes back as the ascending list S
pdmp_status condition_plane(const char* who, int64_t d, const double* p, const double* n, int64_t max_hits, std::vector<int32_t>* S) {
    if (!p || !n) return fail(PDMP_ERR_INVALID, "%s: null argument", who);
    if (max_hits < 1) return fail(PDMP_ERR_INVALID, "%s: max_hits = %lld must be at least 1", who, (long long)max_hits);
    for (int64_t j = 0; j < d; ++j) {
        if (!std::isfinite(p[j]) || !std::isfinite(n[j])) return fail(PDMP_ERR_INVALID, "%s: p and n must be finite (entry %lld is not)", who, (long long)j);
        if (n[j] != 0.0) S->push_back((int32_t)j);
    }
    if (S->empty()) return fail(PDMP_ERR_INVALID, "%s: the normal n is zero", who);
    return PDMP_OK;
}

// the rows of a conditional trace, [nchains x max_hits x d] doubles, must fit a reservation one device can hold: checked before any product is taken
pdmp_status condition_rows_fit(const char* who, int64_t nchains, int64_t d, int64_t max_hits) {
    const uint64_t per_hit = (uint64_t)nchains * (uint64_t)d * sizeof(double);  // (nchains x d x 8 fits: the cursors are that size)
    if ((uint64_t)max_hits > COND_MAX_ROW_BYTES / per_hit)
        return fail(PDMP_ERR_INVALID, "%s: max_hits = %lld rows of %llu bytes exceed the %llu GiB a condition may reserve", who, (long long)max_hits,
                    (unsigned long long)per_hit, (unsigned long long)(COND_MAX_ROW_BYTES >> 30));
    return PDMP_OK;
}

// what both families check of a pair list: npairs, the two index lists, no pair twice in either orientation, a finite centre, and that the
// accumulators [nchains x npairs] fit the reservation a condition may make (checked before the list is read)
pdmp_status pairs_list(const char* who, int64_t nchains, int64_t d, int64_t npairs, const int64_t* pi, const int64_t* pj, const double* center,
                       std::vector<int32_t>* vi, std::vector<int32_t>* vj, std::vector<double>* c) {
    if (npairs < 1) return fail(PDMP_ERR_INVALID, "%s: npairs = %lld must be at least 1", who, (long long)npairs);
    if (!pi || !pj) return fail(PDMP_ERR_INVALID, "%s: null pair list", who);
    const uint64_t per_pair = (uint64_t)nchains * sizeof(double);
    if ((uint64_t)npairs > COND_MAX_ROW_BYTES / per_pair || npairs >= (int64_t)1 << 30)  // (slots, and the 2 npairs entries of the adjacency table, are 32-bit)
        return fail(PDMP_ERR_INVALID, "%s: npairs = %lld entries of %llu bytes exceed the %llu GiB a condition may reserve", who, (long long)npairs,
                    (unsigned long long)per_pair, (unsigned long long)(COND_MAX_ROW_BYTES >> 30));
    c->assign((size_t)d, 0.0);
    if (center)
        for (int64_t j = 0; j < d; ++j) {
            if (!std::isfinite(center[j])) return fail(PDMP_ERR_INVALID, "%s: the centre must be finite (entry %lld is not)", who, (long long)j);
            (*c)[(size_t)j] = center[j];
        }
    vi->resize((size_t)npairs), vj->resize((size_t)npairs);
    std::vector<uint64_t> key((size_t)npairs);
    for (int64_t k = 0; k < npairs; ++k) {
        if (pi[k] < 0 || pi[k] >= d || pj[k] < 0 || pj[k] >= d)
            return fail(PDMP_ERR_INVALID, "%s: pair %lld = (%lld, %lld) has an index outside [0, %lld)", who, (long long)k, (long long)pi[k], (long long)pj[k],
                        (long long)d);
        (*vi)[(size_t)k] = (int32_t)pi[k];
        (*vj)[(size_t)k] = (int32_t)pj[k];
        const uint64_t lo = (uint64_t)std::min(pi[k], pj[k]), hi = (uint64_t)std::max(pi[k], pj[k]);
        key[(size_t)k] = lo * (uint64_t)d + hi;
    }
    std::sort(key.begin(), key.end());
    const auto dup = std::adjacent_find(key.begin(), key.end());
    if (dup != key.end())
        return fail(PDMP_ERR_INVALID, "%s: the pair (%llu, %llu) is listed twice (either orientation counts)", who, (unsigned long long)(*dup / (uint64_t)d),
                    (unsigned long long)(*dup % (uint64_t)d));
    return PDMP_OK;
}

// what both families check of a histogram request: m, the bin count, that the rows [nchains x m x (bins + 2)] fit the reservation a condition
// may make (checked before the lists are read), the lists, every coordinate once, finite ranges lo < hi with a finite positive width
pdmp_status hist_list(const char* who, int64_t nchains, int64_t d, int64_t m, const int64_t* coords, const double* lo, const double* hi, int64_t bins,
                      std::vector<int32_t>* vc, std::vector<double>* vlo, std::vector<double>* vhi, std::vector<double>* vw) {
    if (m < 1) return fail(PDMP_ERR_INVALID, "%s: m = %lld must be at least 1", who, (long long)m);
    if (bins < 1 || bins > 4096) return fail(PDMP_ERR_INVALID, "%s: bins = %lld is outside 1..4096", who, (long long)bins);
    const uint64_t per_coord = (uint64_t)nchains * (uint64_t)(bins + 2) * sizeof(double);
    if ((uint64_t)m > COND_MAX_ROW_BYTES / per_coord)
        return fail(PDMP_ERR_INVALID, "%s: m = %lld rows of %llu bytes exceed the %llu GiB a condition may reserve", who, (long long)m,
                    (unsigned long long)per_coord, (unsigned long long)(COND_MAX_ROW_BYTES >> 30));
    if (!coords || !lo || !hi) return fail(PDMP_ERR_INVALID, "%s: null list", who);
    if (m > d) return fail(PDMP_ERR_INVALID, "%s: m = %lld coordinates of %lld: one of them is listed twice", who, (long long)m, (long long)d);
    vc->resize((size_t)m), vlo->resize((size_t)m), vhi->resize((size_t)m), vw->resize((size_t)m);
    std::vector<char> seen((size_t)d, 0);
    for (int64_t s = 0; s < m; ++s) {
        if (coords[s] < 0 || coords[s] >= d)
            return fail(PDMP_ERR_INVALID, "%s: coordinate %lld = %lld is outside [0, %lld)", who, (long long)s, (long long)coords[s], (long long)d);
        if (seen[(size_t)coords[s]]) return fail(PDMP_ERR_INVALID, "%s: the coordinate %lld is listed twice", who, (long long)coords[s]);
        seen[(size_t)coords[s]] = 1;
        const double w = (hi[s] - lo[s]) / (double)bins;
        if (!std::isfinite(lo[s]) || !std::isfinite(hi[s]) || !(lo[s] < hi[s]) || !std::isfinite(w) || !(w > 0))
            return fail(PDMP_ERR_INVALID, "%s: the range of entry %lld must be finite with lo < hi (and a finite positive bin width)", who, (long long)s);
        (*vc)[(size_t)s] = (int32_t)coords[s];
        (*vlo)[(size_t)s] = lo[s];
        (*vhi)[(size_t)s] = hi[s];
        (*vw)[(size_t)s] = w;
    }
    return PDMP_OK;
}

static pdmp::HistArgs hist_args(const pdmp_ensemble* e) {
    pdmp::HistArgs a{};
    a.slot_of = e->d_hs_slot.p;
    a.coords = e->d_hs_coords.p;
    a.lo = e->d_hs_lo.p;
    a.hi = e->d_hs_hi.p;
    a.w = e->d_hs_w.p;
    a.cur = e->d_hs_cur.p;
    a.meta = e->d_hs_meta.p;
    a.H = e->d_hs_H.p;
    a.m = e->hs_m;
    a.B = e->hs_B;
    return a;
}

static pdmp::PairArgs pair_args(const pdmp_ensemble* e) {
    pdmp::PairArgs a{};
    a.adj_ptr = e->d_pr_ptr.p;
    a.adj = e->d_pr_adj.p;
    a.pi = e->d_pr_pi.p;
    a.pj = e->d_pr_pj.p;
    a.center = e->d_pr_c.p;
    a.cur = e->d_pr_cur.p;
    a.meta = e->d_pr_meta.p;
    a.S = e->d_pr_S.p;
    a.npairs = e->pr_np;
    return a;
}

extern "C" {

pdmp_status pdmp_ensemble_batch_means(pdmp_ensemble* e, double T_prev, double T, double* sum_y, double* sum_y2) {
    PDMP_TRY(ess_ready(e));
    if (!(T > T_prev)) return fail(PDMP_ERR_INVALID, "T must exceed T_prev");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    const bool bps = e->cfg.sampler == PDMP_SAMPLER_BPS;
    if (bps) PDMP_TRY(bps_moments_at(e, T, 0, n, false));  // J1(T) of every chain into b_jT (the validity rule first)
    if (!bps) PDMP_TRY(fact_integrals_at(e, T));  // (before jprev is allocated or touched)
    if (e->d_jprev.n != (size_t)(n * d)) {
        PDMP_TRY(e->d_jprev.alloc((size_t)(n * d)));
        HIP_TRY(hipMemsetAsync(e->d_jprev.p, 0, (size_t)(n * d) * sizeof(double), e->stream));  // (same stream as the kernel: the ensemble's stream is non-blocking, the null stream does not order against it)
    }
    if (e->d_sum.n != (size_t)(2 * d)) PDMP_TRY(e->d_sum.alloc((size_t)(2 * d)));
    if (!bps) PDMP_TRY(ensure_canon(e));
    HIP_TRY(hipMemsetAsync(e->d_sum.p, 0, (size_t)(2 * d) * sizeof(double), e->stream));
    int rc = bps ? pdmp::launch_dense_batch_means(e->b_jT.p, e->d_jprev.p, d, n, T_prev, T, e->d_sum.p, e->d_sum.p + d, e->stream)
                 : pdmp::launch_zz_batch_means(e->d_rec.p, e->track ? 128 : 64, e->d_jprev.p, d, n, T_prev, T, e->d_sum.p, e->d_sum.p + d,
                                               e->stream);
    LAUNCH_TRY("batch_means", rc);
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (sum_y) HIP_TRY(hipMemcpy(sum_y, e->d_sum.p, (size_t)d * sizeof(double), hipMemcpyDeviceToHost));
    if (sum_y2) HIP_TRY(hipMemcpy(sum_y2, e->d_sum.p + d, (size_t)d * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_ess_begin(pdmp_ensemble* e, double T0) {
    PDMP_TRY(ess_ready(e));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    const bool bps = e->cfg.sampler == PDMP_SAMPLER_BPS;
    if (bps) PDMP_TRY(bps_moments_at(e, T0, 0, n, false));
    if (!bps) PDMP_TRY(fact_integrals_at(e, T0));
    if (e->d_jprev.n != (size_t)(n * d)) PDMP_TRY(e->d_jprev.alloc((size_t)(n * d)));
    if (e->d_jstart.n != (size_t)(n * d)) PDMP_TRY(e->d_jstart.alloc((size_t)(n * d)));
    if (e->d_essacc.n != (size_t)(4 * d)) PDMP_TRY(e->d_essacc.alloc((size_t)(4 * d)));
    if (!bps) PDMP_TRY(ensure_canon(e));
    HIP_TRY(hipMemsetAsync(e->d_essacc.p, 0, (size_t)(4 * d) * sizeof(double), e->stream));
    LAUNCH_TRY("ess", launch_ess(e, e->b_jT.p, 0, T0, T0));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->ess_T0 = e->ess_Tlast = T0;
    e->ess_batches = 0;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_ess_batch(pdmp_ensemble* e, double T) {
    PDMP_TRY(ess_ready(e));
    if (e->ess_batches < 0) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_ess_begin first");
    if (!(T > e->ess_Tlast)) return fail(PDMP_ERR_INVALID, "batch end %g does not exceed the previous one %g", T, e->ess_Tlast);
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    if (e->cfg.sampler == PDMP_SAMPLER_BPS) {
        PDMP_TRY(bps_moments_at(e, T, 0, e->cfg.nchains, false));
    } else {
        PDMP_TRY(fact_integrals_at(e, T));
        PDMP_TRY(ensure_canon(e));
    }
    LAUNCH_TRY("ess", launch_ess(e, e->b_jT.p, 1, e->ess_Tlast, T));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->ess_Tlast = T;
    e->ess_batches += 1;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_ess_end(pdmp_ensemble* e, double* sum_y, double* sum_y2, double* sum_m, double* sum_m2,
                                  int64_t* nbatches, double* T0, double* T1) {
    PDMP_TRY(ess_ready(e));
    if (e->ess_batches < 1) return fail(PDMP_ERR_INVALID, "no batch accumulated (ess_begin, then ess_batch)");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d;
    const bool bps = e->cfg.sampler == PDMP_SAMPLER_BPS;
    if (!bps) PDMP_TRY(ensure_canon(e));
    HIP_TRY(hipMemsetAsync(e->d_essacc.p + 2 * d, 0, (size_t)(2 * d) * sizeof(double), e->stream));
    // (BPS: J at the last batch end is the jprev that batch left -- the state may since have run past it)
    LAUNCH_TRY("ess", launch_ess(e, e->d_jprev.p, 2, e->ess_T0, e->ess_Tlast));
    HIP_TRY(hipStreamSynchronize(e->stream));
    double* outs[4] = {sum_y, sum_y2, sum_m, sum_m2};
    for (int k = 0; k < 4; ++k)
        if (outs[k]) HIP_TRY(hipMemcpy(outs[k], e->d_essacc.p + k * d, (size_t)d * sizeof(double), hipMemcpyDeviceToHost));
    if (nbatches) *nbatches = e->ess_batches;
    if (T0) *T0 = e->ess_T0;
    if (T1) *T1 = e->ess_Tlast;
    return PDMP_OK;
}

// consume_begin, barrier_consume_begin and refresh_consume_begin: one call order, one set of checks, one allocation; `barrier` adds the occupation
// state behind the cursors, `refresh` selects the unordered walk (a trace sorted within a coordinate only: DESIGN.md §20)
static pdmp_status consume_begin_impl(pdmp_ensemble* e, double grid_dt, int64_t grid_points, bool barrier, bool refresh = false) {
    if (!e->has_state || e->ran) return fail(PDMP_ERR_INVALID, "consume_begin follows set_state and precedes the first run (it snapshots x0, θ0)");
    if (refresh && (e->cfg.sampler == PDMP_SAMPLER_BARRIER_ZIGZAG || e->cfg.sampler == PDMP_SAMPLER_STICKY_ZIGZAG))
        return fail(PDMP_ERR_INVALID, "refresh_consume_begin: the ensemble is not a ZigZag with a refresh clock or a FactBoomerang (a barrier ensemble: "
                                      "pdmp_ensemble_barrier_consume_begin; a sticky one: pdmp_ensemble_consume_begin)");
    if (!barrier && e->cfg.sampler == PDMP_SAMPLER_BARRIER_ZIGZAG)
        return fail(PDMP_ERR_UNSUPPORTED, "the device consumers' time away from 0 has no meaning between barriers at other levels: "
                                          "pdmp_ensemble_barrier_consume_begin serves a barrier ensemble (occupation per barrier instead)");
    if (e->cfg.trace_capacity <= 0) return fail(PDMP_ERR_INVALID, "ensemble was created with trace_capacity = 0");
    if (refresh && e->flow_kind == 0 && !(e->lambda_ref > 0))
        return fail(PDMP_ERR_INVALID, "refresh_consume_begin: a ZigZag without refresh clock has a time-ordered trace: pdmp_ensemble_consume_begin serves it");
    if (!refresh && (e->flow_kind != 0 || e->lambda_ref > 0))
        return fail(PDMP_ERR_UNSUPPORTED, "the device consumers take time-ordered traces of piecewise-linear paths: ZigZag without refresh clock");
    if (grid_points < 0 || (grid_points > 0 && !(grid_dt > 0))) return fail(PDMP_ERR_INVALID, "grid_dt must be positive");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    e->cons_z = e->cfg.sampler == PDMP_SAMPLER_STICKY_ZIGZAG;  // (the time away from 0, inclusion_prob: a sum of its own where coordinates can freeze)
    e->cons_occ = barrier;
    e->cons_unordered = refresh;
    PDMP_TRY(e->d_ccur.alloc((size_t)(n * d) * (pdmp::consume_cursor_bytes(e->cons_z) + (barrier ? pdmp::consume_occ_bytes() : 0))));
    PDMP_TRY(e->d_cmeta.alloc((size_t)n * pdmp::consume_meta_bytes()));
    e->d_cgrid.release();
    if (grid_points > 0) {
        PDMP_TRY(e->d_cgrid.alloc((size_t)(n * grid_points * d)));
        HIP_TRY(hipMemsetAsync(e->d_cgrid.p, 0, (size_t)(n * grid_points * d) * sizeof(double), e->stream));
    }
    PDMP_TRY(ensure_canon(e));
    discard_async_consumer(e);
    e->cons_cummean = false;
    e->cn_on = e->cons_started = false;
    e->d_cn_cur.release(), e->d_cn_t.release(), e->d_cn_x.release(), e->d_cn_pn.release();
    e->d_cn_loc.release(), e->d_cn_idx.release(), e->d_cn_meta.release();
    e->pr_on = false;
    e->d_pr_ptr.release(), e->d_pr_pi.release(), e->d_pr_pj.release(), e->d_pr_adj.release(), e->d_pr_c.release(), e->d_pr_S.release();
    e->d_pr_out.release(), e->d_pr_cur.release(), e->d_pr_meta.release();
    e->hs_on = false;
    e->d_hs_slot.release(), e->d_hs_coords.release(), e->d_hs_lo.release(), e->d_hs_hi.release(), e->d_hs_w.release(), e->d_hs_H.release();
    e->d_hs_out.release(), e->d_hs_cur.release(), e->d_hs_meta.release();
    LAUNCH_TRY("consume_init", pdmp::launch_consume_init(e->d_rec.p, e->track ? 128 : 64, d, n, e->t0_state, e->d_ccur.p, e->cons_z, e->d_cmeta.p,
                                       grid_points > 0 ? e->d_cgrid.p : nullptr, grid_points, e->stream));
    if (barrier)  // (the records at t0 hold θ = 0 for a coordinate that starts frozen; d_thf holds every coordinate's θ0 as v_old)
        LAUNCH_TRY("barrier_occ_init", pdmp::launch_barrier_occ_init(e->d_thf.p, d, n, e->d_ccur.p, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->consuming = true;
    e->cons_dt = grid_dt;
    e->cons_K = grid_points;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_consume_begin(pdmp_ensemble* e, double grid_dt, int64_t grid_points) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    return consume_begin_impl(e, grid_dt, grid_points, false);
}

// The synchronous consumers of a barrier ensemble (stickyzz / sspdmp2): consume_begin plus the occupation state (DESIGN.md "Barrier occupation")
pdmp_status pdmp_ensemble_barrier_consume_begin(pdmp_ensemble* e, double grid_dt, int64_t grid_points) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BARRIER_ZIGZAG)
        return fail(PDMP_ERR_INVALID, "barrier_consume_begin: the ensemble is not a barrier ZigZag (PDMP_SAMPLER_BARRIER_ZIGZAG); pdmp_ensemble_consume_begin");
    return consume_begin_impl(e, grid_dt, grid_points, true);
}

// The synchronous consumers of a trace that is sorted within a coordinate only: a ZigZag with a refresh clock (λref > 0) or a FactBoomerang, whatever
// kernel samples it.  consume_begin itself keeps refusing these flows.
pdmp_status pdmp_ensemble_refresh_consume_begin(pdmp_ensemble* e, double grid_dt, int64_t grid_points) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    return consume_begin_impl(e, grid_dt, grid_points, false, true);
}

// what the consumers with a time-ordered cursor answer after refresh_consume_begin
static pdmp_status refuse_unordered(const char* who) {
    return fail(PDMP_ERR_UNSUPPORTED, "%s: after pdmp_ensemble_refresh_consume_begin the trace is sorted within a coordinate only (a refresh is recorded at "
                                      "the coordinate's own, stale clock); this consumer walks a time-ordered trace", who);
}

// time frozen at the lower / upper barrier [n x d] and hits of each [n x d] of chains [chain_first, chain_first + n), T_last [n]; any output may be NULL
pdmp_status pdmp_ensemble_barrier_consume_occupation(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* z_lo, double* z_hi, uint64_t* n_lo,
                                                     uint64_t* n_hi, double* T_last) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->consuming || !e->cons_occ) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_barrier_consume_begin first");
    if (chain_first < 0 || n <= 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "chain range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d;
    const size_t nd = (size_t)(n * d);
    DevBuf<double> bz, bt;
    DevBuf<uint64_t> bn;
    PDMP_TRY(bz.alloc(2 * nd));
    PDMP_TRY(bn.alloc(2 * nd));
    PDMP_TRY(bt.alloc((size_t)n));
    LAUNCH_TRY("barrier_occ_read", pdmp::launch_barrier_occ_read(d, e->cfg.nchains, chain_first, n, e->d_ccur.p, e->d_cmeta.p, bz.p, bz.p + nd, bn.p,
                                                                  bn.p + nd, bt.p, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (z_lo) HIP_TRY(hipMemcpy(z_lo, bz.p, nd * sizeof(double), hipMemcpyDeviceToHost));
    if (z_hi) HIP_TRY(hipMemcpy(z_hi, bz.p + nd, nd * sizeof(double), hipMemcpyDeviceToHost));
    if (n_lo) HIP_TRY(hipMemcpy(n_lo, bn.p, nd * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (n_hi) HIP_TRY(hipMemcpy(n_hi, bn.p + nd, nd * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (T_last) HIP_TRY(hipMemcpy(T_last, bt.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_consume(pdmp_ensemble* e) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->consuming || !e->has_state) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_consume_begin first");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    e->cons_started = true;
    if (e->cn_on)  // (cursors of its own: its place beside consume_events_kernel does not matter)
        LAUNCH_TRY("consume_condition", pdmp::launch_cond_events(e->d_ev.p, e->cfg.trace_capacity, e->d_hdr.p, e->cfg.d, e->cfg.nchains, e->d_cn_loc.p, e->d_cn_idx.p,
                                                                 e->cn_nS, e->d_cn_pn.p, e->d_cn_cur.p, e->d_cn_meta.p, e->d_cn_t.p, e->d_cn_x.p, e->cn_max_hits,
                                                                 e->stream));
    if (e->pr_on)  // (cursors of its own, like the condition's)
        LAUNCH_TRY("consume_pairs", pdmp::launch_pair_events(e->d_ev.p, e->cfg.trace_capacity, e->d_hdr.p, e->cfg.d, e->cfg.nchains, pair_args(e), e->stream));
    if (e->hs_on)  // (cursors of its own too)
        LAUNCH_TRY("consume_hist", pdmp::launch_hist_events(e->d_ev.p, e->cfg.trace_capacity, e->d_hdr.p, e->cfg.d, e->cfg.nchains, hist_args(e), e->stream));
    if (e->cons_unordered)
        LAUNCH_TRY("consume", pdmp::launch_consume_events_unordered(e->d_ev.p, e->cfg.trace_capacity, e->d_hdr.p, e->cfg.d, e->cfg.nchains, e->d_ccur.p, e->d_cmeta.p,
                                             e->d_cgrid.p, e->cons_K, e->t0_state, e->cons_dt, e->stream, e->cons_cummean ? e->d_ccm.p : nullptr,
                                             e->flow_kind == 1 ? e->d_mu.p : nullptr));
    else
        LAUNCH_TRY("consume", pdmp::launch_consume_events(e->d_ev.p, e->cfg.trace_capacity, e->d_hdr.p, nullptr, e->cfg.d, e->cfg.nchains, e->d_ccur.p, e->cons_z, e->d_cmeta.p,
                                             e->d_cgrid.p, e->cons_K, e->t0_state, e->cons_dt, e->stream, e->cons_cummean ? e->d_ccm.p : nullptr, e->cons_occ));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return PDMP_OK;
}

// cummean(Ξ) on the device (src/trace.jl:203-226): with it enabled, pdmp_ensemble_consume also leaves, for every event of the segment it consumes, the
// running pair (t_i, Σ (x_prev + x_k)(t_k − t_prev) / (2 t_i)) of the event's coordinate -- the cursors carry the sums from segment to segment, so the
// pairs are those of the whole run's trace.  Enable after consume_begin (the synchronous consumer only).
pdmp_status pdmp_ensemble_consume_cummean(pdmp_ensemble* e, int enable) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->consuming) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_consume_begin first");
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (enable) {
        const size_t n = (size_t)e->cfg.nchains * (size_t)e->cfg.trace_capacity * 2;
        if (e->d_ccm.n != n) PDMP_TRY(e->d_ccm.alloc(n));
    }
    e->cons_cummean = enable != 0;
    return PDMP_OK;
}
// ... the pairs of slots [first, first + count) of `chain`'s segment (the same slots pdmp_ensemble_trace_copy returns the events of)
pdmp_status pdmp_ensemble_consume_cummean_copy(pdmp_ensemble* e, int64_t chain, int64_t first, int64_t count, double* t_out, double* y_out) {
    if (!e || !t_out || !y_out) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->cons_cummean) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_consume_cummean(ens, 1) first");
    if (chain < 0 || chain >= e->cfg.nchains || first < 0 || count < 0 || first + count > e->cfg.trace_capacity) return fail(PDMP_ERR_INVALID, "range out of bounds");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    std::vector<double> pairs((size_t)count * 2);
    if (count) HIP_TRY(hipMemcpy(pairs.data(), e->d_ccm.p + 2 * (chain * e->cfg.trace_capacity + first), (size_t)count * 2 * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < count; ++k) {
        t_out[k] = pairs[(size_t)(2 * k)];
        y_out[k] = pairs[(size_t)(2 * k + 1)];
    }
    return PDMP_OK;
}

// subtrace(Ξ, J) on the device (src/trace.jl:275-290): the events of `chain`'s current segment whose coordinate lies in the ascending index set J,
// renumbered by their position in J, compacted by a kernel and copied out (n_out: how many there are; at most out_cap are written)
pdmp_status pdmp_ensemble_subtrace_copy(pdmp_ensemble* e, int64_t chain, const int64_t* J, int64_t nJ, pdmp_event* out, int64_t out_cap, int64_t* n_out) {
    if (!e || !J || !n_out || (out_cap > 0 && !out)) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (e->cfg.trace_capacity <= 0) return fail(PDMP_ERR_INVALID, "ensemble was created with trace_capacity = 0");
    if (chain < 0 || chain >= e->cfg.nchains || nJ < 0 || out_cap < 0) return fail(PDMP_ERR_INVALID, "bad argument");
    const int64_t d = e->cfg.d;
    std::vector<int32_t> loc((size_t)d, -1);
    for (int64_t k = 0; k < nJ; ++k) {
        if (J[k] < 0 || J[k] >= d || (k > 0 && J[k] <= J[k - 1])) return fail(PDMP_ERR_INVALID, "J must be ascending coordinates in [0, d) (@assert issorted(J), src/trace.jl:276)");
        loc[(size_t)J[k]] = (int32_t)k;
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    pdmp::DevChain h;
    HIP_TRY(hipMemcpy(&h, e->d_hdr.p + chain, sizeof h, hipMemcpyDeviceToHost));
    const int64_t n = (int64_t)std::min<uint64_t>(h.c.ntrace, (uint64_t)e->cfg.trace_capacity);
    DevBuf<int32_t> dloc;
    DevBuf<pdmp_event> dout;
    DevBuf<unsigned long long> dn;
    PDMP_TRY(dloc.upload(loc));
    PDMP_TRY(dout.alloc((size_t)std::max<int64_t>(out_cap, 1)));
    PDMP_TRY(dn.alloc(1));
    LAUNCH_TRY("trace_subtrace", pdmp::launch_trace_subtrace(e->d_ev.p + chain * e->cfg.trace_capacity, n, dloc.p, dout.p, out_cap, dn.p, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    unsigned long long cnt = 0;
    HIP_TRY(hipMemcpy(&cnt, dn.p, sizeof cnt, hipMemcpyDeviceToHost));
    *n_out = (int64_t)cnt;
    const int64_t ncopy = std::min<int64_t>((int64_t)cnt, out_cap);
    if (ncopy > 0) HIP_TRY(hipMemcpy(out, dout.p, (size_t)ncopy * sizeof(pdmp_event), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

// The consumer beside the sampler: what the last launch wrote is handed to the consumers on a SECOND stream, and the segments come back empty at
// once -- the next pdmp_ensemble_run writes the other of two trace buffers while this slice is consumed (a C3 slice is 1.7 GB of events: at the
// sampler's rate the host could not drain it over PCIe; src/sfact.jl:211 returns Ξ, and discretize / mean are what every caller does with it next,
// src/trace.jl:106-125,182-200).  Stream order: [run k] -> snapshot of the per-chain counts + reset (run stream) -> consumer k (second stream,
// after the snapshot); run k + 1 waits for consumer k − 1, which read the buffer it is about to write.  Returns without waiting.
pdmp_status pdmp_ensemble_consume_async(pdmp_ensemble* e, void* stream) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->consuming || !e->has_state) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_consume_begin first");
    if (e->cons_unordered) return refuse_unordered("consume_async");
    if (e->cons_occ)
        return fail(PDMP_ERR_UNSUPPORTED, "consume_async: a barrier ensemble (pdmp_ensemble_barrier_consume_begin) is served by the synchronous consumer, "
                                          "pdmp_ensemble_consume");
    if (e->cn_on)
        return fail(PDMP_ERR_UNSUPPORTED, "consume_async: the conditional trace (pdmp_ensemble_consume_condition) is served by the synchronous consumer, "
                                          "pdmp_ensemble_consume");
    if (e->pr_on)
        return fail(PDMP_ERR_UNSUPPORTED, "consume_async: the pair integrals (pdmp_ensemble_consume_pairs) are served by the synchronous consumer, "
                                          "pdmp_ensemble_consume");
    if (e->hs_on)
        return fail(PDMP_ERR_UNSUPPORTED, "consume_async: the marginal histograms (pdmp_ensemble_consume_hist) are served by the synchronous consumer, "
                                          "pdmp_ensemble_consume");
    HIP_TRY(hipSetDevice(e->cfg.device));
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    const int64_t n = e->cfg.nchains;
    PDMP_TRY(launch_deferred_consumer(e));  // (two calls without a run between them)
    if (!e->stream2) {
        // created into locals and committed to the ensemble together: a failure half-way leaves nothing behind that a later call would trust
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        hipStream_t s2 = nullptr;
        hipEvent_t evs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        hipError_t err = hipStreamCreateWithPriority(&s2, hipStreamNonBlocking, least);  // (the event loop's launches go first)
        for (int q = 0; q < 5 && err == hipSuccess; ++q) err = hipEventCreate(&evs[q]);
        if (err != hipSuccess) {
            for (hipEvent_t ev : evs)
                if (ev) (void)hipEventDestroy(ev);
            if (s2) (void)hipStreamDestroy(s2);
            return fail(PDMP_ERR_HIP, "consume_async: stream / event creation failed: %s", hipGetErrorString(err));
        }
        e->stream2 = s2;
        e->ev_run_done = evs[0];
        e->ev_cons_done[0] = evs[1];
        e->ev_cons_done[1] = evs[2];
        e->ev_c0 = evs[3];
        e->ev_c1 = evs[4];
    }
    if (e->d_ev2.n != e->d_ev.n) PDMP_TRY(e->d_ev2.alloc(e->d_ev.n));
    const int k = e->async_k;
    if (e->d_snap[k].n != (size_t)(2 * n)) PDMP_TRY(e->d_snap[k].alloc((size_t)(2 * n)));
    LAUNCH_TRY("consume_snapshot", pdmp::launch_consume_snapshot(e->d_hdr.p, n, e->d_snap[k].p, s));
    HIP_TRY(hipEventRecord(e->ev_run_done, s));
    pdmp_event* const filled = e->d_ev.p;
    std::swap(e->d_ev.p, e->d_ev2.p);  // (same sizes) the next launch writes the other buffer ...
    if (e->cons_pending[k ^ 1]) HIP_TRY(hipStreamWaitEvent(s, e->ev_cons_done[k ^ 1], 0));  // ... once the consumer that read it is done
    HIP_TRY(hipStreamWaitEvent(e->stream2, e->ev_run_done, 0));
    e->deferred_buf = filled;
    e->deferred_k = k;  // (launched behind the next event-loop launch: launch_deferred_consumer)
    // An ensemble that fills the device is bound by the memory system, and a consumer beside it costs it more than the consumer's own time
    // (measured on C3, 4096 chains: 39 -> 56 ms per slice beside a 7 ms consumer): there the consumer runs BETWEEN the slices -- the next launch
    // waits for it -- and the second trace buffer only saves the reset.  Narrower ensembles leave SIMDs idle: the consumer runs beside the next slice.
    const bool beside = e->dbg_cons_overlap == 1 || (e->dbg_cons_overlap == -1 && e->cfg.nchains <= 2048);
    if (!beside) {
        PDMP_TRY(launch_deferred_consumer(e));
        HIP_TRY(hipStreamWaitEvent(s, e->ev_cons_done[k], 0));
    }
    e->async_k = k ^ 1;
    e->cons_started = true;  // (the slice is handed to the consumer: a condition can no longer start from t0)
    return PDMP_OK;
}

// kernel time of the last asynchronous consumer (waits for it)
pdmp_status pdmp_ensemble_last_consume_ms(pdmp_ensemble* e, float* ms) {
    if (!e || !ms) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->cons_timed && e->deferred_k < 0) return fail(PDMP_ERR_INVALID, "no asynchronous consumer has run");
    HIP_TRY(hipSetDevice(e->cfg.device));
    PDMP_TRY(launch_deferred_consumer(e));
    return elapsed_ms(e->ev_c0, e->ev_c1, ms);
}

pdmp_status pdmp_ensemble_consume_mean(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* mean, double* T_last) {
    return consume_reduce(e, chain_first, n, mean, T_last, "consume_mean", [&](double* bm, double* bt) {
        return pdmp::launch_consume_mean(e->cfg.d, chain_first, n, e->d_ccur.p, e->d_cmeta.p, bm, bt, e->stream);
    });
}

pdmp_status pdmp_ensemble_consume_inclusion(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* prob, double* T_last) {
    if (e && e->consuming && e->cons_occ)
        return fail(PDMP_ERR_UNSUPPORTED, "consume_inclusion: the time away from 0 has no meaning between barriers at other levels: "
                                          "pdmp_ensemble_barrier_consume_occupation returns the time frozen at each barrier (1 − z/T)");
    if (e && e->consuming && e->cons_unordered) return refuse_unordered("consume_inclusion");
    return consume_reduce(e, chain_first, n, prob, T_last, "consume_inclusion", [&](double* bm, double* bt) {
        return pdmp::launch_consume_inclusion(e->cfg.d, e->cfg.nchains, e->cons_z, e->t0_state, chain_first, n, e->d_ccur.p, e->d_cmeta.p, bm, bt, e->stream);
    });
}

pdmp_status pdmp_ensemble_consume_discretized(pdmp_ensemble* e, int64_t chain, int64_t k_first, int64_t k_count, double* out, int64_t* npoints,
                                              void** grid_dev) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->consuming || e->cons_K <= 0) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_consume_begin with a grid first");
    if (chain < 0 || chain >= e->cfg.nchains || k_first < 0 || k_count < 0 || k_first + k_count > e->cons_K)
        return fail(PDMP_ERR_INVALID, "chain / grid range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));  // (asynchronous consumers run on a second stream)
    const int64_t d = e->cfg.d;
    // the points after every coordinate's last event, up to the chain's last event time (idempotent); not for an unordered trace, whose rows are
    // exactly the ones the walk wrote (the cursors behind a stale event are not the state the reference shows at an earlier row)
    if (!e->cons_unordered) {
        LAUNCH_TRY("consume_flush", pdmp::launch_consume_flush(d, e->cfg.nchains, e->d_ccur.p, e->d_cmeta.p, e->d_cgrid.p, e->cons_K, e->t0_state, e->cons_dt, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    if (out && k_count)
        HIP_TRY(hipMemcpy(out, e->d_cgrid.p + (chain * e->cons_K + k_first) * d, (size_t)(k_count * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (npoints) {
        // collect(discretize(Ξ, dt)) emits a grid time while it lies before the last event (src/trace.jl:111-113); at least t0 itself
        std::vector<unsigned char> mh(pdmp::consume_meta_bytes());
        HIP_TRY(hipMemcpy(mh.data(), e->d_cmeta.p + (size_t)chain * pdmp::consume_meta_bytes(), mh.size(), hipMemcpyDeviceToHost));
        double tl;  // { consumed, t_last, row_next, t_max }: an unordered trace's grid extends to the running maximum of its event times
        memcpy(&tl, mh.data() + (e->cons_unordered ? 24 : 8), sizeof tl);
        // NOT clamped to the grid: a value above grid_points tells the caller that the grid was too short for the run (rows beyond it do not exist)
        int64_t np = (int64_t)floor((tl - e->t0_state) / e->cons_dt);
        np = np > 1 ? np - 1 : 0;
        while (e->t0_state + e->cons_dt * (double)np < tl) ++np;
        *npoints = np > 0 ? np : 1;
    }
    if (grid_dev) *grid_dev = e->d_cgrid.p;
    return PDMP_OK;
}

// conditional_trace(Ξ, (p, n)) on the device (src/condition.jl; DESIGN.md "Conditional trace"): after consume_begin and before the first consume
pdmp_status pdmp_ensemble_consume_condition(pdmp_ensemble* e, const double* p, const double* n, int64_t max_hits) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (e->flow_kind != 0)
        return fail(PDMP_ERR_UNSUPPORTED, "consume_condition: the hitting time of a hyperplane has no method for the Boomerang flows (src/condition.jl:18)");
    if (!e->consuming || !e->has_state) return fail(PDMP_ERR_INVALID, "consume_condition: pdmp_ensemble_consume_begin first");
    if (e->cons_unordered) return refuse_unordered("consume_condition");
    if (e->cons_started) return fail(PDMP_ERR_INVALID, "consume_condition precedes the first consume (its cursors start from t0, x0, θ0)");
    const int64_t d = e->cfg.d, nch = e->cfg.nchains;
    std::vector<int32_t> S;
    PDMP_TRY(condition_plane("consume_condition", d, p, n, max_hits, &S));
    PDMP_TRY(condition_rows_fit("consume_condition", nch, d, max_hits));
    if ((int64_t)S.size() > pdmp::COND_MAX_S)
        return fail(PDMP_ERR_UNSUPPORTED, "consume_condition: n has %zu non-zero entries, the device walks at most %d (condition the returned trace on the host)",
                    S.size(), pdmp::COND_MAX_S);
    std::vector<int32_t> loc((size_t)d, -1);
    std::vector<double> pn(2 * S.size());
    for (size_t k = 0; k < S.size(); ++k) {
        loc[(size_t)S[k]] = (int32_t)k;
        pn[k] = p[S[k]];
        pn[S.size() + k] = n[S[k]];
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    e->cn_on = false;
    PDMP_TRY(e->d_cn_loc.upload(loc));
    PDMP_TRY(e->d_cn_idx.upload(S));
    PDMP_TRY(e->d_cn_pn.upload(pn));
    PDMP_TRY(e->d_cn_cur.alloc((size_t)(3 * nch * d)));
    PDMP_TRY(e->d_cn_meta.alloc((size_t)nch * pdmp::cond_meta_bytes()));
    PDMP_TRY(e->d_cn_t.alloc((size_t)(nch * max_hits)));
    PDMP_TRY(e->d_cn_x.alloc((size_t)(nch * max_hits) * (size_t)d));
    HIP_TRY(hipMemsetAsync(e->d_cn_t.p, 0, (size_t)(nch * max_hits) * sizeof(double), e->stream));
    HIP_TRY(hipMemsetAsync(e->d_cn_x.p, 0, (size_t)(nch * max_hits) * (size_t)d * sizeof(double), e->stream));
    LAUNCH_TRY("consume_condition_init", pdmp::launch_cond_init(e->d_ccur.p, d, nch, e->t0_state, e->d_cn_cur.p, e->d_cn_meta.p, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->cn_nS = (int)S.size();
    e->cn_max_hits = max_hits;
    e->cn_on = true;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_consume_conditioned(pdmp_ensemble* e, int64_t chain, int64_t first, int64_t count, double* t, double* x, int64_t* nhits,
                                              void** rows_dev) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->consuming || !e->cn_on) return fail(PDMP_ERR_INVALID, "consume_conditioned: pdmp_ensemble_consume_condition first");
    if (chain < 0 || chain >= e->cfg.nchains || first < 0 || count < 0 || first + count > e->cn_max_hits)
        return fail(PDMP_ERR_INVALID, "consume_conditioned: chain / row range (max_hits = %lld)", (long long)e->cn_max_hits);
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d, at = chain * e->cn_max_hits + first;
    if (t && count) HIP_TRY(hipMemcpy(t, e->d_cn_t.p + at, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    if (x && count) HIP_TRY(hipMemcpy(x, e->d_cn_x.p + at * d, (size_t)(count * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (nhits) {  // { consumed, t_b, nhits, done }: NOT clamped to max_hits -- a value above it means that later rows were dropped
        uint64_t nh;
        HIP_TRY(hipMemcpy(&nh, e->d_cn_meta.p + (size_t)chain * pdmp::cond_meta_bytes() + 16, sizeof nh, hipMemcpyDeviceToHost));
        *nhits = (int64_t)nh;
    }
    if (rows_dev) *rows_dev = e->d_cn_x.p;
    return PDMP_OK;
}

// pair integrals S_ij = ∫ (x_i − c_i)(x_j − c_j) dt, J_i = ∫ (x_i − c_i) dt on the device (DESIGN.md "Pair integrals"): after consume_begin and before the
// first consume
pdmp_status pdmp_ensemble_consume_pairs(pdmp_ensemble* e, int64_t npairs, const int64_t* pi, const int64_t* pj, const double* center) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->consuming || !e->has_state) return fail(PDMP_ERR_INVALID, "consume_pairs: pdmp_ensemble_consume_begin first");
    if (e->cons_unordered) return refuse_unordered("consume_pairs");
    if (e->cons_started) return fail(PDMP_ERR_INVALID, "consume_pairs precedes the first consume (its cursors start from t0, x0, θ0)");
    const int64_t d = e->cfg.d, nch = e->cfg.nchains;
    std::vector<int32_t> vi, vj;
    std::vector<double> c;
    PDMP_TRY(pairs_list("consume_pairs", nch, d, npairs, pi, pj, center, &vi, &vj, &c));
    // coordinate -> (partner, slot): every pair under both of its coordinates, (i, i) once; a row keeps the order of the list
    std::vector<int32_t> ptr((size_t)d + 1, 0);
    for (int64_t k = 0; k < npairs; ++k) {
        ptr[(size_t)vi[k] + 1] += 1;
        if (vj[k] != vi[k]) ptr[(size_t)vj[k] + 1] += 1;
    }
    for (int64_t j = 0; j < d; ++j) ptr[(size_t)j + 1] += ptr[(size_t)j];
    std::vector<pdmp::PairAdj> adj((size_t)ptr[(size_t)d]);
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (int64_t k = 0; k < npairs; ++k) {
        adj[(size_t)fill[(size_t)vi[k]]++] = pdmp::PairAdj{vj[k], (int32_t)k};
        if (vj[k] != vi[k]) adj[(size_t)fill[(size_t)vj[k]]++] = pdmp::PairAdj{vi[k], (int32_t)k};
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    e->pr_on = false;
    PDMP_TRY(e->d_pr_ptr.upload(ptr));
    PDMP_TRY(e->d_pr_adj.upload(adj));
    PDMP_TRY(e->d_pr_pi.upload(vi));
    PDMP_TRY(e->d_pr_pj.upload(vj));
    PDMP_TRY(e->d_pr_c.upload(c));
    PDMP_TRY(e->d_pr_cur.alloc((size_t)(nch * d) * pdmp::pair_cursor_bytes()));
    PDMP_TRY(e->d_pr_meta.alloc((size_t)nch * pdmp::pair_meta_bytes()));
    PDMP_TRY(e->d_pr_S.alloc((size_t)(nch * npairs)));
    e->d_pr_out.release();
    e->pr_np = npairs;
    HIP_TRY(hipMemsetAsync(e->d_pr_S.p, 0, (size_t)(nch * npairs) * sizeof(double), e->stream));
    LAUNCH_TRY("consume_pairs_init", pdmp::launch_pair_init(e->d_ccur.p, d, nch, e->t0_state, pair_args(e), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->pr_on = true;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_consume_pair_integrals(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* S, double* J, double* T_last, void** S_dev) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->consuming || !e->pr_on) return fail(PDMP_ERR_INVALID, "consume_pair_integrals: pdmp_ensemble_consume_pairs first");
    if (chain_first < 0 || n < 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "consume_pair_integrals: chain range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d, np = e->pr_np;
    const size_t need = (size_t)(n * (np + d + 1));
    if (e->d_pr_out.n < need) PDMP_TRY(e->d_pr_out.alloc(need));
    if (S_dev) *S_dev = e->d_pr_out.p;
    if (n == 0) return PDMP_OK;
    double *oS = e->d_pr_out.p, *oJ = oS + n * np, *oT = oJ + n * d;
    LAUNCH_TRY("consume_pair_integrals", pdmp::launch_pair_read(d, pair_args(e), chain_first, n, oS, oJ, oT, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (S) HIP_TRY(hipMemcpy(S, oS, (size_t)(n * np) * sizeof(double), hipMemcpyDeviceToHost));
    if (J) HIP_TRY(hipMemcpy(J, oJ, (size_t)(n * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (T_last) HIP_TRY(hipMemcpy(T_last, oT, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

// marginal histograms on the device: the time each listed coordinate spends in each bin of its own range (DESIGN.md "Marginal histograms"): after
// consume_begin / barrier_consume_begin and before the first consume
pdmp_status pdmp_ensemble_consume_hist(pdmp_ensemble* e, int64_t m, const int64_t* coords, const double* lo, const double* hi, int64_t bins) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->consuming || !e->has_state) return fail(PDMP_ERR_INVALID, "consume_hist: pdmp_ensemble_consume_begin first");
    if (e->cons_unordered) return refuse_unordered("consume_hist");
    if (e->cons_started) return fail(PDMP_ERR_INVALID, "consume_hist precedes the first consume (its cursors start from t0, x0, θ0)");
    const int64_t d = e->cfg.d, nch = e->cfg.nchains;
    std::vector<int32_t> vc;
    std::vector<double> vlo, vhi, vw;
    PDMP_TRY(hist_list("consume_hist", nch, d, m, coords, lo, hi, bins, &vc, &vlo, &vhi, &vw));
    std::vector<int32_t> slot((size_t)d, -1);
    for (int64_t s = 0; s < m; ++s) slot[(size_t)vc[(size_t)s]] = (int32_t)s;
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    e->hs_on = false;
    PDMP_TRY(e->d_hs_slot.upload(slot));
    PDMP_TRY(e->d_hs_coords.upload(vc));
    PDMP_TRY(e->d_hs_lo.upload(vlo));
    PDMP_TRY(e->d_hs_hi.upload(vhi));
    PDMP_TRY(e->d_hs_w.upload(vw));
    PDMP_TRY(e->d_hs_cur.alloc((size_t)(nch * m) * pdmp::hist_cursor_bytes()));
    PDMP_TRY(e->d_hs_meta.alloc((size_t)nch * pdmp::hist_meta_bytes()));
    PDMP_TRY(e->d_hs_H.alloc((size_t)(nch * m * (bins + 2))));
    e->d_hs_out.release();
    e->hs_m = m;
    e->hs_B = (int32_t)bins;
    HIP_TRY(hipMemsetAsync(e->d_hs_H.p, 0, (size_t)(nch * m * (bins + 2)) * sizeof(double), e->stream));
    LAUNCH_TRY("consume_hist_init", pdmp::launch_hist_init(e->d_ccur.p, d, nch, e->t0_state, hist_args(e), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->hs_on = true;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_consume_histogram(pdmp_ensemble* e, int64_t chain_first, int64_t n, int pooled, double* H, double* Z, double* T_last,
                                            void** H_dev) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->consuming || !e->hs_on) return fail(PDMP_ERR_INVALID, "consume_histogram: pdmp_ensemble_consume_hist first");
    if (chain_first < 0 || n < 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "consume_histogram: chain range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t rows = (pooled ? 1 : n) * e->hs_m, len = rows * (e->hs_B + 2);
    const size_t need = (size_t)(len + rows + n);
    if (e->d_hs_out.n < need) PDMP_TRY(e->d_hs_out.alloc(need));
    if (H_dev) *H_dev = e->d_hs_out.p;
    if (n == 0) return PDMP_OK;
    double *oH = e->d_hs_out.p, *oZ = oH + len, *oT = oZ + rows;
    LAUNCH_TRY("consume_histogram", pdmp::launch_hist_read(hist_args(e), chain_first, n, pooled != 0, oH, oZ, oT, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (H) HIP_TRY(hipMemcpy(H, oH, (size_t)len * sizeof(double), hipMemcpyDeviceToHost));
    if (Z) HIP_TRY(hipMemcpy(Z, oZ, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost));
    if (T_last) HIP_TRY(hipMemcpy(T_last, oT, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_path_integrals(pdmp_ensemble* e, int enable) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    e->keep_integrals = enable != 0;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_path_integrals(pdmp_ensemble* e, double T, int64_t nprobe, const int64_t* probes, double* out) {
    PDMP_TRY(ess_ready(e));
    if (!probes || !out || nprobe <= 0) return fail(PDMP_ERR_INVALID, "bad argument");
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    for (int64_t k = 0; k < nprobe; ++k)
        if (probes[k] < 0 || probes[k] >= d) return fail(PDMP_ERR_INVALID, "probe coordinate %lld out of range", (long long)probes[k]);
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    DevBuf<int64_t> dp;
    DevBuf<double> dout;
    PDMP_TRY(dp.upload(std::vector<int64_t>(probes, probes + nprobe)));
    PDMP_TRY(dout.alloc((size_t)(n * nprobe)));
    int rc;
    if (e->cfg.sampler == PDMP_SAMPLER_BPS) {
        PDMP_TRY(bps_moments_at(e, T, 0, n, false));
        rc = pdmp::launch_dense_gather(e->b_jT.p, d, n, dp.p, nprobe, dout.p, e->stream);
    } else {
        PDMP_TRY(fact_integrals_at(e, T));
        PDMP_TRY(ensure_canon(e));
        rc = pdmp::launch_zz_path_integrals(e->d_rec.p, e->track ? 128 : 64, d, n, dp.p, nprobe, T, dout.p, e->stream);
    }
    LAUNCH_TRY("path_integrals", rc);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out, dout.p, (size_t)(n * nprobe) * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}
}  // extern "C"
