// pdmp_capi_consume_bps.hip -- the trace consumers of the Bouncy Particle family (pdmp_ensemble_bps_consume_*): host side of pdmp_consume_bps.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pdmp_ensemble.hpp"

static pdmp_status need_bps(const pdmp_ensemble* e, const char* who) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS)
        return fail(PDMP_ERR_INVALID, "%s: the ensemble was not created with PDMP_SAMPLER_BPS (the factorised samplers use pdmp_ensemble_consume_*)", who);
    return PDMP_OK;
}
static pdmp_status need_begun(const pdmp_ensemble* e, const char* who) {
    PDMP_TRY(need_bps(e, who));
    if (!e->bc_on || !e->has_state) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_bps_consume_begin first");
    return PDMP_OK;
}

// what the three kernels read and write, from the ensemble as it stands
static pdmp::BpsConsumeArgs consume_args(const pdmp_ensemble* e) {
    pdmp::BpsConsumeArgs a{};
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    a.ev_t = e->b_ev_t.p;
    a.ev_x = e->b_ev_x.p;
    a.ev_th = e->b_ev_th.p;
    a.ev_f = e->bps.sticky ? e->b_ev_f.p : nullptr;
    a.hdr = e->d_hdr.p;
    a.mu = e->bps.flow_kind == 1 ? e->b_mu_flow.p : nullptr;
    a.x0 = e->b_x.p;
    a.th0 = e->b_th.p;
    a.cx = e->bc_cur.p;
    a.cth = e->bc_cur.p + n * d;
    a.cy = e->bc_cur.p + 2 * n * d;
    a.cft = e->bps.sticky ? e->bc_cur.p + 3 * n * d : nullptr;
    a.meta = e->bc_meta.p;
    a.grid = e->bc_K > 0 ? e->bc_grid.p : nullptr;
    a.cm = e->bc_cummean ? e->bc_cm.p : nullptr;
    a.d = d;
    a.cap = e->cfg.trace_capacity;
    a.nchains = n;
    a.nstrips = (d + 63) / 64;
    a.K = e->bc_K;
    a.t0 = e->t0_state;
    a.dt = e->bc_dt;
    return a;
}

static pdmp::BpsCondArgs cond_args(const pdmp_ensemble* e) {
    pdmp::BpsCondArgs q{};
    q.p = e->bcn_pn.p;
    q.n = e->bcn_pn.p + e->cfg.d;
    q.tau = e->bcn_tau.p;
    q.hit_t = e->bcn_t.p;
    q.hit_x = e->bcn_x.p;
    q.nhits = e->bcn_nh.p;
    q.max_hits = e->bcn_max_hits;
    return q;
}

static pdmp::BpsPairArgs pair_args(const pdmp_ensemble* e) {
    pdmp::BpsPairArgs q{};
    q.pi = e->bpr_pi.p;
    q.pj = e->bpr_pj.p;
    q.center = e->bpr_c.p;
    q.S = e->bpr_S.p;
    q.J = e->bpr_J.p;
    q.npairs = e->bpr_np;
    return q;
}

static pdmp::BpsHistArgs hist_args(const pdmp_ensemble* e) {
    pdmp::BpsHistArgs q{};
    q.coords = e->bhs_coords.p;
    q.lo = e->bhs_lo.p;
    q.hi = e->bhs_hi.p;
    q.w = e->bhs_w.p;
    q.H = e->bhs_H.p;
    q.Z = e->bhs_Z.p;
    q.m = e->bhs_m;
    q.B = e->bhs_B;
    return q;
}

// bps_consume_mean / _inclusion: one [n x d] read of the cursors of chains [chain_first, chain_first + n) and the chains' last event times
static pdmp_status consume_read(pdmp_ensemble* e, int inclusion, int64_t chain_first, int64_t n, double* out, double* T_last, const char* who) {
    PDMP_TRY(need_begun(e, who));
    if (!out) return fail(PDMP_ERR_INVALID, "null argument");
    if (inclusion && !e->bps.sticky) return fail(PDMP_ERR_INVALID, "%s: the free masks are a sticky ensemble's (pdmp_ensemble_set_bps_sticky)", who);
    if (chain_first < 0 || n <= 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "chain range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d;
    DevBuf<double> bm, bt;
    PDMP_TRY(bm.alloc((size_t)(n * d)));
    PDMP_TRY(bt.alloc((size_t)n));
    LAUNCH_TRY(who, pdmp::launch_bps_consume_read(consume_args(e), inclusion, chain_first, n, bm.p, bt.p, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out, bm.p, (size_t)(n * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (T_last) HIP_TRY(hipMemcpy(T_last, bt.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

// what a consumer of the path between two records refuses, in the order its callers see: the line forms the Boomerang flows first, the arc forms
// the speed-recorded flow first; wrong_flow is the text behind "who: " where the flow's pieces are not the caller's
static pdmp_status need_corners(const pdmp_ensemble* e, const char* who, bool arc, const char* wrong_flow) {
    const bool boom = e->bps.flow_kind == 1;
    if (!arc && boom) return fail(PDMP_ERR_UNSUPPORTED, "%s: %s", who, wrong_flow);
    if (e->bps.modern)
        return fail(PDMP_ERR_UNSUPPORTED, "%s: the records of the speed-recorded flow are not the corners of the path%s", who,
                    arc ? "" : " (a straight line between two of them is not the path)");
    if (arc && !boom) return fail(PDMP_ERR_UNSUPPORTED, "%s: %s", who, wrong_flow);
    if (e->bps.subsample)
        return fail(PDMP_ERR_UNSUPPORTED, "%s: with subsample the records are not the corners of the path (%s between two of them is not the path)", who,
                    arc ? "an arc" : "a straight line");
    return PDMP_OK;
}

// bps_consume_pairs / _arc_pairs behind their refusals: the list, its accumulators and the flags.  The line form may be called again before the
// first bps_consume and replaces the list; the arc form keeps one list per bps_consume_begin.
static pdmp_status setup_pairs(pdmp_ensemble* e, const char* who, bool arc, int64_t npairs, const int64_t* pi, const int64_t* pj, const double* center) {
    PDMP_TRY(need_begun(e, who));
    if (e->bc_started) return fail(PDMP_ERR_INVALID, "%s precedes the first bps_consume (its first piece starts from t0, x0, θ0)", who);
    if (arc && e->bpr_on) return fail(PDMP_ERR_UNSUPPORTED, "%s: the ensemble already keeps a pair list (one list per bps_consume_begin)", who);
    const int64_t d = e->cfg.d, nch = e->cfg.nchains;
    std::vector<int32_t> vi, vj;
    std::vector<double> c;
    PDMP_TRY(pairs_list(who, nch, d, npairs, pi, pj, center, &vi, &vj, &c));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    e->bpr_on = false;
    PDMP_TRY(e->bpr_pi.upload(vi));
    PDMP_TRY(e->bpr_pj.upload(vj));
    PDMP_TRY(e->bpr_c.upload(c));
    PDMP_TRY(e->bpr_S.alloc((size_t)(nch * npairs)));
    PDMP_TRY(e->bpr_J.alloc((size_t)(nch * d)));
    PDMP_TRY(e->bpr_T.alloc((size_t)nch));
    HIP_TRY(hipMemsetAsync(e->bpr_S.p, 0, (size_t)(nch * npairs) * sizeof(double), e->stream));
    HIP_TRY(hipMemsetAsync(e->bpr_J.p, 0, (size_t)(nch * d) * sizeof(double), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->bpr_np = npairs;
    e->bpr_arc = arc;  // (bps_consume_begin cleared it, and a flow serves one of the two forms)
    e->bpr_on = true;
    return PDMP_OK;
}

// bps_consume_hist / _arc_hist behind their refusals, in the same way
static pdmp_status setup_hist(pdmp_ensemble* e, const char* who, bool arc, int64_t m, const int64_t* coords, const double* lo, const double* hi,
                              int64_t bins) {
    PDMP_TRY(need_begun(e, who));
    if (e->bc_started) return fail(PDMP_ERR_INVALID, "%s precedes the first bps_consume (its first piece starts from t0, x0, θ0)", who);
    if (arc && e->bhs_on) return fail(PDMP_ERR_UNSUPPORTED, "%s: the ensemble already keeps a histogram list (one list per bps_consume_begin)", who);
    const int64_t d = e->cfg.d, nch = e->cfg.nchains;
    std::vector<int32_t> vc;
    std::vector<double> vlo, vhi, vw;
    // The arc form: one wavefront per chain and listed coordinate, four to a workgroup of 256 threads: a launch holds fewer than 2^32 threads.
    // Refused before the lists are read, as hist_list refuses rows beyond 256 GiB (which stays its refusal: 2^35 doubles).
    if (arc && m > 0 && (double)nch * (double)((m + 3) / 4) >= 0x1.0p+24 && (double)nch * (double)m * (double)(bins + 2) <= 0x1.0p+35)
        return fail(PDMP_ERR_INVALID, "%s: nchains x m is beyond 2^26 wavefronts, more than one launch holds (list fewer coordinates per ensemble)", who);
    PDMP_TRY(hist_list(who, nch, d, m, coords, lo, hi, bins, &vc, &vlo, &vhi, &vw));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    e->bhs_on = false;
    PDMP_TRY(e->bhs_coords.upload(vc));
    PDMP_TRY(e->bhs_lo.upload(vlo));
    PDMP_TRY(e->bhs_hi.upload(vhi));
    PDMP_TRY(e->bhs_w.upload(vw));
    PDMP_TRY(e->bhs_H.alloc((size_t)(nch * m * (bins + 2))));
    PDMP_TRY(e->bhs_Z.alloc((size_t)(nch * m)));
    e->bhs_out.release();
    HIP_TRY(hipMemsetAsync(e->bhs_H.p, 0, (size_t)(nch * m * (bins + 2)) * sizeof(double), e->stream));
    HIP_TRY(hipMemsetAsync(e->bhs_Z.p, 0, (size_t)(nch * m) * sizeof(double), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->bhs_m = m;
    e->bhs_B = (int32_t)bins;
    e->bhs_arc = arc;
    e->bhs_on = true;
    return PDMP_OK;
}

extern "C" {

pdmp_status pdmp_ensemble_bps_consume_begin(pdmp_ensemble* e, double grid_dt, int64_t grid_points) {
    PDMP_TRY(need_bps(e, __func__));
    if (!e->has_state || e->ran)
        return fail(PDMP_ERR_INVALID, "bps_consume_begin follows set_state_bps and precedes the first run (it snapshots x0, θ0)");
    if (e->cfg.trace_capacity <= 0) return fail(PDMP_ERR_INVALID, "ensemble was created with trace_capacity = 0");
    if (grid_points < 0 || (grid_points > 0 && !(grid_dt > 0))) return fail(PDMP_ERR_INVALID, "grid_dt must be positive");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    PDMP_TRY(e->bc_cur.alloc((size_t)(n * d) * (e->bps.sticky ? 4 : 3)));
    PDMP_TRY(e->bc_meta.alloc((size_t)(n * ((d + 63) / 64)) * pdmp::bps_consume_meta_bytes()));
    e->bc_grid.release();
    e->bc_cm.release();
    if (grid_points > 0) {
        PDMP_TRY(e->bc_grid.alloc((size_t)(n * grid_points * d)));
        HIP_TRY(hipMemsetAsync(e->bc_grid.p, 0, (size_t)(n * grid_points * d) * sizeof(double), e->stream));
    }
    e->bc_cummean = false;
    e->bcn_on = e->bc_started = false;
    e->bcn_tau.release(), e->bcn_t.release(), e->bcn_x.release(), e->bcn_pn.release(), e->bcn_nh.release();
    e->bpr_on = e->bpr_arc = false;
    e->bpr_pi.release(),e->bpr_pj.release(), e->bpr_c.release(), e->bpr_S.release(), e->bpr_J.release(), e->bpr_T.release();
    e->bhs_on = e->bhs_arc = false;
    e->bhs_coords.release(), e->bhs_lo.release(), e->bhs_hi.release(), e->bhs_w.release(), e->bhs_H.release(), e->bhs_Z.release(), e->bhs_out.release();
    e->bc_dt = grid_dt;
    e->bc_K = grid_points;
    LAUNCH_TRY("bps_consume_init", pdmp::launch_bps_consume_init(consume_args(e), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->bc_on = true;
    return PDMP_OK;
}

// after EVERY run slice and before trace_reset.  The kernel is timed with HIP events: pdmp_ensemble_last_consume_ms reads them.
pdmp_status pdmp_ensemble_bps_consume(pdmp_ensemble* e) {
    PDMP_TRY(need_begun(e, __func__));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    if (!e->ev_c0) HIP_TRY(hipEventCreate(&e->ev_c0));
    if (!e->ev_c1) HIP_TRY(hipEventCreate(&e->ev_c1));
    e->bc_started = true;
    HIP_TRY(hipEventRecord(e->ev_c0, e->stream));
    if (e->bcn_on)  // (before the consumer: it reads the cursors and the progress the consumer is about to advance)
        LAUNCH_TRY("bps_consume_condition", pdmp::launch_bps_cond(consume_args(e), cond_args(e), e->stream));
    if (e->bpr_on)  // (before the consumer, like the condition: it reads the cursors and the progress the consumer is about to advance)
        LAUNCH_TRY(e->bpr_arc ? "bps_consume_arc_pairs" : "bps_consume_pairs", pdmp::launch_bps_pairs(consume_args(e), pair_args(e), e->bpr_arc, e->stream));
    if (e->bhs_on && e->bhs_arc)  // (before the consumer too, for the same reason)
        LAUNCH_TRY("bps_consume_arc_hist", pdmp::launch_bps_arc_hist(consume_args(e), hist_args(e), e->stream));
    else if (e->bhs_on)
        LAUNCH_TRY("bps_consume_hist", pdmp::launch_bps_hist(consume_args(e), hist_args(e), e->stream));
    LAUNCH_TRY("bps_consume", pdmp::launch_bps_consume_events(consume_args(e), e->stream));
    HIP_TRY(hipEventRecord(e->ev_c1, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->cons_timed = true;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_bps_consume_mean(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* mean, double* T_last) {
    return consume_read(e, 0, chain_first, n, mean, T_last, "bps_consume_mean");
}

pdmp_status pdmp_ensemble_bps_consume_inclusion(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* prob, double* T_last) {
    return consume_read(e, 1, chain_first, n, prob, T_last, "bps_consume_inclusion");
}

pdmp_status pdmp_ensemble_bps_consume_discretized(pdmp_ensemble* e, int64_t chain, int64_t k_first, int64_t k_count, double* out, int64_t* npoints,
                                                  void** grid_dev) {
    PDMP_TRY(need_begun(e, __func__));
    if (e->bc_K <= 0) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_bps_consume_begin with a grid first");
    if (chain < 0 || chain >= e->cfg.nchains || k_first < 0 || k_count < 0 || k_first + k_count > e->bc_K)
        return fail(PDMP_ERR_INVALID, "chain / grid range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d;
    if (out && k_count)
        HIP_TRY(hipMemcpy(out, e->bc_grid.p + (chain * e->bc_K + k_first) * d, (size_t)(k_count * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (npoints) {
        // the number of k with t0 + k·dt < T_last, at least 1 (row 0 is x0) and NOT clamped to the grid: a value above grid_points tells the caller
        // that the grid was too short for the run.  T_last of strip 0's copy of the chain's progress
        double tl;
        HIP_TRY(hipMemcpy(&tl, e->bc_meta.p + (size_t)(chain * ((d + 63) / 64)) * pdmp::bps_consume_meta_bytes() + pdmp::bps_consume_meta_tlast_offset(),
                          sizeof tl, hipMemcpyDeviceToHost));
        const double t0 = e->t0_state, dt = e->bc_dt, q = floor((tl - t0) / dt);
        if (q >= 0x1.0p+62) return fail(PDMP_ERR_INVALID, "bps_consume_discretized: (T_last - t0) / grid_dt = %g grid times do not fit an int64", q);
        int64_t np = q > 1.0 ? (int64_t)q - 1 : 0;
        while (t0 + (double)np * dt < tl) ++np;
        *npoints = np > 0 ? np : 1;
    }
    if (grid_dev) *grid_dev = e->bc_grid.p;
    return PDMP_OK;
}

// cummean(Ξ::PDMPTrace) (src/trace.jl:248-266): with it enabled, bps_consume also leaves y / (2 t) of every coordinate at the slot of every event of the
// segment it consumes; the cursors carry y from segment to segment, so the rows are those of the whole run's trace.  After bps_consume_begin.
pdmp_status pdmp_ensemble_bps_consume_cummean(pdmp_ensemble* e, int enable) {
    PDMP_TRY(need_begun(e, __func__));
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (enable) {
        const size_t n = (size_t)e->cfg.nchains * (size_t)e->cfg.trace_capacity * (size_t)e->cfg.d;
        if (e->bc_cm.n != n) PDMP_TRY(e->bc_cm.alloc(n));
    }
    e->bc_cummean = enable != 0;
    return PDMP_OK;
}
// ... rows [first, first + count) of `chain`'s segment, [count x d]: the slots pdmp_ensemble_bps_trace_copy returns the events of
pdmp_status pdmp_ensemble_bps_consume_cummean_copy(pdmp_ensemble* e, int64_t chain, int64_t first, int64_t count, double* y) {
    PDMP_TRY(need_begun(e, __func__));
    if (!e->bc_cummean) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_bps_consume_cummean(ens, 1) first");
    if (count > 0 && !y) return fail(PDMP_ERR_INVALID, "null argument");
    PDMP_TRY(check_trace_range(e, chain, first, count));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d;
    if (count) HIP_TRY(hipMemcpy(y, e->bc_cm.p + (chain * e->cfg.trace_capacity + first) * d, (size_t)(count * d) * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

// conditional_trace(Ξ::PDMPTrace, (p, n)) on the device (src/condition.jl:56-76; DESIGN.md "Conditional trace"): after bps_consume_begin and before the
// first bps_consume; from then on bps_consume also collects the hyperplane hits of every slice
pdmp_status pdmp_ensemble_bps_consume_condition(pdmp_ensemble* e, const double* p, const double* n, int64_t max_hits) {
    PDMP_TRY(need_bps(e, __func__));
    PDMP_TRY(need_corners(e, "bps_consume_condition", false, "the hitting time of a hyperplane has no method for the Boomerang flows (src/condition.jl:18)"));
    PDMP_TRY(need_begun(e, __func__));
    if (e->bc_started) return fail(PDMP_ERR_INVALID, "bps_consume_condition precedes the first bps_consume (its first segment starts from t0, x0, θ0)");
    const int64_t d = e->cfg.d, nch = e->cfg.nchains, cap = e->cfg.trace_capacity;
    std::vector<int32_t> S;
    PDMP_TRY(condition_plane("bps_consume_condition", d, p, n, max_hits, &S));
    PDMP_TRY(condition_rows_fit("bps_consume_condition", nch, d, max_hits));  // (no limit on |supp n|: a wavefront sums all d entries of a segment)
    std::vector<double> pn((size_t)(2 * d));
    std::copy(p, p + d, pn.begin());
    std::copy(n, n + d, pn.begin() + d);
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    e->bcn_on = false;
    PDMP_TRY(e->bcn_pn.upload(pn));
    PDMP_TRY(e->bcn_tau.alloc((size_t)(nch * cap)));
    PDMP_TRY(e->bcn_nh.alloc((size_t)nch));
    PDMP_TRY(e->bcn_t.alloc((size_t)(nch * max_hits)));
    PDMP_TRY(e->bcn_x.alloc((size_t)(nch * max_hits) * (size_t)d));
    HIP_TRY(hipMemsetAsync(e->bcn_nh.p, 0, (size_t)nch * sizeof(unsigned long long), e->stream));
    HIP_TRY(hipMemsetAsync(e->bcn_t.p, 0, (size_t)(nch * max_hits) * sizeof(double), e->stream));
    HIP_TRY(hipMemsetAsync(e->bcn_x.p, 0, (size_t)(nch * max_hits) * (size_t)d * sizeof(double), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->bcn_max_hits = max_hits;
    e->bcn_on = true;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_bps_consume_conditioned(pdmp_ensemble* e, int64_t chain, int64_t first, int64_t count, double* t, double* x, int64_t* nhits,
                                                  void** rows_dev) {
    PDMP_TRY(need_bps(e, __func__));
    if (!e->bc_on || !e->bcn_on) return fail(PDMP_ERR_INVALID, "bps_consume_conditioned: pdmp_ensemble_bps_consume_condition first");
    if (chain < 0 || chain >= e->cfg.nchains || first < 0 || count < 0 || first + count > e->bcn_max_hits)
        return fail(PDMP_ERR_INVALID, "bps_consume_conditioned: chain / row range (max_hits = %lld)", (long long)e->bcn_max_hits);
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d, at = chain * e->bcn_max_hits + first;
    if (t && count) HIP_TRY(hipMemcpy(t, e->bcn_t.p + at, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    if (x && count) HIP_TRY(hipMemcpy(x, e->bcn_x.p + at * d, (size_t)(count * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (nhits) {  // NOT clamped to max_hits: a value above it means that later rows were dropped
        unsigned long long nh;
        HIP_TRY(hipMemcpy(&nh, e->bcn_nh.p + chain, sizeof nh, hipMemcpyDeviceToHost));
        *nhits = (int64_t)nh;
    }
    if (rows_dev) *rows_dev = e->bcn_x.p;
    return PDMP_OK;
}

// pair integrals S_ij = ∫ (x_i − c_i)(x_j − c_j) dt, J_i = ∫ (x_i − c_i) dt of a PDMPTrace on the device (DESIGN.md "Pair integrals"): after bps_consume_begin
// and before the first bps_consume; from then on bps_consume also adds every slice's pieces
pdmp_status pdmp_ensemble_bps_consume_pairs(pdmp_ensemble* e, int64_t npairs, const int64_t* pi, const int64_t* pj, const double* center) {
    PDMP_TRY(need_bps(e, __func__));
    PDMP_TRY(need_corners(e, "bps_consume_pairs", false,
                          "on a Boomerang flow the product of two rotations is another integral than that of two lines "
                          "(pdmp_ensemble_bps_consume_arc_pairs keeps that one)"));
    return setup_pairs(e, "bps_consume_pairs", false, npairs, pi, pj, center);
}

// the same integrals on a Boomerang flow (DESIGN.md "Pair integrals of arcs"): between two events a coordinate is an arc about μ, a pair's piece a
// combination of five trigonometric integrals.  Same position, list and accumulators as bps_consume_pairs; bps_consume_pair_integrals reads them.
pdmp_status pdmp_ensemble_bps_consume_arc_pairs(pdmp_ensemble* e, int64_t npairs, const int64_t* pi, const int64_t* pj, const double* center) {
    PDMP_TRY(need_bps(e, __func__));
    PDMP_TRY(need_corners(e, "bps_consume_arc_pairs", true,
                          "the pieces of this flow are lines, not the arcs of a Boomerang (pdmp_ensemble_bps_consume_pairs keeps their integrals)"));
    return setup_pairs(e, "bps_consume_arc_pairs", true, npairs, pi, pj, center);
}

pdmp_status pdmp_ensemble_bps_consume_pair_integrals(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* S, double* J, double* T_last, void** S_dev) {
    PDMP_TRY(need_bps(e, __func__));
    if (!e->bc_on || !e->bpr_on) return fail(PDMP_ERR_INVALID, "bps_consume_pair_integrals: pdmp_ensemble_bps_consume_pairs first");
    if (chain_first < 0 || n < 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "bps_consume_pair_integrals: chain range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d, np = e->bpr_np;
    if (S_dev) *S_dev = e->bpr_S.p + chain_first * np;  // (nothing lies behind the last event: the accumulators are the integrals)
    if (n == 0) return PDMP_OK;
    if (S) HIP_TRY(hipMemcpy(S, e->bpr_S.p + chain_first * np, (size_t)(n * np) * sizeof(double), hipMemcpyDeviceToHost));
    if (J) HIP_TRY(hipMemcpy(J, e->bpr_J.p + chain_first * d, (size_t)(n * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (T_last) {
        LAUNCH_TRY("bps_consume_pair_integrals", pdmp::launch_bps_tlast(consume_args(e), chain_first, n, e->bpr_T.p, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipMemcpy(T_last, e->bpr_T.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    }
    return PDMP_OK;
}

// marginal histograms of a PDMPTrace on the device (DESIGN.md "Marginal histograms"): after bps_consume_begin and before the first bps_consume; from
// then on bps_consume also adds every slice's pieces
pdmp_status pdmp_ensemble_bps_consume_hist(pdmp_ensemble* e, int64_t m, const int64_t* coords, const double* lo, const double* hi, int64_t bins) {
    PDMP_TRY(need_bps(e, __func__));
    PDMP_TRY(need_corners(e, "bps_consume_hist", false,
                          "on a Boomerang flow a coordinate moves on an arc between two events, not on a line "
                          "(pdmp_ensemble_bps_consume_arc_hist keeps those histograms)"));
    return setup_hist(e, "bps_consume_hist", false, m, coords, lo, hi, bins);
}

// the same histograms on a Boomerang flow (DESIGN.md "Marginal histograms of arcs"): between two events a free coordinate is an arc about μ, and the
// time it spends below a level is a closed form in acos and atan2.  Same position, list, rows and rest times as bps_consume_hist;
// bps_consume_histogram reads them.
pdmp_status pdmp_ensemble_bps_consume_arc_hist(pdmp_ensemble* e, int64_t m, const int64_t* coords, const double* lo, const double* hi, int64_t bins) {
    PDMP_TRY(need_bps(e, __func__));
    PDMP_TRY(need_corners(e, "bps_consume_arc_hist", true,
                          "the pieces of this flow are lines, not the arcs of a Boomerang (pdmp_ensemble_bps_consume_hist keeps their histograms)"));
    return setup_hist(e, "bps_consume_arc_hist", true, m, coords, lo, hi, bins);
}

pdmp_status pdmp_ensemble_bps_consume_histogram(pdmp_ensemble* e, int64_t chain_first, int64_t n, int pooled, double* H, double* Z, double* T_last,
                                                void** H_dev) {
    PDMP_TRY(need_bps(e, __func__));
    if (!e->bc_on || !e->bhs_on) return fail(PDMP_ERR_INVALID, "bps_consume_histogram: pdmp_ensemble_bps_consume_hist first");
    if (chain_first < 0 || n < 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "bps_consume_histogram: chain range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t m = e->bhs_m, len = m * (e->bhs_B + 2);
    const size_t need = (size_t)(len + m + n);  // the pooled sums, T_last
    if (e->bhs_out.n < need) PDMP_TRY(e->bhs_out.alloc(need));
    double *oH = e->bhs_out.p, *oZ = oH + len, *oT = oZ + m;
    // (nothing lies behind the last event: a chain's rows are its result, and only the pooled read computes)
    const double *srcH = pooled ? oH : e->bhs_H.p + chain_first * len, *srcZ = pooled ? oZ : e->bhs_Z.p + chain_first * m;
    if (H_dev) *H_dev = const_cast<double*>(srcH);
    if (n == 0) return PDMP_OK;
    if (pooled && (H || Z || H_dev)) LAUNCH_TRY("bps_consume_histogram", pdmp::launch_bps_hist_pool(hist_args(e), chain_first, n, oH, oZ, e->stream));
    if (T_last) LAUNCH_TRY("bps_consume_histogram", pdmp::launch_bps_tlast(consume_args(e), chain_first, n, oT, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const int64_t rows = pooled ? 1 : n;
    if (H) HIP_TRY(hipMemcpy(H, srcH, (size_t)(rows * len) * sizeof(double), hipMemcpyDeviceToHost));
    if (Z) HIP_TRY(hipMemcpy(Z, srcZ, (size_t)(rows * m) * sizeof(double), hipMemcpyDeviceToHost));
    if (T_last) HIP_TRY(hipMemcpy(T_last, oT, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}
}  // extern "C"
