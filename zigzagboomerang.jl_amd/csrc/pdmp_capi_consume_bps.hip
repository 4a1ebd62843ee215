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
    HIP_TRY(hipEventRecord(e->ev_c0, e->stream));
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
        // that the grid was too short for the run.  Strip 0's copy of the chain's progress: { t_cur, t_last, ... }
        double tl;
        HIP_TRY(hipMemcpy(&tl, e->bc_meta.p + (size_t)(chain * ((d + 63) / 64)) * pdmp::bps_consume_meta_bytes() + sizeof(double), sizeof tl,
                          hipMemcpyDeviceToHost));
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
}  // extern "C"
