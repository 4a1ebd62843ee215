// pdmp_capi.hip -- implementation of the C ABI declared in include/pdmp_mi355.h.
//
// Host-side work only: argument checking, building the read-only "neighbourhood program" tables from the
// flow's CSC pattern (G1, G2 of src/sfact.jl:170-179), HBM allocation, kernel launches.  There is NO CPU
// fallback: without a gfx950 device every entry point that needs one fails with PDMP_ERR_NO_DEVICE.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "pdmp_ensemble.hpp"

namespace {
thread_local std::string g_err;
thread_local std::string g_deferred_err;  // the message of a deferred consumer launch that failed inside device_sync (kept through HIP_TRY)
}  // namespace

pdmp_status fail(pdmp_status st, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return st;
}
pdmp_status fail_hip(const char* expr, hipError_t err) {
    const std::string dm = g_deferred_err;
    g_deferred_err.clear();
    return fail(PDMP_ERR_HIP, "%s failed: %s%s%s", expr, hipGetErrorString(err), dm.empty() ? "" : " -- ", dm.c_str());
}
pdmp_status fail_launch(const char* launcher, int rc, bool hip_rc) {
    if (hip_rc) return fail(PDMP_ERR_HIP, "%s launch failed: %s", launcher, hipGetErrorString((hipError_t)rc));
    return fail(PDMP_ERR_HIP, "%s launch failed (%d)", launcher, rc);
}

// zz_local_trackp: ensembles of at most this many chains PER COMPUTE UNIT run the two-wave form (pdmp_trackp.hip).  Measured on C3 (profiles/r05_*):
// the helper wave pays as long as every chain is resident with room to spare -- 18.7 KB of LDS and 128 registers admit eight chains per CU; up to
// seven (1792 on the MI355X's 256 CUs) two waves win: 1536 chains 18.7 against 21.2 ms for one wave, 1792 chains 20.6 against 21.7, 1920 chains 23.1
// against 22.2.
#ifndef HELPER_WAVE_MAX_CHAINS_PER_CU
#define HELPER_WAVE_MAX_CHAINS_PER_CU 7
#endif
#define PDMP_LG_ROWS_DEFAULT 0  // chains per wavefront of the LDS-resident logistic kernel by default: 0 = one (pdmp_logistic.hip), 16 / 32 = rows (pdmp_logrows.hip)
#define PDMP_LG_FILL 0.95       // lanes of a 64-entry chunk a range fills on average (ranged sweep of long logistic rows; 0.6 .. 1.1 measured on C5)

// what each KernelFamily does with the phase profile and how its launcher's failure reads (pdmp_ensemble.hpp: FamilyInfo)
static const FamilyInfo FAMILY[] = {
    /* FAM_BPS           */ {0, "bps_run", false},
    /* FAM_GENERAL       */ {2, "zz_general_run", true},   // [0..6] = select, move G1, gradient, coin + G2, re-bound, re-queue, tail; [10] = proposals
    /* FAM_LOGISTIC_LDS  */ {2, "zz_general_run", true},
    /* FAM_LOGISTIC_ROWS */ {0, "zz_general_run", true},   // (zz_logistic_rows_supported: never chosen for a profiled run)
    /* FAM_TRACKL        */ {1, "zz_local_trackl", false},
    /* FAM_TRACKP        */ {1, "zz_local_trackp", false},
    /* FAM_TRACK_GROUPS  */ {1, "zz_local_track", false},
    /* FAM_EXACTP        */ {1, "zz_local_exactp", false},  // [10] iterations, [11] candidates, [12] left by the zone test, [13] committed, [14] events among the candidates
    /* FAM_STICKY_SPEC   */ {0, "zz_local_run", true},
    /* FAM_STICKY_RUN    */ {0, "zz_local_run", true},
    /* FAM_SPEC          */ {1, "zz_local_run", true},     // speculative kernels: [0..8] = cycles per phase, [10] = iterations
    /* FAM_ONE_EVENT     */ {0, "zz_local_run", true},
    /* FAM_BARRIER       */ {0, "zz_barrier_run", true},
    /* FAM_BRIDGE        */ {0, "zz_bridge_run", true},
    /* FAM_PRECISION     */ {0, "zz_precision_run", true},
};

pdmp_status launch_deferred_consumer(pdmp_ensemble* e) {
    if (e->deferred_k < 0) return PDMP_OK;
    const int k = e->deferred_k;
    e->deferred_k = -1;
    HIP_TRY(hipEventRecord(e->ev_c0, e->stream2));
    LAUNCH_TRY("consume", pdmp::launch_consume_events(e->deferred_buf, e->cfg.trace_capacity, e->d_hdr.p, e->d_snap[k].p, e->cfg.d, e->cfg.nchains, e->d_ccur.p,
                                         e->cons_z, e->d_cmeta.p, e->d_cgrid.p, e->cons_K, e->t0_state, e->cons_dt, e->stream2));
    HIP_TRY(hipEventRecord(e->ev_c1, e->stream2));
    HIP_TRY(hipEventRecord(e->ev_cons_done[k], e->stream2));
    e->cons_pending[k] = true;
    e->cons_timed = true;
    return PDMP_OK;
}
// A consumer that was deferred behind the next run, the pending flags and the buffer parity of pdmp_ensemble_consume_async are dropped (set_state,
// consume_begin: the cursors they would write are about to be re-initialised); whatever already runs on the consumer's stream is waited for
void discard_async_consumer(pdmp_ensemble* e) {
    e->deferred_k = -1;
    e->deferred_buf = nullptr;
    if (e->stream2) (void)hipStreamSynchronize(e->stream2);
    e->cons_pending[0] = e->cons_pending[1] = false;
    e->cons_timed = false;
    e->async_k = 0;
}
// hipDeviceSynchronize for an ensemble: a deferred consumer is launched first (what follows reads its results or the buffers it reads)
hipError_t device_sync(pdmp_ensemble* e) {
    if (e && e->deferred_k >= 0 && launch_deferred_consumer(e) != PDMP_OK) {
        // (the launch's own message is in g_err; HIP_TRY would overwrite it with "unknown error": keep it as the prefix of what follows)
        g_deferred_err = g_err;
        return hipErrorLaunchFailure;
    }
    return hipDeviceSynchronize();
}

// the records / pairs of pdmp_trackp.hip's layout from the lines (pdmp_trackl.hip), where a run has left them behind
pdmp_status ensure_canon(pdmp_ensemble* e) {
    if (!e->track_lines || !e->canon_stale) return PDMP_OK;
    HIP_TRY(device_sync(e));
    LAUNCH_TRY("trackl_unpack", pdmp::launch_zz_trackl_unpack(e->d_tl_lines.p, e->d_tl_cold.p, e->d_rec.p, e->d_kp.p, e->cfg.d, e->dk, e->cfg.nchains, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->canon_stale = false;
    return PDMP_OK;
}

// The one check of a CSC pattern handed over the C ABI: colptr starts at 0 and never decreases, every row index of the ncols columns lies in
// [0, d) and the rows of a column ascend strictly.  diag_leads: every column also begins with its diagonal entry (a lower-triangular factor).
pdmp_status check_csc(const char* what, const int64_t* colptr, const int64_t* rowval, int64_t d, int64_t ncols, bool diag_leads) {
    if (colptr[0] != 0) return fail(PDMP_ERR_INVALID, "%s: colptr[0] must be 0 (0-based CSC)", what);
    for (int64_t j = 0; j < ncols; ++j)
        if (colptr[j + 1] < colptr[j]) return fail(PDMP_ERR_INVALID, "%s: colptr decreases at column %lld", what, (long long)j);
    for (int64_t j = 0; j < ncols; ++j) {
        for (int64_t p = colptr[j]; p < colptr[j + 1]; ++p) {
            if (rowval[p] < 0 || rowval[p] >= d)
                return fail(PDMP_ERR_INVALID, "%s: row index %lld out of range in column %lld", what, (long long)rowval[p], (long long)j);
            if (p > colptr[j] && rowval[p - 1] >= rowval[p])
                return fail(PDMP_ERR_INVALID, "%s: rows of column %lld are not strictly ascending", what, (long long)j);
        }
        if (diag_leads && (colptr[j + 1] == colptr[j] || rowval[colptr[j]] != j))
            return fail(PDMP_ERR_INVALID, "%s: column %lld must begin with its diagonal entry (a LOWER triangular factor with a stored diagonal)", what, (long long)j);
    }
    return PDMP_OK;
}
pdmp_status elapsed_ms(hipEvent_t from, hipEvent_t to, float* ms) {
    HIP_TRY(hipEventSynchronize(to));
    HIP_TRY(hipEventElapsedTime(ms, from, to));
    return PDMP_OK;
}
pdmp_status check_trace_range(const pdmp_ensemble* e, int64_t chain, int64_t first, int64_t count) {
    if (chain < 0 || chain >= e->cfg.nchains || first < 0 || count < 0 || first + count > e->cfg.trace_capacity)
        return fail(PDMP_ERR_INVALID, "trace range out of bounds");
    return PDMP_OK;
}
pdmp_status check_chain_range(const pdmp_ensemble* e, int64_t chain_first, int64_t n) {
    if (chain_first < 0 || n < 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "chain range");
    return PDMP_OK;
}

// Everything the ZigZag event-loop kernels read of a run to T, but the dump / profile buffer (dbg, dbg_cap: ensemble_run_impl allocates them)
pdmp::ZzRunParams run_params(const pdmp_ensemble* e, double T, int flags) {
    pdmp::ZzRunParams P{};
    P.count_limit = e->dbg_count_limit ? e->dbg_count_limit : pdmp::PDMP_LAUNCH_COUNT_LIMIT;
    P.tb = e->tables();
    P.rec = e->d_rec.p;
    P.keys = e->d_keys.p;
    P.hdr = e->d_hdr.p;
    P.ev = e->cfg.trace_capacity > 0 ? e->d_ev.p : nullptr;
    P.c_chain = e->cfg.adapt ? e->d_c_chain.p : nullptr;
    P.blob = e->d_blob.p;
    P.tix = e->d_tix.p;
    P.common_tix = e->common_tix;
    if (e->has_g8) {
        P.g8_line = e->d_g8_line.p;
        P.g8_member = e->d_g8_member.p;
        P.g8_gamt = e->g8_same ? nullptr : e->d_g8_gamt.p;
        P.g8_gw = e->g8_gw;
    }
    P.blob_w = e->blob_w;
    P.blob_w_pad = e->blob_w_pad;
    P.blob_sw = e->blob_sw;
    P.blob_pw = e->blob_pw;
    P.blob_kmax = e->blob_kmax;
    P.d = e->cfg.d;
    P.dk = e->dk;
    P.trace_cap = e->cfg.trace_capacity;
    P.nblk = e->nblk;
    P.nblk_pad = e->nblk_pad;
    P.T = T;
    P.factor = e->cfg.factor;
    P.lambda_ref = e->lambda_ref;
    // G2[i] is fetched only once an event is accepted (18 % of proposals): same throughput at 4 waves/SIMD, 37 % less HBM
    // traffic; pdmp_debug_set_spec_g2 restores the speculative fetch (3 % faster when the SIMDs are under-occupied)
    P.flags = flags | (e->dbg_spec_g2 ? 0 : 0x100);
    P.force_spec4 = e->dbg_kernel == PDMP_DEBUG_KERNEL_SPEC4 ? 1 : 0;
    P.adapt = e->cfg.adapt;
    P.has_refresh = e->lambda_ref > 0;
    P.move_all = e->cfg.sampler == PDMP_SAMPLER_ZIGZAG_ALL;
    P.kappa = e->d_kappa.p;
    P.thf = e->d_thf.p;
    P.reversible = e->reversible;
    P.strong_upperbounds = e->strong_upperbounds;
    P.barriers = e->d_barriers.p;
    if (general_path(e)) return P;
    if (e->track || e->exactp) {  // the kernels that take a coordinate's neighbours from its index on the plain lattice
        P.lattice_n = e->lattice_n;
        P.lattice_magic = e->lattice_n ? (uint32_t)(((uint64_t)1 << 32) / (uint64_t)e->lattice_n + 1) : 0u;
    }
    if (!e->track) return P;
    P.track_two_sums = e->track_two_sums ? 1 : 0;
    if (!e->track_pairs) return P;  // (the 8-lane-group kernel)
    // one proposal per lane (pdmp_trackp.hip, and pdmp_trackl.hip on its line layout)
    P.typ_extra = e->typ_extra;
    P.hw_gain = e->dbg_hw_steer[0];  // (pdmp_debug_set_helper_steering: block minima per quantum, events per window -- A/B; 0: the kernel's)
    P.hw_target = (uint32_t)e->dbg_hw_steer[1];
    P.hw_ahead = e->dbg_hw_steer[2];  // (a block to watch: the -DPDMP_TL_CHECK build of pdmp_trackl.hip)
    if (e->track_lines) {
        P.tl_lines = e->d_tl_lines.p;
        P.tl_cold = e->d_tl_cold.p;
        return P;
    }
    P.keys = e->d_kp.p;
    P.track_mean = e->track_mean;
    if (e->track_mean == 2) P.tb.gmu_t = nullptr;  // (the rate's mean rides in the record lines)
    P.n_cu = e->n_cu;
    // the two-wave form (a helper wave per chain) where the ensemble leaves SIMDs idle: at most two resident waves per SIMD with it
    // (1024 SIMDs, two waves per chain) -- a rank's share of a strong-scaled job; wider ensembles hide a wave's latency with other chains
    P.helper_wave = (e->dbg_helper_wave == 1 || (e->dbg_helper_wave == -1 && e->cfg.nchains <= (int64_t)HELPER_WAVE_MAX_CHAINS_PER_CU * (e->n_cu > 0 ? e->n_cu : 256))) ? 1 : 0;
    if (pdmp::zz_trackp_big(e->cfg.d)) P.helper_wave = 0;
    return P;
}

// (hot: the run allocates d_hot before it asks, where rows are long)
pdmp::ZzGeneralParams general_params(const pdmp_ensemble* e) {
    pdmp::ZzGeneralParams Q{};
    Q.local_bound = e->local_bound ? 1 : 0;
    Q.masked = e->has_g1mask ? 1 : 0;
    Q.sticky = e->cfg.sampler == PDMP_SAMPLER_STICKY_ZIGZAG ? 1 : 0;
    Q.qtval = e->d_qtval.p;
    Q.renew_chain = e->local_bound ? e->d_thf.p : nullptr;
    Q.sig_chain = e->adaptscale ? e->d_sig_chain.p : nullptr;
    Q.adaptscale = e->adaptscale ? 1 : 0;
    Q.pos16 = e->d_pos16.p;
    Q.qbval = e->d_qbval.p;
    Q.member = reinterpret_cast<const uint4*>(e->d_member.p);
    Q.selfpos16 = e->d_selfpos16.p;
    Q.mmax_pad = (e->mmax_all + 63u) & ~63u;
    Q.target_kind = e->target_kind;
    Q.A_colptr = e->lg_Acp.p;
    Q.A_rowval = e->lg_Arv.p;
    Q.A_nzval = e->lg_Anz.p;
    Q.At_colptr = e->lg_Atcp.p;
    Q.At_rowval = e->lg_Atrv.p;
    Q.At_row32 = e->lg_Atrv32.p;
    Q.At_nzval = e->lg_Atnz.p;
    Q.y = e->lg_y.p;
    Q.ny = e->lg_ny.p;
    Q.sn0 = e->lg_u0.p;
    Q.ns0 = e->lg_ns0.p;
    Q.gamma0 = e->lg_gamma0;
    Q.ksub = e->lg_k;
    Q.lg_ne_max = (int32_t)std::min<int64_t>(e->lg_nemax, 1 << 30);
    // rows of thousands of coefficients: ranges that hold about 50 of a row's entries (64 lanes per chunk)
    const bool long_rows = e->lg_nemax >= 1024;
    Q.hot = long_rows ? e->d_hot.p : nullptr;
    Q.lg_range = long_rows ? (int32_t)std::max<int64_t>(16, (int64_t)(PDMP_LG_FILL * 64.0 * (double)e->cfg.d / (double)e->lg_nemax)) : 0;
    Q.flow_kind = e->flow_kind;
    Q.mu = e->d_mu.p;
    Q.diag = e->d_diag.p;
    Q.rho = e->rho;
    return Q;
}

static int logistic_rows_width(const pdmp_ensemble* e) { return e->dbg_lg_rows >= 0 ? e->dbg_lg_rows : PDMP_LG_ROWS_DEFAULT; }  // lanes per chain of FAM_LOGISTIC_ROWS
pdmp::ZzLogisticTables logistic_tables(const pdmp_ensemble* e) {
    pdmp::ZzLogisticTables LT{};
    LT.coord = e->lg_coord.p;
    LT.obs = e->lg_obs.p;
    LT.a_row = e->lg_arow.p;
    LT.a_val = e->lg_Anz.p;
    LT.qrow16 = e->d_qrow16.p;
    LT.trk = e->track_lg ? e->d_trk.p : nullptr;
    return LT;
}

// The family that serves the next run of this ensemble (P, Q, LT: its filled parameters), or the refusal the run raises -- *fam is then the family
// that was asked for.  Reads, launches nothing.
pdmp_status select_family(const pdmp_ensemble* e, const pdmp::ZzRunParams& P, const pdmp::ZzGeneralParams& Q, const pdmp::ZzLogisticTables& LT,
                                 KernelFamily* fam) {
    *fam = FAM_BPS;
    if (e->cfg.sampler == PDMP_SAMPLER_BPS) return PDMP_OK;
    const bool sticky = e->cfg.sampler == PDMP_SAMPLER_STICKY_ZIGZAG, dump = e->dbg_dump > 0, profile = e->dbg_phase != 0;
    if (e->cfg.sampler == PDMP_SAMPLER_BARRIER_ZIGZAG) {  // (set_state has refused everything zz_barrier_run_kernel does not take)
        *fam = FAM_BARRIER;
        if (dump) return fail(PDMP_ERR_UNSUPPORTED, "the proposal dump belongs to the one-event kernel");
        return PDMP_OK;
    }
    if (e->target_kind == TARGET_BRIDGE) {  // (set_state has refused everything zz_bridge_run_kernel does not take)
        *fam = FAM_BRIDGE;
        if (dump) return fail(PDMP_ERR_UNSUPPORTED, "the proposal dump belongs to the one-event kernel");
        return PDMP_OK;
    }
    if (e->target_kind == TARGET_PRECISION) {  // (set_state has refused everything zz_precision_run_kernel does not take)
        *fam = FAM_PRECISION;
        if (dump) return fail(PDMP_ERR_UNSUPPORTED, "the proposal dump belongs to the one-event kernel");
        return PDMP_OK;
    }
    if (general_path(e)) {
        // small d: the chain's state lives in LDS for the whole slice (PDMP_DEBUG_KERNEL_SEQ keeps the records in HBM: A/B runs, parity tests)
        const bool lds_resident = e->dbg_kernel != PDMP_DEBUG_KERNEL_SEQ && pdmp::zz_logistic_lds_supported(P, Q, LT);
        *fam = (lds_resident || e->track_lg) ? FAM_LOGISTIC_LDS : FAM_GENERAL;
        if (e->track_lg && !lds_resident)
            return fail(PDMP_ERR_UNSUPPORTED, "gradient tracking with the logistic target runs on the LDS-resident kernel: d <= 512, k_sub <= 32, rows of <= 6 regressors");
#ifdef PDMP_EXTRA_KERNELS
        // ... several chains per wavefront where the draws of a proposal fit a row (pdmp_logrows.hip); pdmp_debug_set_logistic_rows picks the width.
        // The rows kernel takes neither a dump nor a profile buffer: the run hands one to every general kernel that is asked for either
        pdmp::ZzRunParams Pb = P;
        if (dump || profile) Pb.dbg = const_cast<double*>(e->dbg_phase_out);  // (read as "not null" only)
        const int rows_w = (!lds_resident || e->track_lg) ? 0 : logistic_rows_width(e);
        const bool rows = rows_w > 0 && pdmp::zz_logistic_rows_supported(Pb, Q, LT, rows_w);
        if (rows || (lds_resident && e->dbg_lg_rows > 0)) *fam = FAM_LOGISTIC_ROWS;
        if (lds_resident && e->dbg_lg_rows > 0 && !rows) return fail(PDMP_ERR_UNSUPPORTED, "pdmp_debug_set_logistic_rows: this ensemble does not fit rows of %d lanes", rows_w);
#endif
        return PDMP_OK;
    }
    if (e->track) {
        // one proposal per lane where the graph is the plain lattice or tabulated (pdmp_trackp.hip; its line layout on request); elsewhere, and on
        // request, the 8-lane-group kernel -- decided with the layout, by set_state
        *fam = e->track_lines ? FAM_TRACKL : e->track_pairs ? FAM_TRACKP : FAM_TRACK_GROUPS;
        if (dump) return fail(PDMP_ERR_UNSUPPORTED, "the proposal dump belongs to the one-event kernel");
        return PDMP_OK;
    }
    // (33 <= |S| <= 64: no blob kernel takes it, but zz_local_spec8g_kernel<.., GW = 16> does where its own conditions hold)
    const bool g16_ok = e->has_g8 && e->g8_gw == 16 && e->dbg_kernel == PDMP_DEBUG_KERNEL_AUTO && (P.flags & 0x100) && !profile;
    // (a refresh clock, src/sfact.jl:78-114: the speculative kernels process the clock's events by themselves between their iterations -- round 6)
    const bool spec_ok = (e->use_spec || g16_ok) && !dump && !P.move_all && !sticky;
    *fam = FAM_EXACTP;
#ifdef PDMP_EXTRA_KERNELS
    if (e->exactp && spec_ok && !P.has_refresh && pdmp::zz_exactp_supported(P)) return PDMP_OK;
#endif
    if (e->dbg_kernel == PDMP_DEBUG_KERNEL_EXACTP)  // asked for by name: never another kernel in its place
#ifndef PDMP_EXTRA_KERNELS
        return fail(PDMP_ERR_UNSUPPORTED, "PDMP_DEBUG_KERNEL_EXACTP: zz_local_exactp_kernel is not part of this library: it lives in the parity build (build.py --variant parity, -DPDMP_EXTRA_KERNELS)");
#else
        return fail(PDMP_ERR_UNSUPPORTED, "PDMP_DEBUG_KERNEL_EXACTP: spdmp on a plain lattice (16 <= n <= 128, d >= 2048) with the bounding matrix equal to the target's, no adaptation, and a trace or no trace");
#endif
    const bool sticky_spec = sticky && e->use_spec && e->blob_mmax <= 16 && !dump;  // the ZigZag speculative kernel's requirements, one zone member per lane
    *fam = sticky ? (sticky_spec ? FAM_STICKY_SPEC : FAM_STICKY_RUN) : spec_ok ? FAM_SPEC : FAM_ONE_EVENT;
    return PDMP_OK;
}

// validate, fill, select, launch, finish
pdmp_status ensemble_run_impl(pdmp_ensemble* e, double T, int flags, void* stream) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "set_state must be called before run");
    if (e->trace_appended) return fail(PDMP_ERR_INVALID, "pdmp_debug_trace_append was used on this ensemble: its records no longer match its trace (set_state first)");
    if (flags != PDMP_RUN_REFERENCE_TAIL && flags != PDMP_RUN_STOP_BEFORE) return fail(PDMP_ERR_INVALID, "bad flags");
    HIP_TRY(hipSetDevice(e->cfg.device));
    e->ran = true;
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    const int64_t n = e->cfg.nchains;
    const bool bps = e->cfg.sampler == PDMP_SAMPLER_BPS;
    if (!bps) e->dbg_phase_valid = 0;
    if (!bps && general_path(e) && e->lg_nemax >= 1024 && !e->d_hot.p) PDMP_TRY(e->d_hot.alloc((size_t)n * (size_t)e->cfg.d * 4));
    // (plain fills of pointers and numbers: the other sampler's block goes unread)
    const pdmp::BpsRunParams B = bps_run_params(e, T, flags);
    pdmp::ZzRunParams P = run_params(e, T, flags);
    const pdmp::ZzGeneralParams Q = general_params(e);
    const pdmp::ZzLogisticTables LT = logistic_tables(e);
    KernelFamily fam;
    PDMP_TRY(select_family(e, P, Q, LT, &fam));
    const FamilyInfo& F = FAMILY[fam];
    // on the stream: the dump buffer's memset, ev0, the profile buffer's memset, the kernel, ev1
    DevBuf<double> dbgbuf, phbuf;
    const int64_t dbg_cap = bps ? 0 : e->dbg_dump;
    if (dbg_cap > 0) {
        PDMP_TRY(dbgbuf.alloc((size_t)dbg_cap * 16));
        HIP_TRY(hipMemsetAsync(dbgbuf.p, 0, (size_t)dbg_cap * 16 * sizeof(double), s));
        P.dbg = dbgbuf.p;
        P.dbg_cap = dbg_cap;
    }
    if (fam == FAM_TRACKP && e->dbg_prio_policy != 0) {
        // priority by rank of progress (pdmp_engine.hpp: PrioLag): the board is zeroed once -- epoch 0 is never a launch's -- and every launch takes the next epoch
        if (!e->d_prio_board.p) {
            PDMP_TRY(e->d_prio_board.alloc(pdmp::PDMP_PRIO_BOARD_WORDS));
            HIP_TRY(hipMemsetAsync(e->d_prio_board.p, 0, (size_t)pdmp::PDMP_PRIO_BOARD_WORDS * sizeof(uint32_t), s));
        }
        e->prio_epoch = e->prio_epoch % 255u + 1u;
        P.prio_board = e->d_prio_board.p;
        P.prio_epoch = e->prio_epoch;
    }
    HIP_TRY(hipEventRecord(e->ev0, s));
    const bool profiled = e->dbg_phase != 0 && F.phase_kind != 0;
    if (profiled) {
        PDMP_TRY(phbuf.alloc(16));
        HIP_TRY(hipMemsetAsync(phbuf.p, 0, 16 * sizeof(double), s));
        P.dbg = phbuf.p;
        P.dbg_cap = 0;
    }
    int rc = 0;
    switch (fam) {
    case FAM_BPS:
        if (e->bps.modern && e->bps.logit) {
            e->last_kernel = "bps_logit_run_kernel";
            rc = pdmp::launch_bps_logit_run(B, bps_modern_params(e), bps_logit_params(e), n, s);
        } else if (e->bps.modern) {
            e->last_kernel = "bps_modern_run_kernel";
            rc = pdmp::launch_bps_modern_run(B, bps_modern_params(e), n, s);
        } else if (e->bps.sticky) {
            e->last_kernel = "bps_sticky_run_kernel";
            rc = pdmp::launch_bps_sticky_run(B, bps_sticky_params(e), n, s);
        } else {
            e->last_kernel = "bps_run_kernel";
            rc = pdmp::launch_bps_run(B, n, e->bps.diag, s, bps_moments_params(e));
        }
        break;
    case FAM_GENERAL: e->last_kernel = "zz_general_run_kernel"; rc = pdmp::launch_zz_general_run(P, Q, n, s); break;
    case FAM_LOGISTIC_LDS: e->last_kernel = "zz_logistic_lds_kernel"; rc = pdmp::launch_zz_logistic_lds(P, Q, LT, e->keep_integrals, n, s); break;
    case FAM_TRACKL: e->last_kernel = "zz_local_trackl_kernel"; e->canon_stale = true; rc = pdmp::launch_zz_local_trackl(P, n, s); break;
    case FAM_TRACKP: rc = pdmp::launch_zz_local_trackp(P, n, s, &e->last_kernel); break;
    case FAM_TRACK_GROUPS: e->last_kernel = "zz_local_track_kernel"; rc = pdmp::launch_zz_local_track(P, n, s); break;
    case FAM_STICKY_SPEC: e->last_kernel = "zz_sticky_spec_kernel"; rc = pdmp::launch_zz_sticky_spec(P, n, s); break;
    case FAM_STICKY_RUN: e->last_kernel = "zz_sticky_run_kernel"; rc = pdmp::launch_zz_sticky_run(P, n, s); break;
    case FAM_SPEC: rc = pdmp::launch_zz_local_spec(P, n, s, &e->last_kernel); break;
    case FAM_ONE_EVENT: e->last_kernel = "zz_local_run_kernel"; rc = pdmp::launch_zz_local_run(P, n, s); break;
    case FAM_BARRIER: e->last_kernel = "zz_barrier_run_kernel"; rc = pdmp::launch_zz_barrier_run(P, n, s); break;
    case FAM_BRIDGE: e->last_kernel = "zz_bridge_run_kernel"; rc = pdmp::launch_zz_bridge_run(P, e->bridge, n, s); break;
    case FAM_PRECISION: e->last_kernel = "zz_precision_run_kernel"; rc = pdmp::launch_zz_precision_run(P, e->precision, n, s); break;
#ifdef PDMP_EXTRA_KERNELS
    case FAM_LOGISTIC_ROWS: e->last_kernel = "zz_logistic_rows_kernel"; rc = pdmp::launch_zz_logistic_rows(P, Q, LT, e->keep_integrals, logistic_rows_width(e), n, s); break;
    case FAM_EXACTP: e->last_kernel = "zz_local_exactp_kernel"; rc = pdmp::launch_zz_local_exactp(P, n, s); break;
#else
    case FAM_LOGISTIC_ROWS: case FAM_EXACTP: return fail(PDMP_ERR_UNSUPPORTED, "kernel family %d is not part of this library", (int)fam);  // (select_family never returns them here)
#endif
    }
    if (rc != 0) return fail_launch(F.launcher, rc, F.hip_rc);
    HIP_TRY(hipEventRecord(e->ev1, s));
    e->timed = true;
    if (profiled) {
        HIP_TRY(device_sync(e));
        HIP_TRY(hipMemcpy(e->dbg_phase_out, phbuf.p, sizeof e->dbg_phase_out, hipMemcpyDeviceToHost));
        e->dbg_phase_valid = F.phase_kind;
    }
    if (dbg_cap > 0 && (fam == FAM_ONE_EVENT || fam == FAM_STICKY_RUN)) {  // (the general kernels take the buffer for a profile of theirs: nothing to print)
        HIP_TRY(device_sync(e));
        std::vector<double> hd((size_t)dbg_cap * 16);
        HIP_TRY(hipMemcpy(hd.data(), dbgbuf.p, hd.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < dbg_cap; ++r) {
            const double* D = hd.data() + r * 16;
            fprintf(stderr, "DBG %3lld tp=%.6f i=%g acc=%g k=%g m=%g self=%g l=%.6g lb=%.6g u=%.6f key=%.6f t=%.6f L=%.6f g=%.6g a_i=%.6g x0=%.6g cj=%.6g\n",
                    (long long)r, D[0], D[1], D[2], D[3], D[4], D[5], D[6], D[7], D[8], D[9], D[10], D[11], D[12], D[13], D[14], D[15]);
        }
    }
    return PDMP_OK;
}

extern "C" {

const char* pdmp_last_error(void) {
    return g_err.c_str();
}
void pdmp_set_last_error_(const char* msg) {  // (pdmp_comm.hip: the other translation unit of the library)
    g_err = msg ? msg : "";
}
pdmp_status pdmp_ensemble_info(pdmp_ensemble* e, int64_t* nchains, int64_t* d, int64_t* trace_capacity, int* device) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (nchains) *nchains = e->cfg.nchains;
    if (d) *d = e->cfg.d;
    if (trace_capacity) *trace_capacity = e->cfg.trace_capacity;
    if (device) *device = e->cfg.device;
    return PDMP_OK;
}

int pdmp_abi_version(void) {
    return PDMP_ABI_VERSION;
}

int pdmp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int k = 0; k < n; ++k) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, k) != hipSuccess) continue;
        if (strncmp(prop.gcnArchName, "gfx950", 6) == 0) ok++;
    }
    return ok;
}

pdmp_status pdmp_ensemble_create(const pdmp_config* cfg, pdmp_ensemble** out) {
    if (!cfg || !out) return fail(PDMP_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(pdmp_config))
        return fail(PDMP_ERR_INVALID, "pdmp_config.struct_size %u != %zu", cfg->struct_size, sizeof(pdmp_config));
    if (cfg->nchains <= 0 || cfg->d <= 0) return fail(PDMP_ERR_INVALID, "nchains and d must be positive");
    if (cfg->d >= (int64_t)1 << 31) return fail(PDMP_ERR_UNSUPPORTED, "d must be < 2^31");
    if (cfg->sampler != PDMP_SAMPLER_ZIGZAG_LOCAL && cfg->sampler != PDMP_SAMPLER_ZIGZAG_ALL &&
        cfg->sampler != PDMP_SAMPLER_BPS && cfg->sampler != PDMP_SAMPLER_STICKY_ZIGZAG && cfg->sampler != PDMP_SAMPLER_BARRIER_ZIGZAG)
        return fail(PDMP_ERR_UNSUPPORTED, "sampler %d has no device kernel yet", cfg->sampler);
    if (cfg->sampler == PDMP_SAMPLER_BPS && cfg->d > 4096)
        return fail(PDMP_ERR_UNSUPPORTED, "BPS keeps x, θ, ∇ϕ in registers (d <= 1024) or registers + scratch (d <= 4096): got %lld", (long long)cfg->d);
    if (cfg->trace_capacity < 0) return fail(PDMP_ERR_INVALID, "trace_capacity < 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible: libpdmp_mi355 has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(PDMP_ERR_INVALID, "device %d out of range", cfg->device);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PDMP_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 code only", cfg->device,
                    prop.gcnArchName);
    HIP_TRY(hipSetDevice(cfg->device));
    pdmp_ensemble* e = new pdmp_ensemble();
    e->cfg = *cfg;
    e->n_cu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&e->ev0) != hipSuccess || hipEventCreate(&e->ev1) != hipSuccess) {
        delete e;
        return fail(PDMP_ERR_HIP, "stream/event creation failed");
    }
    *out = e;
    return PDMP_OK;
}

void pdmp_ensemble_destroy(pdmp_ensemble* e) {
    if (!e) return;
    (void)hipSetDevice(e->cfg.device);
    (void)hipDeviceSynchronize();
    for (hipEvent_t ev : {e->ev_run_done, e->ev_cons_done[0], e->ev_cons_done[1], e->ev_c0, e->ev_c1})
        if (ev) (void)hipEventDestroy(ev);
    if (e->stream2) (void)hipStreamDestroy(e->stream2);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

pdmp_status pdmp_ensemble_run(pdmp_ensemble* e, double T, int flags, void* stream) {
    pdmp_status st = ensemble_run_impl(e, T, flags, stream);
    if (st == PDMP_OK && e->cfg.sampler != PDMP_SAMPLER_BPS) e->run_T = T;  // (only a launch that went out moves the horizon: fact_integrals_at)
    if (st == PDMP_OK && e->deferred_k >= 0) st = launch_deferred_consumer(e);  // (behind the event loop's launch: see pdmp_ensemble_consume_async)
    return st;
}

pdmp_status pdmp_ensemble_run_partitioned(pdmp_ensemble* e, double T, int K, double delta, const uint8_t* g1_mask, int64_t mask_len,
                                          void* stream) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "set_state must be called before run");
    if (e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL || e->target_kind != 0 || e->flow_kind != 0 || e->lambda_ref > 0 || e->adaptscale ||
        e->local_bound || e->track || e->has_kappa)
        return fail(PDMP_ERR_UNSUPPORTED,
                    "parallel_spdmp (src/parallel.jl) is built for the local ZigZag on a Gaussian target without refresh clock, "
                    "adaptscale, LocalBound or gradient tracking");
    if (e->trace_appended) return fail(PDMP_ERR_INVALID, "pdmp_debug_trace_append was used on this ensemble: its records no longer match its trace (set_state first)");
    if (e->ran) return fail(PDMP_ERR_UNSUPPORTED, "a partitioned run starts from a fresh state (call set_state first)");
    if (e->has_g1mask) return fail(PDMP_ERR_UNSUPPORTED, "parallel_spdmp takes G as the flow's pattern + g1_mask, not pdmp_ensemble_set_neighbourhood");
    const int64_t d = e->cfg.d;
    if (K < 1 || K > 16 || d % K != 0)
        return fail(PDMP_ERR_INVALID, "K = %d: need 1 <= K <= 16 chunks of equal size d / K (Partition, src/parallel.jl:26)", K);
    if (!(delta > 0)) return fail(PDMP_ERR_INVALID, "the horizon Δ must be positive");
    const int64_t k = d / K;
    const int64_t nnz = e->nnz;
    // G = the pattern of the flow tables, G1 = the structural entries of the bounding Γ inside it (all of it without a mask)
    std::vector<uint8_t> mask((size_t)nnz, 1);
    if (g1_mask && mask_len != nnz)
        return fail(PDMP_ERR_INVALID, "g1_mask has %lld entries, the flow's pattern %lld (one flag per stored entry of the Γ given to set_flow_zigzag)",
                    (long long)mask_len, (long long)nnz);
    if (g1_mask) mask.assign(g1_mask, g1_mask + nnz);
    std::vector<uint8_t> inner((size_t)d, 1);
    for (int64_t i = 0; i < d; ++i) {
        if (e->colptr[i + 1] - e->colptr[i] > 64u)
            return fail(PDMP_ERR_UNSUPPORTED, "column %lld has %u entries: the partitioned kernel holds one neighbour per lane (64)",
                        (long long)i, e->colptr[i + 1] - e->colptr[i]);
        for (uint32_t p = e->colptr[i]; p < e->colptr[i + 1]; ++p) {
            const int64_t j = e->rowval[p];
            if (j / k != i / k) {
                inner[(size_t)i] = 0;  // :114
                if (mask[p])
                    return fail(PDMP_ERR_INVALID, "Upper bounds may not depend across chunks. (src/parallel.jl:124-127: Γ[%lld,%lld])",
                                (long long)j, (long long)i);
            } else if (!mask[p] && e->bval[p] != 0.0) {
                return fail(PDMP_ERR_INVALID, "slot (%lld,%lld) is outside the bounding pattern but carries a bound value", (long long)j,
                            (long long)i);
            }
        }
    }
    // G2[i] = union of G1[j], j in G1[i], without G[i] (:121); inside the chunk because G1 is
    std::vector<uint32_t> g2ptr((size_t)d + 1, 0), g2idx;
    {
        std::vector<uint32_t> tmp;
        for (int64_t i = 0; i < d; ++i) {
            tmp.clear();
            for (uint32_t p = e->colptr[i]; p < e->colptr[i + 1]; ++p) {
                if (!mask[p]) continue;
                const uint32_t j = e->rowval[p];
                for (uint32_t q = e->colptr[j]; q < e->colptr[j + 1]; ++q)
                    if (mask[q]) tmp.push_back(e->rowval[q]);
            }
            std::sort(tmp.begin(), tmp.end());
            tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
            for (uint32_t v : tmp) {
                bool in_g = false;
                for (uint32_t p = e->colptr[i]; p < e->colptr[i + 1] && !in_g; ++p) in_g = e->rowval[p] == v;
                if (!in_g) g2idx.push_back(v);
            }
            g2ptr[(size_t)i + 1] = (uint32_t)g2idx.size();
        }
    }
    if (g2idx.empty()) g2idx.push_back(0);
    const int nbc = (int)((k + 63) / 64);
    const size_t lds = pdmp::zz_partitioned_lds_bytes(K, nbc);
    if (lds > 64 * 1024)
        return fail(PDMP_ERR_UNSUPPORTED, "d = %lld needs %zu bytes of LDS for the chunk queues (64 KB per workgroup)", (long long)d, lds);
    HIP_TRY(hipSetDevice(e->cfg.device));
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    DevBuf<uint8_t> d_inner, d_mask;
    DevBuf<uint32_t> d_g2ptr, d_g2idx;
    PDMP_TRY(d_inner.upload(inner));
    PDMP_TRY(d_mask.upload(mask));
    PDMP_TRY(d_g2ptr.upload(g2ptr));
    PDMP_TRY(d_g2idx.upload(g2idx));
    pdmp::ZzPartParams P{};
    P.tb = e->tables();
    P.rec = e->d_rec.p;
    P.keys = e->d_keys.p;
    P.hdr = e->d_hdr.p;
    P.ev = e->cfg.trace_capacity > 0 ? e->d_ev.p : nullptr;
    P.c_chain = e->cfg.adapt ? e->d_c_chain.p : nullptr;
    P.inner = d_inner.p;
    P.g1mask = d_mask.p;
    P.g2ptr = d_g2ptr.p;
    P.g2idx = d_g2idx.p;
    P.d = d;
    P.dk = e->dk;
    P.trace_cap = e->cfg.trace_capacity;
    P.k = k;
    P.K = K;
    P.nbc = nbc;
    P.adapt = e->cfg.adapt;
    P.T = T;
    P.delta = delta;
    P.factor = e->cfg.factor;
    e->ran = true;
    HIP_TRY(hipEventRecord(e->ev0, s));
    LAUNCH_TRY_CODE("zz_partitioned_run", pdmp::launch_zz_partitioned(P, e->cfg.nchains, s));
    e->run_T = T;
    HIP_TRY(hipEventRecord(e->ev1, s));
    e->timed = true;
    HIP_TRY(hipStreamSynchronize(s));  // (the tables of this call live until here)
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_sync(pdmp_ensemble* e) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_last_run_ms(pdmp_ensemble* e, float* ms) {
    if (!e || !ms) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->timed) return fail(PDMP_ERR_INVALID, "no run has been launched");
    HIP_TRY(hipSetDevice(e->cfg.device));
    return elapsed_ms(e->ev0, e->ev1, ms);
}

pdmp_status pdmp_ensemble_counters(pdmp_ensemble* e, pdmp_chain_counters* out) {
    if (!e || !out) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "no state");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    std::vector<pdmp::DevChain> h((size_t)e->cfg.nchains);
    HIP_TRY(hipMemcpy(h.data(), e->d_hdr.p, h.size() * sizeof(pdmp::DevChain), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < h.size(); ++k) out[k] = h[k].c;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_totals(pdmp_ensemble* e, uint64_t* num, uint64_t* nacc, uint64_t* nevents) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    std::vector<pdmp_chain_counters> c((size_t)e->cfg.nchains);
    PDMP_TRY(pdmp_ensemble_counters(e, c.data()));
    uint64_t a = 0, b = 0, n = 0;
    for (auto& k : c) {
        n += k.num;
        a += k.nacc;
        b += k.nevents;
    }
    if (num) *num = n;
    if (nacc) *nacc = a;
    if (nevents) *nevents = b;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_trace_copy(pdmp_ensemble* e, int64_t chain, int64_t first, int64_t count, pdmp_event* out) {
    if (!e || !out) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (e->cfg.trace_capacity <= 0) return fail(PDMP_ERR_INVALID, "ensemble was created with trace_capacity = 0");
    PDMP_TRY(check_trace_range(e, chain, first, count));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    if (count)
        HIP_TRY(hipMemcpy(out, e->d_ev.p + chain * e->cfg.trace_capacity + first, (size_t)count * sizeof(pdmp_event),
                          hipMemcpyDeviceToHost));
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_trace_reset(pdmp_ensemble* e) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "no state");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    // ntrace lives at a fixed offset inside each 128-byte header: zero it with a strided 2-D memset
    const size_t off = offsetof(pdmp::DevChain, c) + offsetof(pdmp_chain_counters, ntrace);
    HIP_TRY(hipMemset2DAsync(reinterpret_cast<char*>(e->d_hdr.p) + off, sizeof(pdmp::DevChain), 0, sizeof(uint64_t),
                             (size_t)e->cfg.nchains, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));  // (a memset on the null stream is not ordered against the ensemble's non-blocking stream)
    // status TRACE_FULL -> OK is handled by the kernel at entry (only BOUND_VIOLATED / STALLED are sticky)
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_final_state(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* t, double* x,
                                      double* theta, int64_t* acc, double* c) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "no state");
    PDMP_TRY(check_chain_range(e, chain_first, n));
    if (n == 0) return PDMP_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    PDMP_TRY(ensure_canon(e));
    const int64_t d = e->cfg.d;
    const size_t cnt = (size_t)(n * d);
    DevBuf<double> bt, bx, bth, bc;
    DevBuf<int64_t> bacc;
    if (t) PDMP_TRY(bt.alloc(cnt));
    if (x) PDMP_TRY(bx.alloc(cnt));
    if (theta) PDMP_TRY(bth.alloc(cnt));
    if (acc) PDMP_TRY(bacc.alloc(cnt));
    if (c) PDMP_TRY(bc.alloc(cnt));
    const double* c_src = e->cfg.adapt ? e->d_c_chain.p : e->d_c.p;
    const int64_t c_stride = e->cfg.adapt ? d : 0;
    if (e->track_pairs && e->cfg.adapt) {  // (the one-proposal-per-lane kernel keeps the adapted bounds in its record lines)
        LAUNCH_TRY("trackp_c_out", pdmp::launch_zz_trackp_c_out(e->d_rec.p, e->d_c_chain.p, e->cfg.nchains * d, e->stream));
    }
    int rc = e->track ? pdmp::launch_zz_track_unpack(reinterpret_cast<const pdmp::TrRec*>(e->d_rec.p), e->tables(), c_src, c_stride, d,
                                                     chain_first, n, e->t0_state, bt.p, bx.p, bth.p, bacc.p, bc.p, e->track_pairs ? e->d_kp.p : nullptr, e->dk, e->stream)
                       : pdmp::launch_zz_unpack(e->d_rec.p, c_src, c_stride, d, chain_first, n, bt.p, bx.p, bth.p, bacc.p, bc.p,
                                                e->stream);
    LAUNCH_TRY("unpack", rc);
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (t) HIP_TRY(hipMemcpy(t, bt.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
    if (x) HIP_TRY(hipMemcpy(x, bx.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
    if (theta) HIP_TRY(hipMemcpy(theta, bth.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
    if (acc) HIP_TRY(hipMemcpy(acc, bacc.p, cnt * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (c) HIP_TRY(hipMemcpy(c, bc.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_trace_dev(pdmp_ensemble* e, void** events_dev, int64_t* capacity) {
    if (!e || !events_dev || !capacity) return fail(PDMP_ERR_INVALID, "null argument");
    *events_dev = e->d_ev.p;
    *capacity = e->cfg.trace_capacity;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_bps_trace_dev(pdmp_ensemble* e, void** t_dev, void** x_dev, void** theta_dev) {
    if (!e || !t_dev || !x_dev || !theta_dev) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS) return fail(PDMP_ERR_INVALID, "not a BouncyParticle / Boomerang ensemble");
    *t_dev = e->b_ev_t.p;
    *x_dev = e->b_ev_x.p;
    *theta_dev = e->b_ev_th.p;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_counters_dev(pdmp_ensemble* e, void** counters_dev) {
    if (!e || !counters_dev) return fail(PDMP_ERR_INVALID, "null argument");
    *counters_dev = e->d_hdr.p;
    return PDMP_OK;
}

}  // extern "C"
