// pdmp_capi.hip -- implementation of the C ABI declared in include/pdmp_mi355.h.
//
// Host-side work only: argument checking, building the read-only "neighbourhood program" tables from the
// flow's CSC pattern (G1, G2 of src/sfact.jl:170-179), HBM allocation, kernel launches.  There is NO CPU
// fallback: without a gfx950 device every entry point that needs one fails with PDMP_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <chrono>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/pdmp_detmath.h"
#include "../../include/pdmp_debug.h"
#include "pdmp_engine.hpp"

namespace {

thread_local std::string g_err;
thread_local std::string g_deferred_err;  // the message of a deferred consumer launch that failed inside device_sync (kept through HIP_TRY)

pdmp_status fail(pdmp_status st, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return st;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            const std::string dm_ = g_deferred_err;                                                     \
            g_deferred_err.clear();                                                                     \
            return fail(PDMP_ERR_HIP, "%s failed: %s%s%s", #expr, hipGetErrorString(e_), dm_.empty() ? "" : " -- ", dm_.c_str()); \
        }                                                                                               \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    pdmp::Placement placed;  // arrays of several GB: chunks of the three memory classes in turn (pdmp_place.hip); otherwise empty, and p is a hipMalloc
    pdmp_status alloc(size_t count, const pdmp::PlaceConfig* pc = nullptr, const std::string* pattern = nullptr) {
        release();
        if (count == 0) return PDMP_OK;
        if (pc && pdmp::placed_alloc(count * sizeof(T), placed, pc, pattern)) {
            p = static_cast<T*>(placed.va);
            n = count;
            return PDMP_OK;
        }
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return fail(PDMP_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
        }
        n = count;
        return PDMP_OK;
    }
    pdmp_status upload(const std::vector<T>& h) {
        pdmp_status st = alloc(h.size());
        if (st != PDMP_OK) return st;
        if (!h.empty()) HIP_TRY(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
        return PDMP_OK;
    }
    void release() {
        if (placed.va) pdmp::placed_free(placed);
        else if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

}  // namespace

// zz_local_trackp: ensembles of at most this many chains PER COMPUTE UNIT run the two-wave form (pdmp_trackp.hip).  Measured on C3 (profiles/r05_*):
// the helper wave pays as long as every chain is resident with room to spare -- 18.7 KB of LDS and 128 registers admit eight chains per CU; up to
// seven (1792 on the MI355X's 256 CUs) two waves win: 1536 chains 18.7 against 21.2 ms for one wave, 1792 chains 20.6 against 21.7, 1920 chains 23.1
// against 22.2.
#ifndef HELPER_WAVE_MAX_CHAINS_PER_CU
#define HELPER_WAVE_MAX_CHAINS_PER_CU 7
#endif
struct pdmp_ensemble {
    pdmp_config cfg{};
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    bool has_flow = false, has_target = false, has_state = false;
    bool ran = false;  // a run happened since set_state (pdmp_ensemble_run_partitioned starts from a fresh state only)

    // host copies of the flow (needed to align the target and to rebuild tables)
    std::vector<uint32_t> colptr, rowval;
    std::vector<double> bval, mu, sigma;
    double lambda_ref = 0.0, rho = 0.0;
    int64_t nnz = 0;
    uint32_t nblk = 0, nblk_pad = 0;
    int64_t dk = 0;
    bool has_tmu = false;

    // host copies of the derived tables (inputs of the per-coordinate blob)
    std::vector<double> h_gmu_b, h_gmu_t, h_tval;
    int track_mean = 0;  // zz_local_trackp: 0 no mean, 1 the flow's Γμ in the bounds, 2 also in the rate (the target's Γμ equals it); decided by set_state
    std::vector<uint32_t> h_sptr, h_sidx, h_qptr;
    std::vector<uint8_t> h_pos, h_selfpos;
    uint32_t blob_w = 0, blob_w_pad = 0, blob_sw = 0, blob_pw = 0, blob_kmax = 0, blob_mmax = 0;
    bool use_spec = false;  // speculative 4-events-per-iteration kernel (zz_local_spec_kernel)
    DevBuf<uint64_t> d_blob;
    DevBuf<uint32_t> d_tix;
    size_t n_templates = 0;
    uint32_t common_tix = 0;

    // device tables
    DevBuf<uint32_t> d_colptr, d_rowval, d_sptr, d_sidx, d_qptr;
    DevBuf<uint8_t> d_pos, d_selfpos;
    DevBuf<double> d_bval, d_tval, d_gmu_b, d_gmu_t, d_c, d_c2, d_sigma;
    DevBuf<pdmp::CoordConst> d_cc;
    // device state
    DevBuf<pdmp::ZzRec> d_rec;
    DevBuf<double> d_keys, d_c_chain, d_jprev, d_sum;
    // diagnostics (include/pdmp_debug.h): per-ensemble state, no process globals
    int dbg_kernel = 0;            // PDMP_DEBUG_KERNEL_*
    int dbg_lg_rows = -1;          // chains per wavefront of the LDS-resident logistic kernel: -1 default, 0 / 16 / 32 = one chain, rows of 16, of 32 lanes
    int dbg_spec_g2 = 0;           // 4-event kernel: fetch the G2 records speculatively
    int dbg_phase = 0;             // record the per-phase cycle profile of chain 0 during the next runs
    double dbg_phase_out[16] = {0};
    int dbg_phase_valid = 0;
    int64_t dbg_dump = 0;          // dump the first n proposals of chain 0 (one-event kernel) to stderr
    int dbg_track_groups = 0;      // gradient tracking: keep the 8-lane-group kernel where the one-proposal-per-lane kernel would run
    double dbg_hw_steer[3] = {0, 0, 0};  // pdmp_debug_set_helper_steering: gain, target, ahead (0: the kernel's defaults)
    uint32_t dbg_count_limit = 0;  // pdmp_debug_set_launch_count_limit (0: PDMP_LAUNCH_COUNT_LIMIT)
    int dbg_cons_overlap = -1;     // pdmp_debug_set_consumer_overlap: -1 by ensemble width, 0 the consumer runs between slices, 1 beside the next slice
    int n_cu = 0;                  // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    int dbg_helper_wave = -1;      // zz_local_trackp: -1 = the two-wave form where the launch leaves SIMDs idle (HELPER_WAVE_MAX_CHAINS_PER_CU), 0 = never, 1 = always
    // tracked-gradient kernel (pdmp_ensemble_set_gradient_tracking)
    bool track_requested = false, track = false, track_two_sums = false;
    bool track_lg = false;     // tracked bounds under the logistic target (zz_logistic_lds_kernel<.., TRK>); d_trk holds (g, gd, tg) per coordinate
    DevBuf<double> d_trk;
    bool exactp = false;       // the moving evaluation runs on zz_local_exactp_kernel (plain lattice; decided by set_state)
    bool track_pairs = false;  // the queue's level 0 is (key, time) pairs in d_kp (pdmp_trackp.hip); decided by set_state
    DevBuf<double> d_kp;
    // the line layout (pdmp_trackl.hip): full-width launches on the plain lattice run on d_tl_lines / d_tl_cold; d_rec / d_kp are brought up to
    // date (canon_stale) only when something reads the state -- final_state, the path-integral kernels, consume_begin
    bool track_lines = false, canon_stale = false;
    pdmp::PlaceConfig place_cfg;  // pdmp_debug_set_placement
    int place_tune = 1;          // init_state_tuned: 1 (default) probe and re-allocate, 0 take what hipMalloc gives
    std::string tune_log;  // init_state_tuned: the placement probes of the last set_state (pdmp_debug_placement)
    int dbg_track_lines = -1;  // pdmp_debug_set_track_lines: 1 = the line layout wherever it serves; -1 / 0 = never (it lost the A/B: DESIGN.md §5)
    DevBuf<pdmp::TrLine> d_tl_lines;
    DevBuf<pdmp::TrCold> d_tl_cold;
    // zz_local_spec8g_kernel's tables (any graph with |G1| <= 8, |S| <= 32; built with the blob)
    bool has_g8 = false, g8_same = false;
    int g8_gw = 8;  // lanes per event of zz_local_spec8g_kernel: 8 (|S| <= 32) or 16 (|S| <= 64)
    DevBuf<uint64_t> d_g8_line;
    DevBuf<double> d_g8_member, d_g8_gamt;
    bool track_generic = false;  // ... on a graph that is not the plain lattice: G1 ids in the records, Γ values in d_gam8 (|G1| <= 8)
    DevBuf<double> d_gam8;
    DevBuf<uint16_t> d_nb16;
    const char* last_kernel = "";  // event-loop kernel of the last pdmp_ensemble_run (pdmp_debug_last_kernel)
    int32_t lattice_n = 0;  // the flow's graph is the n x n 5-point lattice in column-major numbering (0: it is not)
    uint32_t typ_extra = 0;  // the most frequent |G1[i]| - 1 of the flow's graph (set_flow): what the one-proposal-per-lane tracked kernels unroll for
    double t0_state = 0.0;
    double run_T = 0.0;  // horizon of the last run (t0 before the first): no read of the path integrals beyond it (fact_integrals_at)
    DevBuf<double> d_jstart, d_essacc;  // pdmp_ensemble_ess_*
    double ess_T0 = 0.0, ess_Tlast = 0.0;
    int64_t ess_batches = -1;  // -1: no ess_begin yet
    DevBuf<pdmp::DevChain> d_hdr;
    DevBuf<pdmp_event> d_ev;
    // general-degree kernel + logistic target + FactBoomerang
    int flow_kind = 0;
    DevBuf<double> d_mu, d_diag;
    bool needs_general = false;
    bool has_g1mask = false;  // pdmp_ensemble_set_neighbourhood: the tables' pattern is G ⊋ G1
    uint32_t mmax_all = 0;
    int target_kind = 0;
    DevBuf<uint16_t> d_pos16, d_selfpos16;
    DevBuf<double> d_qbval;
    DevBuf<uint32_t> d_member;
    DevBuf<int64_t> lg_Acp, lg_Arv, lg_Atcp, lg_Atrv;
    DevBuf<uint32_t> lg_Atrv32;
    DevBuf<double> d_hot;  // the moving halves of the records, packed, while a launch sweeps long logistic rows (pdmp_general.hip)
    DevBuf<double> lg_Anz, lg_Atnz, lg_y, lg_ny, lg_u0, lg_ns0;
    // packed tables of the LDS-resident logistic kernel (pdmp_logistic.hip); empty when the design does not qualify
    bool keep_integrals = true;  // pdmp_ensemble_set_path_integrals
    // streaming trace consumers (pdmp_ensemble_consume_*): cursor per (chain, coordinate), per-chain progress, the discretisation grid
    DevBuf<unsigned char> d_ccur, d_cmeta;
    DevBuf<double> d_cgrid;
    DevBuf<double> d_ccm;      // pdmp_ensemble_consume_cummean: (t, y / (2 t)) per event slot of the last consumed segment [nchains x cap x 2], or empty
    bool cons_cummean = false;
    bool consuming = false, cons_z = false;
    bool trace_appended = false;  // pdmp_debug_trace_append put events into the trace that no record knows of: run is refused until the next set_state
    // pdmp_ensemble_consume_async: a second trace buffer (the event loop writes one while the consumer reads the other), the consumer's stream,
    // the (ntrace, nevents) snapshots of the two most recent slices and the events that order the two streams
    DevBuf<pdmp_event> d_ev2;
    DevBuf<uint64_t> d_snap[2];
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_run_done = nullptr, ev_cons_done[2] = {nullptr, nullptr}, ev_c0 = nullptr, ev_c1 = nullptr;
    bool cons_pending[2] = {false, false}, cons_timed = false;
    int async_k = 0;
    // the consumer of the last pdmp_ensemble_consume_async is LAUNCHED behind the next event-loop launch (or at the next entry point that waits
    // for the device): the event loop's workgroups take the device first and the low-priority consumer fills what they leave -- launched first,
    // its workgroups would hold the slots the event loop's 4096 single-wave workgroups need and push part of them into a second round
    pdmp_event* deferred_buf = nullptr;
    int deferred_k = -1;
    double cons_dt = 0.0;
    int64_t cons_K = 0;
    DevBuf<pdmp::LgCoord> lg_coord;
    DevBuf<pdmp::LgObs> lg_obs;
    DevBuf<uint32_t> lg_arow;
    DevBuf<uint16_t> d_qrow16;
    double lg_gamma0 = 0.0;
    int64_t lg_k = 0;
    // sticky ZigZag
    DevBuf<double> d_kappa, d_thf;
    bool has_kappa = false;
    bool adaptscale = false;
    int64_t lg_nemax = 0;
    bool local_bound = false;
    DevBuf<double> d_qtval;
    DevBuf<double> d_sig_chain;
    int reversible = 0, strong_upperbounds = 0;
    // BPS
    DevBuf<int64_t> b_colptr, b_rowval;
    DevBuf<double> b_nzval, b_mu, b_mu_flow, b_x, b_th, b_scal, b_ev_t, b_ev_x, b_ev_th;
    int bps_flow_kind = 0;
    bool bps_ident = false;
    bool bps_diag = false;
    double bps_lambda = 0.0, bps_rho = 0.0;
    bool bps_gamma_is_I = false;  // flow Γ == I exactly: cholesky(Γ).L = I needs no factor from the caller
    bool bps_has_mass = false;    // a factor was supplied (identity factors are dropped: has_mass_tables stays false)
    bool bps_mass_tables = false;
    int bps_local_bound = 0, bps_subsample = 0;
    bool bps_own_target = false;  // set_target_gaussian_csc on a BouncyParticle ensemble: ∇ϕ! differs from B.Γ(x − B.μ)
    int bps_mom = 0;                // pdmp_ensemble_set_bps_moments: 0 off, 1 ∫x dt, 2 ∫x dt and ∫x² dt
    DevBuf<double> b_j1, b_j2;      // [nchains x d] the moments up to each chain's clock (kept by the event loop)
    DevBuf<double> b_jT, b_jT2;     // [nchains x d] the moments at the T of a read (pdmp_ensemble_bps_moments, the batch means / ESS sums)
    // sticky Bouncy Particle / Boomerang (pdmp_ensemble_set_bps_sticky, src/ss_not_fact.jl)
    bool bps_sticky = false;
    int bps_strong = 0;
    DevBuf<double> b_kappa, b_thf, b_tfrez;  // [d]; [nchains x d] saved speeds; [nchains x d] freezing / thaw times
    DevBuf<uint64_t> b_fmask, b_ev_f;        // [nchains x 16], [nchains x cap x 16] free masks (bit e & 63 of word e >> 6)
    // speed-recorded Bouncy Particle (pdmp_ensemble_set_flow_bps_modern, src/not_fact_samplers.jl:151-384)
    bool bps_modern = false;
    bool bps_udiag = false;
    int bps_oscn = 0;
    int64_t bps_record_limit = 0;
    DevBuf<double> b_udiag, b_sudiag, b_mstate;  // [d] u, [d] sqrt(u), [nchains x 4] {Δ, action, V, Δrec}
    DevBuf<int64_t> bt_colptr, bt_rowval;
    DevBuf<double> bt_nzval, bt_mu;
    DevBuf<int32_t> m_Lcp, m_Lrv, m_Ucp, m_Urv;
    DevBuf<double> m_Lnz, m_Unz;

    pdmp::ZzTables tables() const {
        pdmp::ZzTables tb{};
        tb.colptr = d_colptr.p;
        tb.rowval = d_rowval.p;
        tb.bval = d_bval.p;
        tb.tval = d_tval.p;
        tb.gmu_b = d_gmu_b.p;
        tb.gmu_t = has_tmu ? d_gmu_t.p : nullptr;
        tb.sptr = d_sptr.p;
        tb.sidx = d_sidx.p;
        tb.qptr = d_qptr.p;
        tb.pos = d_pos.p;
        tb.selfpos = d_selfpos.p;
        tb.c_shared = d_c.p;
        tb.c2_shared = reinterpret_cast<const double2*>(d_c2.p);
        tb.cc_shared = d_cc.p;
        tb.sigma = d_sigma.p;
        tb.gam8 = track_generic ? d_gam8.p : nullptr;
        tb.nb16 = track_generic ? d_nb16.p : nullptr;
        return tb;
    }
};

#define PDMP_LG_ROWS_DEFAULT 0  // chains per wavefront of the LDS-resident logistic kernel by default: 0 = one (pdmp_logistic.hip), 16 / 32 = rows (pdmp_logrows.hip)
#define PDMP_LG_FILL 0.95       // lanes of a 64-entry chunk a range fills on average (ranged sweep of long logistic rows; 0.6 .. 1.1 measured on C5)

// The event-loop kernel families of pdmp_ensemble_run.  select_family alone decides which one serves an ensemble; what a family does with the phase
// profile (pdmp_debug_set_phase_profile) and how its launcher's failure reads is stated here, once.
enum KernelFamily { FAM_BPS, FAM_GENERAL, FAM_LOGISTIC_LDS, FAM_LOGISTIC_ROWS, FAM_TRACKL, FAM_TRACKP, FAM_TRACK_GROUPS, FAM_EXACTP,
                    FAM_STICKY_SPEC, FAM_STICKY_RUN, FAM_SPEC, FAM_ONE_EVENT };
struct FamilyInfo {
    int phase_kind;        // the `kind` of pdmp_debug_phase_profile its kernels record (pdmp_debug.h), 0: they have no profiling form -- no buffer, no read-back
    const char* launcher;  // "<launcher> launch failed ..."
    bool hip_rc;           // ... with the return code spelled out as a hipError_t, or as a number
};
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
};

// neighbourhoods beyond 64 members, G ⊋ G1, FactBoomerang, the logistic target, adaptscale, LocalBound: pdmp_general.hip / pdmp_logistic.hip
static bool general_path(const pdmp_ensemble* e) { return e->needs_general || e->target_kind == 1 || e->adaptscale || e->local_bound; }

static pdmp_status launch_deferred_consumer(pdmp_ensemble* e) {
    if (e->deferred_k < 0) return PDMP_OK;
    const int k = e->deferred_k;
    e->deferred_k = -1;
    HIP_TRY(hipEventRecord(e->ev_c0, e->stream2));
    int rc = pdmp::launch_consume_events(e->deferred_buf, e->cfg.trace_capacity, e->d_hdr.p, e->d_snap[k].p, e->cfg.d, e->cfg.nchains, e->d_ccur.p,
                                         e->cons_z, e->d_cmeta.p, e->d_cgrid.p, e->cons_K, e->t0_state, e->cons_dt, e->stream2);
    if (rc != 0) return fail(PDMP_ERR_HIP, "consume launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipEventRecord(e->ev_c1, e->stream2));
    HIP_TRY(hipEventRecord(e->ev_cons_done[k], e->stream2));
    e->cons_pending[k] = true;
    e->cons_timed = true;
    return PDMP_OK;
}
// A consumer that was deferred behind the next run, the pending flags and the buffer parity of pdmp_ensemble_consume_async are dropped (set_state,
// consume_begin: the cursors they would write are about to be re-initialised); whatever already runs on the consumer's stream is waited for
static void discard_async_consumer(pdmp_ensemble* e) {
    e->deferred_k = -1;
    e->deferred_buf = nullptr;
    if (e->stream2) (void)hipStreamSynchronize(e->stream2);
    e->cons_pending[0] = e->cons_pending[1] = false;
    e->cons_timed = false;
    e->async_k = 0;
}
// hipDeviceSynchronize for an ensemble: a deferred consumer is launched first (what follows reads its results or the buffers it reads)
static hipError_t device_sync(pdmp_ensemble* e) {
    if (e && e->deferred_k >= 0 && launch_deferred_consumer(e) != PDMP_OK) {
        // (the launch's own message is in g_err; HIP_TRY would overwrite it with "unknown error": keep it as the prefix of what follows)
        g_deferred_err = g_err;
        return hipErrorLaunchFailure;
    }
    return hipDeviceSynchronize();
}

// the records / pairs of pdmp_trackp.hip's layout from the lines (pdmp_trackl.hip), where a run has left them behind
static pdmp_status ensure_canon(pdmp_ensemble* e) {
    if (!e->track_lines || !e->canon_stale) return PDMP_OK;
    HIP_TRY(device_sync(e));
    int rc = pdmp::launch_zz_trackl_unpack(e->d_tl_lines.p, e->d_tl_cold.p, e->d_rec.p, e->d_kp.p, e->cfg.d, e->dk, e->cfg.nchains, e->stream);
    if (rc != 0) return fail(PDMP_ERR_HIP, "trackl_unpack launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->canon_stale = false;
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

pdmp_status pdmp_debug_write_probe(int device, int64_t nchains, int64_t d, int64_t nrec, int iters, double* ms_out) {
    if (!ms_out || nchains <= 0 || d <= 0 || nrec <= 0 || iters <= 0) return fail(PDMP_ERR_INVALID, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible: libpdmp_mi355 has no CPU fallback");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> bx, bt;
    pdmp_status st;
    if ((st = bx.alloc((size_t)(nchains * nrec * d))) != PDMP_OK) return st;
    if ((st = bt.alloc((size_t)(nchains * nrec * d))) != PDMP_OK) return st;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    pdmp::launch_bps_write_probe(bx.p, bt.p, d, nrec, nrec, nchains, nullptr);  // warm-up (page faults, TLB)
    HIP_TRY(hipEventRecord(e0, nullptr));
    for (int k = 0; k < iters; ++k) {
        int rc = pdmp::launch_bps_write_probe(bx.p, bt.p, d, nrec, nrec, nchains, nullptr);
        if (rc != 0) return fail(PDMP_ERR_HIP, "write probe launch failed (%d)", rc);
    }
    HIP_TRY(hipEventRecord(e1, nullptr));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = (double)ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return PDMP_OK;
}

pdmp_status pdmp_debug_sector_probe(int device, int64_t nchains, int64_t d, int rounds, int write, int iters, double* ms_out) {
    if (!ms_out || nchains <= 0 || d <= 0 || rounds <= 0 || iters <= 0) return fail(PDMP_ERR_INVALID, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible: libpdmp_mi355 has no CPU fallback");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> rec, sink;
    pdmp_status st;
    if ((st = rec.alloc((size_t)(nchains * d * 8))) != PDMP_OK) return st;
    if ((st = sink.alloc(8)) != PDMP_OK) return st;
    HIP_TRY(hipMemset(rec.p, 0, (size_t)(nchains * d * 8) * sizeof(double)));
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    pdmp::launch_sector_probe(rec.p, d, nchains, rounds, write, sink.p, nullptr);  // warm-up
    HIP_TRY(hipEventRecord(e0, nullptr));
    for (int k = 0; k < iters; ++k) {
        int rc = pdmp::launch_sector_probe(rec.p, d, nchains, rounds, write, sink.p, nullptr);
        if (rc != 0) return fail(PDMP_ERR_HIP, "sector probe launch failed (%d)", rc);
    }
    HIP_TRY(hipEventRecord(e1, nullptr));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = (double)ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return PDMP_OK;
}

pdmp_status pdmp_debug_math_probe(int device, uint64_t seed, int64_t n, double* out) {
    if (!out || n <= 0) return fail(PDMP_ERR_INVALID, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> buf;
    pdmp_status st = buf.alloc((size_t)(8 * n));
    if (st != PDMP_OK) return st;
    int rc = pdmp::launch_math_probe(seed, n, buf.p, nullptr);
    if (rc != 0) return fail(PDMP_ERR_HIP, "math probe launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, buf.p, (size_t)(8 * n) * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

pdmp_status pdmp_debug_math_eval(int device, int fn, int64_t n, const double* a, const double* b, const double* c, double* out) {
#ifndef PDMP_EXTRA_KERNELS
    (void)device, (void)fn, (void)n, (void)a, (void)b, (void)c, (void)out;
    return fail(PDMP_ERR_UNSUPPORTED, "pdmp_debug_math_eval: the probe kernels live in the parity build (build.py --variant parity, -DPDMP_EXTRA_KERNELS)");
#else
    if (!a || !b || !c || !out || n <= 0 || n > ((int64_t)1 << 30)) return fail(PDMP_ERR_INVALID, "bad argument");
    decltype(&pdmp::launch_math_eval_kernels) launch = nullptr;
    switch (fn) {
    case PDMP_MATH_U01: case PDMP_MATH_LOG: case PDMP_MATH_EXP: case PDMP_MATH_SINCOS: case PDMP_MATH_SINCOS2PI: case PDMP_MATH_RANDN:
    case PDMP_MATH_RANDN2: case PDMP_MATH_RANDINT: case PDMP_MATH_DIV: case PDMP_MATH_SQRT:
    case PDMP_MATH_PT_DEV: case PDMP_MATH_PT_DEV_L: case PDMP_MATH_POS_DEV: launch = pdmp::launch_math_eval_kernels; break;
    case PDMP_MATH_PT_BPS: case PDMP_MATH_PT_BPS_L: case PDMP_MATH_POS_BPS: launch = pdmp::launch_math_eval_bps; break;
    case PDMP_MATH_PT_D1: case PDMP_MATH_POS_D1: launch = pdmp::launch_math_eval_1d; break;
    case PDMP_MATH_PT_G: case PDMP_MATH_PT_G_L: case PDMP_MATH_SIGMOID_G: case PDMP_MATH_POS_G: launch = pdmp::launch_math_eval_general; break;
    case PDMP_MATH_PT_Q: case PDMP_MATH_POS_Q: launch = pdmp::launch_math_eval_partition; break;
    case PDMP_MATH_PT_W_L: case PDMP_MATH_POS_W: launch = pdmp::launch_math_eval_trackp; break;
    case PDMP_MATH_PT_LOGISTIC_L: case PDMP_MATH_SIGMOID_LOGISTIC: case PDMP_MATH_POS_LOGISTIC: launch = pdmp::launch_math_eval_logistic; break;
    case PDMP_MATH_PT_TRACKL_L: case PDMP_MATH_POS_TRACKL: launch = pdmp::launch_math_eval_trackl; break;
    case PDMP_MATH_PT_X_L: case PDMP_MATH_POS_X: launch = pdmp::launch_math_eval_exactp; break;
    case PDMP_MATH_PT_R_L: case PDMP_MATH_SIGMOID_R: case PDMP_MATH_POS_R: launch = pdmp::launch_math_eval_logrows; break;
    default: return fail(PDMP_ERR_INVALID, "pdmp_debug_math_eval: unknown function id %d", fn);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> in, res;
    pdmp_status st = in.alloc((size_t)(3 * n));
    if (st == PDMP_OK) st = res.alloc((size_t)(2 * n));
    if (st != PDMP_OK) return st;
    HIP_TRY(hipMemcpy(in.p, a, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in.p + n, b, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in.p + 2 * n, c, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    int rc = launch(fn, n, in.p, in.p + n, in.p + 2 * n, res.p, nullptr);
    if (rc != 0) return fail(PDMP_ERR_HIP, "math eval launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, res.p, (size_t)(2 * n) * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
#endif
}

// The factorised samplers (ZigZag / FactBoomerang / sticky) and the non-factorised ones (BouncyParticle / Boomerang) keep different
// device state: an entry point of the wrong family is a call-order error, reported as a status (never a crash).
#define NEED_FACTORISED(e)                                                                                               \
    do {                                                                                                                 \
        if ((e) && (e)->cfg.sampler == PDMP_SAMPLER_BPS)                                                                 \
            return fail(PDMP_ERR_INVALID, "%s: the ensemble was created with PDMP_SAMPLER_BPS (use the pdmp_ensemble_*bps* calls)", \
                        __func__);                                                                                       \
    } while (0)

pdmp_status pdmp_debug_set_kernel(pdmp_ensemble* e, int kernel) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (kernel != PDMP_DEBUG_KERNEL_AUTO && kernel != PDMP_DEBUG_KERNEL_SEQ && kernel != PDMP_DEBUG_KERNEL_SPEC4 && kernel != PDMP_DEBUG_KERNEL_SPEC8 &&
        kernel != PDMP_DEBUG_KERNEL_EXACTP)
        return fail(PDMP_ERR_INVALID, "unknown kernel selector %d", kernel);
    if (e->has_flow) return fail(PDMP_ERR_INVALID, "pdmp_debug_set_kernel must precede set_flow_*");
    e->dbg_kernel = kernel;
    return PDMP_OK;
}
pdmp_status pdmp_debug_set_spec_g2(pdmp_ensemble* e, int on) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    e->dbg_spec_g2 = on ? 1 : 0;
    return PDMP_OK;
}
pdmp_status pdmp_debug_set_phase_profile(pdmp_ensemble* e, int on) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    e->dbg_phase = on ? 1 : 0;
    e->dbg_phase_valid = 0;
    return PDMP_OK;
}
pdmp_status pdmp_debug_phase_profile(pdmp_ensemble* e, double* out16, int* kind) {
    if (!e || !out16) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->dbg_phase_valid) return fail(PDMP_ERR_INVALID, "no phase profile recorded by the last run");
    memcpy(out16, e->dbg_phase_out, sizeof e->dbg_phase_out);
    if (kind) *kind = e->dbg_phase_valid;
    return PDMP_OK;
}
pdmp_status pdmp_debug_last_kernel(pdmp_ensemble* e, char* out, int64_t cap) {
    if (!e || !out || cap < 1) return fail(PDMP_ERR_INVALID, "null argument");
    snprintf(out, (size_t)cap, "%s", e->last_kernel);
    return PDMP_OK;
}
pdmp_status pdmp_debug_set_track_groups(pdmp_ensemble* e, int on) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    e->dbg_track_groups = (on == 1) ? 1 : 0;
    return PDMP_OK;
}
pdmp_status pdmp_debug_set_track_lines(pdmp_ensemble* e, int mode) {
    if (!e || mode < -1 || mode > 1) return fail(PDMP_ERR_INVALID, "track lines: -1 (by ensemble width), 0 (never), 1 (wherever the layout serves)");
    e->dbg_track_lines = mode;
    return PDMP_OK;
}
pdmp_status pdmp_debug_buffer_addresses(pdmp_ensemble* e, uint64_t* out8) {
    // where the state lives: tracked records, (key, t_old) pairs, trace slots, chain headers, canonical records, keys, the consts, the blob
    if (!e || !out8) return fail(PDMP_ERR_INVALID, "null argument");
    out8[0] = (uint64_t)(uintptr_t)e->d_trk.p;
    out8[1] = (uint64_t)(uintptr_t)e->d_kp.p;
    out8[2] = (uint64_t)(uintptr_t)e->d_ev.p;
    out8[3] = (uint64_t)(uintptr_t)e->d_hdr.p;
    out8[4] = (uint64_t)(uintptr_t)e->d_rec.p;
    out8[5] = (uint64_t)(uintptr_t)e->d_keys.p;
    out8[6] = (uint64_t)(uintptr_t)e->d_cc.p;
    out8[7] = (uint64_t)(uintptr_t)e->d_blob.p;
    return PDMP_OK;
}
pdmp_status pdmp_debug_set_placement(pdmp_ensemble* e, int tune, int place, const char* rec, const char* kp, const char* ev) {
    if (!e || tune < -1 || tune > 1 || place < 0 || place > 1) return fail(PDMP_ERR_INVALID, "placement: tune -1 (keep) / 0 / 1, place 0 / 1");
    for (const char* ptn : {rec, kp, ev})
        for (const char* q = ptn; q && *q; ++q)
            if (*q < '0' || *q > '2') return fail(PDMP_ERR_INVALID, "placement: a class pattern is a string of the digits 0, 1, 2");
    if (tune >= 0) e->place_tune = tune;
    e->place_cfg.enabled = place;
    e->place_cfg.rec = rec ? rec : "";
    e->place_cfg.kp = kp ? kp : "";
    e->place_cfg.ev = ev ? ev : "";
    return PDMP_OK;
}
pdmp_status pdmp_debug_placement(pdmp_ensemble* e, char* buf, size_t nbuf) {
    // how the large arrays were laid over the device's memory classes (pdmp_place.hip): "records 012012012 (31 chunks walked, 0.92 s); ..."
    if (!e || !buf || nbuf == 0) return fail(PDMP_ERR_INVALID, "null argument");
    std::string r;
    auto add = [&](const char* name, const pdmp::Placement& p, size_t bytes) {
        if (bytes < ((size_t)256 << 20)) return;
        char t[160];
        if (p.va) snprintf(t, sizeof t, "%s%s %s (%zu chunks walked, %.2f s)", r.empty() ? "" : "; ", name, p.classes.c_str(), p.walked, p.seconds);
        else snprintf(t, sizeof t, "%s%s hipMalloc (%.1f GB)", r.empty() ? "" : "; ", name, bytes / 1073741824.0);
        r += t;
    };
    add("records", e->d_rec.placed, e->d_rec.n * sizeof(pdmp::ZzRec));
    add("pairs", e->d_kp.placed, e->d_kp.n * sizeof(double));
    add("keys", e->d_keys.placed, e->d_keys.n * sizeof(double));
    add("trace", e->d_ev.placed, e->d_ev.n * sizeof(pdmp_event));
    add("lines", e->d_tl_lines.placed, e->d_tl_lines.n * sizeof(pdmp::TrLine));
    if (!e->tune_log.empty()) r += (r.empty() ? "" : "; ") + e->tune_log;
    snprintf(buf, nbuf, "%s", r.c_str());
    return PDMP_OK;
}
pdmp_status pdmp_debug_move_buffer(pdmp_ensemble* e, int which) {
    if (!e || !e->has_state) return fail(PDMP_ERR_INVALID, "move buffer: an ensemble with a state");
    if ((which >= 6) != (e->cfg.sampler == PDMP_SAMPLER_BPS)) return fail(PDMP_ERR_INVALID, "move buffer: 6-10 are the Bouncy Particle's arrays, 0-5 the ZigZag's");
    HIP_TRY(device_sync(e));
    // a copy of the array in newly allocated memory; the old allocation is KEPT (so the copy cannot land on the same pages) until the process ends
    auto move_buf = [](auto& b) -> hipError_t {
        if (!b.p || b.n == 0) return hipSuccess;
        void* np = nullptr;
        const size_t bytes = b.n * sizeof(*b.p);
        hipError_t r = hipMalloc(&np, bytes);
        if (r != hipSuccess) return r;
        r = hipMemcpy(np, b.p, bytes, hipMemcpyDeviceToDevice);
        if (r != hipSuccess) return r;
        b.p = static_cast<decltype(b.p)>(np);
        return hipSuccess;
    };
    switch (which) {
        case 0: HIP_TRY(move_buf(e->d_rec)); break;
        case 1: HIP_TRY(move_buf(e->d_kp)); break;
        case 2: HIP_TRY(move_buf(e->d_ev)); break;
        case 3: HIP_TRY(move_buf(e->d_hdr)); break;
        case 4: HIP_TRY(move_buf(e->d_cc)); break;
        case 5: HIP_TRY(move_buf(e->d_keys)); break;
        case 6: HIP_TRY(move_buf(e->b_ev_x)); break;
        case 7: HIP_TRY(move_buf(e->b_ev_th)); break;
        case 8: HIP_TRY(move_buf(e->b_x)); break;
        case 9: HIP_TRY(move_buf(e->b_th)); break;
        case 10: HIP_TRY(move_buf(e->b_ev_t)); break;
        default: return fail(PDMP_ERR_INVALID, "move buffer: 0 records, 1 pairs, 2 trace, 3 headers, 4 constants, 5 keys; BPS: 6 / 7 event x / theta, 8 / 9 x / theta, 10 event t");
    }
    return PDMP_OK;
}
pdmp_status pdmp_debug_set_helper_wave(pdmp_ensemble* e, int mode) {
    if (!e || mode < -1 || mode > 1) return fail(PDMP_ERR_INVALID, "helper wave: -1 (by occupancy), 0 (never), 1 (always)");
    e->dbg_helper_wave = mode;
    return PDMP_OK;
}
pdmp_status pdmp_debug_set_consumer_overlap(pdmp_ensemble* e, int mode) {
    if (!e || mode < -1 || mode > 1) return fail(PDMP_ERR_INVALID, "consumer overlap: -1 (by width), 0 (between slices), 1 (beside the next slice)");
    e->dbg_cons_overlap = mode;
    return PDMP_OK;
}
pdmp_status pdmp_debug_set_launch_count_limit(pdmp_ensemble* e, uint32_t n) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    e->dbg_count_limit = n;
    return PDMP_OK;
}
pdmp_status pdmp_debug_set_helper_steering(pdmp_ensemble* e, double gain, int target, double ahead) {
    // (zz_local_trackl reads them as block minima per quantum and events per window: hence the wide range of the first)
    if (!e || !(gain > 0.0 && gain <= 4096.0) || target < 1 || target > 64 || !(ahead >= 0.0))
        return fail(PDMP_ERR_INVALID, "helper steering: 0 < gain <= 4096 (<= 1 for the two-wave form), 1 <= target <= 64, ahead >= 0");
    e->dbg_hw_steer[0] = gain;
    e->dbg_hw_steer[1] = (double)target;
    e->dbg_hw_steer[2] = ahead;
    return PDMP_OK;
}
pdmp_status pdmp_debug_set_logistic_rows(pdmp_ensemble* e, int w) {
    if (!e || (w != -1 && w != 0 && w != 16 && w != 32)) return fail(PDMP_ERR_INVALID, "row width: -1 (default), 0 (one chain per wavefront), 16 or 32");
#ifndef PDMP_EXTRA_KERNELS
    if (w > 0) return fail(PDMP_ERR_UNSUPPORTED, "zz_logistic_rows_kernel is not part of this library: it lives in the parity build (build.py --variant parity, -DPDMP_EXTRA_KERNELS)");
#endif
    e->dbg_lg_rows = w;
    return PDMP_OK;
}
pdmp_status pdmp_debug_set_proposal_dump(pdmp_ensemble* e, int64_t n) {
    if (!e || n < 0) return fail(PDMP_ERR_INVALID, "bad argument");
    e->dbg_dump = n;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_create(const pdmp_config* cfg, pdmp_ensemble** out) {
    if (!cfg || !out) return fail(PDMP_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(pdmp_config))
        return fail(PDMP_ERR_INVALID, "pdmp_config.struct_size %u != %zu", cfg->struct_size, sizeof(pdmp_config));
    if (cfg->nchains <= 0 || cfg->d <= 0) return fail(PDMP_ERR_INVALID, "nchains and d must be positive");
    if (cfg->d >= (int64_t)1 << 31) return fail(PDMP_ERR_UNSUPPORTED, "d must be < 2^31");
    if (cfg->sampler != PDMP_SAMPLER_ZIGZAG_LOCAL && cfg->sampler != PDMP_SAMPLER_ZIGZAG_ALL &&
        cfg->sampler != PDMP_SAMPLER_BPS && cfg->sampler != PDMP_SAMPLER_STICKY_ZIGZAG)
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

// g1mask (optional, one flag per stored entry): the structural entries of the bounding Γ, i.e. G1 (src/sfact.jl:170), when the pattern handed
// over is the larger neighbourhood G ⊇ G1 of spdmp(∇ϕ, t0, x0, θ0, T, c, G, F, ...) (:162,171-179) with explicit zeros outside G1
static pdmp_status set_flow_common(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                                   const double* mu, const double* sigma, double lambda_ref, double rho, int kind,
                                   const uint8_t* g1mask = nullptr) {
    if (!e || !colptr || !rowval || !nzval) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d;
    if (colptr[0] != 0) return fail(PDMP_ERR_INVALID, "colptr[0] must be 0 (0-based CSC)");
    const int64_t nnz = colptr[d];
    if (nnz <= 0 || nnz >= (int64_t)1 << 31) return fail(PDMP_ERR_INVALID, "bad nnz %lld", (long long)nnz);
    if (lambda_ref < 0) return fail(PDMP_ERR_INVALID, "lambda_ref < 0");
    e->colptr.assign(d + 1, 0);
    e->rowval.assign(nnz, 0);
    e->bval.assign(nzval, nzval + nnz);
    for (int64_t i = 0; i <= d; ++i) {
        if (colptr[i] < 0 || colptr[i] > nnz || (i > 0 && colptr[i] < colptr[i - 1]))
            return fail(PDMP_ERR_INVALID, "colptr not monotone at %lld", (long long)i);
        e->colptr[i] = (uint32_t)colptr[i];
    }
    std::vector<uint8_t> selfpos(d, 0);
    std::vector<uint16_t> selfpos16(d, 0);
    bool general = false;
    uint32_t mmax_all = 0;
    for (int64_t i = 0; i < d; ++i) {
        const int64_t k = colptr[i + 1] - colptr[i];
        if (k > 4096) return fail(PDMP_ERR_UNSUPPORTED, "column %lld has %lld > 4096 non-zeros", (long long)i, (long long)k);
        bool has_diag = false;
        for (int64_t p = colptr[i]; p < colptr[i + 1]; ++p) {
            const int64_t r = rowval[p];
            if (r < 0 || r >= d) return fail(PDMP_ERR_INVALID, "row index out of range in column %lld", (long long)i);
            if (p > colptr[i] && rowval[p - 1] >= r)
                return fail(PDMP_ERR_INVALID, "rows of column %lld are not strictly ascending", (long long)i);
            if (r == i && (!g1mask || g1mask[p])) {
                has_diag = true;
                selfpos[i] = (uint8_t)(p - colptr[i]);
                selfpos16[i] = (uint16_t)(p - colptr[i]);
            }
            e->rowval[p] = (uint32_t)r;
        }
        if (!has_diag)
            return fail(PDMP_ERR_UNSUPPORTED, "Γ[%lld,%lld] is structurally zero: i must belong to G1[i]", (long long)i,
                        (long long)i);
    }
    e->nnz = nnz;
    e->mu.assign(d, 0.0);
    if (mu) e->mu.assign(mu, mu + d);
    e->sigma.assign(d, 1.0);
    if (sigma) e->sigma.assign(sigma, sigma + d);
    e->lambda_ref = lambda_ref;
    e->rho = rho;

    // gmu_b[i] = idot(Γ, i, μ) (src/fact_samplers.jl:51), summed in CSC order like idot (src/common.jl:16-24)
    std::vector<double> gmu(d, 0.0);
    for (int64_t i = 0; i < d; ++i) {
        double s = 0.0;
        for (uint32_t p = e->colptr[i]; p < e->colptr[i + 1]; ++p) s += e->bval[p] * e->mu[e->rowval[p]];
        gmu[i] = s;
    }

    // S[i] = G1[i] ++ G2[i], G2[i] = (∪_{j∈G1[i]} G1[j]) \ G1[i]  (src/sfact.jl:178), both ascending
    std::vector<uint32_t> sptr(d + 1, 0), sidx;
    sidx.reserve((size_t)nnz * 3);
    std::vector<uint32_t> qptr(nnz + 1, 0);
    std::vector<uint8_t> pos;
    pos.reserve((size_t)nnz * 5);
    std::vector<uint16_t> pos16, qrow16;
    std::vector<double> qbval;     // Γ value of every (member j of G1[i], entry of column j) pair, same order as pos16
    std::vector<uint32_t> member;  // per entry p of column i: {j, k_j, qptr[p], 0} -- one 16-byte load per member
    pos16.reserve((size_t)nnz * 5);
    std::vector<uint32_t> tmp;
    for (int64_t i = 0; i < d; ++i) {
        const uint32_t c0 = e->colptr[i], c1 = e->colptr[i + 1];
        tmp.clear();
        for (uint32_t p = c0; p < c1; ++p) {
            if (g1mask && !g1mask[p]) continue;  // G2[i] = ∪_{j ∈ G1[i]} G1[j] \ G[i], src/sfact.jl:178
            const uint32_t j = e->rowval[p];
            for (uint32_t q = e->colptr[j]; q < e->colptr[j + 1]; ++q)
                if (!g1mask || g1mask[q]) tmp.push_back(e->rowval[q]);
        }
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        const size_t s0 = sidx.size();
        for (uint32_t p = c0; p < c1; ++p) sidx.push_back(e->rowval[p]);
        for (uint32_t v : tmp) {
            if (!std::binary_search(e->rowval.begin() + c0, e->rowval.begin() + c1, v)) sidx.push_back(v);
        }
        const size_t m = sidx.size() - s0;
        if (m > 4096)
            return fail(PDMP_ERR_UNSUPPORTED, "two-hop neighbourhood of coordinate %lld has %zu > 4096 members",
                        (long long)i, m);
        if (m > 64 || (c1 - c0) > 64) general = true;  // beyond one lane per member: pdmp_general.hip
        mmax_all = std::max<uint32_t>(mmax_all, (uint32_t)m);
        sptr[i + 1] = (uint32_t)sidx.size();
        // positions inside S[i] of the members of G1[j], j = G1[i][jj]
        for (uint32_t p = c0; p < c1; ++p) {
            const uint32_t j = e->rowval[p];
            qptr[p] = (uint32_t)pos.size();
            if (g1mask && !g1mask[p]) continue;  // (a member of G[i] \ G1[i]: moved, never re-bounded)
            for (uint32_t q = e->colptr[j]; q < e->colptr[j + 1]; ++q) {
                if (g1mask && !g1mask[q]) continue;
                const uint32_t r = e->rowval[q];
                size_t where = m;
                for (size_t w = 0; w < m; ++w) {
                    if (sidx[s0 + w] == r) {
                        where = w;
                        break;
                    }
                }
                if (where == m)
                    return fail(PDMP_ERR_UNSUPPORTED,
                                "pattern of Γ is not symmetric: row %u of column %u is not reachable from %lld", r, j,
                                (long long)i);
                pos.push_back((uint8_t)where);
                pos16.push_back((uint16_t)where);
                qrow16.push_back((uint16_t)r);  // (used by the small-d kernel only: d < 65536 is checked there)
                qbval.push_back(e->bval[q]);
            }
        }
    }
    qptr[nnz] = (uint32_t)pos.size();
    if (pos.empty()) pos.push_back(0);
    if (pos16.empty()) pos16.push_back(0);
    if (qbval.empty()) qbval.push_back(0.0);
    if (qrow16.empty()) qrow16.push_back(0);
    member.resize((size_t)nnz * 4 + 4, 0u);
    for (int64_t p = 0; p < nnz; ++p) {
        const uint32_t j = e->rowval[p];
        member[(size_t)p * 4 + 0] = j;
        uint32_t kj = 0;
        for (uint32_t q = e->colptr[j]; q < e->colptr[j + 1]; ++q) kj += (!g1mask || g1mask[q]) ? 1u : 0u;
        member[(size_t)p * 4 + 1] = (g1mask && !g1mask[p]) ? 0u : kj;
        member[(size_t)p * 4 + 2] = qptr[p];
        member[(size_t)p * 4 + 3] = (!g1mask || g1mask[p]) ? 1u : 0u;
    }
    {
        uint32_t hist[16] = {0}, best = 0;
        for (int64_t k = 0; k < d; ++k) hist[std::min<uint32_t>(e->colptr[(size_t)k + 1] - e->colptr[(size_t)k], 15u)] += 1;
        for (uint32_t k = 1; k < 16; ++k)
            if (hist[k] > hist[best]) best = k;
        e->typ_extra = best > 0 ? best - 1u : 0u;
    }
    e->flow_kind = kind;
    e->has_g1mask = g1mask != nullptr;
    e->needs_general = general || kind == 1 || e->has_g1mask;  // FactBoomerang and G ⊋ G1 run on the general kernel
    e->mmax_all = mmax_all;
    {
        std::vector<double> diag((size_t)d, 0.0);
        for (int64_t i = 0; i < d; ++i) diag[i] = e->bval[e->colptr[i] + selfpos16[i]];
        pdmp_status sd = e->d_diag.upload(diag);
        if (sd != PDMP_OK) return sd;
        if ((sd = e->d_mu.upload(e->mu)) != PDMP_OK) return sd;
    }

    e->h_gmu_b = gmu;
    e->h_sptr = sptr;
    e->h_sidx = sidx;
    e->h_qptr = qptr;
    e->h_pos = pos;
    e->h_selfpos = selfpos;

    pdmp_status st;
    if ((st = e->d_colptr.upload(e->colptr)) != PDMP_OK) return st;
    if ((st = e->d_rowval.upload(e->rowval)) != PDMP_OK) return st;
    if ((st = e->d_bval.upload(e->bval)) != PDMP_OK) return st;
    if ((st = e->d_gmu_b.upload(gmu)) != PDMP_OK) return st;
    if ((st = e->d_sptr.upload(sptr)) != PDMP_OK) return st;
    if ((st = e->d_sidx.upload(sidx)) != PDMP_OK) return st;
    if ((st = e->d_qptr.upload(qptr)) != PDMP_OK) return st;
    if ((st = e->d_pos.upload(pos)) != PDMP_OK) return st;
    if ((st = e->d_selfpos.upload(selfpos)) != PDMP_OK) return st;
    if ((st = e->d_sigma.upload(e->sigma)) != PDMP_OK) return st;
    if ((st = e->d_pos16.upload(pos16)) != PDMP_OK) return st;
    if ((st = e->d_qbval.upload(qbval)) != PDMP_OK) return st;
    if ((st = e->d_qrow16.upload(qrow16)) != PDMP_OK) return st;
    if ((st = e->d_member.upload(member)) != PDMP_OK) return st;
    if ((st = e->d_selfpos16.upload(selfpos16)) != PDMP_OK) return st;
    e->target_kind = 0;

    const int64_t nkeys = d + 1;  // slot d is the refresh clock (+Inf when λref = 0)
    e->nblk = (uint32_t)((nkeys + 63) / 64);
    e->nblk_pad = (e->nblk + 1u) & ~1u;
    e->dk = (int64_t)e->nblk * 64;
    e->local_bound = false;
    e->adaptscale = false;
    e->has_flow = true;
    e->has_target = false;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_flow_zigzag(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval,
                                          const double* nzval, const double* mu, const double* sigma,
                                          double lambda_ref, double rho) {
    return set_flow_common(e, colptr, rowval, nzval, mu, sigma, lambda_ref, rho, 0);
}

pdmp_status pdmp_ensemble_set_flow_factboomerang(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval,
                                                 const double* nzval, const double* mu, const double* sigma,
                                                 double lambda_ref, double rho) {
    if (e && e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL && e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_ALL)
        return fail(PDMP_ERR_UNSUPPORTED, "FactBoomerang is available for the factorised drivers spdmp / pdmp (PDMP_SAMPLER_ZIGZAG_LOCAL / _ALL)");
    if (!(lambda_ref > 0)) return fail(PDMP_ERR_INVALID, "FactBoomerang needs a strictly positive refreshment rate");
    return set_flow_common(e, colptr, rowval, nzval, mu, sigma, lambda_ref, rho, 1);
}

pdmp_status pdmp_ensemble_set_neighbourhood(pdmp_ensemble* e, const int64_t* g_colptr, const int64_t* g_rowval) {
    if (!e || !g_colptr || !g_rowval) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_zigzag / set_flow_factboomerang first");
    if (e->has_g1mask) return fail(PDMP_ERR_INVALID, "the neighbourhood was set already: call set_flow_* again first");
    if (e->cfg.sampler == PDMP_SAMPLER_ZIGZAG_ALL) return fail(PDMP_ERR_INVALID, "pdmp is spdmp with G = All(): it takes no G");
    const int64_t d = e->cfg.d;
    if (g_colptr[0] != 0) return fail(PDMP_ERR_INVALID, "colptr[0] must be 0");
    const int64_t gn = g_colptr[d];
    if (gn < e->nnz || gn >= (int64_t)1 << 31) return fail(PDMP_ERR_INVALID, "G must contain G1 (src/sfact.jl:177)");
    std::vector<int64_t> cp(g_colptr, g_colptr + d + 1), rv(g_rowval, g_rowval + gn);
    std::vector<double> nz((size_t)gn, 0.0);
    std::vector<uint8_t> mask((size_t)gn, 0);
    for (int64_t i = 0; i < d; ++i) {
        if (cp[i + 1] < cp[i]) return fail(PDMP_ERR_INVALID, "G colptr not monotone at %lld", (long long)i);
        uint32_t q = e->colptr[i];
        const uint32_t q1 = e->colptr[i + 1];
        for (int64_t p = cp[i]; p < cp[i + 1]; ++p) {
            const int64_t r = rv[p];
            if (r < 0 || r >= d || (p > cp[i] && rv[p - 1] >= r)) return fail(PDMP_ERR_INVALID, "G[%lld] must be ascending and in range", (long long)i);
            if (q < q1 && (int64_t)e->rowval[q] == r) {
                nz[(size_t)p] = e->bval[q];
                mask[(size_t)p] = 1;
                ++q;
            }
        }
        if (q != q1)  // @assert all(a.second ⊇ b.second for (a, b) in zip(G, G1)), src/sfact.jl:177
            return fail(PDMP_ERR_INVALID, "G[%lld] does not contain G1[%lld] = rowvals(F.Γ)[nzrange(F.Γ, %lld)] (src/sfact.jl:177)", (long long)i,
                        (long long)i, (long long)i);
    }
    if (gn == e->nnz) return PDMP_OK;  // G == G1: Matched()
    const std::vector<double> mu = e->mu, sigma = e->sigma;
    return set_flow_common(e, cp.data(), rv.data(), nz.data(), mu.data(), sigma.data(), e->lambda_ref, e->rho, e->flow_kind, mask.data());
}

pdmp_status pdmp_ensemble_set_target_gaussian_csc(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval,
                                                  const double* nzval, const double* mu) {
    if (!e || !colptr || !rowval || !nzval) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler == PDMP_SAMPLER_BPS) {
        // pdmp(∇ϕ!, t0, x0, θ0, T, c, B::BouncyParticle): ∇ϕ! is the caller's (src/not_fact_samplers.jl:122), ab(…GlobalBound…) uses B.Γ, B.μ
        // (:26-28).  A Gaussian target of its own: ∇ϕ!(y, x) = Γt(x − μt).
        if (!e->has_flow || e->bps_flow_kind != 0)
            return fail(PDMP_ERR_INVALID, "a target of its own follows set_flow_bps (set_flow_boomerang takes the target directly)");
        HIP_TRY(hipSetDevice(e->cfg.device));
        const int64_t dd = e->cfg.d;
        if (colptr[0] != 0) return fail(PDMP_ERR_INVALID, "colptr[0] must be 0 (0-based CSC)");
        const int64_t tn = colptr[dd];
        if (tn <= 0 || tn >= (int64_t)1 << 31) return fail(PDMP_ERR_INVALID, "bad nnz %lld", (long long)tn);
        for (int64_t i = 0; i < dd; ++i) {
            if (colptr[i + 1] < colptr[i]) return fail(PDMP_ERR_INVALID, "target colptr not monotone at %lld", (long long)i);
            for (int64_t p = colptr[i]; p < colptr[i + 1]; ++p)
                if (rowval[p] < 0 || rowval[p] >= dd || (p > colptr[i] && rowval[p - 1] >= rowval[p]))
                    return fail(PDMP_ERR_INVALID, "target column %lld: rows must be ascending and in range", (long long)i);
        }
        pdmp_status stb;
        if ((stb = e->bt_colptr.upload(std::vector<int64_t>(colptr, colptr + dd + 1))) != PDMP_OK) return stb;
        if ((stb = e->bt_rowval.upload(std::vector<int64_t>(rowval, rowval + tn))) != PDMP_OK) return stb;
        if ((stb = e->bt_nzval.upload(std::vector<double>(nzval, nzval + tn))) != PDMP_OK) return stb;
        std::vector<double> tm((size_t)dd, 0.0);
        if (mu) tm.assign(mu, mu + dd);
        if ((stb = e->bt_mu.upload(tm)) != PDMP_OK) return stb;
        e->bps_own_target = true;
        e->has_state = false;
        return PDMP_OK;
    }
    NEED_FACTORISED(e);
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_zigzag must be called first");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d;
    if (colptr[0] != 0) return fail(PDMP_ERR_INVALID, "colptr[0] must be 0 (0-based CSC)");
    for (int64_t i = 0; i < d; ++i) {
        if (colptr[i + 1] < colptr[i]) return fail(PDMP_ERR_INVALID, "target colptr not monotone at %lld", (long long)i);
        for (int64_t p = colptr[i]; p < colptr[i + 1]; ++p)
            if (rowval[p] < 0 || rowval[p] >= d)
                return fail(PDMP_ERR_INVALID, "target row index %lld out of range in column %lld", (long long)rowval[p], (long long)i);
    }
    // align Γt to the flow's pattern: slots absent from Γt carry 0.0 (s + 0.0*x == s bit-for-bit)
    std::vector<double> tval(e->nnz, 0.0), gmu_t(d, 0.0);
    for (int64_t i = 0; i < d; ++i) {
        uint32_t q = e->colptr[i];
        const uint32_t q1 = e->colptr[i + 1];
        double s = 0.0;
        for (int64_t p = colptr[i]; p < colptr[i + 1]; ++p) {
            const int64_t r = rowval[p];
            if (p > colptr[i] && rowval[p - 1] >= r)
                return fail(PDMP_ERR_INVALID, "rows of target column %lld are not strictly ascending", (long long)i);
            while (q < q1 && (int64_t)e->rowval[q] < r) ++q;
            if (q == q1 || (int64_t)e->rowval[q] != r)
                return fail(PDMP_ERR_UNSUPPORTED,
                            "target Γt[%lld,%lld] lies outside the flow's pattern G[%lld] (src/sfact.jl:116)",
                            (long long)r, (long long)i, (long long)i);
            tval[q] = nzval[p];
            if (mu) s += nzval[p] * mu[r];
        }
        gmu_t[i] = s;
    }
    e->has_tmu = (mu != nullptr);
    e->h_gmu_t = gmu_t;
    e->target_kind = 0;
    e->h_tval = tval;
    pdmp_status st;
    if ((st = e->d_tval.upload(tval)) != PDMP_OK) return st;
    if ((st = e->d_gmu_t.upload(gmu_t)) != PDMP_OK) return st;
    e->has_target = true;
    e->has_state = false;
    return PDMP_OK;
}

// Per-coordinate "neighbourhood program": everything a proposal at coordinate i needs that depends on i alone,
// packed in 64-bit words so that ONE coalesced wave load brings it on chip (kernel: zz_local_run_kernel).
//   [0]                 k | m<<8 | selfpos<<16 | kjmax<<24          (kjmax = max_j |G1[j]|, j in G1[i])
//   [1 .. 1+SW)         S[i] = G1[i] ++ G2[i], two u32 ids per word                (SW = ceil(MMAX/2))
//   then k sub-records of R = 4 + PW + KMAX words, one per j = G1[i][jj]:
//     [0] Γt[j,i] (target)   [1] Γ[:,j]·μ   [2] c[j]   [3] |G1[j]|
//     [4 .. 4+PW)        positions inside S[i] of the members of G1[j], 8 bytes per word (PW = ceil(KMAX/8))
//     [4+PW .. +KMAX)    Γ[G1[j], j] (bounding precision values, CSC order)
static pdmp_status build_blob(pdmp_ensemble* e, const double* c) {
    const int64_t d = e->cfg.d;
    uint32_t kmax = 0, mmax = 0;
    for (int64_t i = 0; i < d; ++i) {
        kmax = std::max(kmax, e->colptr[i + 1] - e->colptr[i]);
        mmax = std::max(mmax, e->h_sptr[i + 1] - e->h_sptr[i]);
    }
    const uint32_t SW = (mmax + 1) / 2, PW = (kmax + 7) / 8, R = 4 + PW + kmax;
    const uint32_t W = 1 + SW + kmax * R;
    const uint32_t Wpad = (W + 1u) & ~1u;
    if ((double)W * 8.0 * (double)d > 4.0e9)
        return fail(PDMP_ERR_UNSUPPORTED, "neighbourhood programs would take %.1f GB (d=%lld, max column nnz %u)",
                    (double)W * 8.0 * (double)d / 1e9, (long long)d, kmax);
    if (pdmp::zz_local_lds_bytes(e->nblk_pad, Wpad) > 160 * 1024)
        return fail(PDMP_ERR_UNSUPPORTED, "d = %lld / max column nnz %u need %zu bytes of LDS per chain (> 160 KiB)",
                    (long long)d, kmax, pdmp::zz_local_lds_bytes(e->nblk_pad, Wpad));
    std::vector<uint64_t> blob((size_t)Wpad * (size_t)d, 0);
    auto bits = [](double v) {
        uint64_t u;
        memcpy(&u, &v, sizeof u);
        return u;
    };
    for (int64_t i = 0; i < d; ++i) {
        uint64_t* B = blob.data() + (size_t)i * Wpad;
        const uint32_t c0 = e->colptr[i], k = e->colptr[i + 1] - c0;
        const uint32_t s0 = e->h_sptr[i], m = e->h_sptr[i + 1] - s0;
        uint32_t kjmax = 0;
        for (uint32_t w = 0; w < m; ++w) {
            // member ids RELATIVE to i (two's complement u32): coordinates with the same local structure -- every interior
            // point of a lattice -- then share one program, and the table shrinks from d programs to a few dozen
            const uint64_t id = (uint32_t)(e->h_sidx[s0 + w] - (uint32_t)i);
            B[1 + (w >> 1)] |= (w & 1) ? (id << 32) : id;
        }
        for (uint32_t jj = 0; jj < k; ++jj) {
            const uint32_t j = e->rowval[c0 + jj];
            const uint32_t cj0 = e->colptr[j], kj = e->colptr[j + 1] - cj0;
            kjmax = std::max(kjmax, kj);
            uint64_t* S = B + 1 + SW + (size_t)jj * R;
            S[0] = bits(e->h_tval[c0 + jj]);
            S[1] = bits(e->h_gmu_b[j]);
            S[2] = bits(c[j]);
            S[3] = kj;
            const uint32_t q0 = e->h_qptr[c0 + jj];
            for (uint32_t pp = 0; pp < kj; ++pp) {
                S[4 + (pp >> 3)] |= (uint64_t)e->h_pos[q0 + pp] << (8 * (pp & 7));
                S[4 + PW + pp] = bits(e->bval[cj0 + pp]);
            }
        }
        B[0] = (uint64_t)k | ((uint64_t)m << 8) | ((uint64_t)e->h_selfpos[i] << 16) | ((uint64_t)kjmax << 24);
    }
    // de-duplicate identical programs
    std::vector<uint32_t> tix((size_t)d, 0);
    std::vector<uint64_t> templates;
    {
        std::unordered_map<std::string, uint32_t> seen;
        seen.reserve(1024);
        for (int64_t i = 0; i < d; ++i) {
            const uint64_t* B = blob.data() + (size_t)i * Wpad;
            std::string key(reinterpret_cast<const char*>(B), (size_t)Wpad * 8);
            auto it = seen.find(key);
            if (it == seen.end()) {
                const uint32_t id = (uint32_t)seen.size();
                seen.emplace(std::move(key), id);
                templates.insert(templates.end(), B, B + Wpad);
                tix[i] = id;
            } else {
                tix[i] = it->second;
            }
        }
        e->n_templates = seen.size();
        std::vector<int64_t> cnt(seen.size(), 0);
        for (int64_t i = 0; i < d; ++i) cnt[tix[i]] += 1;
        e->common_tix = (uint32_t)(std::max_element(cnt.begin(), cnt.end()) - cnt.begin());
    }
    blob.swap(templates);
    pdmp_status stt = e->d_tix.upload(tix);
    if (stt != PDMP_OK) return stt;
    e->blob_w = W;
    e->blob_w_pad = Wpad;
    e->blob_sw = SW;
    e->blob_pw = PW;
    e->blob_kmax = kmax;
    e->blob_mmax = mmax;
    // (pdmp_debug_set_kernel(PDMP_DEBUG_KERNEL_SEQ) forces the one-event-per-iteration kernel: A/B runs, parity tests)
    // eight events per iteration off the lattice: per-coordinate tables instead of blob templates (pdmp_spec8g.inc)
    e->has_g8 = false;
    e->g8_same = false;
    // (every graph of that size whose blob geometry is not EXACTLY the 2-d lattice's, which zz_local_spec8_kernel serves from LDS templates)
    e->g8_gw = 8;
    if (kmax <= 8 && mmax <= 64 && d >= 2048 && d <= 16384 && !(SW == 7 && PW == 1 && kmax == 5 && Wpad == 58)) {
        // 8 lanes per event (eight events per iteration) up to |S| = 32, 16 lanes (four events) up to 64: a lane owns zone positions gl + q GW
        const uint32_t GW = (mmax <= 32) ? 8u : 16u, LSTR = GW + 8u;
        e->g8_gw = (int)GW;
        std::vector<uint64_t> line((size_t)d * LSTR, 0ull);
        std::vector<double> member((size_t)d * 16, 0.0), gamt((size_t)d * 8, 0.0);
        bool same = true;
        for (int64_t i = 0; i < d; ++i) {
            const uint32_t c0 = e->colptr[i], k = e->colptr[i + 1] - c0;
            const uint32_t s0 = e->h_sptr[i], m = e->h_sptr[i + 1] - s0;
            uint16_t ids[64];
            for (uint32_t w = 0; w < 4 * GW; ++w) ids[w] = (w < m) ? (uint16_t)(e->h_sidx[s0 + w] | (w < k ? 0x8000u : 0u)) : (uint16_t)0x7FFF;
            for (uint32_t gl = 0; gl < GW; ++gl)
                line[(size_t)i * LSTR + gl] = (uint64_t)ids[gl] | ((uint64_t)ids[gl + GW] << 16) | ((uint64_t)ids[gl + 2 * GW] << 32) | ((uint64_t)ids[gl + 3 * GW] << 48);
            for (uint32_t jj = 0; jj < k; ++jj) {
                gamt[(size_t)i * 8 + jj] = e->h_tval[c0 + jj];
                member[(size_t)i * 16 + jj] = e->bval[c0 + jj];
                same = same && e->h_tval[c0 + jj] == e->bval[c0 + jj];
                const uint32_t j = e->rowval[c0 + jj];
                const uint32_t kj = e->colptr[j + 1] - e->colptr[j];
                const uint32_t q0 = e->h_qptr[c0 + jj];
                uint64_t pw = 0;
                for (uint32_t pp = 0; pp < kj; ++pp) pw |= (uint64_t)e->h_pos[q0 + pp] << (8 * pp);
                line[(size_t)i * LSTR + GW + jj] = pw;
            }
            member[(size_t)i * 16 + 8] = c[i];
            member[(size_t)i * 16 + 9] = e->h_gmu_b[i];
        }
        pdmp_status sg;
        if ((sg = e->d_g8_line.upload(line)) != PDMP_OK) return sg;
        if ((sg = e->d_g8_member.upload(member)) != PDMP_OK) return sg;
        if (!same && (sg = e->d_g8_gamt.upload(gamt)) != PDMP_OK) return sg;
        e->g8_same = same;
        e->has_g8 = true;
    }
    e->use_spec = pdmp::zz_spec_supported(e->nblk, mmax, kmax) && e->dbg_kernel != PDMP_DEBUG_KERNEL_SEQ &&
                  (mmax > 16 ? pdmp::zz_spec_wide_lds_bytes(e->nblk_pad, Wpad) : pdmp::zz_spec_lds_bytes(e->nblk_pad, Wpad)) <= 64 * 1024;
    return e->d_blob.upload(blob);
}

} // extern "C" (reopened below)

extern "C" pdmp_status pdmp_ensemble_set_target_logistic(pdmp_ensemble* e, int64_t n, const int64_t* A_colptr,
                                                         const int64_t* A_rowval, const double* A_nzval,
                                                         const int64_t* At_colptr, const int64_t* At_rowval,
                                                         const double* At_nzval, const double* y, const double* ny,
                                                         const double* mu, double gamma0, int64_t k_sub) {
    if (!e || !A_colptr || !A_rowval || !A_nzval || !At_colptr || !At_rowval || !At_nzval || !y || !ny || !mu)
        return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_zigzag must be called first");
    if (n <= 0 || k_sub <= 0) return fail(PDMP_ERR_INVALID, "n and k_sub must be positive");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t p = e->cfg.d;
    const int64_t nnzA = A_colptr[p], nnzAt = At_colptr[n];
    if (A_colptr[0] != 0 || At_colptr[0] != 0 || nnzA != nnzAt) return fail(PDMP_ERR_INVALID, "A / At are inconsistent");
    for (int64_t j = 0; j < p; ++j)
        if (A_colptr[j + 1] <= A_colptr[j])
            return fail(PDMP_ERR_UNSUPPORTED, "coordinate %lld has no observation (rand over an empty range)", (long long)j);
    // control-variate terms sigmoidn(u0), nsigmoid(u0) with u0 = idot(At, row, μ) (src/common.jl:16-24 order): constants of
    // the observation, evaluated here with the SAME deterministic exp the kernels use (bit-identical on x86-64 and gfx950)
    std::vector<double> sn0((size_t)n, 0.0), ns0((size_t)n, 0.0);
    for (int64_t r = 0; r < n; ++r) {
        double s = 0.0;
        for (int64_t q = At_colptr[r]; q < At_colptr[r + 1]; ++q) {
            if (At_rowval[q] < 0 || At_rowval[q] >= p) return fail(PDMP_ERR_INVALID, "At row index out of range");
            s += At_nzval[q] * mu[At_rowval[q]];
        }
        sn0[r] = 1.0 / (1.0 + pdmp_exp(s));     // sigmoidn(u0) = sigmoid(-u0) = inv(1 + exp(u0))
        ns0[r] = -(1.0 / (1.0 + pdmp_exp(-s)));  // nsigmoid(u0) = -sigmoid(u0)
    }
    pdmp_status st;
    if ((st = e->lg_Acp.upload(std::vector<int64_t>(A_colptr, A_colptr + p + 1))) != PDMP_OK) return st;
    if ((st = e->lg_Arv.upload(std::vector<int64_t>(A_rowval, A_rowval + nnzA))) != PDMP_OK) return st;
    if ((st = e->lg_Anz.upload(std::vector<double>(A_nzval, A_nzval + nnzA))) != PDMP_OK) return st;
    if ((st = e->lg_Atcp.upload(std::vector<int64_t>(At_colptr, At_colptr + n + 1))) != PDMP_OK) return st;
    if ((st = e->lg_Atrv.upload(std::vector<int64_t>(At_rowval, At_rowval + nnzAt))) != PDMP_OK) return st;
    {
        std::vector<uint32_t> r32((size_t)nnzAt);
        for (int64_t q = 0; q < nnzAt; ++q) r32[(size_t)q] = (uint32_t)At_rowval[q];
        if ((st = e->lg_Atrv32.upload(r32)) != PDMP_OK) return st;
    }
    if ((st = e->lg_Atnz.upload(std::vector<double>(At_nzval, At_nzval + nnzAt))) != PDMP_OK) return st;
    if ((st = e->lg_y.upload(std::vector<double>(y, y + n))) != PDMP_OK) return st;
    if ((st = e->lg_ny.upload(std::vector<double>(ny, ny + n))) != PDMP_OK) return st;
    if ((st = e->lg_u0.upload(sn0)) != PDMP_OK) return st;
    if ((st = e->lg_ns0.upload(ns0)) != PDMP_OK) return st;
    // the kernels' table struct wants tval / gmu_t allocated even if unused
    if ((st = e->d_tval.upload(std::vector<double>((size_t)e->nnz, 0.0))) != PDMP_OK) return st;
    if ((st = e->d_gmu_t.upload(std::vector<double>((size_t)p, 0.0))) != PDMP_OK) return st;
    e->has_tmu = false;
    e->lg_gamma0 = gamma0;
    e->lg_k = k_sub;
    e->lg_nemax = 0;
    for (int64_t r = 0; r < n; ++r) e->lg_nemax = std::max<int64_t>(e->lg_nemax, At_colptr[r + 1] - At_colptr[r]);
    // packed tables of the LDS-resident kernel (pdmp_logistic.hip): observations with at most 6 regressors, d and nnz(A) within 16 / 32 bits
    e->lg_coord.release();
    e->lg_obs.release();
    e->lg_arow.release();
    if (e->lg_nemax <= 6 && p < 65536 && nnzA < ((int64_t)1 << 32) && n < ((int64_t)1 << 32)) {
        std::vector<pdmp::LgCoord> hc((size_t)p);
        for (int64_t j = 0; j < p; ++j) {
            pdmp::LgCoord& c = hc[(size_t)j];
            c.cp0 = e->colptr[(size_t)j];
            c.k = e->colptr[(size_t)j + 1] - c.cp0;
            c.sp0 = e->h_sptr[(size_t)j];
            c.m = e->h_sptr[(size_t)j + 1] - c.sp0;
            c.l = (uint32_t)(A_colptr[j + 1] - A_colptr[j]);
            c.r0 = (uint32_t)A_colptr[j];
            c.lk = (double)c.l / (double)(uint32_t)k_sub;
        }
        std::vector<pdmp::LgObs> ho((size_t)n);
        memset(ho.data(), 0, ho.size() * sizeof(pdmp::LgObs));
        for (int64_t r = 0; r < n; ++r) {
            pdmp::LgObs& o = ho[(size_t)r];
            o.y = y[r];
            o.ny = ny[r];
            o.sn0 = sn0[(size_t)r];
            o.ns0 = ns0[(size_t)r];
            o.ne = (uint16_t)(At_colptr[r + 1] - At_colptr[r]);
            for (int64_t q = At_colptr[r]; q < At_colptr[r + 1]; ++q) {
                o.val[q - At_colptr[r]] = At_nzval[q];
                o.idx[q - At_colptr[r]] = (uint16_t)At_rowval[q];
            }
        }
        std::vector<uint32_t> ar((size_t)nnzA);
        for (int64_t q = 0; q < nnzA; ++q) {
            if (A_rowval[q] < 0 || A_rowval[q] >= n) return fail(PDMP_ERR_INVALID, "A row index out of range");
            ar[(size_t)q] = (uint32_t)A_rowval[q];
        }
        if ((st = e->lg_coord.upload(hc)) != PDMP_OK) return st;
        if ((st = e->lg_obs.upload(ho)) != PDMP_OK) return st;
        if ((st = e->lg_arow.upload(ar)) != PDMP_OK) return st;
    }
    e->target_kind = 1;
    e->has_target = true;
    e->has_state = false;
    return PDMP_OK;
}

extern "C" {

// the n x n 5-point lattice in column-major numbering (scripts/gridlaplace.jl): G1[i] = {i-n, i-1, i, i+1, i+n} inside the grid
static void detect_lattice(pdmp_ensemble* e) {
    const int64_t d = e->cfg.d;
    e->lattice_n = 0;
    int64_t nl = (int64_t)std::llround(std::sqrt((double)d));
    bool lat = nl * nl == d && nl >= 16 && nl <= 256 && !e->colptr.empty();  // (256: pdmp_trackp.hip's 8192 block bounds; other users check their own limit)
    for (int64_t col = 0; lat && col < nl; ++col)
        for (int64_t row = 0; lat && row < nl; ++row) {
            const int64_t ii = row + nl * col;
            uint32_t want[5];
            int nw = 0;
            if (col > 0) want[nw++] = (uint32_t)(ii - nl);
            if (row > 0) want[nw++] = (uint32_t)(ii - 1);
            want[nw++] = (uint32_t)ii;
            if (row < nl - 1) want[nw++] = (uint32_t)(ii + 1);
            if (col < nl - 1) want[nw++] = (uint32_t)(ii + nl);
            if ((int64_t)(e->colptr[ii + 1] - e->colptr[ii]) != nw) {
                lat = false;
                break;
            }
            for (int q = 0; q < nw; ++q)
                if (e->rowval[e->colptr[ii] + q] != want[q]) lat = false;
        }
    if (lat) e->lattice_n = (int32_t)nl;
}

static pdmp_status alloc_state(pdmp_ensemble* e) {
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    pdmp_status st;
    const size_t nrec = (size_t)(n * d) * (e->track ? 2 : 1);  // TrRec is two ZzRec long
    if (e->d_rec.n != nrec && (st = e->d_rec.alloc(nrec, &e->place_cfg, &e->place_cfg.rec)) != PDMP_OK) return st;
    if (e->d_keys.n != (size_t)(n * e->dk) && (st = e->d_keys.alloc((size_t)(n * e->dk))) != PDMP_OK) return st;
    if (e->d_hdr.n != (size_t)n && (st = e->d_hdr.alloc((size_t)n)) != PDMP_OK) return st;
    if (e->cfg.adapt && e->d_c_chain.n != (size_t)(n * d) && (st = e->d_c_chain.alloc((size_t)(n * d))) != PDMP_OK)
        return st;
    if (e->cfg.trace_capacity > 0 && e->d_ev.n != (size_t)(n * e->cfg.trace_capacity) &&
        (st = e->d_ev.alloc((size_t)(n * e->cfg.trace_capacity), &e->place_cfg, &e->place_cfg.ev)) != PDMP_OK)
        return st;
    e->d_jprev.release();
    return PDMP_OK;
}

// Γ[i,j] is read where the reference reads Γ[j,i] (the stored column of the reflecting coordinate): is the bounding matrix symmetric, in pattern and
// values?  With two_sums also the target's, and *two_sums tells whether the two matrices differ anywhere.
static bool symmetric_matrices(const pdmp_ensemble* e, bool* two_sums) {
    bool two = false;
    for (int64_t col = 0; col < e->cfg.d; ++col)
        for (uint32_t pp = e->colptr[col]; pp < e->colptr[col + 1]; ++pp) {
            const uint32_t row = e->rowval[pp];
            const uint32_t* lo = e->rowval.data() + e->colptr[row];
            const uint32_t* hi = e->rowval.data() + e->colptr[row + 1];
            const uint32_t* it = std::lower_bound(lo, hi, (uint32_t)col);
            if (it == hi || *it != (uint32_t)col) return false;
            const size_t q = (size_t)(it - e->rowval.data());
            if (e->bval[q] != e->bval[pp] || (two_sums && e->h_tval[q] != e->h_tval[pp])) return false;
            if (two_sums && e->bval[pp] != e->h_tval[pp]) two = true;
        }
    if (two_sums) *two_sums = two;
    return true;
}

// what zz_trackp_supported / zz_trackl_supported ask about an ensemble whose state is being set (track_mean decided)
static pdmp::ZzRunParams track_query_params(const pdmp_ensemble* e) {
    pdmp::ZzRunParams G{};
    G.tb = e->tables();
    if (e->track_mean == 2) G.tb.gmu_t = nullptr;  // (the target's mean is served: the support tests need not refuse it)
    G.lattice_n = e->lattice_n;
    G.adapt = e->cfg.adapt;
    G.c_chain = e->cfg.adapt ? e->d_c_chain.p : nullptr;
    G.track_two_sums = e->track_two_sums ? 1 : 0;
    G.has_refresh = e->lambda_ref > 0;
    G.d = e->cfg.d;
    return G;
}

static pdmp_status init_state(pdmp_ensemble* e, double t0, const double* x0, const double* th0, const double* c,
                              const uint64_t* seeds, uint64_t seed0) {
    if (!e->has_flow || !e->has_target) return fail(PDMP_ERR_INVALID, "flow and target must be set before the state");
    const bool sticky = e->cfg.sampler == PDMP_SAMPLER_STICKY_ZIGZAG;
    if (sticky && !e->has_kappa) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_set_sticky must be called before the state");
    if (!c) return fail(PDMP_ERR_INVALID, "c is required");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    e->track = false;
    e->track_lg = false;
    if (e->track_requested && e->target_kind == 1) {
        // tracked BOUNDS under the subsampled logistic target (pdmp_logistic.hip, TRK): the plain spdmp configuration of config C4 only
        if (e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL || e->flow_kind != 0 || e->adaptscale || e->local_bound || e->lambda_ref > 0 ||
            e->dbg_kernel != PDMP_DEBUG_KERNEL_AUTO || e->dbg_dump > 0 || e->has_g1mask)
            return fail(PDMP_ERR_UNSUPPORTED, "gradient tracking with the logistic target: spdmp, ZigZag flow without refresh, G = Matched()");
        if (!symmetric_matrices(e, nullptr)) return fail(PDMP_ERR_UNSUPPORTED, "gradient tracking needs a symmetric bounding matrix");
        e->track_lg = true;
    } else
    if (e->track_requested) {
        // opt-in, so never a silent fall-back: everything the tracked-gradient kernel needs is checked here
        if (e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL || e->needs_general || e->target_kind != 0 || e->flow_kind != 0 || e->adaptscale ||
            e->local_bound || e->lambda_ref > 0 || e->dbg_kernel != PDMP_DEBUG_KERNEL_AUTO || e->dbg_dump > 0)
            return fail(PDMP_ERR_UNSUPPORTED, "gradient tracking: spdmp with a ZigZag flow without refresh and the Gaussian target only");
        bool two = false;
        if (!symmetric_matrices(e, &two)) return fail(PDMP_ERR_UNSUPPORTED, "gradient tracking needs symmetric precision matrices (flow and target)");
        e->track_two_sums = two;
        e->track = true;
        detect_lattice(e);
    }
    // the bit-identical one-proposal-per-lane kernel (pdmp_exactp.hip; opt-in with PDMP_DEBUG_KERNEL_EXACTP: measured at 2x the 8-event
    // kernel's time) wants the plain lattice with the bounding Γ equal to the target's
    e->exactp = false;
    if (!e->track_requested && e->cfg.sampler == PDMP_SAMPLER_ZIGZAG_LOCAL && !e->needs_general && e->target_kind == 0 && e->flow_kind == 0 &&
        !e->adaptscale && !e->local_bound && !(e->lambda_ref > 0) && !e->cfg.adapt && !e->has_tmu && e->dbg_kernel == PDMP_DEBUG_KERNEL_EXACTP &&
        e->dbg_dump == 0 && e->h_tval.size() == e->bval.size()) {
        bool same = true, mu0 = true;
        for (size_t q = 0; q < e->bval.size() && same; ++q) same = e->bval[q] == e->h_tval[q];
        for (size_t q = 0; q < e->h_gmu_b.size() && mu0; ++q) mu0 = e->h_gmu_b[q] == 0.0;
        if (same && mu0) {
            detect_lattice(e);
            e->exactp = e->lattice_n != 0;
        }
    }
    pdmp_status st = alloc_state(e);
    if (st != PDMP_OK) return st;
    std::vector<double> cv(c, c + d);
    if ((st = e->d_c.upload(cv)) != PDMP_OK) return st;
    {
        std::vector<double> c2v((size_t)d * 2);
        for (int64_t k = 0; k < d; ++k) {
            c2v[2 * (size_t)k] = c[k];
            c2v[2 * (size_t)k + 1] = c[k] / 100;
        }
        if ((st = e->d_c2.upload(c2v)) != PDMP_OK) return st;
        std::vector<pdmp::CoordConst> ccv((size_t)d);
        for (int64_t k = 0; k < d; ++k) {
            ccv[(size_t)k].c = c[k];
            ccv[(size_t)k].c100 = c[k] / 100;
            ccv[(size_t)k].cp = e->colptr.empty() ? 0u : (uint32_t)e->colptr[(size_t)k];
            ccv[(size_t)k].k = e->colptr.empty() ? 0u : (uint32_t)(e->colptr[(size_t)k + 1] - e->colptr[(size_t)k]);
            for (int q = 0; q < 5; ++q)
                ccv[(size_t)k].gam[q] = ((uint32_t)q < ccv[(size_t)k].k && ccv[(size_t)k].k <= 5u && !e->h_tval.empty()) ? e->h_tval[ccv[(size_t)k].cp + (size_t)q] : 0.0;
        }
        if ((st = e->d_cc.upload(ccv)) != PDMP_OK) return st;
    }
    if (general_path(e)) {
        if (e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL && e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_ALL &&
            e->cfg.sampler != PDMP_SAMPLER_STICKY_ZIGZAG)
            return fail(PDMP_ERR_UNSUPPORTED,
                        "neighbourhoods beyond 64 members / the logistic target / FactBoomerang / adaptscale run on the general "
                        "kernel: spdmp, pdmp and sspdmp only");
        if (sticky && (e->flow_kind == 1 || e->adaptscale || e->local_bound))
            return fail(PDMP_ERR_UNSUPPORTED, "sspdmp on the general kernel: ZigZag flow, Gaussian or logistic target");
        if (e->cfg.sampler == PDMP_SAMPLER_ZIGZAG_ALL && e->target_kind == 1)
            return fail(PDMP_ERR_UNSUPPORTED, "the logistic target moves what it reads (SelfMoving): use PDMP_SAMPLER_ZIGZAG_LOCAL");
        if (e->target_kind == 1 && (e->flow_kind == 1 || e->lambda_ref > 0))
            return fail(PDMP_ERR_UNSUPPORTED, "the logistic target is implemented for ZigZag without refresh");
        if (pdmp::zz_general_lds_bytes(e->nblk_pad, (e->mmax_all + 63u) & ~63u, e->flow_kind == 1) > 160 * 1024)
            return fail(PDMP_ERR_UNSUPPORTED, "LDS budget exceeded by the general kernel");
        if (e->local_bound) {
            if (e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL || e->flow_kind != 0 || e->lambda_ref > 0 || e->target_kind != 0)
                return fail(PDMP_ERR_UNSUPPORTED,
                            "LocalBound (src/local.jl) is implemented for spdmp with a ZigZag flow without refresh and the Gaussian target");
            // the target's Γ values in the (member j of G1[i], entry of column j) layout of the re-bound tables
            std::vector<double> qtval;
            qtval.reserve(e->h_qptr.empty() ? 0 : e->h_qptr.back());
            for (int64_t pp = 0; pp < e->nnz; ++pp) {
                const uint32_t j = e->rowval[pp];
                for (uint32_t q = e->colptr[j]; q < e->colptr[j + 1]; ++q) qtval.push_back(e->h_tval[q]);
            }
            if (qtval.empty()) qtval.push_back(0.0);
            if ((st = e->d_qtval.upload(qtval)) != PDMP_OK) return st;
        }
        if (e->adaptscale) {
            if (e->target_kind == 1) return fail(PDMP_ERR_UNSUPPORTED, "adaptscale needs the refresh clock; the logistic target has none");
            std::vector<double> sg((size_t)(n * d));
            for (int64_t k = 0; k < n; ++k) std::copy(e->sigma.begin(), e->sigma.end(), sg.begin() + (size_t)(k * d));
            if ((st = e->d_sig_chain.upload(sg)) != PDMP_OK) return st;
        }
        e->use_spec = false;
    } else if ((st = build_blob(e, c)) != PDMP_OK) {
        return st;
    }
    DevBuf<double> sx, sth;
    DevBuf<uint64_t> sseed;
    if (x0) {
        if ((st = sx.alloc((size_t)(n * d))) != PDMP_OK) return st;
        if ((st = sth.alloc((size_t)(n * d))) != PDMP_OK) return st;
        HIP_TRY(hipMemcpy(sx.p, x0, (size_t)(n * d) * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(sth.p, th0, (size_t)(n * d) * sizeof(double), hipMemcpyHostToDevice));
    }
    if (seeds) {
        if ((st = sseed.alloc((size_t)n)) != PDMP_OK) return st;
        HIP_TRY(hipMemcpy(sseed.p, seeds, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    pdmp::ZzInitParams P{};
    P.tb = e->tables();
    P.rec = e->d_rec.p;
    P.keys = e->d_keys.p;
    P.hdr = e->d_hdr.p;
    P.c_chain = e->cfg.adapt ? e->d_c_chain.p : nullptr;
    P.x0 = x0 ? sx.p : nullptr;
    P.th0 = x0 ? sth.p : nullptr;
    P.seeds = seeds ? sseed.p : nullptr;
    P.seed0 = seed0;
    P.d = d;
    P.dk = e->dk;
    P.nchains = n;
    P.t0 = t0;
    P.lambda_ref = e->lambda_ref;
    P.has_refresh = e->lambda_ref > 0;
    P.flow_kind = e->flow_kind;
    P.mu = e->d_mu.p;
    P.diag = e->d_diag.p;
    P.sticky = sticky ? 1 : 0;
    P.local_bound = e->local_bound ? 1 : 0;
    e->track_generic = false;
    bool trackp_ok = false;
    if (e->track) {
        // which tracked kernel will run is decided HERE (the pair layout belongs to one of them): pdmp_debug_set_track_groups before set_state.
        // One proposal per lane (pdmp_trackp.hip) on the plain lattice, or on any other symmetric graph with |G1| <= 8 (ids and values tabulated).
        uint32_t kmax_g1 = 0;
        for (int64_t k = 0; k < d; ++k) kmax_g1 = std::max(kmax_g1, e->colptr[(size_t)k + 1] - e->colptr[(size_t)k]);
        if (e->lattice_n == 0 && kmax_g1 <= (uint32_t)pdmp::TRACKP_KMAX && d <= 16384 && e->dbg_track_groups == 0) {
            std::vector<uint16_t> nb((size_t)d * 8, (uint16_t)0xFFFF);
            std::vector<double> g8((size_t)d * 8, 0.0);
            for (int64_t k = 0; k < d; ++k)
                for (uint32_t q = e->colptr[(size_t)k]; q < e->colptr[(size_t)k + 1]; ++q) {
                    nb[(size_t)k * 8 + (q - e->colptr[(size_t)k])] = (uint16_t)e->rowval[q];
                    g8[(size_t)k * 8 + (q - e->colptr[(size_t)k])] = e->h_tval[q];
                }
            if ((st = e->d_nb16.upload(nb)) != PDMP_OK) return st;
            if ((st = e->d_gam8.upload(g8)) != PDMP_OK) return st;
            e->track_generic = true;
        }
        // the means (round 6): the one-proposal-per-lane kernel keeps ONE constant Γ[:,i]·μ per coordinate -- the flow's, which enters every bound
        // (src/fact_samplers.jl:51); a target mean is served where its Γμ is the same numbers (the usual Z = ZigZag(Γ, μ) on ∇ϕ = Γ(x − μ))
        {
            bool flow_mean = false;
            for (double v : e->h_gmu_b) flow_mean = flow_mean || v != 0.0;
            e->track_mean = flow_mean ? 1 : 0;
            if (e->has_tmu) {
                const bool same = e->h_gmu_t.size() == e->h_gmu_b.size() && std::equal(e->h_gmu_t.begin(), e->h_gmu_t.end(), e->h_gmu_b.begin());
                if (same && !e->track_two_sums) e->track_mean = 2;
            }
        }
        pdmp::ZzRunParams G = track_query_params(e);
        trackp_ok = pdmp::zz_trackp_supported(G) && e->dbg_track_groups == 0;
        if (!trackp_ok) e->track_generic = false;
        G.blob_sw = e->blob_sw;
        G.blob_pw = e->blob_pw;
        G.blob_kmax = e->blob_kmax;
        G.blob_w_pad = e->blob_w_pad;
        G.has_refresh = 0;
        if (!trackp_ok && (!e->use_spec || !pdmp::zz_spec8_geometry(G))) {
            e->track = false;
            return fail(PDMP_ERR_UNSUPPORTED,
                        "gradient tracking: without adaptation, target mean or a bounding matrix of its own (one proposal per lane) the n x n lattice "
                        "with 2048 <= d <= 65536 or a symmetric graph with |G1| <= 8 and 2048 <= d <= 16384; else the 8-event kernel's geometry "
                        "(|G1| <= 5, |S| <= 13, 2048 <= d <= 16384)");
        }
    }
    P.track = e->track ? 1 : 0;
    e->t0_state = t0;
    e->run_T = t0;
    if (sticky || e->local_bound) {
        if (e->d_thf.n != (size_t)(n * d) && (st = e->d_thf.alloc((size_t)(n * d))) != PDMP_OK) return st;
        P.thf = e->d_thf.p;
    }
    int rc = pdmp::launch_zz_init(P, e->stream);
    if (rc != 0) return fail(PDMP_ERR_HIP, "zz_init launch failed: %s", hipGetErrorString((hipError_t)rc));
    if (e->track_lg) {
        if (e->d_trk.n != (size_t)(n * d * 4) && (st = e->d_trk.alloc((size_t)(n * d * 4))) != PDMP_OK) return st;
        int rct = pdmp::launch_zz_logistic_track_init(e->d_rec.p, e->tables(), d, n, t0, e->d_trk.p, e->stream);
        if (rct != 0) return fail(PDMP_ERR_HIP, "zz_logistic_track_init launch failed: %s", hipGetErrorString((hipError_t)rct));
    }
    e->track_pairs = false;
    e->track_lines = false;
    e->canon_stale = false;
    discard_async_consumer(e);  // (a consumer deferred behind "the next run" belongs to the state that is being replaced)
    if (e->track) {
        if (trackp_ok) {
            if (e->d_kp.n != (size_t)(2 * n * e->dk) && (st = e->d_kp.alloc((size_t)(2 * n * e->dk), &e->place_cfg, &e->place_cfg.kp)) != PDMP_OK) return st;
            rc = pdmp::launch_zz_keys_to_pairs(e->d_keys.p, e->d_kp.p, n * e->dk, t0, e->stream);
            if (rc != 0) return fail(PDMP_ERR_HIP, "keys_to_pairs launch failed: %s", hipGetErrorString((hipError_t)rc));
            rc = pdmp::launch_zz_trackp_consts(e->d_rec.p, e->d_cc.p, e->track_generic ? e->d_nb16.p : nullptr, e->track_mean ? e->d_gmu_b.p : nullptr, d, n, e->stream);
            if (rc != 0) return fail(PDMP_ERR_HIP, "trackp_consts launch failed: %s", hipGetErrorString((hipError_t)rc));
            e->track_pairs = true;
            // the line layout where the ensemble fills the device (decided here: the layout belongs to the kernel)
            // (measured, round 6: 2.7 instead of 3.2 lines read per proposal, but 72 instead of 54 vector instructions -- 47.9 ms against 45.4 / 38.8 ms
            // for pdmp_trackp.hip's form on boxes in the slow / fast timing mode: the layout is kept as an opt-in form, never chosen by width)
            if (pdmp::zz_trackl_supported(track_query_params(e)) && !e->track_generic && e->track_mean == 0 && e->dbg_track_lines == 1) {
                if (e->d_tl_lines.n != (size_t)(n * e->dk / 2) && (st = e->d_tl_lines.alloc((size_t)(n * e->dk / 2))) != PDMP_OK) return st;
                if (e->d_tl_cold.n != (size_t)(n * e->dk) && (st = e->d_tl_cold.alloc((size_t)(n * e->dk))) != PDMP_OK) return st;
                rc = pdmp::launch_zz_trackl_pack(e->d_rec.p, e->d_kp.p, e->d_tl_lines.p, e->d_tl_cold.p, d, e->dk, n, e->stream);
                if (rc != 0) return fail(PDMP_ERR_HIP, "trackl_pack launch failed: %s", hipGetErrorString((hipError_t)rc));
                e->track_lines = true;
            }
        }
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->has_state = true;
    e->ran = false;
    e->timed = false;
    e->consuming = false;
    e->trace_appended = false;
    return PDMP_OK;
}

// Everything the ZigZag event-loop kernels read of a run to T, but the dump / profile buffer (dbg, dbg_cap: ensemble_run_impl allocates them)
static pdmp::ZzRunParams run_params(const pdmp_ensemble* e, double T, int flags) {
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
static pdmp::ZzGeneralParams general_params(const pdmp_ensemble* e) {
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
static pdmp::ZzLogisticTables logistic_tables(const pdmp_ensemble* e) {
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
static pdmp_status select_family(const pdmp_ensemble* e, const pdmp::ZzRunParams& P, const pdmp::ZzGeneralParams& Q, const pdmp::ZzLogisticTables& LT,
                                 KernelFamily* fam) {
    *fam = FAM_BPS;
    if (e->cfg.sampler == PDMP_SAMPLER_BPS) return PDMP_OK;
    const bool sticky = e->cfg.sampler == PDMP_SAMPLER_STICKY_ZIGZAG, dump = e->dbg_dump > 0, profile = e->dbg_phase != 0;
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

static pdmp_status ensemble_run_impl(pdmp_ensemble* e, double T, int flags, void* stream);

// WHERE the records and the pairs of a full-width tracked ensemble lie decides whether its slices take 38 or 45 ms (DESIGN.md 5 "The timing modes are a
// property of the allocation": the same binary, the same process, by the hipMalloc that backs either array).  No API shows the property, a few
// milliseconds of the event loop do: after the state is set, a short launch (every chain pauses after PLACE_PROBE_DRAWS draws) is timed, the pairs --
// then the records -- are given new allocations (the old ones stay reserved, so the new ones are other memory), the state is set again and the launch
// repeated (pairs and records in turn, a spacer allocation before each so that it lands elsewhere); the fastest combination is kept, the rest freed, and
// the state set one last time.  Every probe does identical work, so the times compare
// directly; the ensemble the caller gets is bit for bit the one set_state alone would have made.  pdmp_debug_set_placement(ens, 0, ...) turns it off.
#define PLACE_PROBE_DRAWS 12000u
#define PLACE_TUNE_MIN_CHAINS 1024  // (the two modes were seen on launches that fill the device: 4096 chains; narrower ones are probed as well, it costs milliseconds)
static pdmp_status init_state_tuned(pdmp_ensemble* e, double t0, const double* x0, const double* th0, const double* c, const uint64_t* seeds,
                                    uint64_t seed0) {
    e->tune_log.clear();
    pdmp_status st = init_state(e, t0, x0, th0, c, seeds, seed0);
    if (st != PDMP_OK) return st;
    // the two arrays the event loop scatters over: the records, and level 0 of the queue -- (key, time) pairs under tracking, plain keys otherwise.
    // The families of pdmp_kernels.hip / pdmp_trackp.hip / pdmp_exactp.hip only, under spdmp (they pause on the draw count; the general-degree, logistic
    // and sticky ones are not probed).  A family the run would refuse is reported too: the probe's run then raises the refusal and set_state returns it.
    DevBuf<double>& keybuf = e->track_pairs ? e->d_kp : e->d_keys;
    const size_t rec_bytes = e->d_rec.n * sizeof(*e->d_rec.p), kp_bytes = keybuf.n * sizeof(double);
    KernelFamily fam;
    (void)select_family(e, run_params(e, t0, PDMP_RUN_STOP_BEFORE), general_params(e), logistic_tables(e), &fam);
    const bool probed_kernel = e->cfg.sampler == PDMP_SAMPLER_ZIGZAG_LOCAL &&
                               (fam == FAM_SPEC || fam == FAM_TRACKP || fam == FAM_EXACTP || fam == FAM_ONE_EVENT);  // (FAM_ONE_EVENT never pauses)
    if (e->place_tune == 0 || !probed_kernel || e->dbg_dump != 0 || e->cfg.nchains < PLACE_TUNE_MIN_CHAINS || rec_bytes < ((size_t)2 << 30) ||
        e->d_rec.placed.va || keybuf.placed.va || e->dbg_count_limit != 0)
        return PDMP_OK;
    size_t freeb = 0, totb = 0;
    if (hipMemGetInfo(&freeb, &totb) != hipSuccess || freeb < 3 * (rec_bytes + kp_bytes) + ((size_t)8 << 30)) {
        (void)hipGetLastError();
        return PDMP_OK;
    }
    const auto t_begin = std::chrono::steady_clock::now();
    auto probe = [&](float& ms) -> pdmp_status {
        e->dbg_count_limit = PLACE_PROBE_DRAWS;
        pdmp_status r = ensemble_run_impl(e, t0 + 1.0e3, PDMP_RUN_STOP_BEFORE, nullptr);
        e->dbg_count_limit = 0;
        if (r != PDMP_OK) return r;
        HIP_TRY(hipEventSynchronize(e->ev1));
        HIP_TRY(hipEventElapsedTime(&ms, e->ev0, e->ev1));
        return PDMP_OK;
    };
    // candidates: (records, pairs) pointers; index 0 is what set_state allocated
    std::vector<void*> recs{(void*)e->d_rec.p}, kps{(void*)keybuf.p};
    struct Trial { size_t r, k; float ms; };
    std::vector<Trial> trials;
    auto measure = [&](size_t r, size_t k) -> pdmp_status {
        const bool moved = (void*)e->d_rec.p != recs[r] || (void*)keybuf.p != kps[k];
        e->d_rec.p = static_cast<decltype(e->d_rec.p)>(recs[r]);
        keybuf.p = static_cast<double*>(kps[k]);
        pdmp_status r2 = PDMP_OK;
        if (moved || !trials.empty()) r2 = init_state(e, t0, x0, th0, c, seeds, seed0);
        if (r2 != PDMP_OK) return r2;
        float ms = 0;
        if ((r2 = probe(ms)) != PDMP_OK) return r2;
        trials.push_back({r, k, ms});
        return PDMP_OK;
    };
    auto best = [&]() { return *std::min_element(trials.begin(), trials.end(), [](const Trial& a, const Trial& b) { return a.ms < b.ms; }); };
    auto worst = [&]() { return *std::max_element(trials.begin(), trials.end(), [](const Trial& a, const Trial& b) { return a.ms < b.ms; }); };
    // both levels seen and the fast one in hand: done (the modes are 17 % apart; probes repeat to 1-2 %)
    auto settled = [&]() { return trials.size() >= 2 && worst().ms > 1.08f * best().ms; };
    st = measure(0, 0);
    // new pairs and new records in turn, at most four of each.  What matters is which REGIONS of the memory the two arrays lie in, and consecutive
    // hipMallocs are neighbours: a spacer allocation (held to the end) goes before every candidate so that it lands somewhere else
    std::vector<void*> spacers;
    const size_t spacer_bytes = (size_t)6 << 30;
    for (int step = 0; st == PDMP_OK && step < 8 && !settled(); ++step) {
        const bool pairs_turn = (step & 1) == 0;
        const size_t want = pairs_turn ? kp_bytes : rec_bytes;
        if (hipMemGetInfo(&freeb, &totb) != hipSuccess || freeb < want + spacer_bytes + rec_bytes + kp_bytes + ((size_t)8 << 30)) {
            (void)hipGetLastError();
            break;
        }
        void *sp = nullptr, *np = nullptr;
        if (hipMalloc(&sp, spacer_bytes) == hipSuccess) spacers.push_back(sp);
        else (void)hipGetLastError();
        if (hipMalloc(&np, want) != hipSuccess) {
            (void)hipGetLastError();
            break;
        }
        if (pairs_turn) {
            kps.push_back(np);
            st = measure(best().r, kps.size() - 1);
        } else {
            recs.push_back(np);
            st = measure(recs.size() - 1, best().k);
        }
    }
    // keep the best pair, free the rest, and leave the state as set_state makes it
    const Trial b = trials.empty() ? Trial{0, 0, 0.f} : best();
    e->d_rec.p = static_cast<decltype(e->d_rec.p)>(recs[b.r]);
    keybuf.p = static_cast<double*>(kps[b.k]);
    HIP_TRY(hipDeviceSynchronize());
    for (size_t k = 0; k < recs.size(); ++k)
        if (k != b.r) (void)hipFree(recs[k]);
    for (size_t k = 0; k < kps.size(); ++k)
        if (k != b.k) (void)hipFree(kps[k]);
    for (void* sp : spacers) (void)hipFree(sp);
    pdmp_status st2 = init_state(e, t0, x0, th0, c, seeds, seed0);
    e->last_kernel = "";  // (pdmp_debug_last_kernel: '' before the caller's first run)
    char t[96];
    snprintf(t, sizeof t, "placement probes (ms, %u draws per chain):", PLACE_PROBE_DRAWS);
    e->tune_log = t;
    for (const Trial& q : trials) {
        snprintf(t, sizeof t, " %.2f[r%zu p%zu]", q.ms, q.r, q.k);
        e->tune_log += t;
    }
    snprintf(t, sizeof t, "; kept r%zu p%zu; %.2f s", b.r, b.k, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count());
    e->tune_log += t;
    return st != PDMP_OK ? st : st2;
}

pdmp_status pdmp_ensemble_set_state(pdmp_ensemble* e, double t0, const double* x0, const double* theta0,
                                    const double* c, const uint64_t* seeds) {
    if (!e || !x0 || !theta0 || !seeds) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    return init_state_tuned(e, t0, x0, theta0, c, seeds, 0);
}

pdmp_status pdmp_ensemble_set_state_synthetic(pdmp_ensemble* e, double t0, const double* c, uint64_t seed0) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    return init_state_tuned(e, t0, nullptr, nullptr, c, nullptr, seed0);
}

static pdmp::BpsRunParams bps_run_params(const pdmp_ensemble* e, double T, int flags);
static pdmp::BpsMomParams bps_moments_params(const pdmp_ensemble* e);
static pdmp::BpsStickyParams bps_sticky_params(const pdmp_ensemble* e);
static pdmp::BpsModernParams bps_modern_params(const pdmp_ensemble* e);

pdmp_status pdmp_ensemble_run(pdmp_ensemble* e, double T, int flags, void* stream) {
    pdmp_status st = ensemble_run_impl(e, T, flags, stream);
    if (st == PDMP_OK && e->cfg.sampler != PDMP_SAMPLER_BPS) e->run_T = T;  // (only a launch that went out moves the horizon: fact_integrals_at)
    if (st == PDMP_OK && e->deferred_k >= 0) st = launch_deferred_consumer(e);  // (behind the event loop's launch: see pdmp_ensemble_consume_async)
    return st;
}

// validate, fill, select, launch, finish
static pdmp_status ensemble_run_impl(pdmp_ensemble* e, double T, int flags, void* stream) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "set_state must be called before run");
    if (e->trace_appended) return fail(PDMP_ERR_INVALID, "pdmp_debug_trace_append was used on this ensemble: its records no longer match its trace (set_state first)");
    if (flags != PDMP_RUN_REFERENCE_TAIL && flags != PDMP_RUN_STOP_BEFORE) return fail(PDMP_ERR_INVALID, "bad flags");
    HIP_TRY(hipSetDevice(e->cfg.device));
    e->ran = true;
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    const int64_t n = e->cfg.nchains;
    const bool bps = e->cfg.sampler == PDMP_SAMPLER_BPS;
    pdmp_status st;
    if (!bps) e->dbg_phase_valid = 0;
    if (!bps && general_path(e) && e->lg_nemax >= 1024 && !e->d_hot.p && (st = e->d_hot.alloc((size_t)n * (size_t)e->cfg.d * 4)) != PDMP_OK) return st;
    // (plain fills of pointers and numbers: the other sampler's block goes unread)
    const pdmp::BpsRunParams B = bps_run_params(e, T, flags);
    pdmp::ZzRunParams P = run_params(e, T, flags);
    const pdmp::ZzGeneralParams Q = general_params(e);
    const pdmp::ZzLogisticTables LT = logistic_tables(e);
    KernelFamily fam;
    if ((st = select_family(e, P, Q, LT, &fam)) != PDMP_OK) return st;
    const FamilyInfo& F = FAMILY[fam];
    // on the stream: the dump buffer's memset, ev0, the profile buffer's memset, the kernel, ev1
    DevBuf<double> dbgbuf, phbuf;
    const int64_t dbg_cap = bps ? 0 : e->dbg_dump;
    if (dbg_cap > 0) {
        if ((st = dbgbuf.alloc((size_t)dbg_cap * 16)) != PDMP_OK) return st;
        HIP_TRY(hipMemsetAsync(dbgbuf.p, 0, (size_t)dbg_cap * 16 * sizeof(double), s));
        P.dbg = dbgbuf.p;
        P.dbg_cap = dbg_cap;
    }
    HIP_TRY(hipEventRecord(e->ev0, s));
    const bool profiled = e->dbg_phase != 0 && F.phase_kind != 0;
    if (profiled) {
        if ((st = phbuf.alloc(16)) != PDMP_OK) return st;
        HIP_TRY(hipMemsetAsync(phbuf.p, 0, 16 * sizeof(double), s));
        P.dbg = phbuf.p;
        P.dbg_cap = 0;
    }
    int rc = 0;
    switch (fam) {
    case FAM_BPS:
        if (e->bps_modern) {
            e->last_kernel = "bps_modern_run_kernel";
            rc = pdmp::launch_bps_modern_run(B, bps_modern_params(e), n, s);
        } else if (e->bps_sticky) {
            e->last_kernel = "bps_sticky_run_kernel";
            rc = pdmp::launch_bps_sticky_run(B, bps_sticky_params(e), n, s);
        } else {
            e->last_kernel = "bps_run_kernel";
            rc = pdmp::launch_bps_run(B, n, e->bps_diag, s, bps_moments_params(e));
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
#ifdef PDMP_EXTRA_KERNELS
    case FAM_LOGISTIC_ROWS: e->last_kernel = "zz_logistic_rows_kernel"; rc = pdmp::launch_zz_logistic_rows(P, Q, LT, e->keep_integrals, logistic_rows_width(e), n, s); break;
    case FAM_EXACTP: e->last_kernel = "zz_local_exactp_kernel"; rc = pdmp::launch_zz_local_exactp(P, n, s); break;
#else
    case FAM_LOGISTIC_ROWS: case FAM_EXACTP: return fail(PDMP_ERR_UNSUPPORTED, "kernel family %d is not part of this library", (int)fam);  // (select_family never returns them here)
#endif
    }
    if (rc != 0 && F.hip_rc) return fail(PDMP_ERR_HIP, "%s launch failed: %s", F.launcher, hipGetErrorString((hipError_t)rc));
    if (rc != 0) return fail(PDMP_ERR_HIP, "%s launch failed (%d)", F.launcher, rc);
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
    HIP_TRY(hipEventSynchronize(e->ev1));
    HIP_TRY(hipEventElapsedTime(ms, e->ev0, e->ev1));
    return PDMP_OK;
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
    pdmp_status st = pdmp_ensemble_counters(e, c.data());
    if (st != PDMP_OK) return st;
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
    if (chain < 0 || chain >= e->cfg.nchains || first < 0 || count < 0 || first + count > e->cfg.trace_capacity)
        return fail(PDMP_ERR_INVALID, "trace range out of bounds");
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
    if (chain_first < 0 || n < 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "chain range");
    if (n == 0) return PDMP_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    { pdmp_status stc = ensure_canon(e); if (stc != PDMP_OK) return stc; }
    const int64_t d = e->cfg.d;
    const size_t cnt = (size_t)(n * d);
    DevBuf<double> bt, bx, bth, bc;
    DevBuf<int64_t> bacc;
    pdmp_status st;
    if (t && (st = bt.alloc(cnt)) != PDMP_OK) return st;
    if (x && (st = bx.alloc(cnt)) != PDMP_OK) return st;
    if (theta && (st = bth.alloc(cnt)) != PDMP_OK) return st;
    if (acc && (st = bacc.alloc(cnt)) != PDMP_OK) return st;
    if (c && (st = bc.alloc(cnt)) != PDMP_OK) return st;
    const double* c_src = e->cfg.adapt ? e->d_c_chain.p : e->d_c.p;
    const int64_t c_stride = e->cfg.adapt ? d : 0;
    if (e->track_pairs && e->cfg.adapt) {  // (the one-proposal-per-lane kernel keeps the adapted bounds in its record lines)
        int rcc = pdmp::launch_zz_trackp_c_out(e->d_rec.p, e->d_c_chain.p, e->cfg.nchains * d, e->stream);
        if (rcc != 0) return fail(PDMP_ERR_HIP, "trackp_c_out launch failed: %s", hipGetErrorString((hipError_t)rcc));
    }
    int rc = e->track ? pdmp::launch_zz_track_unpack(reinterpret_cast<const pdmp::TrRec*>(e->d_rec.p), e->tables(), c_src, c_stride, d,
                                                     chain_first, n, e->t0_state, bt.p, bx.p, bth.p, bacc.p, bc.p, e->track_pairs ? e->d_kp.p : nullptr, e->dk, e->stream)
                       : pdmp::launch_zz_unpack(e->d_rec.p, c_src, c_stride, d, chain_first, n, bt.p, bx.p, bth.p, bacc.p, bc.p,
                                                e->stream);
    if (rc != 0) return fail(PDMP_ERR_HIP, "unpack launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (t) HIP_TRY(hipMemcpy(t, bt.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
    if (x) HIP_TRY(hipMemcpy(x, bx.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
    if (theta) HIP_TRY(hipMemcpy(theta, bth.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
    if (acc) HIP_TRY(hipMemcpy(acc, bacc.p, cnt * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (c) HIP_TRY(hipMemcpy(c, bc.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

static pdmp_status ess_ready(pdmp_ensemble* e);
static pdmp_status fact_integrals_at(pdmp_ensemble* e, double T);
static pdmp_status bps_moments_at(pdmp_ensemble* e, double T, int64_t chain_first, int64_t n, bool two);

pdmp_status pdmp_ensemble_batch_means(pdmp_ensemble* e, double T_prev, double T, double* sum_y, double* sum_y2) {
    pdmp_status st0 = ess_ready(e);
    if (st0 != PDMP_OK) return st0;
    if (!(T > T_prev)) return fail(PDMP_ERR_INVALID, "T must exceed T_prev");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    const bool bps = e->cfg.sampler == PDMP_SAMPLER_BPS;
    pdmp_status st;
    if (bps && (st = bps_moments_at(e, T, 0, n, false)) != PDMP_OK) return st;  // J1(T) of every chain into b_jT (the validity rule first)
    if (!bps && (st = fact_integrals_at(e, T)) != PDMP_OK) return st;  // (before jprev is allocated or touched)
    if (e->d_jprev.n != (size_t)(n * d)) {
        if ((st = e->d_jprev.alloc((size_t)(n * d))) != PDMP_OK) return st;
        HIP_TRY(hipMemsetAsync(e->d_jprev.p, 0, (size_t)(n * d) * sizeof(double), e->stream));  // (same stream as the kernel: the ensemble's stream is non-blocking, the null stream does not order against it)
    }
    if (e->d_sum.n != (size_t)(2 * d) && (st = e->d_sum.alloc((size_t)(2 * d))) != PDMP_OK) return st;
    if (!bps && (st = ensure_canon(e)) != PDMP_OK) return st;
    HIP_TRY(hipMemsetAsync(e->d_sum.p, 0, (size_t)(2 * d) * sizeof(double), e->stream));
    int rc = bps ? pdmp::launch_dense_batch_means(e->b_jT.p, e->d_jprev.p, d, n, T_prev, T, e->d_sum.p, e->d_sum.p + d, e->stream)
                 : pdmp::launch_zz_batch_means(e->d_rec.p, e->track ? 128 : 64, e->d_jprev.p, d, n, T_prev, T, e->d_sum.p, e->d_sum.p + d,
                                               e->stream);
    if (rc != 0) return fail(PDMP_ERR_HIP, "batch_means launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (sum_y) HIP_TRY(hipMemcpy(sum_y, e->d_sum.p, (size_t)d * sizeof(double), hipMemcpyDeviceToHost));
    if (sum_y2) HIP_TRY(hipMemcpy(sum_y2, e->d_sum.p + d, (size_t)d * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

static pdmp_status ess_ready(pdmp_ensemble* e) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler == PDMP_SAMPLER_BPS && e->bps_mom < 1)
        return fail(PDMP_ERR_INVALID, "path integrals are kept by the factorised samplers only");  // (and by a BPS ensemble with moments on)
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "no state");
    if (e->cfg.sampler == PDMP_SAMPLER_BPS) return PDMP_OK;
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

pdmp_status pdmp_ensemble_ess_begin(pdmp_ensemble* e, double T0) {
    pdmp_status st = ess_ready(e);
    if (st != PDMP_OK) return st;
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    const bool bps = e->cfg.sampler == PDMP_SAMPLER_BPS;
    if (bps && (st = bps_moments_at(e, T0, 0, n, false)) != PDMP_OK) return st;
    if (!bps && (st = fact_integrals_at(e, T0)) != PDMP_OK) return st;
    if (e->d_jprev.n != (size_t)(n * d) && (st = e->d_jprev.alloc((size_t)(n * d))) != PDMP_OK) return st;
    if (e->d_jstart.n != (size_t)(n * d) && (st = e->d_jstart.alloc((size_t)(n * d))) != PDMP_OK) return st;
    if (e->d_essacc.n != (size_t)(4 * d) && (st = e->d_essacc.alloc((size_t)(4 * d))) != PDMP_OK) return st;
    if (!bps && (st = ensure_canon(e)) != PDMP_OK) return st;
    HIP_TRY(hipMemsetAsync(e->d_essacc.p, 0, (size_t)(4 * d) * sizeof(double), e->stream));
    int rc = bps ? pdmp::launch_dense_ess(e->b_jT.p, e->d_jprev.p, e->d_jstart.p, d, n, 0, T0, T0, e->d_essacc.p, e->stream)
                 : pdmp::launch_zz_ess(e->d_rec.p, e->track ? 128 : 64, e->d_jprev.p, e->d_jstart.p, d, n, 0, T0, T0, e->d_essacc.p, e->stream);
    if (rc != 0) return fail(PDMP_ERR_HIP, "ess launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->ess_T0 = e->ess_Tlast = T0;
    e->ess_batches = 0;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_ess_batch(pdmp_ensemble* e, double T) {
    pdmp_status st = ess_ready(e);
    if (st != PDMP_OK) return st;
    if (e->ess_batches < 0) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_ess_begin first");
    if (!(T > e->ess_Tlast)) return fail(PDMP_ERR_INVALID, "batch end %g does not exceed the previous one %g", T, e->ess_Tlast);
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    int rc;
    if (e->cfg.sampler == PDMP_SAMPLER_BPS) {
        if ((st = bps_moments_at(e, T, 0, e->cfg.nchains, false)) != PDMP_OK) return st;
        rc = pdmp::launch_dense_ess(e->b_jT.p, e->d_jprev.p, e->d_jstart.p, e->cfg.d, e->cfg.nchains, 1, e->ess_Tlast, T, e->d_essacc.p, e->stream);
    } else {
        if ((st = fact_integrals_at(e, T)) != PDMP_OK) return st;
        if ((st = ensure_canon(e)) != PDMP_OK) return st;
        rc = pdmp::launch_zz_ess(e->d_rec.p, e->track ? 128 : 64, e->d_jprev.p, e->d_jstart.p, e->cfg.d, e->cfg.nchains, 1, e->ess_Tlast, T,
                                 e->d_essacc.p, e->stream);
    }
    if (rc != 0) return fail(PDMP_ERR_HIP, "ess launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->ess_Tlast = T;
    e->ess_batches += 1;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_ess_end(pdmp_ensemble* e, double* sum_y, double* sum_y2, double* sum_m, double* sum_m2,
                                  int64_t* nbatches, double* T0, double* T1) {
    pdmp_status st = ess_ready(e);
    if (st != PDMP_OK) return st;
    if (e->ess_batches < 1) return fail(PDMP_ERR_INVALID, "no batch accumulated (ess_begin, then ess_batch)");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d;
    const bool bps = e->cfg.sampler == PDMP_SAMPLER_BPS;
    if (!bps && (st = ensure_canon(e)) != PDMP_OK) return st;
    HIP_TRY(hipMemsetAsync(e->d_essacc.p + 2 * d, 0, (size_t)(2 * d) * sizeof(double), e->stream));
    // (BPS: J at the last batch end is the jprev that batch left -- the state may since have run past it)
    int rc = bps ? pdmp::launch_dense_ess(e->d_jprev.p, e->d_jprev.p, e->d_jstart.p, d, e->cfg.nchains, 2, e->ess_T0, e->ess_Tlast, e->d_essacc.p,
                                          e->stream)
                 : pdmp::launch_zz_ess(e->d_rec.p, e->track ? 128 : 64, e->d_jprev.p, e->d_jstart.p, d, e->cfg.nchains, 2, e->ess_T0, e->ess_Tlast,
                                       e->d_essacc.p, e->stream);
    if (rc != 0) return fail(PDMP_ERR_HIP, "ess launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipStreamSynchronize(e->stream));
    double* outs[4] = {sum_y, sum_y2, sum_m, sum_m2};
    for (int k = 0; k < 4; ++k)
        if (outs[k]) HIP_TRY(hipMemcpy(outs[k], e->d_essacc.p + k * d, (size_t)d * sizeof(double), hipMemcpyDeviceToHost));
    if (nbatches) *nbatches = e->ess_batches;
    if (T0) *T0 = e->ess_T0;
    if (T1) *T1 = e->ess_Tlast;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_consume_begin(pdmp_ensemble* e, double grid_dt, int64_t grid_points) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->has_state || e->ran) return fail(PDMP_ERR_INVALID, "consume_begin follows set_state and precedes the first run (it snapshots x0, θ0)");
    if (e->cfg.trace_capacity <= 0) return fail(PDMP_ERR_INVALID, "ensemble was created with trace_capacity = 0");
    if (e->flow_kind != 0 || e->lambda_ref > 0)
        return fail(PDMP_ERR_UNSUPPORTED, "the device consumers take time-ordered traces of piecewise-linear paths: ZigZag without refresh clock");
    if (grid_points < 0 || (grid_points > 0 && !(grid_dt > 0))) return fail(PDMP_ERR_INVALID, "grid_dt must be positive");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    pdmp_status st;
    e->cons_z = e->cfg.sampler == PDMP_SAMPLER_STICKY_ZIGZAG;  // (the time away from 0, inclusion_prob: a sum of its own where coordinates can freeze)
    if ((st = e->d_ccur.alloc((size_t)(n * d) * pdmp::consume_cursor_bytes(e->cons_z))) != PDMP_OK) return st;
    if ((st = e->d_cmeta.alloc((size_t)n * pdmp::consume_meta_bytes())) != PDMP_OK) return st;
    e->d_cgrid.release();
    if (grid_points > 0) {
        if ((st = e->d_cgrid.alloc((size_t)(n * grid_points * d))) != PDMP_OK) return st;
        HIP_TRY(hipMemsetAsync(e->d_cgrid.p, 0, (size_t)(n * grid_points * d) * sizeof(double), e->stream));
    }
    if ((st = ensure_canon(e)) != PDMP_OK) return st;
    discard_async_consumer(e);
    e->cons_cummean = false;
    int rc = pdmp::launch_consume_init(e->d_rec.p, e->track ? 128 : 64, d, n, e->t0_state, e->d_ccur.p, e->cons_z, e->d_cmeta.p,
                                       grid_points > 0 ? e->d_cgrid.p : nullptr, grid_points, e->stream);
    if (rc != 0) return fail(PDMP_ERR_HIP, "consume_init launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->consuming = true;
    e->cons_dt = grid_dt;
    e->cons_K = grid_points;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_consume(pdmp_ensemble* e) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->consuming || !e->has_state) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_consume_begin first");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    int rc = pdmp::launch_consume_events(e->d_ev.p, e->cfg.trace_capacity, e->d_hdr.p, nullptr, e->cfg.d, e->cfg.nchains, e->d_ccur.p, e->cons_z, e->d_cmeta.p,
                                         e->d_cgrid.p, e->cons_K, e->t0_state, e->cons_dt, e->stream, e->cons_cummean ? e->d_ccm.p : nullptr);
    if (rc != 0) return fail(PDMP_ERR_HIP, "consume launch failed: %s", hipGetErrorString((hipError_t)rc));
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
        pdmp_status st;
        if (e->d_ccm.n != n && (st = e->d_ccm.alloc(n)) != PDMP_OK) return st;
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
    pdmp_status st;
    if ((st = dloc.upload(loc)) != PDMP_OK) return st;
    if ((st = dout.alloc((size_t)std::max<int64_t>(out_cap, 1))) != PDMP_OK) return st;
    if ((st = dn.alloc(1)) != PDMP_OK) return st;
    int rc = pdmp::launch_trace_subtrace(e->d_ev.p + chain * e->cfg.trace_capacity, n, dloc.p, dout.p, out_cap, dn.p, e->stream);
    if (rc != 0) return fail(PDMP_ERR_HIP, "trace_subtrace launch failed: %s", hipGetErrorString((hipError_t)rc));
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
    HIP_TRY(hipSetDevice(e->cfg.device));
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    const int64_t n = e->cfg.nchains;
    pdmp_status st;
    if ((st = launch_deferred_consumer(e)) != PDMP_OK) return st;  // (two calls without a run between them)
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
    if (e->d_ev2.n != e->d_ev.n && (st = e->d_ev2.alloc(e->d_ev.n)) != PDMP_OK) return st;
    const int k = e->async_k;
    if (e->d_snap[k].n != (size_t)(2 * n) && (st = e->d_snap[k].alloc((size_t)(2 * n))) != PDMP_OK) return st;
    int rc = pdmp::launch_consume_snapshot(e->d_hdr.p, n, e->d_snap[k].p, s);
    if (rc != 0) return fail(PDMP_ERR_HIP, "consume_snapshot launch failed: %s", hipGetErrorString((hipError_t)rc));
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
        if ((st = launch_deferred_consumer(e)) != PDMP_OK) return st;
        HIP_TRY(hipStreamWaitEvent(s, e->ev_cons_done[k], 0));
    }
    e->async_k = k ^ 1;
    return PDMP_OK;
}

// Test hook (include/pdmp_debug.h): n given events behind what `chain`'s current trace segment holds, counted in its header as a run would have
// counted them -- the consumers, trace_copy, trace_reset and subtrace_copy see a segment a sampler could never have produced (events exactly at
// grid times, chains of one coordinate, chosen hash clashes: tests/consumer_cases.py).  No kernel is launched and no record is touched, so the
// ensemble cannot run afterwards.
pdmp_status pdmp_debug_trace_append(pdmp_ensemble* e, int64_t chain, const pdmp_event* ev, int64_t n) {
    if (!e || (n > 0 && !ev)) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->consuming || !e->has_state) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_consume_begin first");
    if (chain < 0 || chain >= e->cfg.nchains || n < 0) return fail(PDMP_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));  // (a deferred asynchronous consumer is launched and waited for: it reads the other buffer and the headers' snapshot)
    pdmp::DevChain h;
    HIP_TRY(hipMemcpy(&h, e->d_hdr.p + chain, sizeof h, hipMemcpyDeviceToHost));
    const int64_t cap = e->cfg.trace_capacity;
    if (h.c.ntrace > (uint64_t)cap || n > cap - (int64_t)h.c.ntrace)
        return fail(PDMP_ERR_INVALID, "trace_append: %lld events behind %llu do not fit trace_capacity = %lld", (long long)n, (unsigned long long)h.c.ntrace, (long long)cap);
    if (n > 0) HIP_TRY(hipMemcpy(e->d_ev.p + chain * cap + (int64_t)h.c.ntrace, ev, (size_t)n * sizeof(pdmp_event), hipMemcpyHostToDevice));
    h.c.ntrace += (uint64_t)n;
    h.c.nevents += (uint64_t)n;
    HIP_TRY(hipMemcpy(&e->d_hdr.p[chain].c, &h.c, sizeof h.c, hipMemcpyHostToDevice));
    e->trace_appended = true;
    return PDMP_OK;
}

// What the host could drain instead: `bytes` of the trace buffer copied to pinned host memory, in GB/s (a measurement for bench.py's pipeline
// object, not a code path of the engine)
pdmp_status pdmp_debug_host_drain_probe(pdmp_ensemble* e, int64_t bytes, double* gbps) {
    if (!e || !gbps || bytes <= 0) return fail(PDMP_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const size_t have = e->d_ev.n * sizeof(pdmp_event);
    const size_t nb = std::min<size_t>((size_t)bytes, have);
    if (nb == 0) return fail(PDMP_ERR_INVALID, "ensemble was created with trace_capacity = 0");
    void* host = nullptr;
    HIP_TRY(hipHostMalloc(&host, nb, hipHostMallocDefault));
    hipError_t err = device_sync(e);
    if (err == hipSuccess) err = hipMemcpy(host, e->d_ev.p, nb, hipMemcpyDeviceToHost);  // (warm-up: page tables, the copy engine's first touch)
    const auto t0 = std::chrono::steady_clock::now();
    if (err == hipSuccess) err = hipMemcpy(host, e->d_ev.p, nb, hipMemcpyDeviceToHost);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    (void)hipHostFree(host);
    if (err != hipSuccess) return fail(PDMP_ERR_HIP, "hipMemcpy: %s", hipGetErrorString(err));
    *gbps = (double)nb / secs / 1e9;
    return PDMP_OK;
}

// kernel time of the last asynchronous consumer (waits for it)
pdmp_status pdmp_ensemble_last_consume_ms(pdmp_ensemble* e, float* ms) {
    if (!e || !ms) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->cons_timed && e->deferred_k < 0) return fail(PDMP_ERR_INVALID, "no asynchronous consumer has run");
    HIP_TRY(hipSetDevice(e->cfg.device));
    pdmp_status st = launch_deferred_consumer(e);
    if (st != PDMP_OK) return st;
    HIP_TRY(hipEventSynchronize(e->ev_c1));
    HIP_TRY(hipEventElapsedTime(ms, e->ev_c0, e->ev_c1));
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_consume_mean(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* mean, double* T_last) {
    if (!e || !mean) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->consuming) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_consume_begin first");
    if (chain_first < 0 || n <= 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "chain range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));  // (asynchronous consumers run on a second stream)
    const int64_t d = e->cfg.d;
    DevBuf<double> bm, bt;
    pdmp_status st;
    if ((st = bm.alloc((size_t)(n * d))) != PDMP_OK) return st;
    if ((st = bt.alloc((size_t)n)) != PDMP_OK) return st;
    int rc = pdmp::launch_consume_mean(d, chain_first, n, e->d_ccur.p, e->d_cmeta.p, bm.p, bt.p, e->stream);
    if (rc != 0) return fail(PDMP_ERR_HIP, "consume_mean launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(mean, bm.p, (size_t)(n * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (T_last) HIP_TRY(hipMemcpy(T_last, bt.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_consume_inclusion(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* prob, double* T_last) {
    if (!e || !prob) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->consuming) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_consume_begin first");
    if (chain_first < 0 || n <= 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "chain range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));  // (asynchronous consumers run on a second stream)
    const int64_t d = e->cfg.d;
    DevBuf<double> bm, bt;
    pdmp_status st;
    if ((st = bm.alloc((size_t)(n * d))) != PDMP_OK) return st;
    if ((st = bt.alloc((size_t)n)) != PDMP_OK) return st;
    int rc = pdmp::launch_consume_inclusion(d, e->cfg.nchains, e->cons_z, e->t0_state, chain_first, n, e->d_ccur.p, e->d_cmeta.p, bm.p, bt.p, e->stream);
    if (rc != 0) return fail(PDMP_ERR_HIP, "consume_inclusion launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(prob, bm.p, (size_t)(n * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (T_last) HIP_TRY(hipMemcpy(T_last, bt.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
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
    // the points after every coordinate's last event, up to the chain's last event time (idempotent)
    int rc = pdmp::launch_consume_flush(d, e->cfg.nchains, e->d_ccur.p, e->d_cmeta.p, e->d_cgrid.p, e->cons_K, e->t0_state, e->cons_dt, e->stream);
    if (rc != 0) return fail(PDMP_ERR_HIP, "consume_flush launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (out && k_count)
        HIP_TRY(hipMemcpy(out, e->d_cgrid.p + (chain * e->cons_K + k_first) * d, (size_t)(k_count * d) * sizeof(double), hipMemcpyDeviceToHost));
    if (npoints) {
        // collect(discretize(Ξ, dt)) emits a grid time while it lies before the last event (src/trace.jl:111-113); at least t0 itself
        std::vector<unsigned char> mh(pdmp::consume_meta_bytes());
        HIP_TRY(hipMemcpy(mh.data(), e->d_cmeta.p + (size_t)chain * pdmp::consume_meta_bytes(), mh.size(), hipMemcpyDeviceToHost));
        double tl;
        memcpy(&tl, mh.data() + 8, sizeof tl);
        // NOT clamped to the grid: a value above grid_points tells the caller that the grid was too short for the run (rows beyond it do not exist)
        int64_t np = (int64_t)floor((tl - e->t0_state) / e->cons_dt);
        np = np > 1 ? np - 1 : 0;
        while (e->t0_state + e->cons_dt * (double)np < tl) ++np;
        *npoints = np > 0 ? np : 1;
    }
    if (grid_dev) *grid_dev = e->d_cgrid.p;
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
    pdmp_status st = ess_ready(e);
    if (st != PDMP_OK) return st;
    if (!probes || !out || nprobe <= 0) return fail(PDMP_ERR_INVALID, "bad argument");
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    for (int64_t k = 0; k < nprobe; ++k)
        if (probes[k] < 0 || probes[k] >= d) return fail(PDMP_ERR_INVALID, "probe coordinate %lld out of range", (long long)probes[k]);
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    DevBuf<int64_t> dp;
    DevBuf<double> dout;
    if ((st = dp.upload(std::vector<int64_t>(probes, probes + nprobe))) != PDMP_OK) return st;
    if ((st = dout.alloc((size_t)(n * nprobe))) != PDMP_OK) return st;
    int rc;
    if (e->cfg.sampler == PDMP_SAMPLER_BPS) {
        if ((st = bps_moments_at(e, T, 0, n, false)) != PDMP_OK) return st;
        rc = pdmp::launch_dense_gather(e->b_jT.p, d, n, dp.p, nprobe, dout.p, e->stream);
    } else {
        if ((st = fact_integrals_at(e, T)) != PDMP_OK) return st;
        if ((st = ensure_canon(e)) != PDMP_OK) return st;
        rc = pdmp::launch_zz_path_integrals(e->d_rec.p, e->track ? 128 : 64, d, n, dp.p, nprobe, T, dout.p, e->stream);
    }
    if (rc != 0) return fail(PDMP_ERR_HIP, "path_integrals launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out, dout.p, (size_t)(n * nprobe) * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_sticky(pdmp_ensemble* e, const double* kappa, int reversible, int strong_upperbounds) {
    if (!e || !kappa) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_STICKY_ZIGZAG) return fail(PDMP_ERR_INVALID, "ensemble is not a sticky ZigZag");
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_zigzag must be called first");
    if (e->lambda_ref > 0) return fail(PDMP_ERR_UNSUPPORTED, "refreshment not implemented (src/ss_fact.jl:86)");
    HIP_TRY(hipSetDevice(e->cfg.device));
    pdmp_status st = e->d_kappa.upload(std::vector<double>(kappa, kappa + e->cfg.d));
    if (st != PDMP_OK) return st;
    e->reversible = reversible;
    e->strong_upperbounds = strong_upperbounds;
    e->has_kappa = true;
    e->has_state = false;
    return PDMP_OK;
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
    pdmp_status st;
    if ((st = d_inner.upload(inner)) != PDMP_OK || (st = d_mask.upload(mask)) != PDMP_OK || (st = d_g2ptr.upload(g2ptr)) != PDMP_OK ||
        (st = d_g2idx.upload(g2idx)) != PDMP_OK)
        return st;
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
    const int rc = pdmp::launch_zz_partitioned(P, e->cfg.nchains, s);
    if (rc != 0) return fail(PDMP_ERR_HIP, "zz_partitioned_run launch failed (%d)", rc);
    e->run_T = T;
    HIP_TRY(hipEventRecord(e->ev1, s));
    e->timed = true;
    HIP_TRY(hipStreamSynchronize(s));  // (the tables of this call live until here)
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_gradient_tracking(pdmp_ensemble* e, int enable) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    e->track_requested = enable != 0;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_local_bound(pdmp_ensemble* e, int enable) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_* must be called first");
    e->local_bound = enable != 0;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_adaptscale(pdmp_ensemble* e, int enable) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_* must be called first");
    if (enable && e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL)
        return fail(PDMP_ERR_UNSUPPORTED, "adaptscale is a keyword of spdmp (src/sfact.jl:163): PDMP_SAMPLER_ZIGZAG_LOCAL only");
    if (enable && !(e->lambda_ref > 0))
        return fail(PDMP_ERR_INVALID, "adaptscale acts in the refresh branch (src/sfact.jl:86): lambda_ref must be positive");
    e->adaptscale = enable != 0;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_final_sigma(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* sigma) {
    if (!e || !sigma) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "no state");
    const int64_t d = e->cfg.d;
    if (chain_first < 0 || n < 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "chain range out of bounds");
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (e->adaptscale) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipMemcpy(sigma, e->d_sig_chain.p + chain_first * d, (size_t)(n * d) * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        for (int64_t k = 0; k < n; ++k) std::copy(e->sigma.begin(), e->sigma.end(), sigma + k * d);
    }
    return PDMP_OK;
}

static pdmp_status set_flow_nf(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                               const double* mu, double lambda_ref, double rho, int kind, const double* mu_flow) {
    if (!e || !colptr || !rowval || !nzval) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS) return fail(PDMP_ERR_INVALID, "ensemble was not created with PDMP_SAMPLER_BPS");
    if (!(lambda_ref > 0)) return fail(PDMP_ERR_INVALID, "BouncyParticle needs a strictly positive refreshment rate");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d;
    if (colptr[0] != 0) return fail(PDMP_ERR_INVALID, "colptr[0] must be 0 (0-based CSC)");
    const int64_t nnz = colptr[d];
    bool diag = (nnz == d);
    for (int64_t i = 0; i < d; ++i) {
        if (colptr[i + 1] < colptr[i]) return fail(PDMP_ERR_INVALID, "colptr not monotone");
        for (int64_t p = colptr[i]; p < colptr[i + 1]; ++p) {
            if (rowval[p] < 0 || rowval[p] >= d) return fail(PDMP_ERR_INVALID, "row index out of range");
            if (p > colptr[i] && rowval[p - 1] >= rowval[p]) return fail(PDMP_ERR_INVALID, "rows not ascending");
        }
        if (diag && !(colptr[i + 1] - colptr[i] == 1 && rowval[colptr[i]] == i)) diag = false;
    }
    e->bps_diag = diag;
    bool ident = diag && kind == 0;
    for (int64_t i = 0; ident && i < d; ++i) ident = (nzval[i] == 1.0) && (!mu || mu[i] == 0.0);
    e->bps_ident = ident;
    bool gI = diag;
    for (int64_t i = 0; gI && i < d; ++i) gI = (nzval[i] == 1.0);
    e->bps_gamma_is_I = gI;
    e->bps_has_mass = e->bps_mass_tables = false;
    e->bps_own_target = false;
    e->bps_local_bound = e->bps_subsample = 0;
    e->bps_mom = 0;
    e->bps_sticky = false;
    e->bps_strong = 0;
    e->bps_modern = e->bps_udiag = false;
    e->bps_oscn = 0;
    e->bps_record_limit = 0;
    e->bps_lambda = lambda_ref;
    e->bps_rho = rho;
    pdmp_status st;
    if ((st = e->b_colptr.upload(std::vector<int64_t>(colptr, colptr + d + 1))) != PDMP_OK) return st;
    if ((st = e->b_rowval.upload(std::vector<int64_t>(rowval, rowval + nnz))) != PDMP_OK) return st;
    if ((st = e->b_nzval.upload(std::vector<double>(nzval, nzval + nnz))) != PDMP_OK) return st;
    std::vector<double> muv(d, 0.0);
    if (mu) muv.assign(mu, mu + d);
    if ((st = e->b_mu.upload(muv)) != PDMP_OK) return st;
    std::vector<double> mfv(d, 0.0);
    if (mu_flow) mfv.assign(mu_flow, mu_flow + d);
    if ((st = e->b_mu_flow.upload(mfv)) != PDMP_OK) return st;
    e->bps_flow_kind = kind;
    e->has_flow = true;
    e->has_target = true;
    e->has_state = false;
    return PDMP_OK;
}

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
    e->bps_diag = e->bps_ident = e->bps_gamma_is_I = false;
    e->bps_has_mass = e->bps_mass_tables = false;
    e->bps_own_target = false;
    e->bps_local_bound = e->bps_subsample = 0;
    e->bps_mom = 0;
    e->bps_sticky = false;
    e->bps_strong = 0;
    e->bps_lambda = lambda_ref;
    e->bps_rho = rho;
    e->bps_flow_kind = 0;
    e->b_colptr.release();
    e->b_rowval.release();
    e->b_nzval.release();
    e->b_mu.release();
    e->b_mu_flow.release();
    pdmp_status st;
    if (u_diag) {
        std::vector<double> u(u_diag, u_diag + d), su((size_t)d);
        for (int64_t i = 0; i < d; ++i) su[(size_t)i] = std::sqrt(u[(size_t)i]);
        if ((st = e->b_udiag.upload(u)) != PDMP_OK) return st;
        if ((st = e->b_sudiag.upload(su)) != PDMP_OK) return st;
    }
    e->bps_modern = true;
    e->bps_udiag = u_diag != nullptr;
    e->bps_oscn = oscn ? 1 : 0;
    e->bps_record_limit = 0;
    e->has_flow = true;
    e->has_target = false;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_bps_record_limit(pdmp_ensemble* e, int64_t n) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->bps_modern)
        return fail(PDMP_ERR_INVALID, "set_bps_record_limit: pdmp_ensemble_set_flow_bps_modern first (PDMP_SAMPLER_BPS)");
    if (n < 0) return fail(PDMP_ERR_INVALID, "record limit %lld: 0 (no limit) or a positive number of records", (long long)n);
    e->bps_record_limit = n;
    return PDMP_OK;
}

static pdmp::BpsModernParams bps_modern_params(const pdmp_ensemble* e) {
    pdmp::BpsModernParams q{};
    q.u_diag = e->bps_udiag ? e->b_udiag.p : nullptr;
    q.su_diag = e->bps_udiag ? e->b_sudiag.p : nullptr;
    q.mstate = e->b_mstate.p;
    q.record_limit = e->bps_record_limit;
    q.count_limit = e->dbg_count_limit ? e->dbg_count_limit : pdmp::PDMP_LAUNCH_COUNT_LIMIT;
    q.oscn = e->bps_oscn;
    return q;
}

static void fill_bps_ext(const pdmp_ensemble* e, pdmp::BpsRunParams& B) {
    B.local_bound = e->bps_local_bound;
    B.subsample = e->bps_subsample;
    B.ext = (e->bps_mass_tables || e->bps_local_bound || e->bps_subsample || e->bps_own_target) ? 1 : 0;
    if (e->bps_own_target) {
        B.t_colptr = e->bt_colptr.p;
        B.t_rowval = e->bt_rowval.p;
        B.t_nzval = e->bt_nzval.p;
        B.t_mu = e->bt_mu.p;
        B.ident = 0;  // (the gradient-free register layout belongs to the isotropic TARGET)
    }
    if (e->bps_mass_tables) {
        B.Lcp = e->m_Lcp.p;
        B.Lrv = e->m_Lrv.p;
        B.Lnz = e->m_Lnz.p;
        B.Ucp = e->m_Ucp.p;
        B.Urv = e->m_Urv.p;
        B.Unz = e->m_Unz.p;
    }
}

static pdmp::BpsRunParams bps_run_params(const pdmp_ensemble* e, double T, int flags) {
    pdmp::BpsRunParams B{};
    B.colptr = e->b_colptr.p;
    B.rowval = e->b_rowval.p;
    B.nzval = e->b_nzval.p;
    B.mu = e->b_mu.p;
    B.mu_flow = e->b_mu_flow.p;
    B.flow_kind = e->bps_flow_kind;
    B.ident = e->bps_ident ? 1 : 0;
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
    B.lambda_ref = e->bps_lambda;
    B.rho = e->bps_rho;
    B.flags = flags;
    B.adapt = e->cfg.adapt;
    fill_bps_ext(e, B);
    return B;
}

pdmp_status pdmp_ensemble_set_mass_cholesky(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval,
                                            const double* nzval) {
    if (!e || !colptr || !rowval || !nzval) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->has_flow)
        return fail(PDMP_ERR_INVALID, "set_flow_bps / set_flow_boomerang first (PDMP_SAMPLER_BPS)");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d;
    if (colptr[0] != 0) return fail(PDMP_ERR_INVALID, "colptr[0] must be 0 (0-based CSC)");
    const int64_t nnz = colptr[d];
    if (nnz < d || nnz >= ((int64_t)1 << 31)) return fail(PDMP_ERR_INVALID, "mass factor: bad number of entries");
    bool identity = (nnz == d);
    for (int64_t j = 0; j < d; ++j) {
        if (colptr[j + 1] <= colptr[j]) return fail(PDMP_ERR_INVALID, "mass factor: empty column %lld", (long long)j);
        if (rowval[colptr[j]] != j) return fail(PDMP_ERR_INVALID, "mass factor must be LOWER triangular with a stored diagonal");
        const double djj = nzval[colptr[j]];
        if (!(djj != 0.0) || djj != djj) return fail(PDMP_ERR_INVALID, "mass factor: zero or NaN diagonal at %lld", (long long)j);
        for (int64_t p = colptr[j] + 1; p < colptr[j + 1]; ++p)
            if (rowval[p] <= rowval[p - 1] || rowval[p] >= d) return fail(PDMP_ERR_INVALID, "mass factor: rows not ascending / out of range");
        if (djj != 1.0) identity = false;
    }
    e->bps_has_mass = true;
    e->bps_mass_tables = false;
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
    pdmp_status st;
    if ((st = e->m_Lcp.upload(lcp)) != PDMP_OK) return st;
    if ((st = e->m_Lrv.upload(lrv)) != PDMP_OK) return st;
    if ((st = e->m_Lnz.upload(lnz)) != PDMP_OK) return st;
    if ((st = e->m_Ucp.upload(ucp)) != PDMP_OK) return st;
    if ((st = e->m_Urv.upload(urv)) != PDMP_OK) return st;
    if ((st = e->m_Unz.upload(unz)) != PDMP_OK) return st;
    e->bps_mass_tables = true;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_bps_options(pdmp_ensemble* e, int local_bound, int subsample) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->has_flow)
        return fail(PDMP_ERR_INVALID, "set_flow_bps / set_flow_boomerang first (PDMP_SAMPLER_BPS)");
    if (local_bound && e->bps_flow_kind != 0)
        return fail(PDMP_ERR_UNSUPPORTED, "c::LocalBound is defined for BouncyParticle only (src/not_fact_samplers.jl:29-31)");
    e->bps_local_bound = local_bound ? 1 : 0;
    e->bps_subsample = subsample ? 1 : 0;
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
    pdmp_status st;
    if (order >= 1) {
        if (e->b_j1.n != nd && (st = e->b_j1.alloc(nd)) != PDMP_OK) return st;
    } else {
        e->b_j1.release();
    }
    if (order >= 2) {
        if (e->b_j2.n != nd && (st = e->b_j2.alloc(nd)) != PDMP_OK) return st;
    } else {
        e->b_j2.release();
    }
    e->bps_mom = order;
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
    pdmp_status st;
    if ((st = e->b_kappa.upload(std::vector<double>(kappa, kappa + d))) != PDMP_OK) return st;
    e->bps_sticky = true;
    e->bps_strong = strong_upperbounds ? 1 : 0;
    return PDMP_OK;
}

static pdmp::BpsStickyParams bps_sticky_params(const pdmp_ensemble* e) {
    pdmp::BpsStickyParams q{};
    q.kappa = e->b_kappa.p;
    q.thf = e->b_thf.p;
    q.tfrez = e->b_tfrez.p;
    q.fmask = e->b_fmask.p;
    q.ev_f = e->b_ev_f.p;
    q.strong_upperbounds = e->bps_strong;
    return q;
}

static pdmp::BpsMomParams bps_moments_params(const pdmp_ensemble* e) {
    pdmp::BpsMomParams m{};
    m.mom = e->bps_mom;
    m.J1 = e->bps_mom >= 1 ? e->b_j1.p : nullptr;
    m.J2 = e->bps_mom >= 2 ? e->b_j2.p : nullptr;
    return m;
}

// The moments of chains [chain_first, chain_first + n) at T into b_jT (and b_jT2 with `two`), rows 0..n-1 -- after checking that T lies
// on the stretch of every chain's path its state describes: t <= T <= min(tp, tau_ref) (no event between the chain's clock and T), the
// chain neither BOUND_VIOLATED nor STALLED.
static pdmp_status bps_moments_at(pdmp_ensemble* e, double T, int64_t chain_first, int64_t n, bool two) {
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
    pdmp_status st;
    if (e->b_jT.n != (size_t)(nch * d) && (st = e->b_jT.alloc((size_t)(nch * d))) != PDMP_OK) return st;
    if (two && e->b_jT2.n != (size_t)(nch * d) && (st = e->b_jT2.alloc((size_t)(nch * d))) != PDMP_OK) return st;
    pdmp::BpsRunParams B{};
    B.x = e->b_x.p;
    B.th = e->b_th.p;
    B.scal = e->b_scal.p;
    B.mu_flow = e->b_mu_flow.p;
    B.flow_kind = e->bps_flow_kind;
    B.d = d;
    int rc = pdmp::launch_bps_moments_tail(B, bps_moments_params(e), chain_first, n, T, e->b_jT.p, two ? e->b_jT2.p : nullptr, e->stream);
    if (rc != 0) return fail(PDMP_ERR_HIP, "bps_moments_tail launch failed: %s", hipGetErrorString((hipError_t)rc));
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_bps_moments(pdmp_ensemble* e, double T, int64_t chain_first, int64_t n, double* j1, double* j2) {
    if (!e || !j1) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || e->bps_mom < 1)
        return fail(PDMP_ERR_INVALID, "no path moments: a BPS ensemble with pdmp_ensemble_set_bps_moments(order >= 1)");
    if (j2 && e->bps_mom < 2) return fail(PDMP_ERR_INVALID, "∫x² dt needs moments of order 2 (this ensemble keeps order %d)", e->bps_mom);
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "no state");
    if (chain_first < 0 || n < 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "chain range");
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

static pdmp_status init_state_bps(pdmp_ensemble* e, double t0, const double* x0, const double* theta0, double c, const uint64_t* seeds) {
    if (!e || !x0 || !theta0 || !seeds) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_bps first");
    if (e->bps_sticky) {
        // sticky_pdmp_inner! (src/ss_not_fact.jl:104-179) has no LocalBound, subsample or path-moment form here, and never reads a BouncyParticle's L
        if (e->cfg.d > 64 * pdmp::BPS_STICKY_WORDS)
            return fail(PDMP_ERR_UNSUPPORTED, "sticky BouncyParticle / Boomerang keeps d <= 1024 coordinates in registers: got %lld", (long long)e->cfg.d);
        if (e->bps_local_bound) return fail(PDMP_ERR_UNSUPPORTED, "set_bps_sticky: not together with local_bound (set_bps_options)");
        if (e->bps_subsample) return fail(PDMP_ERR_UNSUPPORTED, "set_bps_sticky: not together with subsample (set_bps_options)");
        if (e->bps_mom >= 1) return fail(PDMP_ERR_UNSUPPORTED, "set_bps_sticky: not together with set_bps_moments(order >= 1)");
        if (e->bps_flow_kind == 1 && e->bps_mass_tables)
            return fail(PDMP_ERR_UNSUPPORTED, "set_bps_sticky: a Boomerang with a general mass factor L (set_mass_cholesky) is not implemented: identity only");
    }
    if (e->bps_modern) {
        // the speed-recorded driver always bounds locally and always subsamples; its options are its own
        if (!e->bps_own_target)
            return fail(PDMP_ERR_INVALID, "set_flow_bps_modern: the flow has no Γ of its own, pdmp_ensemble_set_target_gaussian_csc must follow it");
        if (e->cfg.d > 1024)
            return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern keeps d <= 1024 coordinates in registers: got d = %lld", (long long)e->cfg.d);
        if (e->bps_mom >= 1) return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: not together with set_bps_moments(order >= 1)");
        if (e->bps_sticky) return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: not together with set_bps_sticky");
        if (e->bps_subsample) return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: not together with subsample (set_bps_options): this driver always subsamples");
        if (e->bps_local_bound) return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: not together with local_bound (set_bps_options): this driver always bounds locally");
        if (e->bps_oscn && e->bps_udiag) return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: oscn with u_diag is not defined (src/not_fact_samplers.jl:267 asserts L == I)");
        if (e->bps_oscn && e->bps_mass_tables)
            return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: oscn with a mass factor (set_mass_cholesky) that is not the identity (src/not_fact_samplers.jl:267)");
        if (e->bps_udiag && e->bps_has_mass) return fail(PDMP_ERR_UNSUPPORTED, "set_flow_bps_modern: u_diag together with a mass factor (set_mass_cholesky): one metric only");
        if (!(c > 0) || !std::isfinite(c)) return fail(PDMP_ERR_INVALID, "LocalBound(c) needs a finite c > 0 (the bound expires after 2√d/c/V): got %g", c);
    }
    if (!e->bps_modern && !e->bps_sticky && e->bps_flow_kind == 0 && !e->bps_gamma_is_I && !e->bps_has_mass)
        return fail(PDMP_ERR_UNSUPPORTED,
                    "BouncyParticle(Γ ≠ I) carries the mass factor L = cholesky(Symmetric(Γ)).L (src/types.jl:43): pass it with "
                    "pdmp_ensemble_set_mass_cholesky (an identity factor selects the identity mass explicitly)");
    if (e->bps_flow_kind == 1 && !e->bps_has_mass)
        return fail(PDMP_ERR_UNSUPPORTED,
                    "Boomerang(Γ, μ, λ) carries L = cholesky(Symmetric(Γ)).L (src/types.jl:66) and this library never sees the flow's Γ: "
                    "pass the factor with pdmp_ensemble_set_mass_cholesky (an identity factor selects the identity mass explicitly)");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d, n = e->cfg.nchains, cap = e->cfg.trace_capacity;
    pdmp_status st;
    // (arrays of the right size are kept: a second set_state -- set_state_bps's placement probes among them -- writes into the same memory)
    if (e->b_x.n != (size_t)(n * d) && (st = e->b_x.alloc((size_t)(n * d))) != PDMP_OK) return st;
    if (e->b_th.n != (size_t)(n * d) && (st = e->b_th.alloc((size_t)(n * d))) != PDMP_OK) return st;
    if (e->b_scal.n != (size_t)(n * 8) && (st = e->b_scal.alloc((size_t)(n * 8))) != PDMP_OK) return st;
    if (e->d_hdr.n != (size_t)n && (st = e->d_hdr.alloc((size_t)n)) != PDMP_OK) return st;
    if (cap > 0) {
        if (e->b_ev_t.n != (size_t)(n * cap) && (st = e->b_ev_t.alloc((size_t)(n * cap))) != PDMP_OK) return st;
        if (e->b_ev_x.n != (size_t)(n * cap * d) && (st = e->b_ev_x.alloc((size_t)(n * cap * d))) != PDMP_OK) return st;
        if (e->b_ev_th.n != (size_t)(n * cap * d) && (st = e->b_ev_th.alloc((size_t)(n * cap * d))) != PDMP_OK) return st;
    }
    HIP_TRY(hipMemcpy(e->b_x.p, x0, (size_t)(n * d) * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->b_th.p, theta0, (size_t)(n * d) * sizeof(double), hipMemcpyHostToDevice));
    DevBuf<uint64_t> sseed;
    if ((st = sseed.alloc((size_t)n)) != PDMP_OK) return st;
    HIP_TRY(hipMemcpy(sseed.p, seeds, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
    const pdmp::BpsRunParams B = bps_run_params(e, t0, 0);  // (the init kernel reads the tables and the state arrays of the event loop's block)
    // the moments start at t0 (also after set_state_bps's placement probes, which run launches in between)
    if (e->bps_mom >= 1) HIP_TRY(hipMemsetAsync(e->b_j1.p, 0, (size_t)(n * d) * sizeof(double), e->stream));
    if (e->bps_mom >= 2) HIP_TRY(hipMemsetAsync(e->b_j2.p, 0, (size_t)(n * d) * sizeof(double), e->stream));
    if (e->bps_modern) {
        if (e->b_mstate.n != (size_t)(n * 4) && (st = e->b_mstate.alloc((size_t)(n * 4))) != PDMP_OK) return st;
        int rcm = pdmp::launch_bps_modern_init(B, bps_modern_params(e), n, sseed.p, t0, c, e->stream);
        if (rcm != 0) return fail(PDMP_ERR_HIP, "bps_modern_init launch failed (%d)", rcm);
        HIP_TRY(hipStreamSynchronize(e->stream));
        e->has_state = true;
        e->ran = false;
        e->timed = false;
        return PDMP_OK;
    }
    if (e->bps_sticky) {
        const size_t W = (size_t)pdmp::BPS_STICKY_WORDS;
        if (e->b_thf.n != (size_t)(n * d) && (st = e->b_thf.alloc((size_t)(n * d))) != PDMP_OK) return st;
        if (e->b_tfrez.n != (size_t)(n * d) && (st = e->b_tfrez.alloc((size_t)(n * d))) != PDMP_OK) return st;
        if (e->b_fmask.n != (size_t)n * W && (st = e->b_fmask.alloc((size_t)n * W)) != PDMP_OK) return st;
        if (cap > 0) {
            if (e->b_ev_f.n != (size_t)(n * cap) * W && (st = e->b_ev_f.alloc((size_t)(n * cap) * W)) != PDMP_OK) return st;
            HIP_TRY(hipMemsetAsync(e->b_ev_f.p, 0, e->b_ev_f.n * sizeof(uint64_t), e->stream));  // (words past the last slot stay 0)
        }
        int rcs = pdmp::launch_bps_sticky_init(B, bps_sticky_params(e), n, sseed.p, t0, c, e->stream);
        if (rcs != 0) return fail(PDMP_ERR_HIP, "bps_sticky_init launch failed (%d)", rcs);
        HIP_TRY(hipStreamSynchronize(e->stream));
        e->has_state = true;
        e->ran = false;
        e->timed = false;
        return PDMP_OK;
    }
    int rc = pdmp::launch_bps_init(B, n, sseed.p, t0, c, e->stream);
    if (rc != 0) return fail(PDMP_ERR_HIP, "bps_init launch failed (%d)", rc);
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->has_state = true;
    e->ran = false;
    e->timed = false;
    return PDMP_OK;
}

// The Bouncy Particle streams every event's (x, θ) into two large arrays; whether those two allocations get along decides 4.5 or 5.3 ms per step of config
// C2 (tools/mode_move_bps.py: moving either flips it; x, θ and the event times do not matter) -- the same property of the memory as init_state_tuned's.
// With a trace of at least 2 GB per array: fill it once (every chain pauses when its segment is full), time that, give the θ array (then the x array) new hipMallocs,
// keep the fastest pair, set the state again.
pdmp_status pdmp_ensemble_set_state_bps(pdmp_ensemble* e, double t0, const double* x0, const double* theta0, double c,
                                        const uint64_t* seeds) {
    if (e) e->tune_log.clear();
    pdmp_status st = init_state_bps(e, t0, x0, theta0, c, seeds);
    if (st != PDMP_OK) return st;
    const size_t ev_bytes = e->b_ev_th.n * sizeof(double);
    size_t freeb = 0, totb = 0;
    if (e->bps_modern) return PDMP_OK;  // (a record per 1/λref of speed-time: the trace writes do not bound this loop, nothing to place)
    if (e->place_tune == 0 || e->cfg.trace_capacity <= 0 || ev_bytes < ((size_t)2 << 30) || e->b_ev_th.placed.va) return PDMP_OK;
    if (hipMemGetInfo(&freeb, &totb) != hipSuccess || freeb < 6 * ev_bytes + ((size_t)8 << 30)) {
        (void)hipGetLastError();
        return PDMP_OK;
    }
    const auto t_begin = std::chrono::steady_clock::now();
    std::vector<void*> ths{(void*)e->b_ev_th.p}, xs{(void*)e->b_ev_x.p};
    struct Trial { size_t x, th; float ms; };
    std::vector<Trial> trials;
    auto measure = [&](size_t kx, size_t kth) -> pdmp_status {
        e->b_ev_x.p = static_cast<double*>(xs[kx]);
        e->b_ev_th.p = static_cast<double*>(ths[kth]);
        pdmp_status r = trials.empty() ? PDMP_OK : init_state_bps(e, t0, x0, theta0, c, seeds);
        if (r != PDMP_OK) return r;
        if ((r = ensemble_run_impl(e, t0 + 1.0e30, PDMP_RUN_STOP_BEFORE, nullptr)) != PDMP_OK) return r;
        float t = 0;
        HIP_TRY(hipEventSynchronize(e->ev1));
        HIP_TRY(hipEventElapsedTime(&t, e->ev0, e->ev1));
        trials.push_back({kx, kth, t});
        return PDMP_OK;
    };
    auto best = [&]() { return *std::min_element(trials.begin(), trials.end(), [](const Trial& a, const Trial& b) { return a.ms < b.ms; }); };
    auto worst = [&]() { return *std::max_element(trials.begin(), trials.end(), [](const Trial& a, const Trial& b) { return a.ms < b.ms; }); };
    // (three levels here: the trace filled in 5.9-6.1, 6.3 or 6.9-7.3 ms -- steps of 4.6, 4.9, 5.4 ms; done once the whole spread has been seen)
    auto settled = [&]() { return trials.size() >= 2 && worst().ms > 1.15f * best().ms; };
    st = measure(0, 0);
    for (int step = 0; st == PDMP_OK && step < 5 && !settled(); ++step) {  // new θ arrays three times, then new x arrays twice
        void* np = nullptr;
        if (hipMalloc(&np, ev_bytes) != hipSuccess) {
            (void)hipGetLastError();
            break;
        }
        if (step < 3) {
            ths.push_back(np);
            st = measure(best().x, ths.size() - 1);
        } else {
            xs.push_back(np);
            st = measure(xs.size() - 1, best().th);
        }
    }
    const Trial b = trials.empty() ? Trial{0, 0, 0.f} : best();
    e->b_ev_x.p = static_cast<double*>(xs[b.x]);
    e->b_ev_th.p = static_cast<double*>(ths[b.th]);
    HIP_TRY(hipDeviceSynchronize());
    for (size_t k = 0; k < ths.size(); ++k)
        if (k != b.th) (void)hipFree(ths[k]);
    for (size_t k = 0; k < xs.size(); ++k)
        if (k != b.x) (void)hipFree(xs[k]);
    pdmp_status st2 = init_state_bps(e, t0, x0, theta0, c, seeds);
    e->last_kernel = "";
    char t[96];
    e->tune_log = "placement probes (ms, the trace filled once):";
    for (const Trial& q : trials) {
        snprintf(t, sizeof t, " %.2f[x%zu th%zu]", q.ms, q.x, q.th);
        e->tune_log += t;
    }
    snprintf(t, sizeof t, "; kept x%zu th%zu; %.2f s", b.x, b.th, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count());
    e->tune_log += t;
    return st != PDMP_OK ? st : st2;
}

pdmp_status pdmp_ensemble_bps_trace_copy(pdmp_ensemble* e, int64_t chain, int64_t first, int64_t count, double* t, double* x,
                                         double* theta) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    const int64_t cap = e->cfg.trace_capacity, d = e->cfg.d;
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || cap <= 0) return fail(PDMP_ERR_INVALID, "no BPS trace buffer");
    if (chain < 0 || chain >= e->cfg.nchains || first < 0 || count < 0 || first + count > cap)
        return fail(PDMP_ERR_INVALID, "trace range out of bounds");
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
    if (chain_first < 0 || n < 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "chain range");
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

// bit e & 63 of word e >> 6 -> one byte per coordinate
static void unpack_free_mask(const uint64_t* w, int64_t d, uint8_t* f) {
    for (int64_t i = 0; i < d; ++i) f[i] = (uint8_t)((w[i >> 6] >> (i & 63)) & 1ull);
}

pdmp_status pdmp_ensemble_bps_trace_free_copy(pdmp_ensemble* e, int64_t chain, int64_t first, int64_t count, uint8_t* f) {
    if (!e || !f) return fail(PDMP_ERR_INVALID, "null argument");
    const int64_t cap = e->cfg.trace_capacity, d = e->cfg.d, W = pdmp::BPS_STICKY_WORDS;
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->bps_sticky || !e->has_state || cap <= 0)
        return fail(PDMP_ERR_INVALID, "no sticky BPS trace buffer (pdmp_ensemble_set_bps_sticky, trace_capacity > 0, set_state_bps)");
    if (chain < 0 || chain >= e->cfg.nchains || first < 0 || count < 0 || first + count > cap)
        return fail(PDMP_ERR_INVALID, "trace range out of bounds");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    if (count == 0) return PDMP_OK;
    std::vector<uint64_t> w((size_t)(count * W));
    HIP_TRY(hipMemcpy(w.data(), e->b_ev_f.p + (chain * cap + first) * W, w.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < count; ++k) unpack_free_mask(w.data() + k * W, d, f + k * d);
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_bps_final_sticky(pdmp_ensemble* e, int64_t chain_first, int64_t n, uint8_t* f, double* theta_f) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS || !e->bps_sticky || !e->has_state) return fail(PDMP_ERR_INVALID, "no sticky BPS state");
    if (chain_first < 0 || n < 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "chain range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d, W = pdmp::BPS_STICKY_WORDS;
    if (n == 0) return PDMP_OK;
    if (f) {
        std::vector<uint64_t> w((size_t)(n * W));
        HIP_TRY(hipMemcpy(w.data(), e->b_fmask.p + chain_first * W, w.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < n; ++k) unpack_free_mask(w.data() + k * W, d, f + k * d);
    }
    if (theta_f) HIP_TRY(hipMemcpy(theta_f, e->b_thf.p + chain_first * d, (size_t)(n * d) * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

pdmp_status pdmp_debug_sticky_eval(int device, int fn, int64_t n, const double* a, const double* b, const double* c, double* out) {
    if (!a || !b || !c || !out || n <= 0 || n > ((int64_t)1 << 30)) return fail(PDMP_ERR_INVALID, "bad argument");
    if (fn < 0 || fn > 2) return fail(PDMP_ERR_INVALID, "pdmp_debug_sticky_eval: fn 0 (atan), 1 (linear freezing time) or 2 (Boomerang freezing time)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> in, res;
    pdmp_status st = in.alloc((size_t)(3 * n));
    if (st == PDMP_OK) st = res.alloc((size_t)n);
    if (st != PDMP_OK) return st;
    HIP_TRY(hipMemcpy(in.p, a, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in.p + n, b, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in.p + 2 * n, c, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    int rc = pdmp::launch_bps_sticky_eval(fn, n, in.p, in.p + n, in.p + 2 * n, res.p, nullptr);
    if (rc != 0) return fail(PDMP_ERR_HIP, "sticky eval launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, res.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
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
