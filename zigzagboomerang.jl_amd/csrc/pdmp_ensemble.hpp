// pdmp_ensemble.hpp -- what the host units of the C ABI (pdmp_capi*.hip) share: error reporting, the device buffer, the ensemble, and the few
// helpers more than one of them calls.  Host code only; nothing here is exported (hidden visibility: the library's symbols are include/*.h's).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pdmp_debug.h"
#include "pdmp_engine.hpp"

#pragma GCC visibility push(hidden)

// pdmp_capi.hip: the thread-local message pdmp_last_error() returns; HIP_TRY's message (it carries the message of a deferred consumer launch that
// failed inside device_sync); a launcher's non-zero return, spelled as a hipError_t or as a number
pdmp_status fail(pdmp_status st, const char* fmt, ...);
pdmp_status fail_hip(const char* expr, hipError_t err);
pdmp_status fail_launch(const char* launcher, int rc, bool hip_rc);

#define HIP_TRY(expr)                                    \
    do {                                                 \
        hipError_t e_ = (expr);                          \
        if (e_ != hipSuccess) return fail_hip(#expr, e_); \
    } while (0)
// "<name> launch failed: <hipGetErrorString>" -- LAUNCH_TRY_CODE: "<name> launch failed (<rc>)"
#define LAUNCH_TRY_AS(name, rc, hip_rc)                            \
    do {                                                           \
        const int rc_ = (rc);                                      \
        if (rc_ != 0) return fail_launch(name, rc_, hip_rc);       \
    } while (0)
#define LAUNCH_TRY(name, rc) LAUNCH_TRY_AS(name, rc, true)
#define LAUNCH_TRY_CODE(name, rc) LAUNCH_TRY_AS(name, rc, false)

#define PDMP_TRY(expr)                       \
    do {                                     \
        const pdmp_status st_ = (expr);      \
        if (st_ != PDMP_OK) return st_;      \
    } while (0)

// The factorised samplers (ZigZag / FactBoomerang / sticky) and the non-factorised ones (BouncyParticle / Boomerang) keep different
// device state: an entry point of the wrong family is a call-order error, reported as a status (never a crash).
#define NEED_FACTORISED(e)                                                                                               \
    do {                                                                                                                 \
        if ((e) && (e)->cfg.sampler == PDMP_SAMPLER_BPS)                                                                 \
            return fail(PDMP_ERR_INVALID, "%s: the ensemble was created with PDMP_SAMPLER_BPS (use the pdmp_ensemble_*bps* calls)", \
                        __func__);                                                                                       \
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
        PDMP_TRY(alloc(h.size()));
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

// What a flow setter of the Bouncy Particle family decides, and what the option setters that follow it switch on: set_flow_bps / _boomerang and
// set_flow_bps_modern both start from BpsOptions{}, so nothing carries over from one flow to the next.
struct BpsOptions {
    int flow_kind = 0;
    bool ident = false, diag = false;
    double lambda = 0.0, rho = 0.0;
    bool gamma_is_I = false;  // flow Γ == I exactly: cholesky(Γ).L = I needs no factor from the caller
    bool has_mass = false;    // a factor was supplied (identity factors are dropped: mass_tables stays false)
    bool mass_tables = false;
    int local_bound = 0, subsample = 0;
    bool own_target = false;  // set_target_gaussian_csc on a BouncyParticle ensemble: ∇ϕ! differs from B.Γ(x − B.μ)
    int mom = 0;              // pdmp_ensemble_set_bps_moments: 0 off, 1 ∫x dt, 2 ∫x dt and ∫x² dt
    bool sticky = false;      // sticky Bouncy Particle / Boomerang (pdmp_ensemble_set_bps_sticky, src/ss_not_fact.jl)
    int strong = 0;
    bool modern = false;      // speed-recorded Bouncy Particle (pdmp_ensemble_set_flow_bps_modern, src/not_fact_samplers.jl:151-384)
    bool udiag = false;
    int oscn = 0;
    int64_t record_limit = 0;
    bool logit = false;       // pdmp_ensemble_set_target_bps_logistic: the speed-recorded driver's logistic-regression target (pdmp_bps_logit.inc)
};

// Members by concern.  pdmp_ensemble_destroy synchronises the device before it deletes the ensemble, so no member's release depends on another's:
// the order of declaration carries no meaning.
// The struct alone stands outside the hidden region: it is the opaque type of the public header, and its implicit constructor, destructor and
// tables() have always been weak default-visibility symbols of the library.  Leaving them so keeps the dynamic symbol table what it was.
#pragma GCC visibility pop
struct pdmp_ensemble {
    // lifecycle
    pdmp_config cfg{};
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    bool has_flow = false, has_target = false, has_state = false;
    bool ran = false;  // a run happened since set_state (pdmp_ensemble_run_partitioned starts from a fresh state only)
    int n_cu = 0;      // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    const char* last_kernel = "";  // event-loop kernel of the last pdmp_ensemble_run (pdmp_debug_last_kernel)

    // flow / tables: host copies of the flow and of the derived tables (inputs of the per-coordinate blob), the blob, spec8g's tables, the device tables
    std::vector<uint32_t> colptr, rowval;
    std::vector<double> bval, mu, sigma;
    double lambda_ref = 0.0, rho = 0.0;
    int64_t nnz = 0;
    uint32_t nblk = 0, nblk_pad = 0;
    int64_t dk = 0;
    bool has_tmu = false;
    int32_t lattice_n = 0;   // the flow's graph is the n x n 5-point lattice in column-major numbering (0: it is not)
    uint32_t typ_extra = 0;  // the most frequent |G1[i]| - 1 of the flow's graph (set_flow): what the one-proposal-per-lane tracked kernels unroll for
    std::vector<double> h_gmu_b, h_gmu_t, h_tval;
    std::vector<uint32_t> h_sptr, h_sidx, h_qptr;
    std::vector<uint8_t> h_pos, h_selfpos;
    uint32_t blob_w = 0, blob_w_pad = 0, blob_sw = 0, blob_pw = 0, blob_kmax = 0, blob_mmax = 0;
    bool use_spec = false;  // speculative 4-events-per-iteration kernel (zz_local_spec_kernel)
    DevBuf<uint64_t> d_blob;
    DevBuf<uint32_t> d_tix;
    size_t n_templates = 0;
    uint32_t common_tix = 0;
    bool has_g8 = false, g8_same = false;
    int g8_gw = 8;  // lanes per event of zz_local_spec8g_kernel: 8 (|S| <= 32) or 16 (|S| <= 64)
    DevBuf<uint64_t> d_g8_line;
    DevBuf<double> d_g8_member, d_g8_gamt;
    DevBuf<uint32_t> d_colptr, d_rowval, d_sptr, d_sidx, d_qptr;
    DevBuf<uint8_t> d_pos, d_selfpos;
    DevBuf<double> d_bval, d_tval, d_gmu_b, d_gmu_t, d_c, d_c2, d_sigma;
    DevBuf<pdmp::CoordConst> d_cc;

    // state
    DevBuf<pdmp::ZzRec> d_rec;
    DevBuf<double> d_keys, d_c_chain;
    DevBuf<pdmp::DevChain> d_hdr;
    DevBuf<pdmp_event> d_ev;
    double t0_state = 0.0;
    double run_T = 0.0;  // horizon of the last run (t0 before the first): no read of the path integrals beyond it (fact_integrals_at)
    bool keep_integrals = true;  // pdmp_ensemble_set_path_integrals

    // tracking and line layout: the tracked-gradient kernels (pdmp_ensemble_set_gradient_tracking)
    bool track_requested = false, track = false, track_two_sums = false;
    int track_mean = 0;  // zz_local_trackp: 0 no mean, 1 the flow's Γμ in the bounds, 2 also in the rate (the target's Γμ equals it); decided by set_state
    bool track_lg = false;     // tracked bounds under the logistic target (zz_logistic_lds_kernel<.., TRK>); d_trk holds (g, gd, tg) per coordinate
    DevBuf<double> d_trk;
    bool exactp = false;       // the moving evaluation runs on zz_local_exactp_kernel (plain lattice; decided by set_state)
    bool track_pairs = false;  // the queue's level 0 is (key, time) pairs in d_kp (pdmp_trackp.hip); decided by set_state
    DevBuf<double> d_kp;
    bool track_generic = false;  // ... on a graph that is not the plain lattice: G1 ids in the records, Γ values in d_gam8 (|G1| <= 8)
    DevBuf<double> d_gam8;
    DevBuf<uint16_t> d_nb16;
    // the line layout (pdmp_trackl.hip): full-width launches on the plain lattice run on d_tl_lines / d_tl_cold; d_rec / d_kp are brought up to
    // date (canon_stale) only when something reads the state -- final_state, the path-integral kernels, consume_begin
    bool track_lines = false, canon_stale = false;
    DevBuf<pdmp::TrLine> d_tl_lines;
    DevBuf<pdmp::TrCold> d_tl_cold;

    // general / logistic: the general-degree kernel's tables, and the logistic target's with the packed ones of its LDS-resident kernel (empty: not qualified)
    int flow_kind = 0;
    DevBuf<double> d_mu, d_diag;
    bool needs_general = false;
    bool has_g1mask = false;  // pdmp_ensemble_set_neighbourhood: the tables' pattern is G ⊋ G1
    uint32_t mmax_all = 0;
    int target_kind = 0;
    DevBuf<uint16_t> d_pos16, d_selfpos16, d_qrow16;
    DevBuf<double> d_qbval, d_qtval, d_sig_chain;
    DevBuf<uint32_t> d_member;
    bool adaptscale = false, local_bound = false;
    DevBuf<int64_t> lg_Acp, lg_Arv, lg_Atcp, lg_Atrv;
    DevBuf<uint32_t> lg_Atrv32, lg_arow;
    DevBuf<double> d_hot;  // the moving halves of the records, packed, while a launch sweeps long logistic rows (pdmp_general.hip)
    DevBuf<double> lg_Anz, lg_Atnz, lg_y, lg_ny, lg_u0, lg_ns0;
    DevBuf<pdmp::LgCoord> lg_coord;
    DevBuf<pdmp::LgObs> lg_obs;
    double lg_gamma0 = 0.0;
    int64_t lg_k = 0, lg_nemax = 0;
    // the diffusion bridge (pdmp_ensemble_set_target_diffusion_bridge): target_kind == TARGET_BRIDGE, its parameters
    pdmp::ZzBridgeParams bridge{};
    // the Cholesky-factor precision target (pdmp_ensemble_set_target_precision_cholesky): target_kind == TARGET_PRECISION, YY on the device
    pdmp::ZzPrecisionParams precision{};
    DevBuf<double> d_prec_yy;

    // sticky ZigZag
    DevBuf<double> d_kappa, d_thf;
    bool has_kappa = false;
    int reversible = 0, strong_upperbounds = 0;

    // stickyzz (PDMP_SAMPLER_BARRIER_ZIGZAG, pdmp_ensemble_set_barriers): the table on the device and its host copy (set_state checks x0, θ0 against it);
    // d_thf holds v_old, strong_upperbounds is the member above
    DevBuf<pdmp::BarrierEntry> d_barriers;
    std::vector<pdmp::BarrierEntry> h_barriers;
    bool has_barriers = false;

    // consumers and async: streaming trace consumers (pdmp_ensemble_consume_*) -- cursor per (chain, coordinate), per-chain progress, the grid
    DevBuf<unsigned char> d_ccur, d_cmeta;
    DevBuf<double> d_cgrid;
    DevBuf<double> d_ccm;      // pdmp_ensemble_consume_cummean: (t, y / (2 t)) per event slot of the last consumed segment [nchains x cap x 2], or empty
    bool cons_cummean = false;
    bool consuming = false, cons_z = false;
    bool cons_occ = false;  // pdmp_ensemble_barrier_consume_begin: the occupation state (time frozen / hits per barrier) lies behind the cursors
    bool cons_unordered = false;  // pdmp_ensemble_refresh_consume_begin: the trace is sorted within a coordinate only (refresh clock); the unordered walk serves it
    double cons_dt = 0.0;
    int64_t cons_K = 0;
    // pdmp_ensemble_consume_condition: the conditional trace's own cursors (t, x, θ) [3 x nchains x d], the list of supp n (cn_idx; cn_loc[] =
    // position in it or −1), p then n over the list, per-chain progress, hit times [nchains x max_hits] and rows [nchains x max_hits x d]
    DevBuf<double> d_cn_cur, d_cn_pn, d_cn_t, d_cn_x;
    DevBuf<int32_t> d_cn_loc, d_cn_idx;
    DevBuf<unsigned char> d_cn_meta;
    bool cn_on = false;
    bool cons_started = false;  // a consume / consume_async happened since consume_begin
    int cn_nS = 0;
    int64_t cn_max_hits = 0;
    // pdmp_ensemble_consume_pairs: the pair list, its adjacency table (coordinate -> (partner, slot of S)), the centre [d], the pair consumer's own
    // cursors (t, x, θ, J) [nchains x d] and progress, the accumulators S [nchains x npairs]; pr_out: what consume_pair_integrals last read
    // (S [n x npairs], J [n x d], T_last [n]), reserved by the first read
    DevBuf<int32_t> d_pr_ptr, d_pr_pi, d_pr_pj;
    DevBuf<pdmp::PairAdj> d_pr_adj;
    DevBuf<double> d_pr_c, d_pr_S, d_pr_out;
    DevBuf<unsigned char> d_pr_cur, d_pr_meta;
    bool pr_on = false;
    int64_t pr_np = 0;
    // pdmp_ensemble_consume_hist: the map coordinate -> slot [d], the listed coordinates with their ranges and widths [m], the histogram consumer's
    // own cursors (t, x, θ, Z) [nchains x m] and progress, the rows H [nchains x m x (bins + 2)]; hs_out: what consume_histogram last read (H, Z,
    // T_last), reserved by the first read
    DevBuf<int32_t> d_hs_slot, d_hs_coords;
    DevBuf<double> d_hs_lo, d_hs_hi, d_hs_w, d_hs_H, d_hs_out;
    DevBuf<unsigned char> d_hs_cur, d_hs_meta;
    bool hs_on = false;
    int64_t hs_m = 0;
    int32_t hs_B = 0;
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

    // ESS (pdmp_ensemble_batch_means, pdmp_ensemble_ess_*)
    DevBuf<double> d_jprev, d_sum, d_jstart, d_essacc;
    double ess_T0 = 0.0, ess_Tlast = 0.0;
    int64_t ess_batches = -1;  // -1: no ess_begin yet

    // placement
    pdmp::PlaceConfig place_cfg;  // pdmp_debug_set_placement
    int place_tune = 1;           // init_state_tuned: 1 (default) probe and re-allocate, 0 take what hipMalloc gives
    std::string tune_log;         // init_state_tuned: the placement probes of the last set_state (pdmp_debug_placement)

    // debug (include/pdmp_debug.h): per-ensemble state, no process globals
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
    int dbg_helper_wave = -1;      // zz_local_trackp: -1 = the two-wave form where the launch leaves SIMDs idle (HELPER_WAVE_MAX_CHAINS_PER_CU), 0 = never, 1 = always
    int dbg_prio_policy = -1;      // pdmp_debug_set_prio_policy: zz_local_trackp's wave priority: -1 = by rank of progress where it applies (one-wave forms of 2048 bounds), 0 = in turns, 1 = by rank
    DevBuf<uint32_t> d_prio_board; // ... the progress board (pdmp_engine.hpp: PrioLag), allocated and zeroed by the first run that uses it
    uint32_t prio_epoch = 0;       // ... the epoch of the last launch on it: 1 .. 255, wrapping
    int dbg_track_lines = -1;      // pdmp_debug_set_track_lines: 1 = the line layout wherever it serves; -1 / 0 = never (it lost the A/B: DESIGN.md §5)

    // BPS: the flow's and the target's tables, the state, the trace, the mass factor, and what each member of the family adds
    BpsOptions bps;
    DevBuf<int64_t> b_colptr, b_rowval, bt_colptr, bt_rowval;
    DevBuf<double> b_nzval, b_mu, b_mu_flow, b_x, b_th, b_scal, b_ev_t, b_ev_x, b_ev_th, bt_nzval, bt_mu;
    DevBuf<int32_t> m_Lcp, m_Lrv, m_Ucp, m_Urv;
    DevBuf<double> m_Lnz, m_Unz;
    DevBuf<double> b_j1, b_j2;      // [nchains x d] the moments up to each chain's clock (kept by the event loop)
    DevBuf<double> b_jT, b_jT2;     // [nchains x d] the moments at the T of a read (pdmp_ensemble_bps_moments, the batch means / ESS sums)
    DevBuf<double> b_kappa, b_thf, b_tfrez;  // sticky: [d]; [nchains x d] saved speeds; [nchains x d] freezing / thaw times
    DevBuf<uint64_t> b_fmask, b_ev_f;        // sticky: [nchains x 16], [nchains x cap x 16] free masks (bit e & 63 of word e >> 6)
    DevBuf<double> b_udiag, b_sudiag, b_mstate;  // speed-recorded: [d] u, [d] sqrt(u), [nchains x 4] {Δ, action, V, Δrec}
    // speed-recorded, logistic-regression target: A and At in CSC, y, m, and the carried η = A x [nchains x n]
    DevBuf<int64_t> bl_Acp, bl_Arv, bl_Atcp, bl_Atrv;
    DevBuf<double> bl_Anz, bl_Atnz, bl_y, bl_m, bl_eta;
    int64_t bl_n = 0;
    double bl_gamma0 = 0.0;
    // the consumers of the BPS trace (pdmp_ensemble_bps_consume_*, pdmp_consume_bps.hip): the cursors x, θ, y -- and a sticky ensemble's free time --
    // [nchains x d] each, the per-(chain, strip) progress, the grid [nchains x K x d], the cummean slots [nchains x cap x d] (empty: not enabled).
    // t0 is t0_state; pdmp_debug_bps_trace_append sets trace_appended like its factorised twin
    DevBuf<double> bc_cur, bc_grid, bc_cm;
    DevBuf<unsigned char> bc_meta;
    bool bc_on = false, bc_cummean = false;
    double bc_dt = 0.0;
    int64_t bc_K = 0;
    // pdmp_ensemble_bps_consume_condition: p then n [2 x d], τ per segment slot [nchains x cap], hit times, rows and counts (pdmp::BpsCondArgs)
    DevBuf<double> bcn_pn, bcn_tau, bcn_t, bcn_x;
    DevBuf<unsigned long long> bcn_nh;
    bool bcn_on = false, bc_started = false;  // bc_started: a bps_consume happened since bps_consume_begin
    int64_t bcn_max_hits = 0;

    // pdmp_ensemble_bps_consume_pairs: the pair list, the centre [d], S [nchains x npairs], J [nchains x d], the T_last of the last read
    DevBuf<int32_t> bpr_pi, bpr_pj;
    DevBuf<double> bpr_c, bpr_S, bpr_J, bpr_T;
    bool bpr_on = false;
    bool bpr_arc = false;  // the list came by pdmp_ensemble_bps_consume_arc_pairs: a Boomerang's pieces are arcs
    int64_t bpr_np = 0;

    // pdmp_ensemble_bps_consume_hist: the listed coordinates with their ranges and widths [m], H [nchains x m x (bins + 2)], Z [nchains x m];
    // bhs_out: the pooled sums and T_last of the last read
    DevBuf<int32_t> bhs_coords;
    DevBuf<double> bhs_lo, bhs_hi, bhs_w, bhs_H, bhs_Z, bhs_out;
    bool bhs_on = false;
    bool bhs_arc = false;  // the list came by pdmp_ensemble_bps_consume_arc_hist: a Boomerang's pieces are arcs
    int64_t bhs_m = 0;
    int32_t bhs_B = 0;

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
#pragma GCC visibility push(hidden)

// The event-loop kernel families of pdmp_ensemble_run.  select_family alone decides which one serves an ensemble; what a family does with the phase
// profile (pdmp_debug_set_phase_profile) and how its launcher's failure reads is stated once, in pdmp_capi.hip's table of FamilyInfo.
enum KernelFamily { FAM_BPS, FAM_GENERAL, FAM_LOGISTIC_LDS, FAM_LOGISTIC_ROWS, FAM_TRACKL, FAM_TRACKP, FAM_TRACK_GROUPS, FAM_EXACTP,
                    FAM_STICKY_SPEC, FAM_STICKY_RUN, FAM_SPEC, FAM_ONE_EVENT, FAM_BARRIER, FAM_BRIDGE, FAM_PRECISION };
constexpr int TARGET_BRIDGE = 2;  // pdmp_ensemble::target_kind beside 0 (Gaussian CSC) and 1 (subsampled logistic)
constexpr int TARGET_PRECISION = 3;  // ... and the Cholesky factor of a precision matrix (sticky ZigZag)
struct FamilyInfo {
    int phase_kind;        // the `kind` of pdmp_debug_phase_profile its kernels record (pdmp_debug.h), 0: they have no profiling form -- no buffer, no read-back
    const char* launcher;  // "<launcher> launch failed ..."
    bool hip_rc;           // ... with the return code spelled out as a hipError_t, or as a number
};

// neighbourhoods beyond 64 members, G ⊋ G1, FactBoomerang, the logistic target, adaptscale, LocalBound: pdmp_general.hip / pdmp_logistic.hip
inline bool general_path(const pdmp_ensemble* e) { return e->needs_general || e->target_kind == 1 || e->adaptscale || e->local_bound; }

// pdmp_capi.hip
pdmp_status launch_deferred_consumer(pdmp_ensemble* e);
void discard_async_consumer(pdmp_ensemble* e);
hipError_t device_sync(pdmp_ensemble* e);
pdmp_status ensure_canon(pdmp_ensemble* e);
pdmp_status check_csc(const char* what, const int64_t* colptr, const int64_t* rowval, int64_t d, int64_t ncols, bool diag_leads = false);
pdmp_status elapsed_ms(hipEvent_t from, hipEvent_t to, float* ms);  // waits for `to`
pdmp_status check_trace_range(const pdmp_ensemble* e, int64_t chain, int64_t first, int64_t count);
pdmp_status check_chain_range(const pdmp_ensemble* e, int64_t chain_first, int64_t n);
pdmp::ZzRunParams run_params(const pdmp_ensemble* e, double T, int flags);
pdmp::ZzGeneralParams general_params(const pdmp_ensemble* e);
pdmp::ZzLogisticTables logistic_tables(const pdmp_ensemble* e);
pdmp_status select_family(const pdmp_ensemble* e, const pdmp::ZzRunParams& P, const pdmp::ZzGeneralParams& Q, const pdmp::ZzLogisticTables& LT,
                          KernelFamily* fam);
pdmp_status ensemble_run_impl(pdmp_ensemble* e, double T, int flags, void* stream);
// pdmp_capi_zigzag.hip, pdmp_capi_bps.hip
pdmp_status init_state(pdmp_ensemble* e, double t0, const double* x0, const double* th0, const double* c, const uint64_t* seeds, uint64_t seed0);
pdmp_status init_state_bps(pdmp_ensemble* e, double t0, const double* x0, const double* theta0, double c, const uint64_t* seeds);
pdmp::BpsRunParams bps_run_params(const pdmp_ensemble* e, double T, int flags);
pdmp::BpsMomParams bps_moments_params(const pdmp_ensemble* e);
pdmp::BpsStickyParams bps_sticky_params(const pdmp_ensemble* e);
pdmp::BpsModernParams bps_modern_params(const pdmp_ensemble* e);
pdmp::BpsLogitParams bps_logit_params(const pdmp_ensemble* e);
pdmp_status bps_moments_at(pdmp_ensemble* e, double T, int64_t chain_first, int64_t n, bool two);
// pdmp_capi_stats.hip
pdmp_status condition_plane(const char* who, int64_t d, const double* p, const double* n, int64_t max_hits, std::vector<int32_t>* S);
pdmp_status condition_rows_fit(const char* who, int64_t nchains, int64_t d, int64_t max_hits);
// ... what both families check of the pair list of pdmp_ensemble_[bps_]consume_pairs; the list and the centre (zeros for NULL) come back
pdmp_status pairs_list(const char* who, int64_t nchains, int64_t d, int64_t npairs, const int64_t* pi, const int64_t* pj, const double* center,
                       std::vector<int32_t>* vi, std::vector<int32_t>* vj, std::vector<double>* c);
// ... what both families check of the arguments of pdmp_ensemble_[bps_]consume_hist; the coordinates, ranges and widths come back
pdmp_status hist_list(const char* who, int64_t nchains, int64_t d, int64_t m, const int64_t* coords, const double* lo, const double* hi, int64_t bins,
                      std::vector<int32_t>* vc, std::vector<double>* vlo, std::vector<double>* vhi, std::vector<double>* vw);
// pdmp_capi_tune.hip: set_state with the placement probes
pdmp_status init_state_tuned(pdmp_ensemble* e, double t0, const double* x0, const double* th0, const double* c, const uint64_t* seeds, uint64_t seed0);
pdmp_status init_state_bps_tuned(pdmp_ensemble* e, double t0, const double* x0, const double* theta0, double c, const uint64_t* seeds);

#pragma GCC visibility pop
