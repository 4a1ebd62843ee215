// pdmp_capi_debug.hip -- the entry points of include/pdmp_debug.h: probes, kernel selectors, test hooks.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "pdmp_ensemble.hpp"

// the mean time of one launch on the null stream: a warm-up (page faults, TLB), then `iters` timed ones
template <class Launch>
static pdmp_status time_launches(const char* name, int iters, double* ms_out, Launch launch) {
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    (void)launch();
    HIP_TRY(hipEventRecord(e0, nullptr));
    for (int k = 0; k < iters; ++k) LAUNCH_TRY_CODE(name, launch());
    HIP_TRY(hipEventRecord(e1, nullptr));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = (double)ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return PDMP_OK;
}

// the three argument vectors of a math probe side by side in `in` [3 x n]
static pdmp_status upload_abc(DevBuf<double>& in, int64_t n, const double* a, const double* b, const double* c) {
    PDMP_TRY(in.alloc((size_t)(3 * n)));
    HIP_TRY(hipMemcpy(in.p, a, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in.p + n, b, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in.p + 2 * n, c, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    return PDMP_OK;
}

extern "C" {

pdmp_status pdmp_debug_write_probe(int device, int64_t nchains, int64_t d, int64_t nrec, int iters, double* ms_out) {
    if (!ms_out || nchains <= 0 || d <= 0 || nrec <= 0 || iters <= 0) return fail(PDMP_ERR_INVALID, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible: libpdmp_mi355 has no CPU fallback");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> bx, bt;
    PDMP_TRY(bx.alloc((size_t)(nchains * nrec * d)));
    PDMP_TRY(bt.alloc((size_t)(nchains * nrec * d)));
    return time_launches("write probe", iters, ms_out, [&]() { return pdmp::launch_bps_write_probe(bx.p, bt.p, d, nrec, nrec, nchains, nullptr); });
}

pdmp_status pdmp_debug_sector_probe(int device, int64_t nchains, int64_t d, int rounds, int write, int iters, double* ms_out) {
    if (!ms_out || nchains <= 0 || d <= 0 || rounds <= 0 || iters <= 0) return fail(PDMP_ERR_INVALID, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible: libpdmp_mi355 has no CPU fallback");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> rec, sink;
    PDMP_TRY(rec.alloc((size_t)(nchains * d * 8)));
    PDMP_TRY(sink.alloc(8));
    HIP_TRY(hipMemset(rec.p, 0, (size_t)(nchains * d * 8) * sizeof(double)));
    return time_launches("sector probe", iters, ms_out, [&]() { return pdmp::launch_sector_probe(rec.p, d, nchains, rounds, write, sink.p, nullptr); });
}

pdmp_status pdmp_debug_math_probe(int device, uint64_t seed, int64_t n, double* out) {
    if (!out || n <= 0) return fail(PDMP_ERR_INVALID, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> buf;
    PDMP_TRY(buf.alloc((size_t)(8 * n)));
    LAUNCH_TRY("math probe", pdmp::launch_math_probe(seed, n, buf.p, nullptr));
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
    PDMP_TRY(upload_abc(in, n, a, b, c));
    PDMP_TRY(res.alloc((size_t)(2 * n)));
    int rc = launch(fn, n, in.p, in.p + n, in.p + 2 * n, res.p, nullptr);
    LAUNCH_TRY("math eval", rc);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, res.p, (size_t)(2 * n) * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
#endif
}

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
pdmp_status pdmp_debug_set_prio_policy(pdmp_ensemble* e, int mode) {
    if (!e || mode < -1 || mode > 1) return fail(PDMP_ERR_INVALID, "priority policy: -1 (default: by rank of progress where it applies), 0 (in turns), 1 (by rank of progress)");
    e->dbg_prio_policy = mode;
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

// Test hook (include/pdmp_debug.h): the BPS twin of pdmp_debug_trace_append.  n given events (t [n], x and θ [n x d], f [n x d] bytes for a sticky
// ensemble) behind what `chain`'s segment holds, counted in its header as a run would have counted them; no kernel is launched and no state changes,
// so the ensemble cannot run afterwards.
pdmp_status pdmp_debug_bps_trace_append(pdmp_ensemble* e, int64_t chain, const double* t, const double* x, const double* theta, const uint8_t* f, int64_t n) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BPS) return fail(PDMP_ERR_INVALID, "bps_trace_append: the ensemble was not created with PDMP_SAMPLER_BPS (pdmp_debug_trace_append)");
    if (!e->bc_on || !e->has_state) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_bps_consume_begin first");
    if (chain < 0 || chain >= e->cfg.nchains || n < 0) return fail(PDMP_ERR_INVALID, "bad argument");
    if (n > 0 && (!t || !x || !theta)) return fail(PDMP_ERR_INVALID, "null argument");
    if (f && !e->bps.sticky) return fail(PDMP_ERR_INVALID, "bps_trace_append: free masks given to an ensemble that is not sticky");
    if (!f && e->bps.sticky && n > 0) return fail(PDMP_ERR_INVALID, "bps_trace_append: a sticky ensemble's events carry free masks");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    pdmp::DevChain h;
    HIP_TRY(hipMemcpy(&h, e->d_hdr.p + chain, sizeof h, hipMemcpyDeviceToHost));
    const int64_t cap = e->cfg.trace_capacity, d = e->cfg.d, W = pdmp::BPS_STICKY_WORDS;
    if (h.c.ntrace > (uint64_t)cap || n > cap - (int64_t)h.c.ntrace)
        return fail(PDMP_ERR_INVALID, "bps_trace_append: %lld events behind %llu do not fit trace_capacity = %lld", (long long)n, (unsigned long long)h.c.ntrace, (long long)cap);
    const int64_t slot = chain * cap + (int64_t)h.c.ntrace;
    if (n > 0) {
        HIP_TRY(hipMemcpy(e->b_ev_t.p + slot, t, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->b_ev_x.p + slot * d, x, (size_t)(n * d) * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->b_ev_th.p + slot * d, theta, (size_t)(n * d) * sizeof(double), hipMemcpyHostToDevice));
        if (f) {
            std::vector<uint64_t> w((size_t)(n * W), 0ull);  // bit i & 63 of word i >> 6
            for (int64_t k = 0; k < n; ++k)
                for (int64_t i = 0; i < d; ++i)
                    if (f[k * d + i]) w[(size_t)(k * W + (i >> 6))] |= 1ull << (i & 63);
            HIP_TRY(hipMemcpy(e->b_ev_f.p + slot * W, w.data(), w.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        }
    }
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

pdmp_status pdmp_debug_sticky_eval(int device, int fn, int64_t n, const double* a, const double* b, const double* c, double* out) {
    if (!a || !b || !c || !out || n <= 0 || n > ((int64_t)1 << 30)) return fail(PDMP_ERR_INVALID, "bad argument");
    if (fn < 0 || fn > 2) return fail(PDMP_ERR_INVALID, "pdmp_debug_sticky_eval: fn 0 (atan), 1 (linear freezing time) or 2 (Boomerang freezing time)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> in, res;
    PDMP_TRY(upload_abc(in, n, a, b, c));
    PDMP_TRY(res.alloc((size_t)n));
    LAUNCH_TRY("sticky eval", pdmp::launch_bps_sticky_eval(fn, n, in.p, in.p + n, in.p + 2 * n, res.p, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, res.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

pdmp_status pdmp_debug_barrier_eval(int device, int fn, int64_t n, const double* a, const double* b, const double* c, double* out) {
#ifndef PDMP_EXTRA_KERNELS
    (void)device, (void)fn, (void)n, (void)a, (void)b, (void)c, (void)out;
    return fail(PDMP_ERR_UNSUPPORTED, "pdmp_debug_barrier_eval: the probe kernel lives in the parity build (build.py --variant parity, -DPDMP_EXTRA_KERNELS)");
#else
    if (!a || !b || !c || !out || n <= 0 || n > ((int64_t)1 << 30)) return fail(PDMP_ERR_INVALID, "bad argument");
    if (fn < PDMP_BARRIER_FN_PT3_L || fn > PDMP_BARRIER_FN_RATES) return fail(PDMP_ERR_INVALID, "pdmp_debug_barrier_eval: unknown function id %d", fn);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> in, res;
    PDMP_TRY(upload_abc(in, n, a, b, c));
    PDMP_TRY(res.alloc((size_t)n * 2));
    LAUNCH_TRY("barrier eval", pdmp::launch_barrier_eval(fn, n, in.p, in.p + n, in.p + 2 * n, res.p, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, res.p, (size_t)n * 2 * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
#endif
}

pdmp_status pdmp_debug_wave_eval(int device, int fn, int64_t nrows, const uint64_t* in0, const uint64_t* in1, uint64_t* out) {
#ifndef PDMP_EXTRA_KERNELS
    (void)device, (void)fn, (void)nrows, (void)in0, (void)in1, (void)out;
    return fail(PDMP_ERR_UNSUPPORTED, "pdmp_debug_wave_eval: the probe kernels live in the parity build (build.py --variant parity, -DPDMP_EXTRA_KERNELS)");
#else
    if (!in0 || !in1 || !out || nrows <= 0 || nrows > ((int64_t)1 << 20)) return fail(PDMP_ERR_INVALID, "bad argument");
    decltype(&pdmp::launch_wave_eval_kernels) launch = nullptr;
    switch (fn) {
    case PDMP_WAVE_MIN_F64: case PDMP_WAVE_GRP8_MIN_F64: case PDMP_WAVE_ROW_MIN_F64: case PDMP_WAVE_MIN_U32: case PDMP_WAVE_MIN_U32_DPP:
    case PDMP_WAVE_SCAN_ADD_U32: case PDMP_WAVE_SCAN_MIN_F64: case PDMP_WAVE_BPERM_F64: launch = pdmp::launch_wave_eval_kernels; break;
    case PDMP_WAVE_SUM_F64: launch = pdmp::launch_wave_eval_bps; break;
    case PDMP_WAVE_GRP8_MIN_U32: launch = pdmp::launch_wave_eval_trackp; break;
    default: return fail(PDMP_ERR_INVALID, "pdmp_debug_wave_eval: unknown function id %d", fn);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    const size_t nw = (size_t)nrows * 64;
    DevBuf<uint64_t> buf;  // in0, in1, out side by side
    PDMP_TRY(buf.alloc(3 * nw));
    HIP_TRY(hipMemcpy(buf.p, in0, nw * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(buf.p + nw, in1, nw * sizeof(uint64_t), hipMemcpyHostToDevice));
    LAUNCH_TRY("wave eval", launch(fn, nrows, buf.p, buf.p + nw, buf.p + 2 * nw, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, buf.p + 2 * nw, nw * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PDMP_OK;
#endif
}

pdmp_status pdmp_debug_queue_eval(int device, int fn, int64_t n, const double* a, const double* b, const double* c, double* out) {
#ifndef PDMP_EXTRA_KERNELS
    (void)device, (void)fn, (void)n, (void)a, (void)b, (void)c, (void)out;
    return fail(PDMP_ERR_UNSUPPORTED, "pdmp_debug_queue_eval: the probe kernels live in the parity build (build.py --variant parity, -DPDMP_EXTRA_KERNELS)");
#else
    if (!a || !b || !c || !out || n <= 0 || n > ((int64_t)1 << 30)) return fail(PDMP_ERR_INVALID, "bad argument");
    decltype(&pdmp::launch_queue_eval_kernels) launch = nullptr;
    switch (fn) {
    case PDMP_QUEUE_P_ENC: case PDMP_QUEUE_P_THR: case PDMP_QUEUE_P_DEC: case PDMP_QUEUE_NB_HAS: case PDMP_QUEUE_NB_COUNT: case PDMP_SELECT_P_MASK32:
        launch = pdmp::launch_queue_eval_trackp; break;
    case PDMP_QUEUE_Q_ENC: case PDMP_QUEUE_Q_THR: case PDMP_QUEUE_Q_DEC: launch = pdmp::launch_queue_eval_exactp; break;
    case PDMP_QUEUE_TL_Q: case PDMP_QUEUE_HB: launch = pdmp::launch_queue_eval_trackl; break;
    case PDMP_QUEUE_BELOW: launch = pdmp::launch_queue_eval_kernels; break;
    default: return fail(PDMP_ERR_INVALID, "pdmp_debug_queue_eval: unknown function id %d", fn);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> in, res;
    PDMP_TRY(upload_abc(in, n, a, b, c));
    PDMP_TRY(res.alloc((size_t)(2 * n)));
    LAUNCH_TRY("queue eval", launch(fn, n, in.p, in.p + n, in.p + 2 * n, res.p, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, res.p, (size_t)(2 * n) * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
#endif
}

pdmp_status pdmp_debug_state_eval(int device, int fn, int64_t nkeys, const double* keys, int64_t d, int has_refresh, int64_t nchg, const uint32_t* idx,
                                  const double* val, double* out) {
#ifndef PDMP_EXTRA_KERNELS
    (void)device, (void)fn, (void)nkeys, (void)keys, (void)d, (void)has_refresh, (void)nchg, (void)idx, (void)val, (void)out;
    return fail(PDMP_ERR_UNSUPPORTED, "pdmp_debug_state_eval: the probe kernels live in the parity build (build.py --variant parity, -DPDMP_EXTRA_KERNELS)");
#else
    if (!out || nchg < 0 || nchg > ((int64_t)1 << 20) || (nchg > 0 && (!idx || !val))) return fail(PDMP_ERR_INVALID, "bad argument");
    if (fn != PDMP_STATE_WHEEL && fn != PDMP_STATE_LEVEL1 && fn != PDMP_STATE_S8_LEVEL1) return fail(PDMP_ERR_INVALID, "pdmp_debug_state_eval: unknown function id %d", fn);
    const int64_t block = (fn == PDMP_STATE_LEVEL1) ? 64 : 32;
    int64_t nout = 8192, limit = 8192;  // (the wheel: LL::NB2 blocks)
    if (fn != PDMP_STATE_WHEEL) {
        if (!keys || nkeys <= 0 || nkeys % block != 0 || nkeys / block > 512) return fail(PDMP_ERR_INVALID, "state eval: whole key blocks, at most 512 of them");
        if (fn == PDMP_STATE_S8_LEVEL1 && has_refresh && (d < 0 || d >= nkeys)) return fail(PDMP_ERR_INVALID, "state eval: the refresh slot d lies inside the keys");
        nout = 4 * ((fn == PDMP_STATE_LEVEL1) ? nkeys / 64 : 512) + 2 * nchg;
        limit = nkeys;
    }
    for (int64_t k = 0; k < nchg; ++k) {  // every index stays inside its array; a wheel image has nine bits
        if ((int64_t)idx[k] >= limit) return fail(PDMP_ERR_INVALID, "state eval: change %lld has index %u, the array has %lld entries", (long long)k, idx[k], (long long)limit);
        if (fn == PDMP_STATE_WHEEL && !(val[k] >= 0.0 && val[k] < 512.0)) return fail(PDMP_ERR_INVALID, "state eval: a wheel image is 0 .. 511");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PDMP_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> dk, dv, res;
    DevBuf<uint32_t> di;
    PDMP_TRY(res.alloc((size_t)nout));
    PDMP_TRY(dv.alloc((size_t)nchg + 1));
    PDMP_TRY(di.alloc((size_t)nchg + 1));
    if (nchg > 0) {
        HIP_TRY(hipMemcpy(dv.p, val, (size_t)nchg * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(di.p, idx, (size_t)nchg * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (fn == PDMP_STATE_WHEEL) {
        LAUNCH_TRY("wheel probe", pdmp::launch_wheel_probe(nchg, di.p, dv.p, res.p, nullptr));
    } else {
        PDMP_TRY(dk.alloc((size_t)nkeys));
        HIP_TRY(hipMemcpy(dk.p, keys, (size_t)nkeys * sizeof(double), hipMemcpyHostToDevice));
        LAUNCH_TRY("level-1 probe", pdmp::launch_level1_probe((int)block, dk.p, nkeys, d, has_refresh, nchg, di.p, dv.p, res.p, nullptr));
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, res.p, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
#endif
}
}  // extern "C"
