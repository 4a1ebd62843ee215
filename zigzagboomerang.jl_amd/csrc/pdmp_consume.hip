// pdmp_consume.hip -- what callers do next with the chains, on the device: path integrals at probe coordinates (ESS estimators on the
// host see N x B x 32 numbers instead of N x d records) and, below, the streaming trace consumers (discretize / mean of src/trace.jl).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pdmp_bps_common.hpp"
#include "pdmp_engine.hpp"

namespace pdmp {

// J_i(T) = ∫_{t0}^{T} x_i(s) ds of every chain at `nprobe` coordinates (the integrand of mean(trace), src/trace.jl:182-200): the record
// carries the integral up to the coordinate's own clock and the linear piece from there (first sector of ZzRec and TrRec alike).
__global__ __launch_bounds__(256) void zz_path_integrals_kernel(const ZzRec* rec0, int64_t rec_stride, int64_t d, int64_t nchains,
                                                                const int64_t* __restrict__ probes, int64_t nprobe, double T,
                                                                double* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nchains * nprobe) return;
    const int64_t ch = k / nprobe, p = k - ch * nprobe;
    const int64_t i = probes[p];
    const ZzRec* r = reinterpret_cast<const ZzRec*>(reinterpret_cast<const char*>(rec0) + (ch * d + i) * rec_stride);
    const double dt = T - r->t;
    out[k] = r->I + dt * (r->x + r->th * (dt * 0.5));
}

int launch_zz_path_integrals(const ZzRec* rec, int64_t rec_stride, int64_t d, int64_t nchains, const int64_t* probes, int64_t nprobe,
                             double T, double* out, void* stream) {
    const int64_t n = nchains * nprobe;
    hipLaunchKernelGGL(zz_path_integrals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rec, rec_stride, d,
                       nchains, probes, nprobe, T, out);
    return (int)hipGetLastError();
}


// ------------------------------------------------------------------------------------------ streaming trace consumers
//
// mean(Ξ) (src/trace.jl:182-200) and collect(discretize(Ξ, dt)) (:94-125) of FactTrace traces, computed ON THE DEVICE from the engine's
// trace buffer, slice by slice: a C3-sized trace set (8 MB per chain x 4096) never crosses PCIe and need not even exist at once -- the
// buffer is recycled after every slice, the consumer keeps a CURSOR per (chain, coordinate): the time, position and velocity after the
// coordinate's last consumed event, and the running Σ (x_prev + x_k)(t_k − t_prev) of the reference's trapezoid rule (:191-195).
// A coordinate's path depends on its own events only, so the events of a slice are applied 256 at a time by a workgroup per chain; two
// events of one coordinate inside a chunk (rare) keep their order: an event waits for the latest earlier event of its coordinate.
// Grid positions are the closed form x_c + θ_c (g − t_c) from the cursor, g = t0 + k dt -- the arithmetic of trace.py (bitwise equal to
// it; the reference itself steps all coordinates through every event and agrees to rounding).  A grid ROW is written by the chain's
// workgroup for all d coordinates at once (coalesced: cursors read and positions written thread by thread), after the events with t <= g and
// as soon as a later event shows that the run has passed g (:111: a point is emitted while it lies before the last event) -- round 5; before,
// every event scattered the points of its own coordinate, 2.5 eight-byte stores per event at C3's rates, which cost more than the events.
// That walk takes SORTED traces (ZigZag without refresh clock; the sticky sampler's traces included).  A refresh clock records the refreshed
// coordinate at its own, stale clock (src/sfact.jl:84-85), so the traces of a ZigZag with λref > 0 and of a FactBoomerang are sorted within a
// coordinate only: the UNORDERED form of the walk (UNORD below) takes them in trace order, as the reference's iterator does.
struct ConsumeCursor {
    double t, x, th, y;  // clock, position, velocity after the coordinate's last consumed event; Σ (x_prev + x_k)(t_k − t_prev)
};
static_assert(sizeof(ConsumeCursor) == 32, "a cursor never straddles a 128-byte line");
// (sticky ensembles keep one more sum per cursor, in an array of its own behind the cursors: z = Σ (x_prev ≠ 0 | x_k ≠ 0)(t_k − t_prev), the time the
// coordinate was not stuck at 0 -- inclusion_prob, src/trace.jl:161-178; without freezes that is the time to the coordinate's last event)
struct ConsumeMeta {
    uint64_t consumed;  // events of this chain consumed so far (global event index)
    double t_last;      // time of the last of them (t0 before the first)
    uint64_t row_next;  // the first grid row not written yet by the streaming consumer
    double t_max;       // the running maximum of their times (t0 before the first): bounds the grid of an unordered trace; the sorted walk carries it along unread
};
// (barrier ensembles keep the OCCUPATION of every coordinate instead, in an array of its own behind the cursors: the time it sat frozen on its lower
// and on its upper barrier, how often it hit each, and the side it is -- or was last -- frozen on; DESIGN.md "Barrier occupation" has the definition)
struct BarrierOcc {
    double z[2];    // time frozen at the lower / upper barrier, over the consumed events
    uint64_t n[2];  // hits of the lower / upper barrier
    uint64_t side;  // 0 lower, 1 upper: where a frozen coordinate sits (from v_old at t0, then from the speed before each hit)
};
static_assert(sizeof(BarrierOcc) == 40, "z, n and the side of one coordinate");

__global__ __launch_bounds__(256) void consume_init_kernel(const ZzRec* rec0, int64_t rec_stride, int64_t d, int64_t nchains, double t0,
                                                           ConsumeCursor* cur, double* zs, ConsumeMeta* meta, double* grid, int64_t K) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < nchains) {
        ConsumeMeta m;
        m.consumed = 0;
        m.t_last = t0;
        m.row_next = 0;
        m.t_max = t0;
        meta[k] = m;
    }
    if (k >= nchains * d) return;
    const ZzRec* r = reinterpret_cast<const ZzRec*>(reinterpret_cast<const char*>(rec0) + k * rec_stride);
    ConsumeCursor c;
    c.t = t0;
    c.x = r->x;  // (before any run: the records hold x0, θ0 at t0)
    c.th = r->th;
    c.y = 0.0;
    cur[k] = c;
    if (zs) zs[k] = 0.0;
    // the first element of collect(discretize(Ξ, dt)) is t0 => x0 whatever follows (src/trace.jl:106-110): also for a chain without an event
    if (grid && K > 0) grid[(k / d) * K * d + (k % d)] = r->x;
}

// grid point k of coordinate i: the closed form from the cursor (events with t <= g applied: src/trace.jl:111-121)
__device__ __forceinline__ void consume_emit(double* grid_chain, int64_t d, int64_t K, double t0, double dt, uint32_t i, const ConsumeCursor& c,
                                             double t_until, bool closed_end) {
    if (!grid_chain || K <= 0) return;
    // candidates: the grid times inside [c.t, t_until) (or [c.t, t_until] at the very end of the run)
    double kf = floor((c.t - t0) / dt) - 1.0;
    int64_t k = (kf > 0.0) ? (int64_t)kf : 0;
    while (k < K && t0 + dt * (double)k < c.t) ++k;
    for (; k < K; ++k) {
        const double g = t0 + dt * (double)k;
        if (closed_end ? !(g <= t_until) : !(g < t_until)) break;
        grid_chain[k * d + i] = c.x + c.th * (g - c.t);
    }
}

// (snap: the (ntrace, nevents) pairs a finished launch left, taken by consume_snapshot_kernel -- the asynchronous consumer reads a buffer the
// event loop no longer writes while the headers already count the next slice; nullptr: the headers themselves)
constexpr int CONSUME_HASH = 4096;  // slots of the per-chunk table that finds two events of one coordinate
// (OCC: the barrier ensembles' form -- zs0 is their BarrierOcc array, updated beside the cursor; every other ensemble runs OCC = false)
// UNORD: 0 the sorted walk; 1 / 2 the walk of a trace that is sorted within a coordinate only, with the rows of the linear flow / of the
// FactBoomerang's rotation about mu (pdmp_ensemble_refresh_consume_begin).  It differs from the sorted walk in four places, each marked UNORD:
//   split   the first slot of [pos, ntrace) whose time exceeds g is found by a forward scan, 256 slots per step, the lowest hit taken (LDS minimum;
//           the step ends on the count barrier, so every thread leaves the scan at the same step).  The scan starts at pos and pos only advances:
//           O(events + rows) per slice.  Events behind the split are not applied to row g even where their time is <= g -- the reference's iterator
//           stops at the first later event (src/trace.jl:111-113).
//   clocks  t_last is the time of the last consumed event in trace order (T of mean); t_max the running maximum (the grid's extent, npoints)
//   rows    the FactBoomerang rotates: (x − μ)·c + θ·s + μ, (s, c) = pdmp_sincos(g − t_cursor), plain doubles
//   flush   none: consume_flush_kernel would re-emit rows from the current cursors, which after a stale event are not the state the reference shows
//           there; every row with g < t_max has been written by the walk when the event that exceeds it is consumed
template <bool OCC, int UNORD = 0>
__global__ __launch_bounds__(256) void consume_events_kernel(const pdmp_event* ev0, int64_t cap, const DevChain* hdr, const uint64_t* __restrict__ snap,
                                                             int64_t d, ConsumeCursor* cur0, double* zs0, ConsumeMeta* meta, double* grid0, int64_t K,
                                                             double t0, double dt, double2* cm0) {
    const int64_t chain = blockIdx.x;
    const int tid = threadIdx.x;
    __shared__ uint32_t s_i[256];
    __shared__ int s_done[256];
    __shared__ uint8_t s_own[CONSUME_HASH];
    __shared__ uint64_t s_split;
    const uint64_t ntrace = snap ? snap[2 * chain] : hdr[chain].c.ntrace, nevents = snap ? snap[2 * chain + 1] : hdr[chain].c.nevents;
    ConsumeMeta m = meta[chain];
    const uint64_t first_global = nevents - ntrace;  // global index of buffer slot 0
    uint64_t pos = (m.consumed > first_global) ? (m.consumed - first_global) : 0;  // first unconsumed slot
    if (pos >= ntrace) return;
    const pdmp_event* ev = ev0 + chain * cap;
    ConsumeCursor* cur = cur0 + chain * d;
    double* zs = (!OCC && UNORD == 0 && zs0) ? zs0 + chain * d : nullptr;
    const double* const mu = zs0;  // (UNORD = 2: the slot of the z sums carries the flow's μ [d], read only -- an unordered walk keeps no z sums, and the
                                   // sorted instantiations keep their signature and with it every instruction)
    BarrierOcc* occ = OCC ? reinterpret_cast<BarrierOcc*>(zs0) + chain * d : nullptr;
    double* grid = grid0 ? grid0 + chain * K * d : nullptr;
    uint64_t row = m.row_next;
    double tmx = m.t_max;  // (UNORD: this thread's share of the running maximum, reduced once behind the walk)
    for (;;) {
        // the events up to the next grid time g (t <= g: an event AT g belongs before the row), then the row -- if the slice goes on beyond g
        const bool want_row = grid && (int64_t)row < K;
        const double g = t0 + dt * (double)row;
        uint64_t split = ntrace;
        if (UNORD != 0 && want_row) {  // first slot in [pos, ntrace) whose time exceeds g, by a forward scan from pos
            if (tid == 0) s_split = ntrace;
            __syncthreads();
            for (uint64_t sb = pos;; sb += 256) {
                const uint64_t e = sb + (uint64_t)tid;
                const bool hit = e < ntrace && ev[e].t > g;
                if (hit) atomicMin(reinterpret_cast<unsigned long long*>(&s_split), (unsigned long long)e);
                if (__syncthreads_count(hit ? 1 : 0) != 0 || sb + 256 >= ntrace) break;  // (the same count in every thread)
            }
            split = s_split;
        } else if (want_row) {
            if (tid == 0) {  // first slot in [pos, ntrace) whose time exceeds g (the trace is sorted by time)
                uint64_t lo = pos, hi = ntrace;
                while (lo < hi) {
                    const uint64_t mid = lo + ((hi - lo) >> 1);
                    if (ev[mid].t <= g) lo = mid + 1;
                    else hi = mid;
                }
                s_split = lo;
            }
            __syncthreads();
            split = s_split;
        }
        for (uint64_t base = pos; base < split; base += 256) {
            const uint64_t e = base + (uint64_t)tid;
            const bool valid = e < split;
            pdmp_event evt;
            evt.t = 0.0;
            evt.i = 0;
            evt.x = evt.theta = 0.0;
            if (valid) evt = ev[e];
            if constexpr (UNORD != 0) {
                if (valid && evt.t > tmx) tmx = evt.t;
            }
            // two events of one coordinate in this chunk?  every event writes its thread into a slot of a hash table; an event that does not find
            // itself there after everybody wrote shares the slot with another one (the same coordinate, or -- ~8 times per chunk -- another that
            // hashes alike): those few sort themselves out by the ordered rounds below, everybody else is alone on its coordinate
            const uint32_t hs = ((uint32_t)evt.i * 0x9E3779B1u) >> 20;  // (12 bits)
            s_i[tid] = valid ? (uint32_t)evt.i : 0xffffffffu;
            s_done[tid] = valid ? 0 : 1;
            if (valid) s_own[hs] = (uint8_t)tid;
            __syncthreads();
            const bool clash = valid && s_own[hs] != (uint8_t)tid;
            __syncthreads();
            if (clash) s_own[hs] = 0xff;  // (marks the slot for the event that owned it: it is part of the clash too)
            __syncthreads();
            const bool contested = valid && (clash || s_own[hs] == 0xff);
            int dep = -1;  // the latest earlier event of the same coordinate inside this chunk
            if (contested)
                for (int q = tid - 1; q >= 0; --q)
                    if (s_i[q] == (uint32_t)evt.i) {
                        dep = q;
                        break;
                    }
            bool mine_done = !valid;
            for (int round = 0; round < 256; ++round) {
                const bool ready = !mine_done && (dep < 0 || s_done[dep] != 0);
                __syncthreads();  // (everybody has read the flags of this round)
                if (ready) {
                    const uint32_t i = (uint32_t)evt.i;
                    ConsumeCursor c = cur[i];
                    c.y += (c.x + evt.x) * (evt.t - c.t);  // src/trace.jl:193 without the common factor 1/(2T)
                    if constexpr (OCC) {  // (the same ordered rounds: two events of one coordinate -- a wall's hit and thaw at one time -- keep their order)
                        BarrierOcc o = occ[i];
                        if (c.th == 0.0) o.z[o.side & 1u] += evt.t - c.t;  // frozen since its last event (−0.0 counts as 0)
                        if (evt.theta == 0.0 && c.th != 0.0) {             // a hit: the barrier in the direction it travelled
                            o.side = c.th > 0.0 ? 1u : 0u;
                            o.n[o.side] += 1;
                        }
                        occ[i] = o;
                    }
                    if (zs && (c.x != 0.0 || evt.x != 0.0)) zs[i] += evt.t - c.t;  // :172 without the common factor 1/T (−0.0 of a freeze counts as 0)
                    c.t = evt.t;
                    c.x = evt.x;
                    c.th = evt.theta;
                    cur[i] = c;
                    // cummean(Ξ), src/trace.jl:203-226: after each event of coordinate i the pair (t[i], y[i] / (2 t[i])) -- the same sum, the same
                    // order of operations per coordinate; written beside the event's slot (round 6)
                    if (cm0) cm0[chain * cap + (int64_t)e] = make_double2(c.t, c.y / (2.0 * c.t));
                    __threadfence_block();
                    s_done[tid] = 1;
                    mine_done = true;
                }
                const int left = __syncthreads_count(mine_done ? 0 : 1);
                if (left == 0) break;
            }
            __syncthreads();
        }
        pos = split;
        if (!want_row || split >= ntrace) break;  // (no later event in this slice: whether the run passes g is not known yet)
        __threadfence_block();
        __syncthreads();
        double* const grow = grid + row * d;
        for (int64_t i = tid; i < d; i += 256) {
            const ConsumeCursor c = cur[i];
            if constexpr (UNORD == 2) {
                double sn, cs;
                pdmp_sincos(g - c.t, &sn, &cs);
                const double m_i = mu[i];
                grow[i] = (c.x - m_i) * cs + c.th * sn + m_i;
            } else {
                grow[i] = c.x + c.th * (g - c.t);
            }
        }
        row += 1;
    }
    if constexpr (UNORD != 0) {  // the maximum over the threads' shares: across each wavefront, then over the four
        __shared__ double s_mx[4];
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_xor(tmx, off, 64);
            if (o > tmx) tmx = o;
        }
        if ((tid & 63) == 0) s_mx[tid >> 6] = tmx;
        __syncthreads();
        if (tid == 0)
            for (int w = 0; w < 4; ++w)
                if (s_mx[w] > m.t_max) m.t_max = s_mx[w];
    }
    if (tid == 0) {
        m.consumed = nevents;
        m.t_last = ev[ntrace - 1].t;
        m.row_next = row;
        meta[chain] = m;
    }
}

// the grid points after a coordinate's last event, up to the chain's last event time (a point is emitted while it lies before it, :111)
__global__ __launch_bounds__(256) void consume_flush_kernel(int64_t d, const ConsumeCursor* cur0, const ConsumeMeta* meta, double* grid0, int64_t K,
                                                            double t0, double dt) {
    const int64_t chain = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= d || !grid0) return;
    consume_emit(grid0 + chain * K * d, d, K, t0, dt, (uint32_t)i, cur0[chain * d + i], meta[chain].t_last, false);
}

__global__ __launch_bounds__(256) void consume_mean_kernel(int64_t d, int64_t chain_first, int64_t n, const ConsumeCursor* cur0, const ConsumeMeta* meta,
                                                           double* mean_out, double* T_out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n * d) return;
    const int64_t q = k / d, i = k - q * d;
    const int64_t chain = chain_first + q;
    const double T = meta[chain].t_last;
    mean_out[k] = cur0[chain * d + i].y * (1 / (2 * T));  // y[i] summed over i's events, scaled once (src/trace.jl:190 scales every term)
    if (i == 0 && T_out) T_out[q] = T;
}

__global__ __launch_bounds__(256) void consume_inclusion_kernel(int64_t d, int64_t chain_first, int64_t n, const ConsumeCursor* cur0, const double* zs0,
                                                                const ConsumeMeta* meta, double t0, double* out, double* T_out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n * d) return;
    const int64_t q = k / d, i = k - q * d;
    const int64_t chain = chain_first + q;
    const double T = meta[chain].t_last;
    // (src/trace.jl:172 divides every term; without freezes every term counts: the sum telescopes to the time of the coordinate's last event)
    out[k] = (zs0 ? zs0[chain * d + i] : cur0[chain * d + i].t - t0) / T;
    if (i == 0 && T_out) T_out[q] = T;
}

// the cursors, and behind them the z sums of a sticky ensemble
size_t consume_cursor_bytes(bool with_z) { return sizeof(ConsumeCursor) + (with_z ? sizeof(double) : 0); }
size_t consume_meta_bytes() { return sizeof(ConsumeMeta); }
size_t consume_occ_bytes() { return sizeof(BarrierOcc); }
static BarrierOcc* occ_of(void* cur, int64_t d, int64_t nchains) { return reinterpret_cast<BarrierOcc*>(static_cast<ConsumeCursor*>(cur) + nchains * d); }
static double* z_of(void* cur, int64_t d, int64_t nchains, bool with_z) {
    return with_z ? reinterpret_cast<double*>(static_cast<ConsumeCursor*>(cur) + nchains * d) : nullptr;
}

int launch_consume_inclusion(int64_t d, int64_t nchains, bool with_z, double t0, int64_t chain_first, int64_t n, void* cur, const void* meta, double* out,
                             double* T_out, void* stream) {
    const int64_t tot = n * d;
    hipLaunchKernelGGL(consume_inclusion_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d, chain_first, n,
                       static_cast<const ConsumeCursor*>(cur), z_of(cur, d, nchains, with_z), static_cast<const ConsumeMeta*>(meta), t0, out, T_out);
    return (int)hipGetLastError();
}

int launch_consume_init(const ZzRec* rec, int64_t rec_stride, int64_t d, int64_t nchains, double t0, void* cur, bool with_z, void* meta, double* grid,
                        int64_t K, void* stream) {
    const int64_t n = nchains * d;
    hipLaunchKernelGGL(consume_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rec, rec_stride, d, nchains, t0,
                       static_cast<ConsumeCursor*>(cur), z_of(cur, d, nchains, with_z), static_cast<ConsumeMeta*>(meta), grid, K);
    return (int)hipGetLastError();
}
int launch_consume_events(const pdmp_event* ev, int64_t cap, const DevChain* hdr, const uint64_t* snap, int64_t d, int64_t nchains, void* cur,
                          bool with_z, void* meta, double* grid, int64_t K, double t0, double dt, void* stream, double* cummean_pairs, bool with_occ) {
    if (with_occ)
        hipLaunchKernelGGL(consume_events_kernel<true>, dim3((unsigned)nchains), dim3(256), 0, (hipStream_t)stream, ev, cap, hdr, snap, d,
                           static_cast<ConsumeCursor*>(cur), reinterpret_cast<double*>(occ_of(cur, d, nchains)), static_cast<ConsumeMeta*>(meta), grid, K,
                           t0, dt, reinterpret_cast<double2*>(cummean_pairs));
    else
        hipLaunchKernelGGL(consume_events_kernel<false>, dim3((unsigned)nchains), dim3(256), 0, (hipStream_t)stream, ev, cap, hdr, snap, d,
                           static_cast<ConsumeCursor*>(cur), z_of(cur, d, nchains, with_z), static_cast<ConsumeMeta*>(meta), grid, K, t0, dt,
                           reinterpret_cast<double2*>(cummean_pairs));
    return (int)hipGetLastError();
}
// the unordered walk (a ZigZag with refresh clock: mu = nullptr; a FactBoomerang: its per-coordinate μ); synchronous, no z sums, no occupation
int launch_consume_events_unordered(const pdmp_event* ev, int64_t cap, const DevChain* hdr, int64_t d, int64_t nchains, void* cur, void* meta, double* grid,
                                    int64_t K, double t0, double dt, void* stream, double* cummean_pairs, const double* mu) {
    if (mu)
        hipLaunchKernelGGL((consume_events_kernel<false, 2>), dim3((unsigned)nchains), dim3(256), 0, (hipStream_t)stream, ev, cap, hdr, nullptr, d,
                           static_cast<ConsumeCursor*>(cur), const_cast<double*>(mu), static_cast<ConsumeMeta*>(meta), grid, K, t0, dt,
                           reinterpret_cast<double2*>(cummean_pairs));
    else
        hipLaunchKernelGGL((consume_events_kernel<false, 1>), dim3((unsigned)nchains), dim3(256), 0, (hipStream_t)stream, ev, cap, hdr, nullptr, d,
                           static_cast<ConsumeCursor*>(cur), nullptr, static_cast<ConsumeMeta*>(meta), grid, K, t0, dt,
                           reinterpret_cast<double2*>(cummean_pairs));
    return (int)hipGetLastError();
}

// occupation of a barrier ensemble: zeros, and the side a coordinate that starts frozen sits on -- the barrier of its saved speed v_old = θ0 (thf)
__global__ __launch_bounds__(256) void barrier_occ_init_kernel(const double* __restrict__ thf, int64_t n, BarrierOcc* occ) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    BarrierOcc o;
    o.z[0] = o.z[1] = 0.0;
    o.n[0] = o.n[1] = 0;
    o.side = thf[k] > 0.0 ? 1u : 0u;
    occ[k] = o;
}
// ... read: a coordinate still frozen is extended to the chain's last consumed event time in registers; the stored sums are not touched
__global__ __launch_bounds__(256) void barrier_occ_read_kernel(int64_t d, int64_t chain_first, int64_t n, const ConsumeCursor* cur0, const BarrierOcc* occ0,
                                                               const ConsumeMeta* meta, double* z_lo, double* z_hi, uint64_t* n_lo, uint64_t* n_hi,
                                                               double* T_out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n * d) return;
    const int64_t q = k / d, i = k - q * d;
    const int64_t chain = chain_first + q;
    const double T = meta[chain].t_last;
    const ConsumeCursor c = cur0[chain * d + i];
    const BarrierOcc o = occ0[chain * d + i];
    const bool frozen = c.th == 0.0;
    if (z_lo) z_lo[k] = o.z[0] + ((frozen && o.side == 0) ? T - c.t : 0.0);
    if (z_hi) z_hi[k] = o.z[1] + ((frozen && o.side == 1) ? T - c.t : 0.0);
    if (n_lo) n_lo[k] = o.n[0];
    if (n_hi) n_hi[k] = o.n[1];
    if (i == 0 && T_out) T_out[q] = T;
}
int launch_barrier_occ_init(const double* thf, int64_t d, int64_t nchains, void* cur, void* stream) {
    const int64_t n = nchains * d;
    hipLaunchKernelGGL(barrier_occ_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, thf, n, occ_of(cur, d, nchains));
    return (int)hipGetLastError();
}
int launch_barrier_occ_read(int64_t d, int64_t nchains, int64_t chain_first, int64_t n, void* cur, const void* meta, double* z_lo, double* z_hi,
                            uint64_t* n_lo, uint64_t* n_hi, double* T_out, void* stream) {
    const int64_t tot = n * d;
    hipLaunchKernelGGL(barrier_occ_read_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d, chain_first, n,
                       static_cast<const ConsumeCursor*>(cur), occ_of(cur, d, nchains), static_cast<const ConsumeMeta*>(meta), z_lo, z_hi, n_lo, n_hi, T_out);
    return (int)hipGetLastError();
}

// subtrace(tr, J), src/trace.jl:275-290, on a chain's trace segment: the events whose coordinate lies in J, renumbered by their position in J (loc[i] =
// position of i in J, or -1), in their order; one workgroup, chunks of 256 events compacted by a block-wide prefix count
__global__ __launch_bounds__(256) void trace_subtrace_kernel(const pdmp_event* __restrict__ ev, int64_t n, const int32_t* __restrict__ loc, pdmp_event* __restrict__ out,
                                                            int64_t out_cap, unsigned long long* n_out) {
    __shared__ uint32_t s_cnt[256];
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    if (tid == 0) s_base = 0ull;
    __syncthreads();
    for (int64_t base = 0; base < n; base += 256) {
        const int64_t k = base + tid;
        pdmp_event e;
        e.t = 0.0;
        e.i = 0;
        e.x = e.theta = 0.0;
        int32_t l = -1;
        if (k < n) {
            e = ev[k];
            l = loc[e.i];
        }
        s_cnt[tid] = (l >= 0) ? 1u : 0u;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {  // inclusive prefix sum
            const uint32_t v = (tid >= off) ? s_cnt[tid - off] : 0u;
            __syncthreads();
            s_cnt[tid] += v;
            __syncthreads();
        }
        const unsigned long long at = s_base + (unsigned long long)s_cnt[tid] - 1ull;
        if (l >= 0 && (int64_t)at < out_cap) {
            e.i = (int64_t)l;
            out[at] = e;
        }
        __syncthreads();
        if (tid == 255) s_base += (unsigned long long)s_cnt[255];
        __syncthreads();
    }
    if (tid == 0) *n_out = s_base;
}
int launch_trace_subtrace(const pdmp_event* ev, int64_t n, const int32_t* loc, pdmp_event* out, int64_t out_cap, unsigned long long* n_out, void* stream) {
    hipLaunchKernelGGL(trace_subtrace_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ev, n, loc, out, out_cap, n_out);
    return (int)hipGetLastError();
}
// what a finished launch left in its trace segments, per chain, and the segments handed back empty (the event loop's next launch writes the OTHER
// buffer from slot 0): one thread per chain, stream-ordered behind the launch
__global__ __launch_bounds__(256) void consume_snapshot_kernel(DevChain* hdr, int64_t nchains, uint64_t* __restrict__ snap) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nchains) return;
    snap[2 * k] = hdr[k].c.ntrace;
    snap[2 * k + 1] = hdr[k].c.nevents;
    hdr[k].c.ntrace = 0;
}
int launch_consume_snapshot(DevChain* hdr, int64_t nchains, uint64_t* snap, void* stream) {
    hipLaunchKernelGGL(consume_snapshot_kernel, dim3((unsigned)((nchains + 255) / 256)), dim3(256), 0, (hipStream_t)stream, hdr, nchains, snap);
    return (int)hipGetLastError();
}
int launch_consume_flush(int64_t d, int64_t nchains, const void* cur, const void* meta, double* grid, int64_t K, double t0, double dt, void* stream) {
    hipLaunchKernelGGL(consume_flush_kernel, dim3((unsigned)((d + 255) / 256), (unsigned)nchains), dim3(256), 0, (hipStream_t)stream, d,
                       static_cast<const ConsumeCursor*>(cur), static_cast<const ConsumeMeta*>(meta), grid, K, t0, dt);
    return (int)hipGetLastError();
}
int launch_consume_mean(int64_t d, int64_t chain_first, int64_t n, const void* cur, const void* meta, double* mean_out, double* T_out, void* stream) {
    const int64_t tot = n * d;
    hipLaunchKernelGGL(consume_mean_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d, chain_first, n,
                       static_cast<const ConsumeCursor*>(cur), static_cast<const ConsumeMeta*>(meta), mean_out, T_out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ conditional trace (src/condition.jl)
//
// collect(conditional_trace(Ξ, (p, n))) of a FactTrace: the points where the path crosses the hyperplane {x : ⟨x − p, n⟩ = 0}, slice by slice like
// the consumers above (DESIGN.md "Conditional trace" has the contract and why the reference's own loop cannot be it).  S = the coordinates with
// n_j ≠ 0, at most COND_MAX_S, as a list (idx, and loc[] = position in the list or −1).  A PIECE runs between two events of S; from the cursors
// of S as of its start t_b:  xs_k = x_c + θ_c (t_b − t_c),  g = Σ n_k (p_k − xs_k),  h = Σ n_k θ_c,k  in the order of dot_wave64 (list position =
// element index),  τ = g / h,  s = t_b + τ;  a candidate iff τ > 0;  a hit, once per piece, when the next event of S arrives at t_e >= s or the
// last consumed event time T_last >= s.  s depends on (t_b, cursors) only, so the hits do not depend on how the run was sliced.
// One workgroup per chain, per slice, in two passes over the slice:
//   1. chunks of 256 events are compacted to their events of S (block prefix count, as trace_subtrace_kernel) in LDS and walked by wavefront 0,
//      which holds the cursors of S, n and p in LDS: lane l sums list entries l, l + 64, ..., then wave_sum_f64.  Hit times go to the hit list.
//   2. the rows of this slice's new hits, for all d coordinates: the events with t < s (strictly: the reference emits before it applies the event)
//      are applied to the condition's OWN cursors (t, x, θ per (chain, coordinate), 24 bytes: the consumers' cursors above are neither read nor
//      written after the init, so mean / discretize stay what they were), then row_j = x_c + θ_c (s − t_c), thread by thread.  Only a coordinate's
//      LAST event of a range counts -- no sums are kept --, so of two events of one coordinate inside a chunk the earlier one is dropped.
struct CondMeta {
    uint64_t consumed;  // events of this chain consumed so far (global event index)
    double t_b;         // where the open piece began
    uint64_t nhits;     // hits so far, NOT clamped to max_hits
    uint64_t done;      // the open piece has had its hit
};
size_t cond_meta_bytes() { return sizeof(CondMeta); }

__global__ __launch_bounds__(256) void cond_init_kernel(const ConsumeCursor* __restrict__ cur, int64_t d, int64_t nchains, double t0, double* ct, double* cx,
                                                        double* cth, CondMeta* meta) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < nchains) {
        CondMeta m;
        m.consumed = 0;
        m.t_b = t0;
        m.nhits = 0;
        m.done = 0;
        meta[k] = m;
    }
    if (k >= nchains * d) return;
    const ConsumeCursor c = cur[k];  // (before the first consume: t0, x0, θ0)
    ct[k] = c.t;
    cx[k] = c.x;
    cth[k] = c.th;
}

// the events [lo, hi) of a chain's segment applied to the condition's cursors: per coordinate the last one of the range
__device__ __forceinline__ void cond_apply(const pdmp_event* __restrict__ ev, uint64_t lo, uint64_t hi, int64_t d, double* ct, double* cx, double* cth,
                                           uint32_t* s_i, uint8_t* s_own) {
    const int tid = threadIdx.x;
    for (uint64_t base = lo; base < hi; base += 256) {
        const uint64_t e = base + (uint64_t)tid;
        const bool valid = e < hi;
        pdmp_event evt;
        evt.t = 0.0;
        evt.i = 0;
        evt.x = evt.theta = 0.0;
        if (valid) evt = ev[e];
        const bool inside = valid && (uint64_t)evt.i < (uint64_t)d;
        const uint32_t hs = ((uint32_t)evt.i * 0x9E3779B1u) >> 20;  // (12 bits: the table of consume_events_kernel)
        s_i[tid] = inside ? (uint32_t)evt.i : 0xffffffffu;
        if (inside) s_own[hs] = (uint8_t)tid;
        __syncthreads();
        const bool clash = inside && s_own[hs] != (uint8_t)tid;
        __syncthreads();
        if (clash) s_own[hs] = 0xff;
        __syncthreads();
        bool write = inside;
        if (inside && (clash || s_own[hs] == 0xff))  // another event of this chunk hashes alike: a later one of the same coordinate wins
            for (int q = tid + 1; q < 256; ++q)
                if (s_i[q] == (uint32_t)evt.i) {
                    write = false;
                    break;
                }
        if (write) {
            ct[evt.i] = evt.t;
            cx[evt.i] = evt.x;
            cth[evt.i] = evt.theta;
        }
        __threadfence_block();
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void cond_events_kernel(const pdmp_event* ev0, int64_t cap, const DevChain* hdr, int64_t d, const int32_t* __restrict__ loc,
                                                          const int32_t* __restrict__ idx, int nS, const double* __restrict__ pn, double* ct0, double* cx0,
                                                          double* cth0, CondMeta* meta, double* hit_t0, double* hit_x0, int64_t max_hits) {
    const int64_t chain = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    __shared__ double s_t[COND_MAX_S], s_x[COND_MAX_S], s_th[COND_MAX_S], s_n[COND_MAX_S], s_p[COND_MAX_S];  // the cursors of S as of t_b; n, p over S
    __shared__ double c_t[256], c_x[256], c_th[256];  // a chunk's events of S, compacted
    __shared__ int32_t c_l[256];
    __shared__ uint32_t s_cnt[256], s_i[256];
    __shared__ uint8_t s_own[CONSUME_HASH];
    __shared__ uint64_t s_split, s_nh;
    const uint64_t ntrace = hdr[chain].c.ntrace, nevents = hdr[chain].c.nevents;
    const uint64_t n = ntrace < (uint64_t)cap ? ntrace : (uint64_t)cap;
    CondMeta m = meta[chain];
    const uint64_t first_global = nevents - ntrace;  // global index of buffer slot 0
    const uint64_t pos0 = (m.consumed > first_global) ? (m.consumed - first_global) : 0;  // first unconsumed slot
    if (pos0 >= n) return;
    const pdmp_event* ev = ev0 + chain * cap;
    double *ct = ct0 + chain * d, *cx = cx0 + chain * d, *cth = cth0 + chain * d;
    double* hit_t = hit_t0 + chain * max_hits;
    for (int k = tid; k < nS; k += 256) {  // (every earlier event is applied: the condition's cursors ARE the cursors of S as of t_b)
        const int32_t j = idx[k];
        s_t[k] = ct[j];
        s_x[k] = cx[j];
        s_th[k] = cth[j];
        s_p[k] = pn[k];
        s_n[k] = pn[nS + k];
    }
    __syncthreads();

    // ---- pass 1: the hit times
    const bool walker = tid < 64;  // wavefront 0
    double t_b = m.t_b, s = 0.0;
    bool cand = false, done = m.done != 0;
    uint64_t nh = m.nhits;
    const uint64_t nh0 = nh;
    auto open_piece = [&]() {
        double pg = 0.0, ph = 0.0;
        for (int k = lane; k < nS; k += 64) {
            const double xs = s_x[k] + s_th[k] * (t_b - s_t[k]);
            pg += s_n[k] * (s_p[k] - xs);
            ph += s_n[k] * s_th[k];
        }
        const double tau = wave_sum_f64(pg) / wave_sum_f64(ph);
        s = t_b + tau;
        cand = tau > 0;  // (false for NaN; s = +Inf is never reached by an event)
    };
    auto emit = [&]() {
        if (lane == 0 && nh < (uint64_t)max_hits) hit_t[nh] = s;
        nh += 1;
        done = true;
    };
    if (walker) open_piece();
    for (uint64_t base = pos0; base < n; base += 256) {
        const uint64_t e = base + (uint64_t)tid;
        pdmp_event evt;
        evt.t = 0.0;
        evt.i = 0;
        evt.x = evt.theta = 0.0;
        int32_t l = -1;
        if (e < n) {
            evt = ev[e];
            if ((uint64_t)evt.i < (uint64_t)d) l = loc[evt.i];
        }
        s_cnt[tid] = (l >= 0) ? 1u : 0u;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {  // inclusive prefix sum
            const uint32_t v = (tid >= off) ? s_cnt[tid - off] : 0u;
            __syncthreads();
            s_cnt[tid] += v;
            __syncthreads();
        }
        if (l >= 0) {
            const uint32_t at = s_cnt[tid] - 1u;
            c_t[at] = evt.t;
            c_x[at] = evt.x;
            c_th[at] = evt.theta;
            c_l[at] = l;
        }
        __syncthreads();
        if (walker) {
            const uint32_t cnt = s_cnt[255];
            for (uint32_t q = 0; q < cnt; ++q) {
                const double te = c_t[q];
                const int32_t lq = c_l[q];
                if (!done && cand && te >= s) emit();  // (inclusive, src/condition.jl:42)
                if (lane == (lq & 63)) {
                    s_t[lq] = te;
                    s_x[lq] = c_x[q];
                    s_th[lq] = c_th[q];
                }
                asm volatile("" ::: "memory");  // (one wavefront: its DS operations retire in order)
                t_b = te;
                done = false;
                open_piece();
            }
        }
        __syncthreads();
    }
    if (walker && !done && cand && ev[n - 1].t >= s) emit();  // T_last >= s
    if (tid == 0) s_nh = nh;
    __threadfence_block();
    __syncthreads();

    // ---- pass 2: the rows of this slice's hits, and the condition's cursors brought to the end of the slice
    const uint64_t nh1 = s_nh;
    const uint64_t stored = nh1 < (uint64_t)max_hits ? nh1 : (uint64_t)max_hits;
    uint64_t pos = pos0;
    for (uint64_t q = nh0; q < stored; ++q) {
        const double sq = hit_t[q];
        if (tid == 0) {  // first slot in [pos, n) whose time is not before sq (the trace is sorted by time)
            uint64_t lo = pos, hi = n;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (ev[mid].t < sq) lo = mid + 1;
                else hi = mid;
            }
            s_split = lo;
        }
        __syncthreads();
        const uint64_t split = s_split;
        cond_apply(ev, pos, split, d, ct, cx, cth, s_i, s_own);
        __syncthreads();
        double* const row = hit_x0 + (chain * max_hits + (int64_t)q) * d;
        for (int64_t j = tid; j < d; j += 256) row[j] = cx[j] + cth[j] * (sq - ct[j]);
        pos = split;
        __syncthreads();
    }
    cond_apply(ev, pos, n, d, ct, cx, cth, s_i, s_own);
    if (tid == 0) {
        m.consumed = nevents;
        m.t_b = t_b;
        m.nhits = nh1;
        m.done = done ? 1 : 0;
        meta[chain] = m;
    }
}

int launch_cond_init(const void* cur, int64_t d, int64_t nchains, double t0, double* ccur, void* meta, void* stream) {
    const int64_t n = nchains * d;
    hipLaunchKernelGGL(cond_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, static_cast<const ConsumeCursor*>(cur), d, nchains,
                       t0, ccur, ccur + n, ccur + 2 * n, static_cast<CondMeta*>(meta));
    return (int)hipGetLastError();
}
int launch_cond_events(const pdmp_event* ev, int64_t cap, const DevChain* hdr, int64_t d, int64_t nchains, const int32_t* loc, const int32_t* idx, int nS,
                       const double* pn, double* ccur, void* meta, double* hit_t, double* hit_x, int64_t max_hits, void* stream) {
    const int64_t n = nchains * d;
    hipLaunchKernelGGL(cond_events_kernel, dim3((unsigned)nchains), dim3(256), 0, (hipStream_t)stream, ev, cap, hdr, d, loc, idx, nS, pn, ccur, ccur + n,
                       ccur + 2 * n, static_cast<CondMeta*>(meta), hit_t, hit_x, max_hits);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ pair integrals (covariance of a FactTrace)
//
// S_ij = ∫ (x_i − c_i)(x_j − c_j) dt and J_i = ∫ (x_i − c_i) dt over a caller-given set of pairs, exactly, slice by slice (DESIGN.md "Pair
// integrals" has the contract; tests/ref/pairs_ref.c states it sequentially).  Coordinates have clocks of their own, so the integrand of a pair is
// a product of two lines whose pieces end at the events of EITHER coordinate: an event (t, i, x, θ) closes, for every listed partner j of i, the
// piece [max(t_i, t_j), t] from the two cursors, then J_i gets [t_i, t] and i's cursor becomes (t, x, θ).  The cursors are the consumer's own
// (t, x, θ, J: 32 bytes per chain and coordinate); those of consume_events_kernel are read once, by the init.
//   pair_events_kernel  one wavefront per chain walks the slice in order.  64 records at a time are loaded one per lane, with the adjacency row
//     of their coordinate (adj_ptr; adj = (partner, slot of S), every pair under both of its coordinates, (i, i) once), and handed round by
//     readlane.  For an event of i lane l takes the l-th partner: j's cursor, c_j and S[slot] are gathered, the piece added and stored; rows
//     longer than 64 go round in strides of 64; lane 0 then writes J_i and i's cursor.  Every lane has read i's old cursor by then: its load
//     precedes the store in the order of the one wavefront.
//   The walk is a chain of dependent round trips, so the gather of the NEXT event is issued before the arithmetic of the current one -- unless
//     the two conflict: the same coordinate, or partners (the next coordinate is in the row held by the lanes: one ballot; a row longer than 64
//     counts as a conflict).  Then the gather waits for the stores (s_waitcnt vmcnt(0): the workgroup is ONE wavefront, for which
//     __threadfence_block() compiles to nothing).  Between events that do not conflict nothing is shared.  An event two or more back that
//     wrote what this gather reads (A, B, A) is ordered by the wavefront itself: its vector memory operations execute in issue order.
//     The adjacency entry of a lane is loaded TWO events ahead (read-only), so a gather is one round trip.
//   pair_read_kernel  closes every pair from max(t_i, t_j) and every J_i from t_i to the chain's last consumed event time, in registers: the
//     accumulators are not touched and the run can go on.
struct PairCursor {
    double t, x, th, J;  // clock, position, velocity after the coordinate's last consumed event; ∫ (x_i − c_i) dt up to t
};
static_assert(sizeof(PairCursor) == 32, "a cursor never straddles a 128-byte line");
struct PairMeta {
    uint64_t consumed;  // events of this chain consumed so far (global event index)
    double t_last;      // time of the last of them (t0 before the first)
};
size_t pair_cursor_bytes() { return sizeof(PairCursor); }
size_t pair_meta_bytes() { return sizeof(PairMeta); }

__global__ __launch_bounds__(256) void pair_init_kernel(const ConsumeCursor* __restrict__ cur, int64_t d, int64_t nchains, double t0, PairCursor* pc,
                                                        PairMeta* meta) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < nchains) {
        PairMeta m;
        m.consumed = 0;
        m.t_last = t0;
        meta[k] = m;
    }
    if (k >= nchains * d) return;
    const ConsumeCursor c = cur[k];  // (before the first consume: t0, x0, θ0)
    PairCursor p;
    p.t = c.t;
    p.x = c.x;
    p.th = c.th;
    p.J = 0.0;
    pc[k] = p;
}

struct PairGather {  // what a lane holds of its partner of an event's coordinate i
    double ti, xi, thi;      // i's cursor
    double tj, xj, thj, cj;  // the partner's, and its centre
    double s;                // S[slot]
    int32_t j, slot;         // slot < 0: the row has no partner for this lane
};

// the lane's entry of an adjacency row [p0, p1): read-only data, loaded ahead of the gather that needs it (slot < 0: no partner for this lane)
__device__ __forceinline__ PairAdj pair_adj(const PairArgs& A, int32_t p, int32_t p1) {
    PairAdj a;
    a.j = a.slot = -1;
    if (p < p1) a = A.adj[p];
    return a;
}

__device__ __forceinline__ PairGather pair_gather(const PairArgs& A, const PairCursor* cur, const double* S, int32_t i, PairAdj a) {
    PairGather g;
    g.ti = cur[i].t;
    g.xi = cur[i].x;
    g.thi = cur[i].th;
    g.tj = g.xj = g.thj = g.cj = g.s = 0.0;
    g.j = a.j;
    g.slot = a.slot;
    if (a.slot >= 0) {
        g.tj = cur[a.j].t;
        g.xj = cur[a.j].x;
        g.thj = cur[a.j].th;
        g.cj = A.center[a.j];
        g.s = S[a.slot];
    }
    return g;
}

// one wavefront: every store it issued has reached memory before a load behind this point is issued (vmcnt counts stores on gfx9)
__device__ __forceinline__ void pair_wait_stores() {
    __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) expcnt(0) lgkmcnt(0)
    asm volatile("" ::: "memory");
}

// the piece of a pair from its two cursors to time t (the arithmetic of ref_pairs_fact, in its order)
__device__ __forceinline__ double pair_close(double ti, double xi, double thi, double ci, double tj, double xj, double thj, double cj, double t) {
    const double s0 = ti > tj ? ti : tj;
    const double a = (xi - ci) + thi * (s0 - ti);
    const double b = (xj - cj) + thj * (s0 - tj);
    return pair_piece(a, b, thi, thj, t - s0);
}

__global__ __launch_bounds__(64) void pair_events_kernel(const pdmp_event* ev0, int64_t cap, const DevChain* hdr, int64_t d, PairArgs A) {
    const int64_t chain = blockIdx.x;
    const int lane = threadIdx.x;
    PairMeta* const meta = static_cast<PairMeta*>(A.meta) + chain;
    const uint64_t ntrace = hdr[chain].c.ntrace, nevents = hdr[chain].c.nevents;
    const uint64_t n = ntrace < (uint64_t)cap ? ntrace : (uint64_t)cap;
    const uint64_t consumed = meta->consumed;
    const uint64_t first_global = nevents - ntrace;  // global index of buffer slot 0
    const uint64_t pos0 = (consumed > first_global) ? (consumed - first_global) : 0;  // first unconsumed slot
    if (pos0 >= n) return;
    const pdmp_event* const ev = ev0 + chain * cap;
    PairCursor* const cur = static_cast<PairCursor*>(A.cur) + chain * d;
    double* const S = A.S + chain * A.npairs;
    for (uint64_t base = pos0; base < n; base += 64) {
        const int cnt = (n - base < 64) ? (int)(n - base) : 64;
        // this lane's record of the chunk and the adjacency row of its coordinate (read-only data: nothing in flight conflicts with it)
        double rt = 0.0, rx = 0.0, rth = 0.0;
        int32_t ri = -1, rp0 = 0, rp1 = 0;
        if (lane < cnt) {
            const pdmp_event r = ev[base + (uint64_t)lane];
            rt = r.t;
            rx = r.x;
            rth = r.theta;
            if ((uint64_t)r.i < (uint64_t)d) {
                ri = (int32_t)r.i;
                rp0 = A.adj_ptr[ri];
                rp1 = A.adj_ptr[ri + 1];
            }
        }
        pair_wait_stores();  // (the stores of the chunk before)
        int32_t i = (int32_t)readlane_u32((uint32_t)ri, 0), p0 = (int32_t)readlane_u32((uint32_t)rp0, 0), p1 = (int32_t)readlane_u32((uint32_t)rp1, 0);
        const int q1 = cnt > 1 ? 1 : 0;
        PairAdj an = pair_adj(A, (int32_t)readlane_u32((uint32_t)rp0, q1) + lane, (int32_t)readlane_u32((uint32_t)rp1, q1));  // event 1's entry
        PairGather g{};
        g.slot = -1;
        if (i >= 0) g = pair_gather(A, cur, S, i, pair_adj(A, p0 + lane, p1));
        for (int q = 0; q < cnt; ++q) {
            const double t = readlane_f64(rt, q), x = readlane_f64(rx, q), th = readlane_f64(rth, q);
            const bool have_next = q + 1 < cnt;
            const int qn = have_next ? q + 1 : q, qnn = q + 2 < cnt ? q + 2 : q;
            const int32_t in = have_next ? (int32_t)readlane_u32((uint32_t)ri, qn) : -1;
            const int32_t np0 = (int32_t)readlane_u32((uint32_t)rp0, qn), np1 = (int32_t)readlane_u32((uint32_t)rp1, qn);
            // the adjacency entry of the event after the next: two events ahead, so the next gather is ONE round trip, not two
            const PairAdj ann = pair_adj(A, (int32_t)readlane_u32((uint32_t)rp0, qnn) + lane, (int32_t)readlane_u32((uint32_t)rp1, qnn));
            // the next event conflicts with this one if it has the same coordinate or its coordinate is one of this one's partners
            const bool conflict = in == i || p1 - p0 > 64 || __any(g.slot >= 0 && g.j == in) != 0;
            PairGather gn{};
            gn.slot = -1;
            if (in >= 0 && !conflict) gn = pair_gather(A, cur, S, in, an);
            if (i >= 0) {
                const double ci = A.center[i];
                if (g.slot >= 0) S[g.slot] = g.s + pair_close(g.ti, g.xi, g.thi, ci, g.tj, g.xj, g.thj, g.cj, t);
                for (int32_t p = p0 + 64; p < p1; p += 64) {  // rows longer than a wavefront: the slots of a row are distinct, nothing to order
                    const PairGather h = pair_gather(A, cur, S, i, pair_adj(A, p + lane, p1));
                    if (h.slot >= 0) S[h.slot] = h.s + pair_close(h.ti, h.xi, h.thi, ci, h.tj, h.xj, h.thj, h.cj, t);
                }
                if (lane == 0) {  // (every lane's load of i's old cursor was issued before this store)
                    PairCursor c;
                    c.J = cur[i].J + line_piece(g.xi - ci, g.thi, t - g.ti);
                    c.t = t;
                    c.x = x;
                    c.th = th;
                    cur[i] = c;
                }
            }
            if (in >= 0 && conflict) {
                pair_wait_stores();  // the cursor and the S slots just written, before they are read again
                gn = pair_gather(A, cur, S, in, an);
            }
            g = gn;
            an = ann;
            i = in;
            p0 = np0;
            p1 = np1;
        }
    }
    if (lane == 0) {
        PairMeta m;
        m.consumed = nevents;
        m.t_last = ev[n - 1].t;
        *meta = m;
    }
}

// S [n x npairs], J [n x d] and T_last [n] of chains [chain_first, chain_first + n), every open piece closed at T_last in registers
__global__ __launch_bounds__(256) void pair_read_kernel(int64_t d, PairArgs A, int64_t chain_first, int64_t n, double* S_out, double* J_out, double* T_out) {
    const int64_t per = A.npairs > d ? A.npairs : d;
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n * per) return;
    const int64_t q = k / per, r = k - q * per;
    const int64_t chain = chain_first + q;
    const PairCursor* const cur = static_cast<const PairCursor*>(A.cur) + chain * d;
    const double T = static_cast<const PairMeta*>(A.meta)[chain].t_last;
    if (r < A.npairs) {
        const int32_t i = A.pi[r], j = A.pj[r];
        const PairCursor a = cur[i], b = cur[j];
        S_out[q * A.npairs + r] = A.S[chain * A.npairs + r] + pair_close(a.t, a.x, a.th, A.center[i], b.t, b.x, b.th, A.center[j], T);
    }
    if (r < d) {
        const PairCursor a = cur[r];
        J_out[q * d + r] = a.J + line_piece(a.x - A.center[r], a.th, T - a.t);
    }
    if (r == 0) T_out[q] = T;
}

int launch_pair_init(const void* cur, int64_t d, int64_t nchains, double t0, const PairArgs& a, void* stream) {
    const int64_t n = nchains * d;
    hipLaunchKernelGGL(pair_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, static_cast<const ConsumeCursor*>(cur), d, nchains,
                       t0, static_cast<PairCursor*>(a.cur), static_cast<PairMeta*>(a.meta));
    return (int)hipGetLastError();
}
int launch_pair_events(const pdmp_event* ev, int64_t cap, const DevChain* hdr, int64_t d, int64_t nchains, const PairArgs& a, void* stream) {
    hipLaunchKernelGGL(pair_events_kernel, dim3((unsigned)nchains), dim3(64), 0, (hipStream_t)stream, ev, cap, hdr, d, a);
    return (int)hipGetLastError();
}
int launch_pair_read(int64_t d, const PairArgs& a, int64_t chain_first, int64_t n, double* S_out, double* J_out, double* T_out, void* stream) {
    const int64_t tot = n * (a.npairs > d ? a.npairs : d);
    hipLaunchKernelGGL(pair_read_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d, a, chain_first, n, S_out, J_out, T_out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ marginal histograms (occupation times of a FactTrace)
//
// H[s][k + 1] = the time listed coordinate s spends in the bin [e_k, e_k+1) of its own range, k = −1 (below lo) .. B (at or above hi), exactly:
// between two of its events a coordinate is a line, so the time in a bin is a closed form (DESIGN.md "Marginal histograms" has the contract;
// tests/ref/hist_ref.c states it sequentially; hist_piece_of / hist_piece_at of pdmp_bps_common.hpp are the piece).  Cursors of its own (t, x, θ and
// the rest time Z: 32 bytes per chain and LISTED coordinate); those of consume_events_kernel are read once, by the init.
//   hist_events_kernel  one workgroup of one wavefront per chain walks the slice in order.  64 records at a time are loaded one per lane with the slot
//     of their coordinate (slot_of [d], shared by the chains; −1 = not listed): one ballot drops the unlisted events of the chunk at once.  A listed
//     event is handed round by readlane; every lane reads the cursor (one address), makes the piece ready and takes the bins k0 + lane, k0 + lane +
//     64, ... of the k0 .. k1 it touches: a piece that crosses many bins is spread over the lanes, a row entry is owned by one lane.  Lane 0 then
//     writes Z and the cursor (every lane's load of the old cursor was issued before that store).  Events of one coordinate keep their order -- the
//     walk is sequential -- and the stores of an event have reached memory before the next listed event's loads are issued (s_waitcnt vmcnt(0): the
//     next event may be the same coordinate's, with other lanes on the same entries).  So a row is updated in the event order of its coordinate and the
//     result does not depend on how the run was sliced.  No atomics.
//   hist_read_kernel  one thread per output entry: out = H + hist_piece_at(the open piece from the cursor to T_last, k), in registers; pooled: the
//     chains of the range added in order.  The rows are not touched: a run can be read midway, and twice.
struct HistCursor {
    double t, x, th, Z;  // clock, position, velocity after the coordinate's last consumed event; the time it rested (θ = 0) up to t
};
static_assert(sizeof(HistCursor) == 32, "a cursor never straddles a 128-byte line");
size_t hist_cursor_bytes() { return sizeof(HistCursor); }
size_t hist_meta_bytes() { return sizeof(PairMeta); }  // (events consumed, T_last: the pair consumer's)

__device__ __forceinline__ HistBins hist_bins(const HistArgs& A, int64_t s) {
    HistBins b;
    b.lo = A.lo[s];
    b.hi = A.hi[s];
    b.w = A.w[s];
    b.B = A.B;
    return b;
}

__global__ __launch_bounds__(256) void hist_init_kernel(const ConsumeCursor* __restrict__ cur, int64_t d, int64_t nchains, double t0, HistArgs A) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < nchains) {
        PairMeta m;
        m.consumed = 0;
        m.t_last = t0;
        static_cast<PairMeta*>(A.meta)[k] = m;
    }
    if (k >= nchains * A.m) return;
    const int64_t chain = k / A.m, s = k - chain * A.m;
    const ConsumeCursor c = cur[chain * d + A.coords[s]];  // (before the first consume: t0, x0, θ0 -- θ = 0 where a barrier ensemble starts frozen)
    HistCursor h;
    h.t = c.t;
    h.x = c.x;
    h.th = c.th;
    h.Z = 0.0;
    static_cast<HistCursor*>(A.cur)[k] = h;
}

__global__ __launch_bounds__(64) void hist_events_kernel(const pdmp_event* ev0, int64_t cap, const DevChain* hdr, int64_t d, HistArgs A) {
    const int64_t chain = blockIdx.x;
    const int lane = threadIdx.x;
    PairMeta* const meta = static_cast<PairMeta*>(A.meta) + chain;
    const uint64_t ntrace = hdr[chain].c.ntrace, nevents = hdr[chain].c.nevents;
    const uint64_t n = ntrace < (uint64_t)cap ? ntrace : (uint64_t)cap;
    const uint64_t consumed = meta->consumed;
    const uint64_t first_global = nevents - ntrace;  // global index of buffer slot 0
    const uint64_t pos0 = (consumed > first_global) ? (consumed - first_global) : 0;  // first unconsumed slot
    if (pos0 >= n) return;
    const pdmp_event* const ev = ev0 + chain * cap;
    HistCursor* const cur = static_cast<HistCursor*>(A.cur) + chain * A.m;
    double* const H = A.H + chain * A.m * (int64_t)(A.B + 2);
    for (uint64_t base = pos0; base < n; base += 64) {
        const int cnt = (n - base < 64) ? (int)(n - base) : 64;
        double rt = 0.0, rx = 0.0, rth = 0.0;
        int32_t rs = -1;
        if (lane < cnt) {
            const pdmp_event r = ev[base + (uint64_t)lane];
            rt = r.t;
            rx = r.x;
            rth = r.theta;
            if ((uint64_t)r.i < (uint64_t)d) rs = A.slot_of[r.i];
        }
        uint64_t listed = __ballot(rs >= 0);  // (wave-uniform: the unlisted events of the chunk are gone)
        while (listed) {
            const int q = __builtin_ctzll(listed);
            listed &= listed - 1;
            const int64_t s = (int32_t)readlane_u32((uint32_t)rs, q);
            const double t = readlane_f64(rt, q), x = readlane_f64(rx, q), th = readlane_f64(rth, q);
            const HistCursor c = cur[s];
            const HistBins bn = hist_bins(A, s);
            const double tau = t - c.t;
            const HistPiece p = hist_piece_of(bn, c.x, c.th, tau);
            double* const row = H + s * (int64_t)(A.B + 2);
            for (int k = p.k0 + lane; k <= p.k1; k += 64) row[k + 1] = row[k + 1] + hist_piece_at(bn, p, k);
            if (lane == 0) {
                HistCursor c2;
                c2.Z = c.Z + hist_piece_rest(c.th, tau);
                c2.t = t;
                c2.x = x;
                c2.th = th;
                cur[s] = c2;
            }
            pair_wait_stores();  // the row and the cursor just written, before the next listed event reads them
        }
    }
    if (lane == 0) {
        PairMeta m;
        m.consumed = nevents;
        m.t_last = ev[n - 1].t;
        *meta = m;
    }
}

// one output entry of the read: row entry r < B + 2 of (chain, s) with the open piece closed at T, or (r == B + 2) the rest time Z
__device__ __forceinline__ double hist_read_entry(const HistArgs& A, int64_t chain, int64_t s, int64_t r) {
    const HistCursor c = static_cast<const HistCursor*>(A.cur)[chain * A.m + s];
    const double tau = static_cast<const PairMeta*>(A.meta)[chain].t_last - c.t;
    if (r == A.B + 2) return c.Z + hist_piece_rest(c.th, tau);
    const HistBins bn = hist_bins(A, s);
    const HistPiece p = hist_piece_of(bn, c.x, c.th, tau);
    return A.H[(chain * A.m + s) * (int64_t)(A.B + 2) + r] + hist_piece_at(bn, p, (int)r - 1);
}

__global__ __launch_bounds__(256) void hist_read_kernel(HistArgs A, int64_t chain_first, int64_t n, int pooled, double* H_out, double* Z_out, double* T_out) {
    const int64_t per = A.m * (int64_t)(A.B + 3);  // a chain's entries: m rows of B + 2, then (per row) Z
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) T_out[k] = static_cast<const PairMeta*>(A.meta)[chain_first + k].t_last;
    if (k >= (pooled ? 1 : n) * per) return;
    const int64_t q = k / per, e = k - q * per;
    const int64_t s = e / (A.B + 3), r = e - s * (A.B + 3);
    double v;
    if (pooled) {
        v = 0.0;
        for (int64_t c = 0; c < n; ++c) v = v + hist_read_entry(A, chain_first + c, s, r);
    } else {
        v = hist_read_entry(A, chain_first + q, s, r);
    }
    if (r == A.B + 2) Z_out[q * A.m + s] = v;
    else H_out[(q * A.m + s) * (int64_t)(A.B + 2) + r] = v;
}

int launch_hist_init(const void* cur, int64_t d, int64_t nchains, double t0, const HistArgs& a, void* stream) {
    const int64_t n = nchains * (a.m > 1 ? a.m : 1);
    hipLaunchKernelGGL(hist_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, static_cast<const ConsumeCursor*>(cur), d, nchains,
                       t0, a);
    return (int)hipGetLastError();
}
int launch_hist_events(const pdmp_event* ev, int64_t cap, const DevChain* hdr, int64_t d, int64_t nchains, const HistArgs& a, void* stream) {
    hipLaunchKernelGGL(hist_events_kernel, dim3((unsigned)nchains), dim3(64), 0, (hipStream_t)stream, ev, cap, hdr, d, a);
    return (int)hipGetLastError();
}
int launch_hist_read(const HistArgs& a, int64_t chain_first, int64_t n, int pooled, double* H_out, double* Z_out, double* T_out, void* stream) {
    const int64_t ent = (pooled ? 1 : n) * a.m * (int64_t)(a.B + 3);
    const int64_t tot = ent > n ? ent : n;
    hipLaunchKernelGGL(hist_read_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, chain_first, n, pooled, H_out, Z_out, T_out);
    return (int)hipGetLastError();
}

}  // namespace pdmp
