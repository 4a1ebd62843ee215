// pdmp_consume_bps.hip -- the streaming trace consumers of the Bouncy Particle family: mean(Ξ), cummean(Ξ) and collect(discretize(Ξ, dt)) of a
// PDMPTrace (src/trace.jl:129-150, 229-266) and the free-time fractions of a sticky one, computed ON THE DEVICE from the trace buffers the
// event loops of pdmp_bps.hip write, slice by slice: consume after every slice, keep a cursor, recycle the buffer (the style of pdmp_consume.hip).
// One event of this family is 8(2d + 1) bytes -- 16 KB at d = 1024 -- and what callers do with the trace next is one of these three.
//
// A PDMPTrace event replaces the WHOLE state, so the coordinates do not interact and there is nothing to order between them: one lane owns one
// (chain, coordinate) and walks the chain's segment in event order; one wavefront takes a 64-coordinate strip of a chain, the tail lanes of the
// last strip read the last coordinate and store nothing.  No LDS, no barrier.  Event times (and a sticky event's mask word: word `strip`, bit
// `lane`) are wave-uniform, the x and θ loads of a wavefront are 512 contiguous bytes each.  What a chain carries from slice to slice besides the
// cursors -- clock, next grid row, events consumed -- is kept once per STRIP (every wavefront reads and writes a copy of its own: the wavefronts of
// one chain run at different times and never look at each other's); the readers take strip 0's.
//
// Per event (t2, x2, θ2[, f2]), in this order (DESIGN.md "PDMPTrace consumers" has the degenerate cases):
//   1. grid: while g = t0 + (double)k·dt < t2: row k = x + θ·τ, τ = g − t_cur -- a Boomerang: (x − μ)·c + θ·s + μ, (s, c) = pdmp_sincos(τ); a
//      coordinate that is not free keeps x --, k += 1.  Events with t <= g are applied before the row, of several events at one time the last
//      counts, and a row is written only once an event lies strictly beyond it (src/trace.jl:129-150 in closed form, trace.py::_discretize_pdmp).
//      The walk stops at k = K: rows the buffer has no room for are counted by the reader (from T_last, in closed form), not by a loop here.
//   2. sums: y += (x + x2)·(t2 − t_cur) (:241,260); cummean on: y / (2·t2) at the event's slot (:263); sticky: free_time += free ? t2 − t_cur : 0.
//   3. cursor: x = x2, θ = θ2, free = f2, t_cur = T_last = t2.
// The loads of the next BC_AHEAD events are issued before the arithmetic of the current ones: at small ensembles the walk is bound by latency.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pdmp_device.hpp"
#include "pdmp_engine.hpp"

namespace pdmp {

struct BpsConsumeMeta {  // per (chain, strip)
    double t_cur;        // time of the latest consumed event (t0 before the first)
    double t_last;       // ... as the readers' T_last
    int64_t k;           // the next grid row, <= K
    uint64_t consumed;   // events of the chain consumed so far (global event index)
    uint64_t free;       // sticky: the latest consumed event's free bits of this strip (bit = lane); all ones before the first
    uint64_t pad;
};
size_t bps_consume_meta_bytes() { return sizeof(BpsConsumeMeta); }

struct BpsConsumeEvent {
    double t, x, th;
    uint64_t f;
};

constexpr int BC_AHEAD = 4;

__global__ __launch_bounds__(256) void bps_consume_init_kernel(BpsConsumeArgs P) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < P.nchains * P.nstrips) {
        BpsConsumeMeta m;
        m.t_cur = m.t_last = P.t0;
        m.k = 0;
        m.consumed = 0;
        m.free = ~0ull;
        m.pad = 0;
        static_cast<BpsConsumeMeta*>(P.meta)[k] = m;
    }
    if (k >= P.nchains * P.d) return;
    const double x0 = P.x0[k];
    P.cx[k] = x0;
    P.cth[k] = P.th0[k];
    P.cy[k] = 0.0;
    if (P.cft) P.cft[k] = 0.0;
    // the first element of collect(discretize(Ξ, dt)) is t0 => x0 whatever follows: also for a chain without an event
    if (P.grid && P.K > 0) P.grid[(k / P.d) * P.K * P.d + (k % P.d)] = x0;
}

template <bool STICKY>
__device__ __forceinline__ BpsConsumeEvent bc_load(const BpsConsumeArgs& P, int64_t slot0, uint64_t e, uint64_t n, int64_t strip, int64_t ic) {
    const int64_t s = slot0 + (int64_t)(e < n ? e : n - 1);  // (behind the segment: its last event once more, never applied)
    BpsConsumeEvent ev;
    ev.t = P.ev_t[s];
    ev.x = P.ev_x[s * P.d + ic];
    ev.th = P.ev_th[s * P.d + ic];
    ev.f = STICKY ? P.ev_f[s * BPS_STICKY_WORDS + strip] : ~0ull;
    return ev;
}

template <bool BOOM, bool STICKY>
__global__ __launch_bounds__(256) void bps_consume_kernel(BpsConsumeArgs P) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= P.nchains * P.nstrips) return;
    const int64_t chain = w / P.nstrips, strip = w - chain * P.nstrips;
    const int64_t d = P.d, i = strip * 64 + lane;
    const bool live = i < d;
    const int64_t ic = live ? i : d - 1;
    BpsConsumeMeta m = static_cast<BpsConsumeMeta*>(P.meta)[w];
    const uint64_t ntrace = P.hdr[chain].c.ntrace, nevents = P.hdr[chain].c.nevents;
    const uint64_t n = ntrace < (uint64_t)P.cap ? ntrace : (uint64_t)P.cap;
    const uint64_t first_global = nevents - ntrace;  // global index of buffer slot 0
    const uint64_t pos = (m.consumed > first_global) ? (m.consumed - first_global) : 0;  // first unconsumed slot
    if (pos >= n) return;
    const int64_t slot0 = chain * P.cap, cur = chain * d + ic;
    double x = P.cx[cur], th = P.cth[cur], y = P.cy[cur];
    double ft = STICKY ? P.cft[cur] : 0.0;
    const double mu = BOOM ? P.mu[ic] : 0.0;
    double* const grid = (P.grid && P.K > 0) ? P.grid + chain * P.K * d : nullptr;

    BpsConsumeEvent now[BC_AHEAD], next[BC_AHEAD];
#pragma unroll
    for (int q = 0; q < BC_AHEAD; ++q) now[q] = bc_load<STICKY>(P, slot0, pos + q, n, strip, ic);
    for (uint64_t base = pos; base < n; base += BC_AHEAD) {
#pragma unroll
        for (int q = 0; q < BC_AHEAD; ++q) next[q] = bc_load<STICKY>(P, slot0, base + BC_AHEAD + q, n, strip, ic);
#pragma unroll
        for (int q = 0; q < BC_AHEAD; ++q) {
            const uint64_t e = base + q;
            if (e >= n) break;
            const double t2 = now[q].t;
            const bool free = !STICKY || ((m.free >> lane) & 1ull);
            while (grid && m.k < P.K) {
                const double g = P.t0 + (double)m.k * P.dt;
                if (!(g < t2)) break;
                const double tau = g - m.t_cur;
                double v;
                if (BOOM) {
                    double s, c;
                    pdmp_sincos(tau, &s, &c);
                    v = (x - mu) * c + th * s + mu;
                } else {
                    v = x + th * tau;
                }
                if (!free) v = x;
                if (live) grid[m.k * d + i] = v;
                m.k += 1;
            }
            const double dtau = t2 - m.t_cur;
            y = y + (x + now[q].x) * dtau;
            if (P.cm && live) P.cm[(slot0 + (int64_t)e) * d + i] = y / (2.0 * t2);
            if (STICKY) ft = ft + (free ? dtau : 0.0);
            x = now[q].x;
            th = now[q].th;
            m.free = now[q].f;
            m.t_cur = m.t_last = t2;
        }
#pragma unroll
        for (int q = 0; q < BC_AHEAD; ++q) now[q] = next[q];
    }
    if (live) {
        P.cx[cur] = x;
        P.cth[cur] = th;
        P.cy[cur] = y;
        if (STICKY) P.cft[cur] = ft;
    }
    if (lane == 0) {
        m.consumed = nevents;
        static_cast<BpsConsumeMeta*>(P.meta)[w] = m;
    }
}

// mean(Ξ) = y / T_last as the reference writes it (src/trace.jl:229-246: no ½), or with `inclusion` the fraction of [t0, T_last] a coordinate of
// a sticky ensemble was free -- the initial mask's own bits (all free) where T_last <= t0, as trace.py::inclusion_prob has it
__global__ __launch_bounds__(256) void bps_consume_read_kernel(BpsConsumeArgs P, int inclusion, int64_t chain_first, int64_t n, double* out, double* T_out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n * P.d) return;
    const int64_t q = k / P.d, i = k - q * P.d;
    const int64_t chain = chain_first + q;
    const double T = static_cast<const BpsConsumeMeta*>(P.meta)[chain * P.nstrips].t_last;
    if (inclusion) out[k] = (T > P.t0) ? P.cft[chain * P.d + i] / (T - P.t0) : 1.0;
    else out[k] = P.cy[chain * P.d + i] / T;
    if (i == 0 && T_out) T_out[q] = T;
}

int launch_bps_consume_init(const BpsConsumeArgs& p, void* stream) {
    const int64_t n = p.nchains * (p.d > p.nstrips ? p.d : p.nstrips);
    hipLaunchKernelGGL(bps_consume_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

int launch_bps_consume_events(const BpsConsumeArgs& p, void* stream) {
    const int64_t waves = p.nchains * p.nstrips;
    const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    const bool boom = p.mu != nullptr, sticky = p.ev_f != nullptr;
    if (boom && sticky) hipLaunchKernelGGL((bps_consume_kernel<true, true>), grid, block, 0, (hipStream_t)stream, p);
    else if (boom) hipLaunchKernelGGL((bps_consume_kernel<true, false>), grid, block, 0, (hipStream_t)stream, p);
    else if (sticky) hipLaunchKernelGGL((bps_consume_kernel<false, true>), grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((bps_consume_kernel<false, false>), grid, block, 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

int launch_bps_consume_read(const BpsConsumeArgs& p, int inclusion, int64_t chain_first, int64_t n, double* out, double* T_out, void* stream) {
    const int64_t tot = n * p.d;
    hipLaunchKernelGGL(bps_consume_read_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, inclusion, chain_first, n, out,
                       T_out);
    return (int)hipGetLastError();
}

}  // namespace pdmp
