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
//
// THE WALK (bps_walk), shared by this kernel and the four consumers behind it (pairs, arc pairs, histograms, arc histograms): a thread applies the
// unconsumed slots [pos, n) of its chain's segment (bps_slice) in event order.  load(e) reads slot e < n of the segment into the consumer's event
// record, apply(ev, e) is the consumer's own arithmetic and cursor update.  The loads of the next BC_AHEAD events are issued before the arithmetic
// of the current ones -- at small ensembles the walk is bound by latency --; a load behind the segment reads its last event once more and is never
// applied.  The four consumers run BEFORE bps_consume_kernel of the same slice and only read what that kernel carries (cursors, clock, free bits,
// events consumed); their threads of a workgroup belong to one chain, so event times are wave-uniform loads.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pdmp_bps_common.hpp"
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
size_t bps_consume_meta_tlast_offset() { return offsetof(BpsConsumeMeta, t_last); }

constexpr int BC_AHEAD = 4;
#define BPS_WALK_INLINE __attribute__((always_inline))  // (on the lambdas handed to bps_walk: one copy of their code per unrolled call, no call)

template <class Ev, class Load, class Apply>
__device__ __forceinline__ void bps_walk(uint64_t pos, uint64_t n, Load load, Apply apply) {
    Ev now[BC_AHEAD], next[BC_AHEAD];
    const auto at = [&](uint64_t e) BPS_WALK_INLINE { return load(e < n ? e : n - 1); };
#pragma unroll
    for (int q = 0; q < BC_AHEAD; ++q) now[q] = at(pos + q);
    for (uint64_t base = pos; base < n; base += BC_AHEAD) {
#pragma unroll
        for (int q = 0; q < BC_AHEAD; ++q) next[q] = at(base + BC_AHEAD + q);
#pragma unroll
        for (int q = 0; q < BC_AHEAD; ++q) {
            if (base + q >= n) break;
            apply(now[q], base + q);
        }
#pragma unroll
        for (int q = 0; q < BC_AHEAD; ++q) now[q] = next[q];
    }
}

// the unconsumed slots [pos, n) of a chain's segment and what the chain carries, as `strip`'s copy of its progress has it (the consumers in front
// of bps_consume_kernel take strip 0's)
struct BpsSlice {
    uint64_t pos, n, nevents;
    BpsConsumeMeta m;
};
__device__ __forceinline__ BpsSlice bps_slice(const BpsConsumeArgs& P, int64_t chain, int64_t strip = 0) {
    BpsSlice s;
    s.m = static_cast<const BpsConsumeMeta*>(P.meta)[chain * P.nstrips + strip];
    const uint64_t ntrace = P.hdr[chain].c.ntrace;
    s.nevents = P.hdr[chain].c.nevents;
    s.n = ntrace < (uint64_t)P.cap ? ntrace : (uint64_t)P.cap;
    const uint64_t first_global = s.nevents - ntrace;  // global index of buffer slot 0
    s.pos = (s.m.consumed > first_global) ? (s.m.consumed - first_global) : 0;  // first unconsumed slot
    return s;
}

// free bit of coordinate i in a mask of one word per strip: an event's words (ev_f + slot·BPS_STICKY_WORDS) or the carried ones (a chain's meta)
__device__ __forceinline__ uint64_t bps_mask_word(const uint64_t* words, int64_t k) { return words[k]; }
__device__ __forceinline__ uint64_t bps_mask_word(const BpsConsumeMeta* strips, int64_t k) { return strips[k].free; }
template <bool STICKY, class Words>
__device__ __forceinline__ bool bps_free_bit(const Words* words, int64_t i) {
    return STICKY ? ((bps_mask_word(words, i >> 6) >> (i & 63)) & 1ull) != 0 : true;
}

// (x, θ, free) of column i at global slot s of the trace, or of a chain's cursor
struct BpsColumn {
    double x, th;
    bool f;
};
template <bool STICKY>
__device__ __forceinline__ BpsColumn bps_column(const BpsConsumeArgs& P, int64_t s, int64_t i) {
    BpsColumn c;
    c.x = P.ev_x[s * P.d + i];
    c.th = P.ev_th[s * P.d + i];
    c.f = bps_free_bit<STICKY>(P.ev_f + s * BPS_STICKY_WORDS, i);
    return c;
}
template <bool STICKY>
__device__ __forceinline__ BpsColumn bps_cursor(const BpsConsumeArgs& P, int64_t chain, int64_t i) {
    BpsColumn c;
    c.x = P.cx[chain * P.d + i];
    c.th = P.cth[chain * P.d + i];
    c.f = bps_free_bit<STICKY>(static_cast<const BpsConsumeMeta*>(P.meta) + chain * P.nstrips, i);
    return c;
}

struct BpsConsumeEvent {
    double t, x, th;
    uint64_t f;  // (the whole mask word of the strip: the meta record carries it)
};

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
__device__ __forceinline__ BpsConsumeEvent bc_load(const BpsConsumeArgs& P, int64_t s, int64_t strip, int64_t ic) {
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
    const BpsSlice sl = bps_slice(P, chain, strip);
    if (sl.pos >= sl.n) return;
    BpsConsumeMeta m = sl.m;
    const int64_t slot0 = chain * P.cap, cur = chain * d + ic;
    double x = P.cx[cur], th = P.cth[cur], y = P.cy[cur];
    double ft = STICKY ? P.cft[cur] : 0.0;
    const double mu = BOOM ? P.mu[ic] : 0.0;
    double* const grid = (P.grid && P.K > 0) ? P.grid + chain * P.K * d : nullptr;

    bps_walk<BpsConsumeEvent>(
        sl.pos, sl.n, [&](uint64_t e) BPS_WALK_INLINE { return bc_load<STICKY>(P, slot0 + (int64_t)e, strip, ic); },
        [&](const BpsConsumeEvent& ev, uint64_t e) BPS_WALK_INLINE {
            const double t2 = ev.t;
            const bool free = !STICKY || ((m.free >> lane) & 1ull);  // (bps_free_bit of the word in hand: bit `lane` of word `strip`)
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
            y = y + (x + ev.x) * dtau;
            if (P.cm && live) P.cm[(slot0 + (int64_t)e) * d + i] = y / (2.0 * t2);
            if (STICKY) ft = ft + (free ? dtau : 0.0);
            x = ev.x;
            th = ev.th;
            m.free = ev.f;
            m.t_cur = m.t_last = t2;
        });
    if (live) {
        P.cx[cur] = x;
        P.cth[cur] = th;
        P.cy[cur] = y;
        if (STICKY) P.cft[cur] = ft;
    }
    if (lane == 0) {
        m.consumed = sl.nevents;
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

// ------------------------------------------------------------------------------------------ conditional trace (src/condition.jl:56-76)
//
// collect(conditional_trace(Ξ, (p, n))) of a PDMPTrace with the linear flow: per event (t_k, x_k, θ_k[, f_k]) with the cursor (t_c, x_c, θ_c, f_c)
// before it,  g = dot_wave64(p − x_c, n),  h = dot_wave64(θ_c, n),  τ = g / h;  a hit iff τ > 0 and t_c + τ < t_k (strictly), at t_c + τ, with
// row_j = f_c,j ? x_c,j + θ_c,j τ : x_c,j; one hit per segment, nothing behind the last event (DESIGN.md "Conditional trace").  An event replaces the
// whole state, so the segments are independent: the cursor of a segment is the event before it, the carried cursor for the first of a slice.  Both
// kernels run BEFORE bps_consume_kernel of the same slice and only read what it carries (cursors, clock, free bits, events consumed).
//   bps_cond_scan_kernel  one wavefront per (chain, segment): 512 contiguous bytes of x_c and of θ_c per load, p and n alongside; lane l sums
//                         elements l, l + 64, ..., then wave_sum_f64; τ of a hit (−1 otherwise) to the segment's slot of a [nchains x cap] array.
//   bps_cond_rows_kernel  one workgroup per chain: chunks of 256 slots compacted in order by a block prefix count, every hit's time and row written by
//                         the whole workgroup, four strips at a time.  The hit count is NOT clamped to max_hits; rows behind it are dropped.
__global__ __launch_bounds__(256) void bps_cond_scan_kernel(BpsConsumeArgs P, BpsCondArgs Q) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= P.nchains * P.cap) return;
    const int64_t chain = w / P.cap;
    const uint64_t e = (uint64_t)(w - chain * P.cap);
    const BpsSlice sl = bps_slice(P, chain);
    if (e < sl.pos || e >= sl.n) return;
    const int64_t d = P.d, slot0 = chain * P.cap;
    const bool first = e == sl.pos;
    const double* const xc = first ? P.cx + chain * d : P.ev_x + (slot0 + (int64_t)e - 1) * d;
    const double* const thc = first ? P.cth + chain * d : P.ev_th + (slot0 + (int64_t)e - 1) * d;
    const double t_c = first ? sl.m.t_cur : P.ev_t[slot0 + (int64_t)e - 1];
    const double t_k = P.ev_t[slot0 + (int64_t)e];
    double pg = 0.0, ph = 0.0;
    for (int64_t k = lane; k < d; k += 64) {
        const double nk = Q.n[k];
        pg += (Q.p[k] - xc[k]) * nk;
        ph += thc[k] * nk;
    }
    const double tau = wave_sum_f64(pg) / wave_sum_f64(ph);
    const bool hit = tau > 0 && t_c + tau < t_k;  // (strict, src/condition.jl:63; false for NaN)
    if (lane == 0) Q.tau[slot0 + (int64_t)e] = hit ? tau : -1.0;
}

template <bool STICKY>
__global__ __launch_bounds__(256) void bps_cond_rows_kernel(BpsConsumeArgs P, BpsCondArgs Q) {
    __shared__ uint32_t s_cnt[256];
    __shared__ uint32_t s_e[256];
    __shared__ double s_tau[256];
    const int tid = threadIdx.x;
    const int64_t chain = blockIdx.x;
    const BpsSlice sl = bps_slice(P, chain);
    if (sl.pos >= sl.n) return;
    const int64_t d = P.d, slot0 = chain * P.cap;
    const BpsConsumeMeta* const meta = static_cast<const BpsConsumeMeta*>(P.meta) + chain * P.nstrips;
    uint64_t nh = Q.nhits[chain];
    for (uint64_t base = sl.pos; base < sl.n; base += 256) {
        const uint64_t e = base + (uint64_t)tid;
        const double tau = e < sl.n ? Q.tau[slot0 + (int64_t)e] : -1.0;
        const bool hit = tau > 0;
        s_cnt[tid] = hit ? 1u : 0u;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {  // inclusive prefix sum
            const uint32_t v = (tid >= off) ? s_cnt[tid - off] : 0u;
            __syncthreads();
            s_cnt[tid] += v;
            __syncthreads();
        }
        if (hit) {
            s_e[s_cnt[tid] - 1u] = (uint32_t)tid;
            s_tau[s_cnt[tid] - 1u] = tau;
        }
        __syncthreads();
        const uint32_t cnt = s_cnt[255];
        for (uint32_t r = 0; r < cnt; ++r) {
            const uint64_t q = nh + r;
            if (q >= (uint64_t)Q.max_hits) break;
            const uint64_t eh = base + s_e[r];
            const double th = s_tau[r];
            const bool first = eh == sl.pos;
            const double* const xc = first ? P.cx + chain * d : P.ev_x + (slot0 + (int64_t)eh - 1) * d;
            const double* const thc = first ? P.cth + chain * d : P.ev_th + (slot0 + (int64_t)eh - 1) * d;
            if (tid == 0) Q.hit_t[chain * Q.max_hits + (int64_t)q] = (first ? sl.m.t_cur : P.ev_t[slot0 + (int64_t)eh - 1]) + th;
            double* const row = Q.hit_x + (chain * Q.max_hits + (int64_t)q) * d;
            for (int64_t j = tid; j < d; j += 256) {
                const bool free = first ? bps_free_bit<STICKY>(meta, j) : bps_free_bit<STICKY>(P.ev_f + (slot0 + (int64_t)eh - 1) * BPS_STICKY_WORDS, j);
                const double x = xc[j];
                row[j] = free ? x + thc[j] * th : x;  // smove_forward!, src/ss_not_fact.jl:78-86
            }
        }
        nh += cnt;
        __syncthreads();
    }
    if (tid == 0) Q.nhits[chain] = nh;
}

int launch_bps_cond(const BpsConsumeArgs& p, const BpsCondArgs& q, void* stream) {
    hipLaunchKernelGGL(bps_cond_scan_kernel, dim3((unsigned)((p.nchains * p.cap + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p, q);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    if (p.ev_f) hipLaunchKernelGGL((bps_cond_rows_kernel<true>), dim3((unsigned)p.nchains), dim3(256), 0, (hipStream_t)stream, p, q);
    else hipLaunchKernelGGL((bps_cond_rows_kernel<false>), dim3((unsigned)p.nchains), dim3(256), 0, (hipStream_t)stream, p, q);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ pair integrals (covariance of a PDMPTrace)
//
// S_ij = ∫ (x_i − c_i)(x_j − c_j) dt over a caller-given set of pairs and J_i = ∫ (x_i − c_i) dt for every coordinate, over [t0, T_last] exactly
// (DESIGN.md "Pair integrals"; tests/ref/pairs_ref.c states the contract).  An event replaces the whole state, so every pair's piece of an event
// (t_k, ...) runs over [t_c, t_k] from the cursor before it: a = x_c,i − c_i, v_i = f_c,i ? θ_c,i : 0 (a coordinate that is not free keeps x).
// One thread per (chain, pair) walks the chain's segment with S in a register; behind the pairs of a chain one thread per coordinate keeps J in the
// same way (so a coordinate in no pair has its J).  The positions and velocities are gathers of the pair's two columns.
//
// Pair integrals of arcs (ARC: the event-recorded Boomerang and its sticky form; DESIGN.md "Pair integrals of arcs"; tests/ref/arc_pairs_ref.c
// states the contract): between two events a free coordinate rotates about μ: on the piece [t_c, t_k] of an event,
// x(s) − z = u·cos s + p·sin s + m with u = x_c − μ, p = θ_c, m = μ − z -- a coordinate that is not free: u = p = 0, m = x_c − z --, so a pair's
// piece is a combination of the five integrals of cos², sin², sin·cos, cos and sin over [0, τ], τ = t_k − t_c signed.  τ is wave-uniform:
// every thread evaluates pdmp_sincos(τ) and the five integrals once per event, without divergence, before its pair arithmetic.
struct BpsPairEvent {
    double t;
    BpsColumn i, j;
};

template <bool STICKY>
__device__ __forceinline__ BpsPairEvent bp_load(const BpsConsumeArgs& P, int64_t s, int64_t i, int64_t j) {
    BpsPairEvent ev;
    ev.t = P.ev_t[s];
    ev.i = bps_column<STICKY>(P, s, i);
    if (j == i) ev.j = ev.i;  // (a diagonal pair, or a J thread: one column)
    else ev.j = bps_column<STICKY>(P, s, j);
    return ev;
}

struct ArcBasis {
    double Icc, Iss, Isc, Ic, Is;
};

__device__ __forceinline__ ArcBasis arc_basis_of(double tau) {
    double s, c;
    pdmp_sincos(tau, &s, &c);
    const double h = s * c;
    ArcBasis b;
    b.Icc = 0.5 * (tau + h);
    b.Iss = 0.5 * (tau - h);
    b.Isc = 0.5 * (s * s);
    b.Ic = s;
    b.Is = c > 0 ? (s * s) / (1.0 + c) : 1.0 - c;  // (1 − cos τ without its cancellation at small τ)
    return b;
}

// symmetric in (i, j) bit for bit: every product commutes, and each sum of two products is one commutative addition
__device__ __forceinline__ double arc_pair_piece(double ui, double pi, double mi, double uj, double pj, double mj, double tau, const ArcBasis& b) {
    return (((ui * uj) * b.Icc + (pi * pj) * b.Iss) + (ui * pj + uj * pi) * b.Isc) +
           ((mi * (uj * b.Ic + pj * b.Is) + mj * (ui * b.Ic + pi * b.Is)) + (mi * mj) * tau);
}
__device__ __forceinline__ double arc_line_piece(double u, double p, double m, double tau, const ArcBasis& b) { return (u * b.Ic + p * b.Is) + m * tau; }

template <bool ARC, bool STICKY>
__global__ __launch_bounds__(256) void bps_pairs_kernel(BpsConsumeArgs P, BpsPairArgs Q, int64_t blocks_per_chain) {
    const int64_t chain = (int64_t)blockIdx.x / blocks_per_chain;
    const int64_t r = ((int64_t)blockIdx.x - chain * blocks_per_chain) * 256 + threadIdx.x;
    const int64_t d = P.d;
    if (r >= Q.npairs + d) return;
    const BpsSlice sl = bps_slice(P, chain);
    if (sl.pos >= sl.n) return;
    const bool is_pair = r < Q.npairs;
    const int64_t i = is_pair ? Q.pi[r] : r - Q.npairs, j = is_pair ? Q.pj[r] : i;
    double* const acc_at = is_pair ? Q.S + chain * Q.npairs + r : Q.J + chain * d + i;
    const int64_t slot0 = chain * P.cap;
    const double mui = ARC ? P.mu[i] : 0.0, muj = ARC ? P.mu[j] : 0.0, ci = Q.center[i], cj = Q.center[j];
    double acc = *acc_at, t_cur = sl.m.t_cur;
    BpsColumn a = bps_cursor<STICKY>(P, chain, i), b = bps_cursor<STICKY>(P, chain, j);

    bps_walk<BpsPairEvent>(
        sl.pos, sl.n, [&](uint64_t e) BPS_WALK_INLINE { return bp_load<STICKY>(P, slot0 + (int64_t)e, i, j); },
        [&](const BpsPairEvent& ev, uint64_t) BPS_WALK_INLINE {
            const double tau = ev.t - t_cur;
            if (ARC) {
                const ArcBasis B = arc_basis_of(tau);
                const double ui = a.f ? a.x - mui : 0.0, pi = a.f ? a.th : 0.0, mi = a.f ? mui - ci : a.x - ci;
                const double uj = b.f ? b.x - muj : 0.0, pj = b.f ? b.th : 0.0, mj = b.f ? muj - cj : b.x - cj;
                acc = acc + (is_pair ? arc_pair_piece(ui, pi, mi, uj, pj, mj, tau, B) : arc_line_piece(ui, pi, mi, tau, B));
            } else {
                const double vi = a.f ? a.th : 0.0, vj = b.f ? b.th : 0.0;
                acc = acc + (is_pair ? pair_piece(a.x - ci, b.x - cj, vi, vj, tau) : line_piece(a.x - ci, vi, tau));
            }
            a = ev.i;
            b = ev.j;
            t_cur = ev.t;
        });
    *acc_at = acc;
}

__global__ __launch_bounds__(256) void bps_tlast_kernel(BpsConsumeArgs P, int64_t chain_first, int64_t n, double* T_out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < n) T_out[q] = static_cast<const BpsConsumeMeta*>(P.meta)[(chain_first + q) * P.nstrips].t_last;
}

int launch_bps_pairs(const BpsConsumeArgs& p, const BpsPairArgs& q, bool arc, void* stream) {
    const int64_t bpc = (q.npairs + p.d + 255) / 256;
    const dim3 grid((unsigned)(p.nchains * bpc)), block(256);
    const bool sticky = p.ev_f != nullptr;
    if (arc && sticky) hipLaunchKernelGGL((bps_pairs_kernel<true, true>), grid, block, 0, (hipStream_t)stream, p, q, bpc);
    else if (arc) hipLaunchKernelGGL((bps_pairs_kernel<true, false>), grid, block, 0, (hipStream_t)stream, p, q, bpc);
    else if (sticky) hipLaunchKernelGGL((bps_pairs_kernel<false, true>), grid, block, 0, (hipStream_t)stream, p, q, bpc);
    else hipLaunchKernelGGL((bps_pairs_kernel<false, false>), grid, block, 0, (hipStream_t)stream, p, q, bpc);
    return (int)hipGetLastError();
}

int launch_bps_tlast(const BpsConsumeArgs& p, int64_t chain_first, int64_t n, double* T_out, void* stream) {
    hipLaunchKernelGGL(bps_tlast_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, chain_first, n, T_out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ marginal histograms (occupation times of a PDMPTrace)
//
// H[s][k + 1] = the time listed coordinate s spends in the bin [e_k, e_k+1) of its own range over [t0, T_last], exactly (DESIGN.md "Marginal
// histograms"; tests/ref/hist_ref.c states the contract; hist_piece_of / hist_piece_at of pdmp_bps_common.hpp are the piece).  An event replaces the
// whole state, so the piece of an event (t_k, ...) is (x_c,i, f_c,i ? θ_c,i : 0, t_k − t_c) from the cursor before it, for every listed coordinate.
// The listed coordinates of a chain lie across the lanes: one thread per (chain, listed coordinate) walks the chain's segment in event order and
// adds each piece to the bins it touches.  A row belongs to one thread, so lanes never share an entry and nothing is atomic; the rest time Z stays
// in a register.  Nothing is open behind the last event: the rows are the result, the pooled read only adds the chains in order.
struct BpsHistEvent {
    double t;
    BpsColumn c;
};

template <bool STICKY>
__device__ __forceinline__ BpsHistEvent bh_load(const BpsConsumeArgs& P, int64_t s, int64_t i) {
    BpsHistEvent ev;
    ev.t = P.ev_t[s];
    ev.c = bps_column<STICKY>(P, s, i);
    return ev;
}

__device__ __forceinline__ HistBins bps_hist_bins(const BpsHistArgs& Q, int64_t s) {
    HistBins bn;
    bn.lo = Q.lo[s];
    bn.hi = Q.hi[s];
    bn.w = Q.w[s];
    bn.B = Q.B;
    return bn;
}

template <bool STICKY>
__global__ __launch_bounds__(256) void bps_hist_kernel(BpsConsumeArgs P, BpsHistArgs Q, int64_t blocks_per_chain) {
    const int64_t chain = (int64_t)blockIdx.x / blocks_per_chain;
    const int64_t s = ((int64_t)blockIdx.x - chain * blocks_per_chain) * 256 + threadIdx.x;
    if (s >= Q.m) return;
    const BpsSlice sl = bps_slice(P, chain);
    if (sl.pos >= sl.n) return;
    const int64_t i = Q.coords[s];
    const HistBins bn = bps_hist_bins(Q, s);
    double* const row = Q.H + (chain * Q.m + s) * (int64_t)(Q.B + 2);
    const int64_t slot0 = chain * P.cap;
    double Z = Q.Z[chain * Q.m + s], t_cur = sl.m.t_cur;
    BpsColumn c = bps_cursor<STICKY>(P, chain, i);

    bps_walk<BpsHistEvent>(
        sl.pos, sl.n, [&](uint64_t e) BPS_WALK_INLINE { return bh_load<STICKY>(P, slot0 + (int64_t)e, i); },
        [&](const BpsHistEvent& ev, uint64_t) BPS_WALK_INLINE {
            const double tau = ev.t - t_cur, v = c.f ? c.th : 0.0;
            const HistPiece p = hist_piece_of(bn, c.x, v, tau);
            for (int k = p.k0; k <= p.k1; ++k) row[k + 1] = row[k + 1] + hist_piece_at(bn, p, k);
            Z = Z + hist_piece_rest(v, tau);
            c = ev.c;
            t_cur = ev.t;
        });
    Q.Z[chain * Q.m + s] = Z;
}

__global__ __launch_bounds__(256) void bps_hist_pool_kernel(BpsHistArgs Q, int64_t chain_first, int64_t n, double* out_H, double* out_Z) {
    const int64_t len = Q.m * (int64_t)(Q.B + 2);
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= len + Q.m) return;
    const bool is_h = k < len;
    const double* const src = is_h ? Q.H + chain_first * len + k : Q.Z + chain_first * Q.m + (k - len);
    const int64_t stride = is_h ? len : Q.m;
    double acc = 0.0;
    for (int64_t c = 0; c < n; ++c) acc = acc + src[c * stride];
    if (is_h) out_H[k] = acc;
    else out_Z[k - len] = acc;
}

int launch_bps_hist(const BpsConsumeArgs& p, const BpsHistArgs& q, void* stream) {
    const int64_t bpc = (q.m + 255) / 256;
    const dim3 grid((unsigned)(p.nchains * bpc)), block(256);
    if (p.ev_f) hipLaunchKernelGGL((bps_hist_kernel<true>), grid, block, 0, (hipStream_t)stream, p, q, bpc);
    else hipLaunchKernelGGL((bps_hist_kernel<false>), grid, block, 0, (hipStream_t)stream, p, q, bpc);
    return (int)hipGetLastError();
}

int launch_bps_hist_pool(const BpsHistArgs& q, int64_t chain_first, int64_t n, double* out_H, double* out_Z, void* stream) {
    const int64_t tot = q.m * (int64_t)(q.B + 3);
    hipLaunchKernelGGL(bps_hist_pool_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q, chain_first, n, out_H, out_Z);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ marginal histograms of arcs (a Boomerang's trace)
//
// The same rows H and rest times Z for the event-recorded Boomerang and its sticky form (DESIGN.md "Marginal histograms of arcs";
// tests/ref/arc_hist_ref.c states the contract).  Between two events a free coordinate is x(s) = μ + R·cos(ψ0 + s) with u = x_c − μ, p = θ_c,
// R = sqrt(u·u + p·p), ψ0 = −atan2(p, u); the time it spends below a level y is W(ψ0 + τ) − W(ψ0) with W(ψ) = n·L + clamp(r − α, 0, L),
// α = acos((y − μ)/R), L = 2π − 2α, ψ = 2π·n + r; a bin's time the difference of its two edges' values.  A coordinate that is not free, or with
// R == 0, is at rest and adds τ to the slot of x_c and to Z.
//
// One WAVEFRONT per (chain, listed coordinate), four to a workgroup: R, ψ0, ψ1 and their turns are uniform over it, the edges lie across the
// lanes, every lane evaluates `below` at its own edge and takes its lower neighbour's value through a lane shuffle.  With bins + 2 <= 128 lane l
// owns the slots l and l + 64 of the row IN REGISTERS for the whole slice (one load before, one store behind); a longer row is added to in
// global memory, 64 slots at a time, slot j always by lane j & 63 (a piece at rest too: one owning lane per slot on either path), slots with
// nothing to add skipped (x + 0.0 has the bits of x: no entry is ever −0.0).  Each slot is added
// to in the event order of its chain from the value in memory and nothing is atomic, so the bits do not depend on the slicing.  All of a
// wavefront's event loads are uniform.
struct ArcPiece {
    double tau, mu, R, n0, r0, n1, r1;
    bool live, rest;
    int krest;
};
constexpr double ARC_TWO_PI = 6.28318530717958623200e+00;  // 2π as ONE double constant

__device__ __forceinline__ ArcPiece arc_piece_of(const HistBins& bn, double xc, double thc, bool is_free, double mu, double tau) {
    ArcPiece a;
    a.tau = tau;
    a.mu = mu;
    a.R = a.n0 = a.r0 = a.n1 = a.r1 = 0.0;
    a.live = tau > 0.0;
    a.rest = true;
    a.krest = 0;
    if (!a.live) return a;
    const double u = xc - mu, p = thc;
    a.R = is_free ? PDMP_SQRT(u * u + p * p) : 0.0;
    if (a.R == 0.0) {
        a.krest = hist_bin_of(bn, xc);
        return a;
    }
    a.rest = false;
    const double psi0 = -pdmp_atan2(p, u), psi1 = psi0 + tau;
    a.n0 = floor(psi0 / ARC_TWO_PI);
    a.r0 = psi0 - ARC_TWO_PI * a.n0;
    a.n1 = floor(psi1 / ARC_TWO_PI);
    a.r1 = psi1 - ARC_TWO_PI * a.n1;
    return a;
}
__device__ __forceinline__ double arc_w(double n, double r, double alpha, double L) {
    const double v = r - alpha;
    return n * L + (v < 0.0 ? 0.0 : (v > L ? L : v));
}
// the time the arc spends below the level y (y = ±∞ included: 0 and τ exactly)
__device__ __forceinline__ double arc_below(const ArcPiece& a, double y) {
    const double z = (y - a.mu) / a.R;
    if (z >= 1.0) return a.tau;
    if (z <= -1.0) return 0.0;
    const double alpha = pdmp_acos(z);
    const double L = ARC_TWO_PI - 2.0 * alpha;
    return arc_w(a.n1, a.r1, alpha, L) - arc_w(a.n0, a.r0, alpha, L);
}
// lane l's value of lane l − 1 (lane 0: of lane 63)
__device__ __forceinline__ double arc_from_below(double v, int lane) { return __shfl(v, (lane + 63) & 63, 64); }

template <bool STICKY, bool LONG_ROW>
__global__ __launch_bounds__(256) void bps_arc_hist_kernel(BpsConsumeArgs P, BpsHistArgs Q, int64_t blocks_per_chain) {
    const int64_t chain = (int64_t)blockIdx.x / blocks_per_chain;
    const int lane = (int)(threadIdx.x & 63);
    const int64_t s = ((int64_t)blockIdx.x - chain * blocks_per_chain) * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (s >= Q.m) return;
    const BpsSlice sl = bps_slice(P, chain);
    if (sl.pos >= sl.n) return;
    const int64_t i = Q.coords[s];
    const HistBins bn = bps_hist_bins(Q, s);
    const int slots = Q.B + 2;
    double* const row = Q.H + (chain * Q.m + s) * (int64_t)slots;
    const int64_t slot0 = chain * P.cap;
    const double mu = P.mu[i];
    double Z = Q.Z[chain * Q.m + s], t_cur = sl.m.t_cur;
    BpsColumn c = bps_cursor<STICKY>(P, chain, i);

    // (the short row: slot j holds the time in [e_j−1, e_j); lane l owns j = l and j = l + 64 and evaluates their upper edges)
    const bool two = !LONG_ROW && slots > 64, own0 = lane < slots, own1 = lane + 64 < slots;
    const double y0 = hist_edge(bn, lane), y1 = hist_edge(bn, lane + 64);
    double h0 = (!LONG_ROW && own0) ? row[lane] : 0.0, h1 = (!LONG_ROW && own1) ? row[lane + 64] : 0.0;

    bps_walk<BpsHistEvent>(
        sl.pos, sl.n, [&](uint64_t e) BPS_WALK_INLINE { return bh_load<STICKY>(P, slot0 + (int64_t)e, i); },
        [&](const BpsHistEvent& ev, uint64_t) BPS_WALK_INLINE {
            const ArcPiece a = arc_piece_of(bn, c.x, c.th, c.f, mu, ev.t - t_cur);  // (uniform over the wavefront, and so is every branch on it)
            if (a.live && a.rest) {
                const int j = a.krest + 1;
                if (LONG_ROW) {
                    if ((j & 63) == lane) row[j] = row[j] + a.tau;  // (the lane that owns slot j in the arc walk below)
                } else {
                    if (j == lane) h0 = h0 + a.tau;
                    if (j == lane + 64) h1 = h1 + a.tau;
                }
                Z = Z + a.tau;
            } else if (a.live && !LONG_ROW) {
                const double b0 = arc_below(a, y0), b1 = two ? arc_below(a, y1) : a.tau;
                const double p0 = arc_from_below(b0, lane), p1 = arc_from_below(b1, lane);
                const double o0 = b0 - (lane == 0 ? 0.0 : p0), o1 = b1 - (lane == 0 ? p0 : p1);
                h0 = h0 + (o0 > 0.0 ? o0 : 0.0);
                h1 = h1 + (o1 > 0.0 ? o1 : 0.0);
            } else if (a.live) {
                double carry = 0.0;  // (below e_−1 = −∞)
                for (int j0 = 0; j0 < slots; j0 += 64) {
                    const int j = j0 + lane;
                    const double b = arc_below(a, hist_edge(bn, j));
                    const double pb = arc_from_below(b, lane);
                    const double o = b - (lane == 0 ? carry : pb);
                    carry = __shfl(b, 63, 64);
                    if (j < slots && o > 0.0) row[j] = row[j] + o;
                }
            }
            c = ev.c;
            t_cur = ev.t;
        });
    if (!LONG_ROW) {
        if (own0) row[lane] = h0;
        if (own1) row[lane + 64] = h1;
    }
    if (lane == 0) Q.Z[chain * Q.m + s] = Z;
}

int launch_bps_arc_hist(const BpsConsumeArgs& p, const BpsHistArgs& q, void* stream) {
    const int64_t bpc = (q.m + 3) / 4;
    const dim3 grid((unsigned)(p.nchains * bpc)), block(256);
    const bool sticky = p.ev_f != nullptr, long_row = q.B + 2 > 128;
    if (sticky && long_row) hipLaunchKernelGGL((bps_arc_hist_kernel<true, true>), grid, block, 0, (hipStream_t)stream, p, q, bpc);
    else if (sticky) hipLaunchKernelGGL((bps_arc_hist_kernel<true, false>), grid, block, 0, (hipStream_t)stream, p, q, bpc);
    else if (long_row) hipLaunchKernelGGL((bps_arc_hist_kernel<false, true>), grid, block, 0, (hipStream_t)stream, p, q, bpc);
    else hipLaunchKernelGGL((bps_arc_hist_kernel<false, false>), grid, block, 0, (hipStream_t)stream, p, q, bpc);
    return (int)hipGetLastError();
}

}  // namespace pdmp
