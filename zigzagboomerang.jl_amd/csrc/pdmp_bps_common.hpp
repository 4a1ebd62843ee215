// pdmp_bps_common.hpp -- the wave-level machinery of the Bouncy Particle family, written ONCE for its three event loops and three init
// kernels: bps_run_kernel / bps_init_kernel (pdmp_bps.hip), bps_sticky_* (pdmp_bps_sticky.inc) and bps_modern_* (pdmp_bps_modern.inc).
//
// The layout they share: one chain per wavefront, the d-vectors in REGISTERS (element e = slot*64 + lane, NS slots per lane), one [d] staging
// buffer `tmp` in LDS.  A workgroup is one wavefront: DS operations retire in order, so a step sees the previous step's LDS writes without a
// barrier; the `asm volatile("" ::: "memory")` fences only keep the COMPILER from moving LDS accesses across them.
// Every sum has ONE fixed order, the one oracle/pdmp_oracle.c restates: per-lane partial sums over the slots in order, then wave_sum_f64.
//
// The split: what is here is the same for every kernel of the family.  A kernel keeps its loop, its rate and bound, its moves, and every
// loop whose body is its own (the register-only Γ arms, the sticky sums with their θ == 0 test, the diagonal-U forms).
#pragma once

#include <type_traits>

#include "pdmp_device.hpp"
#include "pdmp_engine.hpp"

namespace pdmp {

// all-lanes sum in the oracle's order (dot_wave64): xor 1, 2 (quads), 4, 8 (row of 16), then (r0+r1)+(r2+r3)
__device__ __forceinline__ double wave_sum_f64(double v) {
    v = v + dpp_f64<0xB1>(v);   // lane ^ 1
    v = v + dpp_f64<0x4E>(v);   // lane ^ 2
    v = v + dpp_f64<0x141>(v);  // other quad of the half row (same value in every lane of a quad: == lane ^ 4)
    v = v + dpp_f64<0x140>(v);  // other half row (== lane ^ 8)
    const double r0 = readlane_f64(v, 0), r1 = readlane_f64(v, 16), r2 = readlane_f64(v, 32), r3 = readlane_f64(v, 48);
    return (r0 + r1) + (r2 + r3);  // lane ^ 16, then lane ^ 32
}

// the pair consumers' piece (pdmp_consume.hip, pdmp_consume_bps.hip; tests/ref/pairs_ref.c states it): ∫_0^τ (a + vi u)(b + vj u) du and
// ∫_0^τ (a + vi u) du in ONE grouping, symmetric in (i, j) bit for bit (every product and the one sum of two products commute)
__device__ __forceinline__ double pair_piece(double a, double b, double vi, double vj, double tau) {
    return tau * (a * b + tau * (0.5 * (a * vj + b * vi) + tau * ((vi * vj) / 3.0)));
}
__device__ __forceinline__ double line_piece(double a, double vi, double tau) { return tau * (a + 0.5 * (vi * tau)); }

// the histogram consumers' bins and piece (pdmp_consume.hip, pdmp_consume_bps.hip; tests/ref/hist_ref.c states them): B bins on [lo, hi) of width
// w = (hi − lo) / B, the edges e_−1 = −∞, e_0 = lo, e_k = lo + w·k, e_B = hi, e_B+1 = +∞; slot k + 1 of a row holds the time in [e_k, e_k+1)
struct HistBins {
    double lo, hi, w;
    int B;
};
__device__ __forceinline__ double hist_edge(const HistBins& b, int k) {
    if (k <= 0) return k < 0 ? -__builtin_inf() : b.lo;
    if (k >= b.B) return k > b.B ? __builtin_inf() : b.hi;
    return b.lo + b.w * (double)k;
}
// the k in {−1, ..., B} with e_k <= x < e_k+1 against the computed edges: a floor, then one step where rounding put it on the wrong side
// (always inside [−1, B], whatever x is: the row has B + 2 slots)
__device__ __forceinline__ int hist_bin_of(const HistBins& b, double x) {
    if (!(x >= b.lo)) return -1;
    if (x >= b.hi) return b.B;
    const double q = floor((x - b.lo) / b.w);
    int k = q < (double)(b.B - 1) ? (int)q : b.B - 1;
    if (x < hist_edge(b, k)) k -= 1;
    else if (x >= hist_edge(b, k + 1)) k += 1;
    return k;
}
// a piece (a, v, τ) made ready: the ends of the interval it sweeps, the time per unit length r, the bins k0 .. k1 it touches.  At rest
// (v == 0, or a + v·τ == a): xl == xh, r = τ, one bin.  τ <= 0 adds nothing: k0 > k1.
struct HistPiece {
    double xl, xh, r;
    int k0, k1;
};
__device__ __forceinline__ HistPiece hist_piece_of(const HistBins& bn, double a, double v, double tau) {
    HistPiece p;
    p.xl = p.xh = a;
    p.r = tau;
    p.k0 = 0;
    p.k1 = -1;
    if (!(tau > 0.0)) return p;
    const double b = a + v * tau;
    if (v == 0.0 || b == a) {
        p.k0 = p.k1 = hist_bin_of(bn, a);
        return p;
    }
    p.xl = a < b ? a : b;
    p.xh = a < b ? b : a;
    p.r = tau / (p.xh - p.xl);
    p.k0 = hist_bin_of(bn, p.xl);
    p.k1 = hist_bin_of(bn, p.xh);
    return p;
}
// THE function of (piece, k): the time the piece spends in [e_k, e_k+1), k in −1 .. B; the accumulation and the reads both call it
__device__ __forceinline__ double hist_piece_at(const HistBins& bn, const HistPiece& p, int k) {
    if (k < p.k0 || k > p.k1) return 0.0;
    if (p.xl == p.xh) return p.r;
    const double e0 = hist_edge(bn, k), e1 = hist_edge(bn, k + 1);
    const double o = (p.xh < e1 ? p.xh : e1) - (p.xl > e0 ? p.xl : e0);
    return o > 0.0 ? o * p.r : 0.0;
}
__device__ __forceinline__ double hist_piece_rest(double v, double tau) { return (tau > 0.0 && v == 0.0) ? tau : 0.0; }

// draw indices a randn(rng, d) takes (BpsWave::normals): one Box-Muller block per two elements, whole 64-lane rows of blocks
__device__ __forceinline__ uint64_t normal_draws(int64_t d) { return (uint64_t)(((d + 127) >> 7) << 6); }

// (the status gate of every event loop: chain_ended, pdmp_device.hpp)
__device__ __forceinline__ bool bps_chain_ended(uint32_t status) { return chain_ended(status); }

// the header counters an event loop advances, in registers from its first line to its last
struct BpsCounters {
    uint64_t num, nacc, nrefresh, ntrace, nevents, nm;  // nm: next draw index of PDMP_STREAM_MAIN
    __device__ __forceinline__ void load(const DevChain* hdr) {
        nm = hdr->c.ndraw_main;
        num = hdr->c.num, nacc = hdr->c.nacc, nrefresh = hdr->c.nrefresh, ntrace = hdr->c.ntrace, nevents = hdr->c.nevents;
    }
    __device__ __forceinline__ void store(DevChain* hdr, double t, uint32_t status) const {  // (one lane calls it)
        hdr->c.t_last = t;
        hdr->t_event = t;
        hdr->c.num = num;
        hdr->c.nacc = nacc;
        hdr->c.nrefresh = nrefresh;
        hdr->c.ntrace = ntrace;
        hdr->c.nevents = nevents;
        hdr->c.ndraw_main = nm;
        hdr->c.status = status;
    }
};

// scal[0..5] = {t, a, b, t′, τref, c} of a chain (one lane calls it); what slots 6 and 7 mean is the kernel's own
__device__ __forceinline__ void store_scal6(double* sc, double t, double a, double b, double tp, double tau_ref, double c) {
    sc[0] = t;
    sc[1] = a;
    sc[2] = b;
    sc[3] = tp;
    sc[4] = tau_ref;
    sc[5] = c;
}

// FULL: d == 64 NS exactly, so the `element < d` guards (and their exec-mask bookkeeping) are compile-time true.
template <int NS, bool FULL = false>
struct BpsWave {
    int lane;
    int64_t d;
    double* tmp;  // LDS, [d]: operand of the CSC gather, the normals of a refresh, the vector of the substitutions

    __device__ __forceinline__ int64_t elem(int s) const { return (int64_t)s * 64 + lane; }
    __device__ __forceinline__ bool has(int s) const { return FULL || elem(s) < d; }

    // f(s, e) for every element of the lane, slots in order (stores of several vectors keep their per-element order)
    template <class F>
    __device__ __forceinline__ void each(F&& f) const {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (has(s)) f(s, elem(s));
        }
    }
    // the chain's x and θ into registers (0 in the padding; the two loads of a slot stay together)
    __device__ __forceinline__ void load_state(const double* gx, const double* gth, double (&x)[NS], double (&th)[NS]) const {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            x[s] = has(s) ? gx[elem(s)] : 0.0;
            th[s] = has(s) ? gth[elem(s)] : 0.0;
        }
    }
    __device__ __forceinline__ double dot(const double (&u)[NS], const double (&v)[NS]) const {
        double part = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (has(s)) part += u[s] * v[s];
        }
        return wave_sum_f64(part);
    }
    // dx = x − μ_flow (0 in the padding): the Boomerang's bound (src/not_fact_samplers.jl:34-36) and grad_correct! (:9-12)
    __device__ __forceinline__ void sub_mu_flow(const double (&x)[NS], const double* mu_flow, double (&dx)[NS]) const {
#pragma unroll
        for (int s = 0; s < NS; ++s) dx[s] = has(s) ? (x[s] - mu_flow[elem(s)]) : 0.0;
    }

    // y = A v with v = in (− mu if sub_mu), A in CSC: the operand is staged in LDS, then one idot (src/common.jl:16-24) per output
    // element, ascending row order.  The caller chooses whose A and μ (the flow's, or the ensemble's own target's).
    __device__ __forceinline__ void stage(const double (&in)[NS], const double* mu, bool sub_mu) const {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (has(s)) tmp[elem(s)] = sub_mu ? (in[s] - mu[elem(s)]) : in[s];
        }
        asm volatile("" ::: "memory");
    }
    __device__ __forceinline__ double idot(const int64_t* cp, const int64_t* rv, const double* nz, int64_t e) const {
        double y = 0.0;
        for (int64_t p = cp[e]; p < cp[e + 1]; ++p) y += nz[p] * tmp[rv[p]];
        return y;
    }
    __device__ __forceinline__ void gather(const int64_t* cp, const int64_t* rv, const double* nz, double (&out)[NS]) const {
#pragma unroll
        for (int s = 0; s < NS; ++s) out[s] = has(s) ? idot(cp, rv, nz, elem(s)) : 0.0;
    }
    __device__ __forceinline__ void csc_gather(const int64_t* cp, const int64_t* rv, const double* nz, const double* mu, const double (&in)[NS],
                                               bool sub_mu, double (&out)[NS]) const {
        stage(in, mu, sub_mu);
        gather(cp, rv, nz, out);
    }

    // tmp <- L \ tmp and tmp <- L' \ tmp: column-oriented substitution (one column per step, its off-diagonal entries one per lane), every
    // element updated in the order of the columns -- exactly tri_solve_lower / tri_solve_upper of the oracle.
    __device__ __forceinline__ void solve_lower(const BpsRunParams& P) const {
        for (int64_t j = 0; j < d; ++j) {
            asm volatile("" ::: "memory");
            const int32_t p0 = P.Lcp[j], p1 = P.Lcp[j + 1];
            const double yj = tmp[j] / P.Lnz[p0];
            asm volatile("" ::: "memory");
            if (lane == 0) tmp[j] = yj;
            for (int32_t p = p0 + 1 + lane; p < p1; p += 64) {
                const int32_t r = P.Lrv[p];
                tmp[r] = tmp[r] - P.Lnz[p] * yj;
            }
        }
        asm volatile("" ::: "memory");
    }
    __device__ __forceinline__ void solve_upper(const BpsRunParams& P) const {
        for (int64_t j = d - 1; j >= 0; --j) {
            asm volatile("" ::: "memory");
            const int32_t p0 = P.Ucp[j], p1 = P.Ucp[j + 1] - 1;
            const double zj = tmp[j] / P.Unz[p1];
            asm volatile("" ::: "memory");
            if (lane == 0) tmp[j] = zj;
            for (int32_t p = p0 + lane; p < p1; p += 64) {
                const int32_t r = P.Urv[p];
                tmp[r] = tmp[r] - P.Unz[p] * zj;
            }
        }
        asm volatile("" ::: "memory");
    }

    // tmp <- randn(rng, d), draws nm .. nm + normal_draws(d) - 1: element 128a + 64b + lane is Box-Muller branch b of block nm + 64a + lane
    // (one evaluation serves two slots).  The normals go through LDS so that a ROLLED loop holds ONE Box-Muller body, its constants and
    // temporaries live only here; the caller's unrolled update reads them back.  NS inlined bodies, or a call, cost tens of VGPRs across
    // the whole event loop.
    __device__ __forceinline__ void normals(uint64_t seed, uint64_t nm) const {
        asm volatile("" ::: "memory");
#pragma unroll 1
        for (int a2 = 0; a2 < (NS + 1) / 2; ++a2) {
            const int64_t e0 = (int64_t)a2 * 128 + lane, e1 = e0 + 64;
            double z0, z1;
            pdmp_randn2(seed, PDMP_STREAM_MAIN, nm + (uint64_t)(a2 * 64 + lane), &z0, &z1);
            if (FULL || e0 < d) tmp[e0] = z0;
            if (FULL || e1 < d) tmp[e1] = z1;
        }
        asm volatile("" ::: "memory");
    }

    // push!(Ξ, (t, copy(x), copy(θ))) as record `ntrace` of the chain's segment (src/not_fact_samplers.jl:39-41): a coalesced
    // 8(2d+1)-byte record; nothing where the ensemble keeps no trace
    __device__ __forceinline__ void emit_record(const BpsRunParams& P, int64_t chain, uint64_t ntrace, double t, const double (&x)[NS],
                                                const double (&th)[NS]) const {
        if (P.trace_cap > 0) {
            const int64_t slot = chain * P.trace_cap + (int64_t)ntrace;
            if (lane == 0) P.ev_t[slot] = t;
            double* ex = P.ev_x + slot * d;
            double* eth = P.ev_th + slot * d;
            each([&](int s, int64_t e) {
                ex[e] = x[s];
                eth[e] = th[s];
            });
        }
    }
};

// f(std::integral_constant<int, NS>) for the smallest compiled slot count NS (1, 2, 4, ... up to MAXNS) with d <= 64 NS; -1 past MAXNS
template <int MAXNS, class F>
static int bps_dispatch_ns(int64_t d, F&& f) {
    const int64_t ns = (d + 63) / 64;
    if (ns <= 1) return f(std::integral_constant<int, 1>{});
    if (ns <= 2) return f(std::integral_constant<int, 2>{});
    if (ns <= 4) return f(std::integral_constant<int, 4>{});
    if (ns <= 8) return f(std::integral_constant<int, 8>{});
    if (ns <= 16) return f(std::integral_constant<int, 16>{});
    if constexpr (MAXNS >= 64) {
        if (ns <= 32) return f(std::integral_constant<int, 32>{});
        if (ns <= 64) return f(std::integral_constant<int, 64>{});
    }
    return -1;
}

}  // namespace pdmp
