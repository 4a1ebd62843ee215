// pdmp_device.hpp -- the device helpers every event-loop translation unit shares: the contract scalars of the reference (pos, sigmoid,
// poisson_time) and the lane / wave primitives of a 64-lane wavefront.  Device code only, each function defined ONCE; a unit keeps what
// is truly its own.  pdmp_debug_math_eval probes the scalars inside every unit that calls them (include/pdmp_debug.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/pdmp_detmath.h"
#include "../../include/pdmp_mi355.h"  // (the PDMP_CHAIN_* status words)

#define PDMP_INF __builtin_inf()

// Cross-lane hand-off through LDS inside ONE wavefront: DS operations execute in issue order, so no s_barrier
// and no s_waitcnt vmcnt(0) is needed -- but the COMPILER must be told that memory changed behind the thread's
// back (otherwise it may forward a lane's own earlier store to its later load of the same slot).
#define PDMP_LDS_ORDER()                 \
    do {                                 \
        __builtin_amdgcn_wave_barrier(); \
        asm volatile("" ::: "memory");   \
    } while (0)

namespace pdmp {

// ------------------------------------------------------------------------------------------ lane helpers

__device__ __forceinline__ double readlane_f64(double v, int srclane) {
    int lo = __builtin_amdgcn_readlane(__double2loint(v), srclane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), srclane);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ uint32_t readlane_u32(uint32_t v, int srclane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, srclane);
}
__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ double uniform_f64(double v) {
    int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
// value of lane `src` (any lane, per-lane choice): two ds_bpermute_b32
__device__ __forceinline__ double bperm_f64(double v, uint32_t src) {
    const int lo = __builtin_amdgcn_ds_bpermute((int)(src << 2), __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute((int)(src << 2), __double2hiint(v));
    return __hiloint2double(hi, lo);
}

// DPP move of both halves.  The control codes used here and in the units:
//   0xB1 quad_perm [1,0,3,2] (lane ^ 1)    0x4E quad_perm [2,3,0,1] (lane ^ 2)    0x141 row_half_mirror    0x140 row_mirror
//   0x111 .. 0x11F row_shr 1 .. 15         0x142 row_bcast:15 (row r takes lane 15 of row r-1)      0x143 row_bcast:31 (rows 2, 3 take lane 31)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);  // every lane has a valid source: no tied `old` operand, no copies
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t umin3(uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t ab = (a < b) ? a : b;
    return (ab < c) ? ab : c;  // v_min3_u32
}

// One v_min_f64.  Written as the instruction itself: fmin() of a value that came out of a load or a DPP move is preceded by a
// canonicalising v_max_f64 x, x per operand (IEEE-mode minnum lowering), i.e. three DP instructions per minimum in the queue
// reductions.  Keys are never NaN unless a chain has diverged; v_min_f64 then returns the other operand (NaN loses, as +Inf).
__device__ __forceinline__ double min_f64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double max_f64(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// ------------------------------------------------------------------------------------------ wave reductions and scans

// Minimum over the 64 lanes, returned wave-uniform.  4 DPP steps inside each row of 16 lanes (quad xor-1, quad xor-2, half-row
// mirror, row mirror), then row_bcast:15 (row r takes lane 15 of row r-1) and row_bcast:31 (rows 2, 3 take lane 31): lane 63 ends
// with the minimum of the four rows.  Lanes that have no source read 0 and hold garbage afterwards; only lane 63 is read.
__device__ __forceinline__ double wave_min_f64(double v) {
    v = min_f64(v, dpp_f64<0xB1>(v));   // quad_perm [1,0,3,2]
    v = min_f64(v, dpp_f64<0x4E>(v));   // quad_perm [2,3,0,1]
    v = min_f64(v, dpp_f64<0x141>(v));  // row_half_mirror
    v = min_f64(v, dpp_f64<0x140>(v));  // row_mirror
    v = min_f64(v, dpp_f64<0x142>(v));  // row_bcast:15
    v = min_f64(v, dpp_f64<0x143>(v));  // row_bcast:31
    return readlane_f64(v, 63);
}
// minimum over the 8 lanes of a group, returned in every lane of the group
__device__ __forceinline__ double grp8_min_f64(double v) {
    v = min_f64(v, dpp_f64<0xB1>(v));
    v = min_f64(v, dpp_f64<0x4E>(v));
    v = min_f64(v, dpp_f64<0x141>(v));  // row_half_mirror: reverses each half row
    return v;
}
// minimum over the 16 lanes of a DPP row, returned in every lane of the row
__device__ __forceinline__ double row_min_f64(double v) {
    v = min_f64(v, dpp_f64<0xB1>(v));
    v = min_f64(v, dpp_f64<0x4E>(v));
    v = min_f64(v, dpp_f64<0x141>(v));
    v = min_f64(v, dpp_f64<0x140>(v));
    return v;
}
// Minimum of a u32 over the 64 lanes, wave-uniform: the __shfl_xor form of pdmp_kernels.hip's older kernels ...
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    for (int off = 32; off >= 1; off >>= 1) {
        uint32_t o = (uint32_t)__shfl_xor((int)v, off, 64);
        v = (o < v) ? o : v;
    }
    return uniform_u32(v);
}
// ... and the same six steps as wave_min_f64 (DPP: on the vector unit instead of six ds_bpermute round trips) of the tracked kernels
__device__ __forceinline__ uint32_t wave_min_u32_dpp(uint32_t v) {
    auto step = [](uint32_t x, auto ctrl) -> uint32_t {
        const uint32_t o = (uint32_t)__builtin_amdgcn_mov_dpp((int)x, decltype(ctrl)::value, 0xf, 0xf, true);
        return (o < x) ? o : x;
    };
    v = step(v, std::integral_constant<int, 0xB1>{});
    v = step(v, std::integral_constant<int, 0x4E>{});
    v = step(v, std::integral_constant<int, 0x141>{});
    v = step(v, std::integral_constant<int, 0x140>{});
    // (row_bcast: lanes that receive nothing read 0 and are not used: the result is lane 63's)
    v = step(v, std::integral_constant<int, 0x142>{});
    v = step(v, std::integral_constant<int, 0x143>{});
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// DPP prefix operations over the 64 lanes (row_shr 1, 2, 3 of the input, then row_shr 4 / 8 of the partial result inside the enabled banks,
// then row_bcast 15 / 31 across the rows): lanes without a source keep the identity.
template <int CTRL, int ROWM, int BANKM>
__device__ __forceinline__ uint32_t dpp_id_u32(uint32_t identity, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)src, CTRL, ROWM, BANKM, false);
}
__device__ __forceinline__ uint32_t scan_add_u32(uint32_t v) {  // inclusive
    uint32_t x = v;
    x += dpp_id_u32<0x111, 0xf, 0xf>(0u, v);
    x += dpp_id_u32<0x112, 0xf, 0xf>(0u, v);
    x += dpp_id_u32<0x113, 0xf, 0xf>(0u, v);
    x += dpp_id_u32<0x114, 0xf, 0xe>(0u, x);
    x += dpp_id_u32<0x118, 0xf, 0xc>(0u, x);
    x += dpp_id_u32<0x142, 0xa, 0xf>(0u, x);
    x += dpp_id_u32<0x143, 0xc, 0xf>(0u, x);
    return x;
}
template <int CTRL, int ROWM, int BANKM>
__device__ __forceinline__ double dpp_inf(double src) {  // (identity +Inf)
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(src), CTRL, ROWM, BANKM, false);
    const int hi = __builtin_amdgcn_update_dpp(0x7FF00000, __double2hiint(src), CTRL, ROWM, BANKM, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double scan_min_f64(double v) {  // inclusive
    double x = v;
    x = min_f64(x, dpp_inf<0x111, 0xf, 0xf>(v));
    x = min_f64(x, dpp_inf<0x112, 0xf, 0xf>(v));
    x = min_f64(x, dpp_inf<0x113, 0xf, 0xf>(v));
    x = min_f64(x, dpp_inf<0x114, 0xf, 0xe>(x));
    x = min_f64(x, dpp_inf<0x118, 0xf, 0xc>(x));
    x = min_f64(x, dpp_inf<0x142, 0xa, 0xf>(x));
    x = min_f64(x, dpp_inf<0x143, 0xc, 0xf>(x));
    return x;
}

// ------------------------------------------------------------------------------------------ two-level queue

// Level-1 entry (block minimum, argmin) of the block of coordinate j after keys[j] became kj: smaller than the entry -> replace;
// j WAS the entry and grew -> rescan the 64 keys of the block (lowest index on ties); otherwise nothing to do.
__device__ __forceinline__ void level1_update(double* bk, uint32_t* bi, const double* keys, int lane, uint32_t j, double kj) {
    const uint32_t bj = j >> 6;
    PDMP_LDS_ORDER();
    const double cur = bk[bj];
    const uint32_t ci = bi[bj];
    if (kj < cur || (kj == cur && j < ci)) {
        if (lane == 0) {
            bk[bj] = kj;
            bi[bj] = j;
        }
    } else if (ci == j) {
        const double kv = __hip_atomic_load(keys + (size_t)bj * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double mn = wave_min_f64(kv);
        const uint64_t bl = __ballot(kv == mn);
        const int arg = bl ? (__ffsll((unsigned long long)bl) - 1) : 0;
        if (lane == 0) {
            bk[bj] = mn;
            bi[bj] = bj * 64 + (uint32_t)arg;
        }
    }
}

// Level 1 from the keys in HBM, at the start of a launch: (min, argmin) of each 64-key block, lowest index on ties.  Each lane scans
// whole blocks; the caller orders LDS (PDMP_LDS_ORDER) before it reads the entries.
__device__ __forceinline__ void level1_build(double* bk, uint32_t* bi, const double* keys, uint32_t nblk, int lane) {
    for (uint32_t b = lane; b < nblk; b += 64) {
        const double* kp = keys + (size_t)b * 64;
        double mk = kp[0];
        uint32_t mi = 0;
#pragma unroll 8
        for (int q = 1; q < 64; ++q) {
            const double v = kp[q];
            if (v < mk) {
                mk = v;
                mi = q;
            }
        }
        bk[b] = mk;
        bi[b] = b * 64 + mi;
    }
}

// ------------------------------------------------------------------------------------------ launch prologue

// a chain that ended for good (the reference's error(...), or no finite next event) is not run again
__device__ __forceinline__ bool chain_ended(uint32_t status) {
    return status == PDMP_CHAIN_BOUND_VIOLATED || status == PDMP_CHAIN_STALLED;
}
// events a launch may still record: the room left in the chain's trace (trace_cap == 0: no trace, no limit)
__device__ __forceinline__ uint32_t launch_trace_room(int64_t trace_cap, uint64_t ntrace0) {
    return (trace_cap > 0) ? (uint32_t)(((uint64_t)trace_cap > ntrace0) ? ((uint64_t)trace_cap - ntrace0) : 0) : 0xffffffffu;
}

// ------------------------------------------------------------------------------------------ neighbourhood blob

// Word 0 of a coordinate's blob (built on the host, pdmp_capi_zigzag.hip): k = |G1[i]|, m = |S[i]|, self = the position of i inside
// S[i], kjmax = max |G1[j]| over j in G1[i], one byte each.
struct BlobHeader {
    int k, m, self, kjmax;
};
__device__ __forceinline__ BlobHeader blob_header(uint64_t hw) {
    BlobHeader h;
    h.k = (int)(hw & 0xff);
    h.m = (int)((hw >> 8) & 0xff);
    h.self = (int)((hw >> 16) & 0xff);
    h.kjmax = (int)((hw >> 24) & 0xff);
    return h;
}
// the same, wave-uniform (a kernel whose whole wave works on one event)
__device__ __forceinline__ BlobHeader blob_header_uniform(uint64_t hw) {
    BlobHeader h;
    h.k = (int)uniform_u32((uint32_t)(hw & 0xff));
    h.m = (int)uniform_u32((uint32_t)((hw >> 8) & 0xff));
    h.self = (int)uniform_u32((uint32_t)((hw >> 16) & 0xff));
    h.kjmax = (int)uniform_u32((uint32_t)((hw >> 24) & 0xff));
    return h;
}
// Member `pos` of S[i]: the ids follow the header two to a word, stored relative to i.  lb = the blob.
__device__ __forceinline__ uint32_t blob_member(const uint64_t* lb, uint32_t i, int pos) {
    const uint64_t sw = lb[1 + (pos >> 1)];
    return i + ((pos & 1) ? (uint32_t)(sw >> 32) : (uint32_t)sw);
}

// ------------------------------------------------------------------------------------------ contract scalars

// pos(x) = max(zero(x), x), src/common.jl:8
__device__ __forceinline__ double pos_part(double x) {
    return (x > 0.0) ? x : ((x != x) ? x : 0.0);
}
// sigmoid(x) = inv(one(x) + exp(-x)), scripts/logistic.jl:33
__device__ __forceinline__ double sigmoid(double x) {
    return 1.0 / (1.0 + pdmp_exp(-x));
}
// The logistic link and its variance at a linear predictor η, for the non-factorised logistic target (pdmp_bps_logit.inc):
// p = inv(1 + exp(-η)) and w = p (1 − p).  |η| past exp's range gives p = 0 or 1 exactly and w = 0, never a NaN.  Held to
// tests/ref/bps_logistic_ref.c bit for bit through the parity tests of that kernel.
__device__ __forceinline__ void logit_link(const double eta, double* p, double* w) {
    const double q = 1.0 / (1.0 + pdmp_exp(-eta));
    *p = q;
    *w = q * (1.0 - q);
}
// the largest double below a finite x (x > 0, or x < 0, or x == 0 all handled by the integer image)
__device__ __forceinline__ double pdmp_below(double x) {
    long long b = __double_as_longlong(x);
    if (x > 0) b -= 1;
    else if (x < 0) b += 1;
    else b = (long long)0x8000000000000001ull;  // -denorm_min
    return __longlong_as_double(b);
}

// poisson_time(a, b, u) with L = log(u) supplied, src/poissontime.jl:8-30, in the reference's form: a branch per sign of b and of a,
// each with its own divisions and square root (the Bouncy Particle kernels; poisson_time_L below is what the other event loops use)
__device__ __forceinline__ double poisson_time_L_ref(double a, double b, double L) {
    if (b > 0) {
        const double r = a / b;
        if (a < 0) return sqrt(-L * 2.0 / b) - r;
        return sqrt(r * r - L * 2.0 / b) - r;
    } else if (b == 0) {
        return (a > 0) ? (-L / a) : PDMP_INF;
    } else {
        if (a <= 0) return PDMP_INF;
        if (-L <= -(a * a) / b + (a * a) / (2 * b)) {
            const double r = a / b;
            return -sqrt(r * r - L * 2.0 / b) - r;
        }
        return PDMP_INF;
    }
}
// poisson_time(a, b, u), src/poissontime.jl:8-30
__device__ __forceinline__ double poisson_time(double a, double b, double u) {
    return poisson_time_L_ref(a, b, pdmp_log(u));
}
// poisson_time(a, b, u) with L = log(u) supplied (src/poissontime.jl:8-30), merged: the same value as poisson_time_L_ref bit for bit
__device__ __forceinline__ double poisson_time_L(double a, double b, double L) {
    // The three b != 0 formulas share a / b, L * 2 / b and the square root (sqrt(-L * 2.0 / b) is sqrt(-(L * 2.0 / b)) bit for
    // bit), so a wavefront whose lanes disagree on the signs of a and b runs ONE division pair and ONE square root instead of
    // one set per branch; only the admissibility test of the b < 0 branch keeps its own two divisions.
    if (b == 0) return (a > 0) ? -L / a : PDMP_INF;
    const double r = a / b;
    const double q = L * 2.0 / b;
    const double sq = sqrt((b > 0 && a < 0) ? -q : r * r - q);
    if (b > 0) return sq - r;
    if (a <= 0) return PDMP_INF;
    if (-L <= -(a * a) / b + (a * a) / (2 * b)) return -sq - r;
    return PDMP_INF;
}

// poisson_time((a, b, c), u) with L = log(u) supplied, src/poissontime.jl:39-65: the waiting time of the rate c + (a + b t)^+, c > 0 -- never
// infinite.  The same operations on the same operands, in the same order, as the host restatements (oracle/pdmp_oracle.c orc_poisson_time3,
// tests/ref/stickyzz_ref.c), branch by branch.  (const parameters: tests/test_abi.py counts the two-parameter contract scalars by signature;
// this one has its own probe, pdmp_debug_barrier_eval.)
__device__ __forceinline__ double poisson_time3_L(const double a, const double b, const double c, const double L) {
    if (b > 0) {
        if (a < 0) {
            if (-c * a / b + L < 0.0) return sqrt(-2 * b * L + c * c + 2 * a * c) / b - (a + c) / b;  // :43
            return -L / c;                                                                             // :45
        }
        return sqrt(-L * 2.0 * b + (a + c) * (a + c)) / b - (a + c) / b;  // :48
    } else if (b == 0) {
        return (a > 0) ? -L / (a + c) : -L / c;  // :52, :54
    }
    if (a <= 0.0) return -L / c;  // :58
    if (-c * a / b - (a * a) / (2 * b) + L > 0.0) return +sqrt((a + c) * (a + c) - 2.0 * L * b) / b - (a + c) / b;  // :60
    return (-L + (a * a) / (2 * b)) / c;  // :62
}
// hitting_time(barrier, ui, flow), src/stickyzz.jl:119-127, with the barrier level of the direction of travel: Inf when v (x - bar) >= 0 (the
// reference's "sic": a coordinate that sits ON its barrier, a thawed :sticky one, passes through it), else -(x - bar) / v
__device__ __forceinline__ double barrier_hitting_time(const double x, const double v, const double bar) {
    return (v * (x - bar) >= 0) ? PDMP_INF : (-(x - bar) / v);
}
// λ(i, u, ∇ϕi, b, ::NewFlow), src/stickyzz.jl:129-135: the rate pos(∇ϕi θi) and its bound pos(a + b (t_i - t_old)) -- the bound WITHOUT the
// 0.01 the proposal time was drawn with (the reference's arithmetic, kept as it is)
struct RateAndBound {
    double l, lb;
};
__device__ __forceinline__ RateAndBound barrier_rates(const double gth, const double a, const double b, const double dt) {
    RateAndBound r;
    r.l = pos_part(gth);
    r.lb = pos_part(a + b * dt);
    return r;
}

// One batch mean and its square to ONE rounding each.  y = (J − Jprev)/(T − T_prev) formed as written costs three roundings (the
// difference, the reciprocal, the product) and y·y doubles them and adds one: 7u on a term of ΣY², more than the (n + 3)u a sum of n
// terms is held to when n is small (tests/test_gpu_path_integrals.py).  Here the two differences are kept exactly
// as unevaluated pairs (TwoSum), the quotient is carried as a pair (error ~u²) and y and y² are each rounded once from it.  Explicit
// fma() is meant: the units are compiled with -ffp-contract=off, which leaves explicit calls alone.  Used by the reductions of both families
// (zz_batch_means_kernel / zz_ess_kernel, dense_batch_means_kernel / dense_ess_kernel): not on any hot path.
struct BatchMean {
    double y, y2;
};
__device__ __forceinline__ void two_diff(double a, double b, double& h, double& l) {  // a − b = h + l exactly
    h = a - b;
    const double bb = a - h;
    l = (a - (h + bb)) + (bb - b);
}
__device__ __forceinline__ BatchMean batch_mean_exactly_rounded(double J, double Jprev, double wh, double wl) {
    double dh, dl;
    two_diff(J, Jprev, dh, dl);
    const double q1 = dh / wh;
    const double p = q1 * wh;
    const double pe = fma(q1, wh, -p);                      // q1·wh = p + pe exactly
    const double r = (((dh - p) - pe) + dl) - q1 * wl;      // (dh + dl) − q1·(wh + wl), to ~u² of the quotient's scale
    const double q2 = r / wh;
    const double yh = q1 + q2;                              // y rounded once
    const double yl = q2 - (yh - q1);                       // (q1, q2) renormalised: y = yh + yl to ~u²
    const double sh = yh * yh;
    const double se = fma(yh, yh, -sh);
    BatchMean out;
    out.y = yh;
    out.y2 = sh + (se + 2.0 * (yh * yl));                   // (yh + yl)² rounded once
    return out;
}

}  // namespace pdmp
