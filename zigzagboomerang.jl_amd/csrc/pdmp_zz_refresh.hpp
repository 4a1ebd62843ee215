// pdmp_zz_refresh.hpp -- the refresh-clock event of the factorised ZigZag (src/sfact.jl:78-114), written ONCE for the event loops that
// serve a refresh clock from the neighbourhood blobs: zz_local_run_kernel, zz_local_spec8_kernel (pdmp_kernels.hip) and
// zz_local_spec8g_kernel (pdmp_spec8g.inc).  (zz_local_spec_body keeps the same event written out, DESIGN.md §4: a change here is a change
// there.)  In every one of them the clock's event is processed by itself, the whole wave on one event: a
// refresh moves the neighbourhood of one random coordinate and re-bounds that of another, so no zone test covers it, and at rate λref against
// thousands of proposals per unit time it need not be fast.  (pdmp_general.hip's refresh branch -- adaptscale, Boomerang, masked re-bounds --
// goes through that kernel's own lambdas and is not this function.)
//
// The split: the function does the event from the two global draws to the stored records, keys and level-1 entries.  A kernel keeps its
// counters (absolute, or deltas of the launch), its trace slot and where the clock's time lives.
#pragma once

#include "pdmp_device.hpp"
#include "pdmp_engine.hpp"

namespace pdmp {

// smove_forward!(::All, ...) = move every coordinate to tnew (src/sfact.jl:19,23-28): the `pdmp` driver, G = All()
__device__ __forceinline__ void zz_sweep_all(ZzRec* rec, int64_t d, int lane, double tnew) {
    for (int64_t q = lane; q < d; q += 64) {
        ZzRec* r = rec + q;
        const double x0 = r->x, th0 = r->th, t0 = r->t, I0 = r->I;
        const double dt = tnew - t0;
        const double xn = x0 + th0 * dt;
        r->x = xn;
        r->t = tnew;
        r->I = I0 + dt * ((x0 + xn) * 0.5);
    }
}

// The blob geometry as the caller knows it (run-time words of ZzRunParams, or the lattice's constants): w words to stage, w_pad words from
// one blob to the next, sw id words, pw position words and r words in all per member record.
struct BlobGeom {
    uint32_t w, w_pad, sw, pw, r;
};

// The level-1 form of the 64-key blocks: the clock is key d of the queue like any coordinate.  (The 32-key form of the 8-event kernels,
// where the clock's time is a register of the kernel: S8Level1, pdmp_spec8_common.hpp.)
struct Level1Blocks64 {
    static constexpr bool clock_is_key = true;
    double* bk;
    uint32_t* bi;
    __device__ __forceinline__ void operator()(const double* keys, int lane, uint32_t j, double kj) const {
        level1_update(bk, bi, keys, lane, j, kj);
        PDMP_LDS_ORDER();
    }
};

// what a kernel's counters and trace need of the event
struct ZzRefreshed {
    uint32_t ndraw;   // draws of the chain's main stream consumed: the sign and one per member of G1[i2]
    uint64_t ng;      // next draw of the global stream
    double t_ref;     // the clock's next time (already stored and queued where the clock is a key)
    double t, x, th;  // event(i2, t, x, θ, F) = (t[i2], i2, x[i2], θ[i2]), :143
    uint32_t i2;
};

// The clock popped at time tp.  Restated with the reference's quirks: the coordinate whose neighbourhood is moved (:80) and the coordinate
// that is refreshed (:84) are two independent draws from the "global rng" stream, and G1[i2] is re-bounded at the coordinates' OWN, possibly
// stale, clocks.  nm, ng: the next draws of the main and of the global stream.  Scratch of the caller: lb (one blob slot), sx, sth ([64]).
// SWEEP: the kernel knows `move_all` (G = All(): every coordinate is moved instead of G[i1] and G2[i2]).  FIXED_KJ: 0, or |G1[j]| <= FIXED_KJ <= 8
// as a compile-time fact of the geometry (the lattice: 5) -- the gradient's terms are the same ones in the same order either way.
template <bool SWEEP, int FIXED_KJ, class Level1>
__device__ __forceinline__ ZzRefreshed zz_refresh_event(const ZzRunParams& P, const BlobGeom G, ZzRec* rec, double* keys, const double* cmut, int64_t d,
                                                        uint64_t seed, uint64_t nm, uint64_t ng, double tp, int lane, uint64_t* lb, double* sx,
                                                        double* sth, bool move_all, const Level1 level1) {
    const bool all = SWEEP && move_all;
    const uint32_t i1 = pdmp_randint(seed, PDMP_STREAM_GLOBAL, ng, (uint32_t)d);  // :80
    ng += 1;
    if (all) {
        zz_sweep_all(rec, d, lane, tp);
    } else {
        const uint64_t* bsrc = P.blob + (size_t)P.tix[i1] * G.w_pad;
        for (uint32_t w = lane; w < G.w; w += 64) lb[w] = bsrc[w];
        PDMP_LDS_ORDER();
        const int k1 = blob_header_uniform(lb[0]).k;
        if (lane < k1) {  // smove_forward!(G, i1, ...), :82
            ZzRec* r1 = rec + blob_member(lb, i1, lane);
            const double x0 = r1->x, th0 = r1->th, t0 = r1->t, I0 = r1->I;
            const double dt = tp - t0;
            const double xn = x0 + th0 * dt;
            r1->x = xn;
            r1->t = tp;
            r1->I = I0 + dt * ((x0 + xn) * 0.5);
        }
        PDMP_LDS_ORDER();
    }
    const uint32_t i2 = pdmp_randint(seed, PDMP_STREAM_GLOBAL, ng, (uint32_t)d);  // :84
    ng += 1;
    {
        const uint64_t* bsrc = P.blob + (size_t)P.tix[i2] * G.w_pad;
        for (uint32_t w = lane; w < G.w; w += 64) lb[w] = bsrc[w];
    }
    PDMP_LDS_ORDER();
    const BlobHeader bh = blob_header_uniform(lb[0]);
    const int k = bh.k, m = bh.m, self = bh.self, kjmax = bh.kjmax;
    const uint32_t s = (lane < m) ? blob_member(lb, i2, lane) : i2;
    ZzRec* rs = rec + s;
    double x = 0.0, th = 0.0, t = 0.0, I = 0.0;
    if (lane < m) {
        x = rs->x;
        th = rs->th;
        t = rs->t;
        I = rs->I;
    }
    if (!all && lane >= k && lane < m) {  // smove_forward!(G2, i, ...), :85
        const double dt = tp - t;
        const double xn = x + th * dt;
        I = I + dt * ((x + xn) * 0.5);
        x = xn;
        t = tp;
    }
    const double usign = pdmp_u01(seed, PDMP_STREAM_MAIN, nm);  // θ[i] = σ[i]*rand(rng, (-1,1)), :100-101
    if (lane == self) th = P.tb.sigma[i2] * ((usign < 0.5) ? -1.0 : 1.0);
    // Q[n+1] = t′ + waiting_time_ref(F) = t′ + randexp()/λref from the global rng, :108
    const double newref = tp + (-pdmp_log(pdmp_u01(seed, PDMP_STREAM_GLOBAL, ng))) / P.lambda_ref;
    ng += 1;
    if (lane < m) {
        sx[lane] = x;
        sth[lane] = th;
    }
    PDMP_LDS_ORDER();
    const uint32_t sub = 1 + G.sw + (uint32_t)lane * G.r;
    double key = PDMP_INF;
    if (lane < k) {  // :110-114
        const double gmu = __longlong_as_double((long long)lb[sub + 1]);
        const double cj = cmut ? cmut[s] : __longlong_as_double((long long)lb[sub + 2]);
        const int kj = (int)(lb[sub + 3] & 0xff);
        double gx = 0.0, gt = 0.0;
        for (int base = 0; base < (FIXED_KJ ? 1 : kjmax); base += 8) {
            const uint64_t pw = lb[sub + 4 + (base >> 3)];
#pragma unroll
            for (int q = 0; q < (FIXED_KJ ? FIXED_KJ : 8); ++q) {
                const int pp = base + q;
                if (pp < kj) {
                    const double v = __longlong_as_double((long long)lb[sub + 4 + G.pw + pp]);
                    const int ps = (int)((pw >> (8 * q)) & 0xff);
                    gx += v * sx[ps];
                    gt += v * sth[ps];
                }
            }
        }
        const double a = cj + (gx - gmu) * th;
        const double b = cj / 100 + th * gt;
        const double L = pdmp_log(pdmp_u01(seed, PDMP_STREAM_MAIN, nm + 1 + (uint64_t)lane));
        key = t + poisson_time_L(a, b, L);  // Q[j] = t[j] + poisson_time(...): t[j] is j's OWN clock here
        rs->t_old = t;
        rs->a = a;
        rs->b = b;
        keys[s] = key;
    }
    if (lane < m) {
        rs->x = x;
        rs->th = th;
        rs->t = t;
        rs->I = I;
    }
    if (Level1::clock_is_key && lane == 0) keys[d] = newref;
    for (int jj = 0; jj < k + (Level1::clock_is_key ? 1 : 0); ++jj) {  // the members of G1[i2], then the clock where it is a key
        const uint32_t j = (jj < k) ? readlane_u32(s, jj) : (uint32_t)d;
        const double kj = (jj < k) ? readlane_f64(key, jj < k ? jj : 0) : newref;
        level1(keys, lane, j, kj);
    }
    ZzRefreshed out;
    out.ndraw = 1u + (uint32_t)k;
    out.ng = ng;
    out.t_ref = newref;
    out.t = readlane_f64(t, self);
    out.x = readlane_f64(x, self);
    out.th = readlane_f64(th, self);
    out.i2 = i2;
    return out;
}

}  // namespace pdmp
