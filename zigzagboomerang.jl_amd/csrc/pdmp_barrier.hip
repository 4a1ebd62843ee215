// pdmp_barrier.hip -- the ZigZag with sticky and reflecting barriers: stickyzz (src/stickyzz.jl), gfx950 (CDNA4).
//
// stickyzz_inner! (src/stickyzz.jl:239-319) under the driver loop `while t′ < T` (:226-235), G = G1 = the pattern of the flow's Γ.  Mapping, queue,
// records, neighbourhood blob and draws are zz_sticky_run_kernel's (pdmp_kernels.hip): one chain per wavefront, one event per iteration, lane p
// holds member p of S[i] = G1[i] ++ G2[i].  What differs from sspdmp is the process:
//   state    the record's `acc` word holds action[i] (:170-175; BARRIER_ACT_*), thf holds v_old[i].  The cases are tested in the reference's
//            order: action == hit (:247), then v[i] == 0 && v_old[i] != 0 (:266), else a proposal.
//   barriers a lower and an upper level per coordinate, the one in the direction of travel applies (dir, :115); a rule per barrier acts at thaw
//            time on the RESTORED speed (:269-274); a thaw rate κ per barrier, κ = +Inf being a wall: −log(u)/Inf = +0.0, the thaw key equals t′
//            and the same coordinate pops next (lowest index on ties, as everywhere).
//   times    trefl = poisson_time(t[j], b[j], u) − t[j] (:147) with the four-tuple form of src/poissontime.jl:86-92, i.e. the three-parameter
//            poisson_time((a, b, 0.01), u): the proposal rate never drops below 0.01, no key is infinite.  A hit is chosen when thit <= trefl (:149).
//   thinning lb = pos(a + b (t[i] − t_old[i])) WITHOUT that 0.01 (λ, :129-135), the coin is u lb < l (:292): the proposals are drawn from a
//            rate 0.01 above the bound they are thinned against.  This is the reference's arithmetic and is kept as it is.
//   hit      x[i] = the barrier level exactly (:249) -- no −0·θ, no |x| <= 1e-8 check.
// Draws, all from PDMP_STREAM_MAIN: draw nm is the thaw clock (hit) / the sign coin (thaw under :reversible; u < 0.5 -> −1, this engine's
// convention for the reference's global-RNG rand((-1,1))) / the thinning coin (proposal), then one draw per re-bounded coordinate in ascending order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pdmp_detmath.h"
#include "pdmp_device.hpp"
#include "pdmp_engine.hpp"

namespace pdmp {

size_t zz_barrier_lds_bytes(uint32_t nblk_pad, uint32_t blob_w_pad) {
    return (size_t)nblk_pad * 8 + 4 * 64 * 8 + (size_t)blob_w_pad * 8 + (size_t)nblk_pad * 4;
}

__global__ __launch_bounds__(64) void zz_barrier_run_kernel(ZzRunParams P) {
    const int lane = threadIdx.x;
    const int64_t chain = blockIdx.x;
    const int64_t d = P.d;
    const uint32_t nblk = P.nblk;
    const uint32_t W = P.blob_w, SW = P.blob_sw, PW = P.blob_pw, KMAX = P.blob_kmax;
    const uint32_t R = 4 + PW + KMAX;

    extern __shared__ __align__(16) unsigned char smem[];
    double* bk = reinterpret_cast<double*>(smem);  // [nblk_pad] block minima
    double* sx = bk + P.nblk_pad;                  // [64] x of S[i] after the moves
    double* sth = sx + 64;                         // [64] θ of S[i]
    double* LU = sth + 64;                         // logs of the 64 candidate draws nm + lane
    double* UU = LU + 64;                          // the draws themselves
    uint64_t* lb = reinterpret_cast<uint64_t*>(UU + 64);            // [blob_w_pad] neighbourhood blob of i
    uint32_t* bi = reinterpret_cast<uint32_t*>(lb + P.blob_w_pad);  // [nblk_pad] block argmin (coordinate id)

    ZzRec* rec = P.rec + chain * d;
    double* keys = P.keys + chain * P.dk;
    double* thf = P.thf + chain * d;
    DevChain* hdr = P.hdr + chain;
    pdmp_event* ev = P.ev ? P.ev + chain * P.trace_cap : nullptr;
    double* cmut = P.c_chain ? (P.c_chain + chain * d) : nullptr;

    uint32_t status = hdr->c.status;
    if (chain_ended(status)) return;
    const uint64_t seed = hdr->seed;
    const uint64_t nm0 = hdr->c.ndraw_main;
    uint64_t nm = nm0;
    uint64_t num = hdr->c.num, nacc = hdr->c.nacc, ntrace = hdr->c.ntrace, nevents = hdr->c.nevents;
    double t_last = hdr->c.t_last;
    double t_event = hdr->t_event;
    status = PDMP_CHAIN_OK;
    const double T = P.T;
    const bool stop_before = (P.flags & PDMP_RUN_STOP_BEFORE) != 0;
    const bool adapt = P.adapt != 0;

    level1_build(bk, bi, keys, nblk, lane);
    PDMP_LDS_ORDER();

    auto queue_update = [&](uint32_t j, double kj) {
        level1_update(bk, bi, keys, lane, j, kj);
        PDMP_LDS_ORDER();
    };

    bool running = stop_before || (t_event < T);  // `while t′ < T`, :226
    PrioTurn prio;
    while (running) {
        prio.step();
        if (P.trace_cap > 0 && ntrace >= (uint64_t)P.trace_cap) {
            status = PDMP_CHAIN_TRACE_FULL;
            break;
        }
        if (nm - nm0 >= (uint64_t)P.count_limit) {  // (a launch's draws are counted in 32 bits: pause, the host runs again)
            status = PDMP_CHAIN_PAUSED;
            break;
        }
        // ---------------- peek(Q), :243
        double mk = PDMP_INF;
        uint32_t mb = 0xffffffffu;
        for (uint32_t b = lane; b < nblk; b += 64) {
            const double v = bk[b];
            if (v < mk) {
                mk = v;
                mb = b;
            }
        }
        const double tp = wave_min_f64(mk);
        if (!(tp < PDMP_INF)) {  // (no key of this sampler is infinite: a NaN, i.e. a diverged chain)
            status = PDMP_CHAIN_STALLED;
            break;
        }
        if (stop_before && !(tp < T)) break;
        const uint64_t ball = __ballot(mk == tp);
        uint32_t blk;
        if (__popcll(ball) == 1) {
            blk = readlane_u32(mb, __ffsll((unsigned long long)ball) - 1);
        } else {  // exact tie between blocks: lowest coordinate wins
            blk = wave_min_u32((mk == tp) ? mb : 0xffffffffu);
        }
        const uint32_t i = uniform_u32(bi[blk]);
        t_last = tp;

        {
            const uint64_t* bsrc = P.blob + (size_t)P.tix[i] * P.blob_w_pad;
            for (uint32_t w = lane; w < W; w += 64) lb[w] = bsrc[w];
        }
        const ZzRec* ri = rec + i;
        const double told_i = ri->t_old, a_i = ri->a, b_i = ri->b;
        const uint64_t action_i = ri->acc;
        const double th_i0 = ri->th;
        const double vold_i = thf[i];
        {
            const double u = pdmp_u01(seed, PDMP_STREAM_MAIN, nm + (uint64_t)lane);
            UU[lane] = u;
            LU[lane] = pdmp_log(u);
        }
        PDMP_LDS_ORDER();
        const BlobHeader bh = blob_header_uniform(lb[0]);
        const int k = bh.k, m = bh.m, self = bh.self, kjmax = bh.kjmax;
        const uint32_t s = (lane < m) ? blob_member(lb, i, lane) : i;
        ZzRec* rs = rec + s;
        double x = 0.0, th = 0.0, t = 0.0, I = 0.0;
        if (lane < m) {
            x = rs->x;
            th = rs->th;
            t = rs->t;
            I = rs->I;
        }
        const uint32_t sub = 1 + SW + (uint32_t)lane * R;
        double tv = 0.0, cj = 0.0;
        if (lane < k) {
            tv = __longlong_as_double((long long)lb[sub + 0]);
            cj = cmut ? cmut[s] : __longlong_as_double((long long)lb[sub + 2]);
        }
        auto move_lane = [&]() {  // t[j], x[j] = t′, x[j] + θ[j]*(t′ - t[j])
            const double dt = tp - t;
            const double xn = x + th * dt;
            I = I + dt * ((x + xn) * 0.5);
            x = xn;
            t = tp;
        };

        const bool is_hit = uniform_u32(action_i == BARRIER_ACT_HIT ? 1u : 0u) != 0;
        const bool is_thaw = !is_hit && uniform_u32((th_i0 == 0 && vold_i != 0) ? 1u : 0u) != 0;
        uint32_t ndraw0 = 0;       // draws consumed before the per-coordinate re-bound draws
        bool rebound_set = false;  // lane takes part in the re-bound
        bool emit = true;
        bool moved_hi = false;     // lanes k..m were (ss)moved
        double key_self = PDMP_INF;  // hit: the thaw clock of i (i itself is not re-bounded)
        bool frozen_now = false;
        bool violated = false;

        if (is_hit) {  // ---- case 1) to be frozen or to reflect from the boundary, :247-265
            const BarrierEntry be = P.barriers[i];
            const bool up = th_i0 > 0;  // di = dir(geti(u, i)), :248
            const double bar = up ? be.hi : be.lo;
            if (lane == self) {
                const double dt = tp - t;
                I = I + dt * ((x + bar) * 0.5);  // (the path between two events of the trace is the segment that joins them)
                x = bar;                          // x[i] = barriers[i].x[di], :249
                t = tp;                           // t_old[i] = t[i] = t′, :250
                thf[s] = th;                      // v_old[i], v[i] = v[i], 0.0, :251
                th = 0.0;
            }
            key_self = tp - LU[0] / (up ? be.khi : be.klo);  // Q[i] = t′ - log(rand(rng))/barriers[i].κ[di], :253
            ndraw0 = 1;
            frozen_now = true;
            if (!P.strong_upperbounds) {  // :254-264
                if (lane < m && th != 0.0) move_lane();  // ssmove_forward!(G, i, ...), ssmove_forward!(G2, i, ...): frozen members stay
                moved_hi = true;
                rebound_set = (lane < k) && (th != 0.0);  // only non-frozen, especially not i
            }
        } else if (is_thaw) {  // ---- case 2) was frozen, :266-284
            const BarrierEntry be = P.barriers[i];
            const uint32_t rule = (vold_i > 0) ? ((be.rules >> 8) & 0xffu) : (be.rules & 0xffu);  // the rule of the RESTORED direction, :269
            if (lane == self) {
                I = I + (tp - t) * x;  // (frozen since its hit, or since t0: its clock stood still while it sat at the barrier LEVEL, which is not 0 here)
                t = tp;                // t_old[i] = t[i] = t′, :267 (the particle does not move, only time)
                th = vold_i;  // v[i], v_old[i] = v_old[i], 0.0, :268
                thf[s] = 0.0;
                if (rule == PDMP_BARRIER_REVERSIBLE) th *= (UU[0] < 0.5) ? -1.0 : 1.0;  // v[i] *= rand((-1,1)), :271
                else if (rule == PDMP_BARRIER_REFLECT) th = -th;                         // :273
            }
            ndraw0 = (rule == PDMP_BARRIER_REVERSIBLE) ? 1u : 0u;
            if (lane < m && th != 0.0) move_lane();  // :275-276 (i itself: x + θ*0)
            moved_hi = true;
            rebound_set = (lane < k) && (th != 0.0);  // only non-frozen, including i, :277-283
        } else {  // ---- a reflection time or an event time from the upper bound, :285-316
            if (lane < k && th != 0.0) move_lane();  // ssmove_forward!(G, i, ...), :287
            double g = 0.0;  // ∇ϕi = target(t′, u, i, flow), :288
            for (int p = 0; p < k; ++p) g += readlane_f64(tv, p) * readlane_f64(x, p);
            if (P.tb.gmu_t) g = g - P.tb.gmu_t[i];
            const double th_s = readlane_f64(th, self);
            const RateAndBound r = barrier_rates(g * th_s, a_i, b_i, tp - told_i);  // l, lb = λ(i, u, ∇ϕi, b, flow), :289 (lb without the 0.01)
            num += 1;
            ndraw0 = 1;
            if (UU[0] * r.lb < r.l) {  // :292
                nacc += 1;              // accept!, :293
                if (r.l > r.lb) {       // :294
                    if (!adapt) {       // error("Tuning parameter `c` too small. ..."), :295
                        status = PDMP_CHAIN_BOUND_VIOLATED;
                        if (lane < k) {
                            rs->x = x;
                            rs->t = t;
                            rs->I = I;
                        }
                        nm += 1;
                        break;
                    }
                    nacc = 0;  // reset!(acc), :296
                    num = 0;
                    violated = true;  // adapt!(upper_bounds.c, i, multiplier), :297: with i's re-bound below
                }
                if (lane == self) th = -th;                             // reflect!, :299
                if (lane >= k && lane < m && th != 0.0) move_lane();    // ssmove_forward!(G2, i, ...), :300
                moved_hi = true;
                rebound_set = (lane < k) && (th != 0.0);  // :301-307
            } else {  // an event time from the upper bound -> nothing happens, :309-315
                rebound_set = (lane == self);
                emit = false;
            }
        }
        const int nst = moved_hi ? m : k;
        if (lane < nst) {
            sx[lane] = x;
            sth[lane] = th;
        }
        PDMP_LDS_ORDER();
        // ---------------- b[j] = ab(...), t_old[j] = t[j], queue_time! (:144-165) for the re-bound set
        const uint64_t rball = __ballot(rebound_set);
        const uint32_t rank = (uint32_t)__popcll(rball & ((1ull << lane) - 1ull));
        double key = PDMP_INF;
        if (rebound_set) {
            const double gmu = __longlong_as_double((long long)lb[sub + 1]);
            const int kj = (int)(lb[sub + 3] & 0xff);
            double gx = 0.0, gt = 0.0;
            for (int base = 0; base < kjmax; base += 8) {
                const uint64_t pw = lb[sub + 4 + (base >> 3)];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int pp = base + q;
                    if (pp < kj) {
                        const double v = __longlong_as_double((long long)lb[sub + 4 + PW + pp]);
                        const int ps = (int)((pw >> (8 * q)) & 0xff);
                        gx += v * sx[ps];
                        gt += v * sth[ps];
                    }
                }
            }
            if (violated && lane == self) {
                cj *= P.factor;
                cmut[s] = cj;
            }
            const double a = cj + (gx - gmu) * th;  // ab(G1, j, x, v, c, Z::ZigZag), src/fact_samplers.jl:50-54
            const double b = cj / 100 + th * gt;
            const BarrierEntry bj = P.barriers[s];
            const double bar = (th > 0) ? bj.hi : bj.lo;
            const double dt0 = t - t;  // poisson_time(t, b::Tuple, r): Δt = t - b[1], a = b[2] + Δt*b[3], src/poissontime.jl:86-92
            const double trefl = (t + poisson_time3_L(a + dt0 * b, b, 0.01, LU[ndraw0 + rank])) - t;  // :147
            const double thit = barrier_hitting_time(x, th, bar);                                        // :148
            const bool hit = thit <= trefl;                                                               // :149
            key = t + (hit ? thit : trefl);
            rs->t_old = t;
            rs->a = a;
            rs->b = b;
            rs->acc = hit ? BARRIER_ACT_HIT : BARRIER_ACT_REFLECT;
            keys[s] = key;
        }
        nm += (uint64_t)ndraw0 + (uint64_t)__popcll(rball);
        if (lane < nst || lane == self) {
            rs->x = x;
            rs->th = th;
            rs->t = t;
            rs->I = I;
        }
        if (frozen_now && lane == self) {
            rs->t_old = tp;                     // :250
            rs->acc = BARRIER_ACT_UNFREEZE;     // :252
            keys[s] = key_self;
        }
        // ---------------- level 1 of the queue
        if (frozen_now) queue_update(i, key_self);
        for (int jj = 0; jj < k; ++jj) {
            if (!((rball >> jj) & 1ull)) continue;
            queue_update(readlane_u32(s, jj), readlane_f64(key, jj));
        }
        if (emit) {  // push!(Ξ, event(i, t, x, v, flow.old)), :230
            const double t_s = readlane_f64(t, self), x_s = readlane_f64(x, self), th_s2 = readlane_f64(th, self);
            if (ev && lane == 0) {
                pdmp_event e;
                e.t = t_s;
                e.i = (int64_t)i;
                e.x = x_s;
                e.theta = th_s2;
                ev[ntrace] = e;
            }
            ntrace += 1;
            nevents += 1;
            t_event = tp;
            if (!stop_before && !(tp < T)) running = false;
        }
        PDMP_LDS_ORDER();
    }

    if (lane == 0) {
        hdr->c.t_last = t_last;
        hdr->t_event = t_event;
        hdr->c.num = num;
        hdr->c.nacc = nacc;
        hdr->c.ntrace = ntrace;
        hdr->c.nevents = nevents;
        hdr->c.ndraw_main = nm;
        hdr->c.status = status;
    }
}

int launch_zz_barrier_run(const ZzRunParams& p, int64_t nchains, void* stream) {
    const size_t lds = zz_barrier_lds_bytes(p.nblk_pad, p.blob_w_pad);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(zz_barrier_run_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(zz_barrier_run_kernel, dim3((unsigned)nchains), dim3(64), lds, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

#ifdef PDMP_EXTRA_KERNELS
// pdmp_debug_barrier_eval (include/pdmp_debug.h, parity library only): the barrier sampler's scalars as compiled in this unit
__global__ __launch_bounds__(256) void barrier_eval_kernel(int fn, int64_t n, const double* a, const double* b, const double* c, double* out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    double y0 = 0.0, y1 = 0.0;
    if (fn == PDMP_BARRIER_FN_PT3_L) {
        y0 = poisson_time3_L(a[q], b[q], 0.01, pdmp_log(c[q]));
    } else if (fn == PDMP_BARRIER_FN_HIT) {
        y0 = barrier_hitting_time(a[q], b[q], c[q]);
    } else {  // PDMP_BARRIER_FN_RATES
        const RateAndBound r = barrier_rates(a[q], b[q], c[q], 1.0);
        y0 = r.l;
        y1 = r.lb;
    }
    out[q] = y0;
    out[n + q] = y1;
}
int launch_barrier_eval(int fn, int64_t n, const double* a, const double* b, const double* c, double* out, void* stream) {
    hipLaunchKernelGGL(barrier_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fn, n, a, b, c, out);
    return (int)hipGetLastError();
}
#endif

}  // namespace pdmp
