// pdmp_bps_sticky.inc -- the sticky Bouncy Particle / Boomerang: sticky_pdmp_inner! (src/ss_not_fact.jl:104-179) under its driver
// `while t < T` (:182-201).  Included by pdmp_bps.hip (inside namespace pdmp): one chain per wavefront, x, θ, ∇ϕ in registers as in
// bps_run_kernel (element e = slot*64 + lane), plus the per-coordinate clock tfrez (freezing time where free, thaw time where frozen) and the
// free mask f (one bit per slot and lane).  The saved speeds θf and the thaw rates κ are touched at freezes, thaws and refreshments only, each
// element by the lane that owns it: they stay in HBM / L2 (no LDS beyond BpsWave's d-vector staging buffer, no extra registers).
// The general CSC Γ path only (gather through LDS, idot order); the sums are wave_sum_f64's order, the draws PDMP_STREAM_MAIN in program order:
//   driver   draw 0 -> tref = -log(u)/λref (t0 not added, :190), draw 1 -> t′ (:195)
//   refresh  ((d+127)>>7)<<6 Box-Muller blocks (BpsWave::normals' mapping), 1 for tref, 1 for t′, then one per FROZEN i ascending
//   freeze   1 for the thaw time, and 1 for t′ unless strong_upperbounds;   thaw  1 for t′;   proposal  the coin, then 1 for t′
// Ties: findmin(tfrez) and findmin([tref, tᶠ, t′]) take the first minimum (lowest index; tref before tᶠ before t′).
// Fixed differently from the reference: a NaN clock never wins findmin (Julia's findmin returns the NaN); a clock is NaN only for a free
// coordinate with x = 0 and θ = 0 together, which no run reaches.
// Kept as the reference has them: the trace begins with (t0, x0, θ0, all free) (:189); acc += 1 before the bound check (:158-162); a rejected
// proposal recomputes ab in full (:169); reflect_sticky! updates the f[i] coordinates while its sums test θ[i] == 0 (:43-76);
// x[i] = -0*θ[i] at a freeze (:133: the integer 0 times θ[i], i.e. a zero with θ[i]'s sign); a freeze with |x[i]| > 1e-8 is the reference's
// error(...) (:129-132) and ends the chain as PDMP_CHAIN_BOUND_VIOLATED.

// freezing_time(x, θ, F::Union{BouncyParticle, ZigZag}), src/ss_fact.jl:10-16
__device__ __forceinline__ double bps_freeze_lin(double x, double th) {
    return (th * x >= 0.0) ? PDMP_INF : -x / th;
}
// freezing_time(x, θ, μ, F::Boomerang), src/ss_not_fact.jl:5-20.  mod(v, 2pi) is only ever applied to v = ±2atan(·) in [-π, π]:
// v >= 0 ? v : v + 2π.  min / max propagate a NaN as Julia's do.
__device__ __attribute__((noinline)) double bps_freeze_boom(double x, double th, double mu) {
    const double pi = 0x1.921fb54442d18p+1;
    if (mu == 0) {
        if (th * x >= 0.0) return pi - pdmp_atan(x / th);
        return pdmp_atan(-x / th);
    }
    const double u = (x * x - (2 * mu) * x) + th * th;  // x^2 - 2μ*x + θ^2
    if (u < 0) return PDMP_INF;
    const double su = sqrt(u), den = 2 * mu - x;
    const double v1 = 2 * pdmp_atan((su - th) / den);     // t1 = mod(2atan((sqrt(u) - θ)/(2μ - x)), 2pi)
    const double v2 = -(2 * pdmp_atan((su + th) / den));  // t2 = mod(-2atan((sqrt(u) + θ)/(2μ - x)), 2pi)
    const double t1 = v1 >= 0 ? v1 : v1 + 6.283185307179586;
    const double t2 = v2 >= 0 ? v2 : v2 + 6.283185307179586;
    if (t1 != t1) return t1;
    if (t2 != t2) return t2;
    if (x == 0) return t1 > t2 ? t1 : t2;  // x == 0 && return max(t1, t2)
    return t1 < t2 ? t1 : t2;
}
template <bool BOOM>
__device__ __forceinline__ double bps_freeze_dt(double x, double th, double mu) {
    if constexpr (BOOM) return bps_freeze_boom(x, th, mu);
    else return bps_freeze_lin(x, th);
}
// log(rand())/(κ[i]*abs(θf[i])) of draw n: the thaw time is t - this (:124, :136)
__device__ __attribute__((noinline)) double bps_thaw_term(uint64_t seed, uint64_t n, double kappa, double thf) {
    return pdmp_log(pdmp_u01(seed, PDMP_STREAM_MAIN, n)) / (kappa * fabs(thf));
}

// The pieces both sticky kernels share: y = Γ(v − μ), ab(x, θ, c, Flow) (:37 of src/not_fact_samplers.jl: GlobalBound(c) with the FLOW's Γ, μ),
// the freezing times of the free coordinates.
template <int NS, bool BOOM>
struct BpsStickyOps {
    const BpsRunParams& P;
    BpsWave<NS> wv;
    // (target: the ensemble's own Γt, μt where it has one, else the flow's)
    __device__ __forceinline__ void gamma(const double (&in)[NS], bool sub_mu, double (&out)[NS], bool target) const {
        const bool own = target && P.t_colptr != nullptr;
        wv.csc_gather(own ? P.t_colptr : P.colptr, own ? P.t_rowval : P.rowval, own ? P.t_nzval : P.nzval, own ? P.t_mu : P.mu, in, sub_mu, out);
    }
    __device__ __forceinline__ void ab(const double (&x)[NS], const double (&th)[NS], double c, double& a, double& b) const {
        if constexpr (BOOM) {  // (sqrt(normsq(θ) + normsq(x − μ))·c, 0), src/not_fact_samplers.jl:34-36
            double dx[NS];
            wv.sub_mu_flow(x, P.mu_flow, dx);
            a = sqrt(wv.dot(th, th) + wv.dot(dx, dx)) * c;
            b = 0.0;
        } else {  // (c + θ'(Γ(x−μ)), θ'(Γθ)), :26-28
            double w[NS];
            gamma(x, true, w, false);
            a = c + wv.dot(th, w);
            gamma(th, false, w, false);
            b = wv.dot(th, w);
        }
    }
    // freezing_time!(tfrez, t, x, θ, f, Z), src/ss_not_fact.jl:22-29
    __device__ __forceinline__ void freeze_times(double t, const double (&x)[NS], const double (&th)[NS], uint32_t fm, double (&tf)[NS]) const {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if ((fm >> s) & 1u) tf[s] = t + bps_freeze_dt<BOOM>(x[s], th[s], BOOM ? P.mu_flow[wv.elem(s)] : 0.0);
        }
    }
};

template <int NS, bool BOOM>
__global__ __launch_bounds__(64) void bps_sticky_run_kernel(BpsRunParams P, BpsStickyParams Q) {
    const int lane = threadIdx.x;
    const int64_t chain = blockIdx.x;
    const int64_t d = P.d;
    extern __shared__ __align__(16) unsigned char smem[];
    double* tmp = reinterpret_cast<double*>(smem);
    const BpsWave<NS> wv{lane, d, tmp};

    double* gx = P.x + chain * d;
    double* gth = P.th + chain * d;
    double* gthf = Q.thf + chain * d;
    double* gtf = Q.tfrez + chain * d;
    uint64_t* gfm = Q.fmask + chain * BPS_STICKY_WORDS;
    double* sc = P.scal + chain * 8;  // {t, a, b, tp, tau_ref, c, told, -}
    DevChain* hdr = P.hdr + chain;

    if (bps_chain_ended(hdr->c.status)) return;
    uint32_t status = PDMP_CHAIN_OK;
    const uint64_t seed = hdr->seed;
    BpsCounters k;
    k.load(hdr);
    double t = sc[0], a = sc[1], b = sc[2], tp = sc[3], tau_ref = sc[4], c = sc[5], told = sc[6];

    double x[NS], th[NS], g[NS], tf[NS];
    uint32_t fm = 0;  // bit s: element s*64 + lane is free (padding elements: not free, tfrez = Inf, x = θ = 0)
    wv.load_state(gx, gth, x, th);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        tf[s] = wv.has(s) ? gtf[wv.elem(s)] : PDMP_INF;
        g[s] = 0.0;
        fm |= (uint32_t)((gfm[s] >> lane) & 1ull) << s;
    }
    const double rho = P.rho, rhobar = sqrt(1 - rho * rho);  // :32
    const double T = P.T;
    const bool stop_before = (P.flags & PDMP_RUN_STOP_BEFORE) != 0;
    const BpsStickyOps<NS, BOOM> ops{P, wv};

    // b = ab(x, θ, c, Flow); told = t; t′, _ = next_time(t, b, rand())
    auto rebound = [&]() {
        ops.ab(x, th, c, a, b);
        told = t;
        tp = t + bps_next_dt(seed, k.nm, a, b);
        k.nm += 1;
    };

    bool running = stop_before || (t < T);  // `while t < T`, :196
    while (running) {
        if (P.trace_cap > 0 && k.ntrace >= (uint64_t)P.trace_cap) {
            status = PDMP_CHAIN_TRACE_FULL;
            break;
        }
        // tᶠ, i = findmin(tfrez), :110: first minimum of the lane's slots, the wave's minimum, the lowest element that attains it
        double best = tf[0];
        int bs = 0;
#pragma unroll
        for (int s = 1; s < NS; ++s) {
            if (tf[s] < best || best != best) {
                best = tf[s];
                bs = s;
            }
        }
        const double tfm = wave_min_f64(best);
        const uint32_t i = wave_min_u32_dpp((best == tfm) ? (uint32_t)(bs * 64 + lane) : 0xFFFFFFFFu);
        // tt, j = findmin([tref, tᶠ, t′]), :111
        const bool is_ref = tau_ref <= tfm && tau_ref <= tp;
        const bool is_frz = !is_ref && tfm <= tp;
        const double tnext = is_ref ? tau_ref : (is_frz ? tfm : tp);
        if (!(tnext < PDMP_INF)) {
            status = PDMP_CHAIN_STALLED;
            break;
        }
        if (stop_before && !(tnext < T)) break;
        const double tau = tnext - t;  // :112
        // smove_forward!(τ, t, x, θ, f, Flow), :78-97: the free coordinates only
        t += tau;
        if constexpr (BOOM) {
            double sn, cs;
            pdmp_sincos(tau, &sn, &cs);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int64_t e = wv.elem(s);
                if ((fm >> s) & 1u) {
                    const double m = P.mu_flow[e];
                    const double xn = (x[s] - m) * cs + th[s] * sn + m;
                    const double tn = -(x[s] - m) * sn + th[s] * cs;
                    x[s] = xn;
                    th[s] = tn;
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if ((fm >> s) & 1u) x[s] += th[s] * tau;
            }
        }
        if (is_ref) {
            // refresh_sticky_vel!, :31-41: θ[i] = ρθ[i] + ρ̄ randn() where free, θf[i] = abs(ρθf[i] + ρ̄ randn())*sign(θf[i]) where frozen
            wv.normals(seed, k.nm);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int64_t e = wv.elem(s);
                if ((fm >> s) & 1u) {
                    th[s] = rho * th[s] + rhobar * tmp[e];
                } else if (wv.has(s)) {
                    const double f0 = gthf[e];
                    const double v = rho * f0 + rhobar * tmp[e];
                    gthf[e] = fabs(v) * ((f0 > 0) ? 1.0 : ((f0 < 0) ? -1.0 : f0));
                }
            }
            asm volatile("" ::: "memory");
            k.nm += normal_draws(d);
            tau_ref = t + (-pdmp_log(pdmp_u01(seed, PDMP_STREAM_MAIN, k.nm)) / P.lambda_ref);  // :117
            k.nm += 1;
            rebound();                          // :118-120
            ops.freeze_times(t, x, th, fm, tf);  // :121
            // :122-126: tfrez[i] = t - log(rand())/(κ[i]*abs(θf[i])) for the frozen i in ascending order
            uint32_t base = 0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int64_t e = wv.elem(s);
                const bool fz = wv.has(s) && !((fm >> s) & 1u);
                const uint64_t bal = __ballot(fz);
                if (fz) {
                    const uint32_t r = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                    tf[s] = t - bps_thaw_term(seed, k.nm + r, Q.kappa[e], gthf[e]);
                }
                base += (uint32_t)__popcll(bal);
            }
            k.nm += base;
            k.nrefresh += 1;
        } else if (is_frz) {
            const int si = (int)(i >> 6);
            const bool mine = lane == (int)(i & 63u);
            const bool was_free = __ballot(mine && ((fm >> si) & 1u)) != 0ull;
            if (was_free) {  // :128-142
                bool bad = false;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (mine && s == si) bad = fabs(x[s]) > 1e-8;
                }
                if (__ballot(bad) != 0ull) {
                    status = PDMP_CHAIN_BOUND_VIOLATED;  // reference: error("x[i] = ... !≈ 0 ..."), :129-132
                    break;
                }
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (mine && s == si) {
                        x[s] = 0.0 * th[s];  // x[i] = -0*θ[i], :133
                        gthf[i] = th[s];     // θf[i], θ[i] = θ[i], 0.0
                        const double sp = th[s];
                        th[s] = 0.0;
                        fm &= ~(1u << s);
                        tf[s] = t - bps_thaw_term(seed, k.nm, Q.kappa[i], sp);  // :136
                    }
                }
                k.nm += 1;
                if (!Q.strong_upperbounds) rebound();  // :138-142
            } else {  // :143-151 (x[i] == 0 && θ[i] == 0 hold by construction)
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (mine && s == si) {
                        th[s] = gthf[i];  // θ[i], θf[i] = θf[i], 0.0
                        gthf[i] = 0.0;
                        fm |= 1u << s;
                        tf[s] = t + bps_freeze_dt<BOOM>(x[s], th[s], BOOM ? P.mu_flow[i] : 0.0);
                    }
                }
                rebound();
            }
        } else {
            const double coin = pdmp_u01(seed, PDMP_STREAM_MAIN, k.nm);
            // ∇ϕx = ∇ϕ!(∇ϕx, x); grad_correct!: the Boomerang subtracts x − μ (L = I), :153-154
            ops.gamma(x, true, g, true);
            if constexpr (BOOM) wv.each([&](int s, int64_t e) { g[s] -= x[s] - P.mu_flow[e]; });
            const double l = pos_part(wv.dot(g, th));             // λ(∇ϕx, θ, Flow)
            const double lb = pos_part(a + b * (t - told));         // sλ̄(b, t - told), :155
            k.num += 1;
            k.nm += 1;
            if (coin * lb <= l) {  // :157
                k.nacc += 1;
                if (l > lb) {
                    if (!P.adapt) {
                        status = PDMP_CHAIN_BOUND_VIOLATED;  // error("Tuning parameter `c` too small."), :160
                        break;
                    }
                    c *= P.factor;
                }
                // reflect_sticky!, :68-76: c = 2*sdot(∇ϕx, θ, θ)/subnormsq(∇ϕx, θ), both skipping θ[i] == 0
                double p1 = 0.0, p2 = 0.0;
                wv.each([&](int s, int64_t) {
                    if (!(th[s] == 0.0)) {
                        p1 += g[s] * th[s];
                        p2 += g[s] * g[s];
                    }
                });
                const double coef = 2 * wave_sum_f64(p1) / wave_sum_f64(p2);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if ((fm >> s) & 1u) th[s] -= coef * g[s];
                }
                rebound();                          // :164-166
                ops.freeze_times(t, x, th, fm, tf);  // :167
            } else {
                rebound();  // :169-171
                continue;
            }
        }
        // push!(Ξ, sevent(t, x, θ, f, Flow)), :175
        wv.emit_record(P, chain, k.ntrace, t, x, th);
        if (P.trace_cap > 0) {
            uint64_t* ef = Q.ev_f + (chain * P.trace_cap + (int64_t)k.ntrace) * BPS_STICKY_WORDS;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const uint64_t w = __ballot((fm >> s) & 1u);
                if (lane == 0) ef[s] = w;
            }
        }
        k.ntrace += 1;
        k.nevents += 1;
        if (!stop_before && !(t < T)) running = false;
    }

    wv.each([&](int s, int64_t e) {
        gx[e] = x[s];
        gth[e] = th[s];
        gtf[e] = tf[s];
    });
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const uint64_t w = __ballot((fm >> s) & 1u);
        if (lane == 0) gfm[s] = w;
    }
    if (lane == 0) {
        store_scal6(sc, t, a, b, tp, tau_ref, c);
        sc[6] = told;
        k.store(hdr, t, status);
    }
}

// The driver's head, :184-195: θf = 0, f = all free, the event (t0, x0, θ0, f) (:189), tref (draw 0), tfrez, b = ab(...), t′ (draw 1).
template <int NS, bool BOOM>
__global__ __launch_bounds__(64) void bps_sticky_init_kernel(BpsRunParams P, BpsStickyParams Q, const uint64_t* seeds, double t0, double c0) {
    const int lane = threadIdx.x;
    const int64_t chain = blockIdx.x;
    const int64_t d = P.d;
    extern __shared__ __align__(16) unsigned char smem[];
    const BpsWave<NS> wv{lane, d, reinterpret_cast<double*>(smem)};
    const uint64_t seed = seeds[chain];
    double x[NS], th[NS], tf[NS];
    uint32_t fm = 0;
    wv.load_state(P.x + chain * d, P.th + chain * d, x, th);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        tf[s] = PDMP_INF;
        if (wv.has(s)) fm |= 1u << s;
    }
    const BpsStickyOps<NS, BOOM> ops{P, wv};
    const double tau_ref = -pdmp_log(pdmp_u01(seed, PDMP_STREAM_MAIN, 0)) / P.lambda_ref;  // :190
    ops.freeze_times(t0, x, th, fm, tf);                                                   // :192
    double a, b;
    ops.ab(x, th, c0, a, b);                                                               // :194
    const double tp = t0 + bps_next_dt(seed, 1, a, b);                                     // :195
    const bool traced = P.trace_cap > 0;
    const int64_t slot = chain * P.trace_cap;
    wv.each([&](int s, int64_t e) {
        Q.thf[chain * d + e] = 0.0 * th[s];  // θf = 0*θ, :186
        Q.tfrez[chain * d + e] = tf[s];
    });
    wv.emit_record(P, chain, 0, t0, x, th);  // :189
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const uint64_t w = __ballot((fm >> s) & 1u);
        if (lane == 0) {
            Q.fmask[chain * BPS_STICKY_WORDS + s] = w;
            if (traced) Q.ev_f[slot * BPS_STICKY_WORDS + s] = w;
        }
    }
    if (lane == 0) {
        for (int s = NS; s < BPS_STICKY_WORDS; ++s) Q.fmask[chain * BPS_STICKY_WORDS + s] = 0ull;
        double* sc = P.scal + chain * 8;
        store_scal6(sc, t0, a, b, tp, tau_ref, c0);
        sc[6] = t0;  // told
        sc[7] = 0.0;
        P.hdr[chain] = devchain_fresh(seed, t0, 1, 1, 2);
    }
}

template <int NS>
static int launch_sticky_ns(const BpsRunParams& p, const BpsStickyParams& q, int64_t nchains, bool init, const uint64_t* seeds, double t0, double c0,
                            void* stream) {
    const size_t lds = (size_t)p.d * 8;
    dim3 grid((unsigned)nchains), block(64);
    const hipStream_t s = (hipStream_t)stream;
    if (p.flow_kind == 1) {
        if (init) hipLaunchKernelGGL((bps_sticky_init_kernel<NS, true>), grid, block, lds, s, p, q, seeds, t0, c0);
        else hipLaunchKernelGGL((bps_sticky_run_kernel<NS, true>), grid, block, lds, s, p, q);
    } else {
        if (init) hipLaunchKernelGGL((bps_sticky_init_kernel<NS, false>), grid, block, lds, s, p, q, seeds, t0, c0);
        else hipLaunchKernelGGL((bps_sticky_run_kernel<NS, false>), grid, block, lds, s, p, q);
    }
    return (int)hipGetLastError();
}
static int dispatch_sticky(const BpsRunParams& p, const BpsStickyParams& q, int64_t nchains, bool init, const uint64_t* seeds, double t0, double c0,
                           void* stream) {
    // (past NS = 16: set_state_bps refuses d > 1024 on a sticky ensemble)
    return bps_dispatch_ns<16>(p.d, [&](auto ns) { return launch_sticky_ns<decltype(ns)::value>(p, q, nchains, init, seeds, t0, c0, stream); });
}
int launch_bps_sticky_init(const BpsRunParams& p, const BpsStickyParams& q, int64_t nchains, const uint64_t* seeds, double t0, double c0, void* stream) {
    return dispatch_sticky(p, q, nchains, true, seeds, t0, c0, stream);
}
int launch_bps_sticky_run(const BpsRunParams& p, const BpsStickyParams& q, int64_t nchains, void* stream) {
    return dispatch_sticky(p, q, nchains, false, nullptr, 0.0, 0.0, stream);
}

// pdmp_debug_sticky_eval: the sticky loop's scalars as compiled in this unit
__global__ __launch_bounds__(256) void bps_sticky_eval_kernel(int fn, int64_t n, const double* a, const double* b, const double* c, double* out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    if (fn == 0) out[k] = pdmp_atan(a[k]);
    else if (fn == 1) out[k] = bps_freeze_lin(a[k], b[k]);
    else out[k] = bps_freeze_boom(a[k], b[k], c[k]);
}
int launch_bps_sticky_eval(int fn, int64_t n, const double* a, const double* b, const double* c, double* out, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(bps_sticky_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fn, n, a, b, c, out);
    return (int)hipGetLastError();
}
