// pdmp_bps_modern.inc -- the speed-recorded Bouncy Particle ("ModernBPS"): pdmp_inner! (src/not_fact_samplers.jl:213-283) under its driver
// `while T isa Int ? iter < T : t < T` (:336-384), c::LocalBound, Gaussian target dϕ = (θ'Γt(x−μt), θ'Γtθ), ∇ϕ! = Γt(x−μt).  Included by
// pdmp_bps.hip (inside namespace pdmp) after the sticky kernels: one chain per wavefront, x and θ in registers (element e = slot*64 + lane).
// The loop needs only the two scalars of dϕ per bound (two CSC gathers through the LDS staging buffer, two wave sums); the gradient VECTOR
// exists only inside an accepted bounce, so there is no persistent g[NS] beside x and θ.  A record (t, x, θ) is written once per 1/λref of
// speed-time ∫V dt, not once per event.
// Draws, PDMP_STREAM_MAIN in program order: next_event1 takes 2 (poisson_time's uniform, then randexp of τrefresh) at setup and after every
// record, refreshment, expiry and proposal; a proposal takes the coin first; refresh! and oscn! (ρ != 1) take ((d+127)>>7)<<6 Box-Muller
// blocks in bps_run_kernel's refresh mapping.  No τref draw at setup.
// Ties: findmin((τ, Δ, τrefresh)) takes the first minimum (bounce, expire, refresh); a NaN never wins.
// Flow forms: L form (UDIAG = false): V ≡ 1, reflect! :161-164, refresh! :173-180, L = I or the lower CSC factor of BpsRunParams (the
// substitutions of bps_run_kernel); diagonal-U form (UDIAG = true): z = u .* ∇ϕx in reflect! (:156-160), unwhiten = √u .* z in refresh!
// (:165-172), V = ‖θ ./ √u‖ (:197).  OSCN: src/oscn.jl with normalize = false (L = I only).
// Kept as the reference has them: the record branch checks l > lb with τ = Δrec/V (:224-232); acc += 1 before the bound check; the coin is
// <=; the first trace element is the first record; `@assert Δrec > 0` (:239) failing ends the chain as PDMP_CHAIN_STALLED.
// Chain state between launches: scal {t, a, b, t′, -, c, -, -} as the plain kernels keep it, and BpsModernParams::mstate {Δ, action, V, Δrec}.
// From pdmp_bps_common.hpp: the gather, the staging, dot and the substitutions (BpsWave), the status gate, the fresh header, the
// dispatcher.  The run kernel keeps its own Box-Muller fill, fused θ'Γ sum, record store, counters and state load / store: with the
// shared forms its code is no longer the measured one, and it timed 0.4 % slower (DESIGN.md §4).

// What the init and the run kernel share: dϕ, ab and next_event1, record_rate.
template <int NS, bool UDIAG>
struct BpsModernOps {
    const BpsRunParams& P;
    const BpsModernParams& Q;
    double* tmp;
    int lane;
    int64_t d;
    uint64_t seed;
    __device__ __forceinline__ BpsWave<NS> wv() const { return {lane, d, tmp}; }
    // y = Γt(in − μt) or Γt in: the CSC gather through LDS, idot order
    __device__ __forceinline__ void gamma(const double (&in)[NS], bool sub_mu, double (&out)[NS]) const {
        wv().csc_gather(P.t_colptr, P.t_rowval, P.t_nzval, P.t_mu, in, sub_mu, out);
    }
    __device__ __forceinline__ double dot(const double (&u)[NS], const double (&v)[NS]) const { return wv().dot(u, v); }
    // θdϕ, v = dϕ(t, x, θ, flow)
    // (each product's elements go straight into the lane's partial sum, slot by slot as dot() adds them: no d-vector is kept)
    __device__ __forceinline__ double th_gamma(const double (&in)[NS], bool sub_mu, const double (&th)[NS]) const {
        wv().stage(in, P.t_mu, sub_mu);
        double part = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int64_t e = (int64_t)s * 64 + lane;
            if (e < d) {
                double y = 0.0;
                for (int64_t p = P.t_colptr[e]; p < P.t_colptr[e + 1]; ++p) y += P.t_nzval[p] * tmp[P.t_rowval[p]];
                part += th[s] * y;
            }
        }
        return wave_sum_f64(part);
    }
    __device__ __forceinline__ void dphi(const double (&x)[NS], const double (&th)[NS], double& d1, double& d2) const {
        d1 = th_gamma(x, true, th);
        d2 = th_gamma(th, false, th);
    }
    // record_rate(θ, F), :197-198
    __device__ __forceinline__ double record_rate(const double (&th)[NS]) const {
        if constexpr (UDIAG) {
            double part = 0.0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int64_t e = (int64_t)s * 64 + lane;
                if (e < d) {
                    const double q = th[s] / Q.su_diag[e];
                    part += q * q;
                }
            }
            return sqrt(wave_sum_f64(part));
        } else {
            return 1.0;
        }
    }
    // abc = ab(t, x, θ, V, c, θdϕ, v, flow) (:200-202); t′, action = next_event1 (:204-211), draws nm and nm + 1
    __device__ __forceinline__ void rebound(double t, double c, double V, double d1, double d2, uint64_t& nm, double& a, double& b, double& Delta,
                                            double& tp, int& action) const {
        a = c + d1;
        b = d2;
        Delta = t + 2 * sqrt((double)d) / c / V;
        const double tau_b = t + bps_next_dt(seed, nm, a, b);
        const double tau_r = t + (-pdmp_log(pdmp_u01(seed, PDMP_STREAM_MAIN, nm + 1)) / P.lambda_ref) / V;
        nm += 2;
        if (tau_b <= Delta && tau_b <= tau_r) {
            action = 0;
            tp = tau_b;
        } else if (Delta <= tau_r) {
            action = 1;
            tp = Delta;
        } else {
            action = 2;
            tp = tau_r;
        }
    }
    // randn(rng, d) into tmp: the refresh mapping of bps_run_kernel
    __device__ __forceinline__ void normals(uint64_t nm) const {
        asm volatile("" ::: "memory");
#pragma unroll 1
        for (int a2 = 0; a2 < (NS + 1) / 2; ++a2) {
            const int64_t e0 = (int64_t)a2 * 128 + lane, e1 = e0 + 64;
            double z0, z1;
            pdmp_randn2(seed, PDMP_STREAM_MAIN, nm + (uint64_t)(a2 * 64 + lane), &z0, &z1);
            if (e0 < d) tmp[e0] = z0;
            if (e1 < d) tmp[e1] = z1;
        }
        asm volatile("" ::: "memory");
    }
};

template <int NS, bool UDIAG, bool OSCN>
__global__ __launch_bounds__(64) void bps_modern_run_kernel(BpsRunParams P, BpsModernParams Q) {
    const int lane = threadIdx.x;
    const int64_t chain = blockIdx.x;
    const int64_t d = P.d;
    extern __shared__ __align__(16) unsigned char smem[];
    double* tmp = reinterpret_cast<double*>(smem);  // [d] operand of the CSC gather; the normals of a refresh / oscn; the substitutions

    double* gx = P.x + chain * d;
    double* gth = P.th + chain * d;
    double* sc = P.scal + chain * 8;     // {t, a, b, tp, -, c, -, -}
    double* ms = Q.mstate + chain * 4;   // {Δ, action, V, Δrec}
    DevChain* hdr = P.hdr + chain;

    uint32_t status = hdr->c.status;
    if (bps_chain_ended(status)) return;
    status = PDMP_CHAIN_OK;
    const uint64_t seed = hdr->seed;
    uint64_t nm = hdr->c.ndraw_main;
    const uint64_t nm0 = nm;
    uint64_t num = hdr->c.num, nacc = hdr->c.nacc, nrefresh = hdr->c.nrefresh, ntrace = hdr->c.ntrace, nevents = hdr->c.nevents;
    double t = sc[0], a = sc[1], b = sc[2], tp = sc[3], c = sc[5];
    double Delta = ms[0], V = ms[2], Drec = ms[3];
    int action = (int)ms[1];

    double x[NS], th[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int64_t e = (int64_t)s * 64 + lane;
        const bool in = e < d;
        x[s] = in ? gx[e] : 0.0;
        th[s] = in ? gth[e] : 0.0;
    }
    const double rho = P.rho, rhobar = sqrt(1 - rho * rho);
    const double T = P.T;
    const bool stop_before = (P.flags & PDMP_RUN_STOP_BEFORE) != 0;
    const bool has_mass = !UDIAG && !OSCN && P.Lcp != nullptr;
    const uint64_t nlimit = (uint64_t)Q.record_limit;
    const BpsModernOps<NS, UDIAG> ops{P, Q, tmp, lane, d, seed};

    auto move = [&](double tau) {
        t += tau;
#pragma unroll
        for (int s = 0; s < NS; ++s) x[s] += th[s] * tau;
    };

    bool running = (stop_before || (t < T)) && (nlimit == 0 || nevents < nlimit);  // :360
    while (running) {
        if (P.trace_cap > 0 && ntrace >= (uint64_t)P.trace_cap) {
            status = PDMP_CHAIN_TRACE_FULL;
            break;
        }
        if ((uint32_t)(nm - nm0) >= Q.count_limit) {  // (a launch's draws are counted in 32 bits: pause, the host runs again)
            status = PDMP_CHAIN_PAUSED;
            break;
        }
        const double trec = t + Drec / V;
        const bool is_rec = trec <= tp;  // :223
        if (stop_before && !((is_rec ? trec : tp) < T)) break;
        if (is_rec) {  // :224-236
            const double tau = Drec / V;
            move(tau);
            Drec = 1 / P.lambda_ref;
            double d1, d2;
            ops.dphi(x, th, d1, d2);
            const double lb = pos_part(a + b * tau);
            if (d1 > lb) {  // check bounds on recordings
                if (!P.adapt) {
                    status = PDMP_CHAIN_BOUND_VIOLATED;
                    break;
                }
                c *= P.factor;
            }
            ops.rebound(t, c, V, d1, d2, nm, a, b, Delta, tp, action);
            // push!(Ξ, event(t, x, θ, flow)), :362
            if (P.trace_cap > 0) {
                const int64_t slot = chain * P.trace_cap + (int64_t)ntrace;
                if (lane == 0) P.ev_t[slot] = t;
                double* ex = P.ev_x + slot * d;
                double* eth = P.ev_th + slot * d;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int64_t e = (int64_t)s * 64 + lane;
                    if (e < d) {
                        ex[e] = x[s];
                        eth[e] = th[s];
                    }
                }
            }
            ntrace += 1;
            nevents += 1;
            if (!stop_before && !(t < T)) running = false;
            if (nlimit != 0 && nevents >= nlimit) running = false;
            continue;
        }
        Drec = Drec - (tp - t) * V;  // :238
        if (!(Drec > 0.0)) {         // @assert Δrec > 0.0, :239
            status = PDMP_CHAIN_STALLED;
            break;
        }
        const double tau = tp - t;
        move(tau);
        double d1, d2;
        if (action == 2) {  // :240-246
            ops.normals(nm);
            nm += (uint64_t)(((d + 127) >> 7) << 6);
            if (has_mass) ops.wv().solve_upper(P);  // L'\randn(rng, d), :177
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int64_t e = (int64_t)s * 64 + lane;
                th[s] *= rho;
                if (e < d) {
                    if constexpr (UDIAG) th[s] += (1.0 * rhobar) * (Q.su_diag[e] * tmp[e]);  // unwhiten(U, z) = √u .* z, :169
                    else th[s] += (1.0 * rhobar) * tmp[e];
                }
            }
            asm volatile("" ::: "memory");
            V = ops.record_rate(th);
            nrefresh += 1;
            ops.dphi(x, th, d1, d2);
        } else if (action == 1) {  // :247-252
            ops.dphi(x, th, d1, d2);
        } else {  // :253-281
            const double coin = pdmp_u01(seed, PDMP_STREAM_MAIN, nm);
            ops.dphi(x, th, d1, d2);
            const double lb = pos_part(a + b * tau);
            num += 1;
            nm += 1;
            if (coin * lb <= d1) {
                nacc += 1;
                if (d1 > lb) {
                    if (!P.adapt) {
                        status = PDMP_CHAIN_BOUND_VIOLATED;
                        break;
                    }
                    c *= P.factor;
                }
                double g[NS];
                ops.gamma(x, true, g);  // ∇ϕ!, :265
                if constexpr (OSCN) {   // oscn!(rng, θ, ∇ϕx, ρ; normalize=false), src/oscn.jl
                    const double gg = ops.dot(g, g);
                    const double cp = ops.dot(th, g) / gg;
                    if (rho == 1) {
#pragma unroll
                        for (int s = 0; s < NS; ++s) th[s] = th[s] - 2 * (cp * g[s]);
                    } else {
                        ops.normals(nm);
                        nm += (uint64_t)(((d + 127) >> 7) << 6);
                        const double sq = sqrt(1.0 - rho * rho);
                        double z[NS];
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            const int64_t e = (int64_t)s * 64 + lane;
                            z[s] = (e < d) ? tmp[e] * sq : 0.0;
                        }
                        asm volatile("" ::: "memory");
                        const double cz = ops.dot(z, g) / gg;
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            const double vp = cp * g[s];
                            const double vperp = rho * (th[s] - vp);
                            th[s] = (-vp + vperp) + (z[s] - cz * g[s]);
                        }
                    }
                } else if constexpr (UDIAG) {  // :156-160
                    double w[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int64_t e = (int64_t)s * 64 + lane;
                        w[s] = (e < d) ? Q.u_diag[e] * g[s] : 0.0;
                    }
                    const double coef = 2 * ops.dot(g, th) / ops.dot(g, w);
#pragma unroll
                    for (int s = 0; s < NS; ++s) th[s] -= coef * w[s];
                } else if (has_mass) {  // :161-164
                    const double gt = ops.dot(g, th);
                    asm volatile("" ::: "memory");
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int64_t e = (int64_t)s * 64 + lane;
                        if (e < d) tmp[e] = g[s];
                    }
                    ops.wv().solve_lower(P);
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int64_t e = (int64_t)s * 64 + lane;
                        g[s] = (e < d) ? tmp[e] : 0.0;
                    }
                    const double nrm = ops.dot(g, g);
                    ops.wv().solve_upper(P);
                    const double coef = 2 * gt / nrm;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int64_t e = (int64_t)s * 64 + lane;
                        if (e < d) th[s] -= coef * tmp[e];
                    }
                    asm volatile("" ::: "memory");
                } else {
                    const double coef = 2 * ops.dot(g, th) / ops.dot(g, g);
#pragma unroll
                    for (int s = 0; s < NS; ++s) th[s] -= coef * g[s];
                }
                V = ops.record_rate(th);
                ops.dphi(x, th, d1, d2);
            }
        }
        ops.rebound(t, c, V, d1, d2, nm, a, b, Delta, tp, action);
    }

#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int64_t e = (int64_t)s * 64 + lane;
        if (e < d) {
            gx[e] = x[s];
            gth[e] = th[s];
        }
    }
    if (lane == 0) {
        sc[0] = t;
        sc[1] = a;
        sc[2] = b;
        sc[3] = tp;
        sc[5] = c;
        ms[0] = Delta;
        ms[1] = (double)action;
        ms[2] = V;
        ms[3] = Drec;
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
}

// The driver's head, :337-355: V = record_rate(θ), dϕ, abc = ab(...), Δrec = 1/λref, next_event1 (draws 0 and 1).
template <int NS, bool UDIAG>
__global__ __launch_bounds__(64) void bps_modern_init_kernel(BpsRunParams P, BpsModernParams Q, const uint64_t* seeds, double t0, double c0) {
    const int lane = threadIdx.x;
    const int64_t chain = blockIdx.x;
    const int64_t d = P.d;
    extern __shared__ __align__(16) unsigned char smem[];
    double* tmp = reinterpret_cast<double*>(smem);
    const double* gx = P.x + chain * d;
    const double* gth = P.th + chain * d;
    const uint64_t seed = seeds[chain];
    double x[NS], th[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int64_t e = (int64_t)s * 64 + lane;
        x[s] = (e < d) ? gx[e] : 0.0;
        th[s] = (e < d) ? gth[e] : 0.0;
    }
    const BpsModernOps<NS, UDIAG> ops{P, Q, tmp, lane, d, seed};
    const double V = ops.record_rate(th);
    double d1, d2, a, b, Delta, tp;
    int action;
    uint64_t nm = 0;
    ops.dphi(x, th, d1, d2);
    ops.rebound(t0, c0, V, d1, d2, nm, a, b, Delta, tp, action);
    if (lane == 0) {
        double* sc = P.scal + chain * 8;
        store_scal6(sc, t0, a, b, tp, 0.0, c0);
        sc[6] = 0.0;
        sc[7] = 0.0;
        double* ms = Q.mstate + chain * 4;
        ms[0] = Delta;
        ms[1] = (double)action;
        ms[2] = V;
        ms[3] = 1 / P.lambda_ref;
        P.hdr[chain] = devchain_fresh(seed, t0, 0, 0, nm);
    }
}

template <int NS>
static int launch_modern_ns(const BpsRunParams& p, const BpsModernParams& q, int64_t nchains, bool init, const uint64_t* seeds, double t0, double c0,
                            void* stream) {
    const size_t lds = (size_t)p.d * 8;
    dim3 grid((unsigned)nchains), block(64);
    const hipStream_t s = (hipStream_t)stream;
    const bool udiag = q.u_diag != nullptr;
    if (init) {
        if (udiag) hipLaunchKernelGGL((bps_modern_init_kernel<NS, true>), grid, block, lds, s, p, q, seeds, t0, c0);
        else hipLaunchKernelGGL((bps_modern_init_kernel<NS, false>), grid, block, lds, s, p, q, seeds, t0, c0);
    } else if (udiag) {
        hipLaunchKernelGGL((bps_modern_run_kernel<NS, true, false>), grid, block, lds, s, p, q);
    } else if (q.oscn) {
        hipLaunchKernelGGL((bps_modern_run_kernel<NS, false, true>), grid, block, lds, s, p, q);
    } else {
        hipLaunchKernelGGL((bps_modern_run_kernel<NS, false, false>), grid, block, lds, s, p, q);
    }
    return (int)hipGetLastError();
}
static int dispatch_modern(const BpsRunParams& p, const BpsModernParams& q, int64_t nchains, bool init, const uint64_t* seeds, double t0, double c0,
                           void* stream) {
    // (past NS = 16: set_state_bps refuses d > 1024 on this flow)
    return bps_dispatch_ns<16>(p.d, [&](auto ns) { return launch_modern_ns<decltype(ns)::value>(p, q, nchains, init, seeds, t0, c0, stream); });
}
int launch_bps_modern_init(const BpsRunParams& p, const BpsModernParams& q, int64_t nchains, const uint64_t* seeds, double t0, double c0, void* stream) {
    return dispatch_modern(p, q, nchains, true, seeds, t0, c0, stream);
}
int launch_bps_modern_run(const BpsRunParams& p, const BpsModernParams& q, int64_t nchains, void* stream) {
    return dispatch_modern(p, q, nchains, false, nullptr, 0.0, 0.0, stream);
}
