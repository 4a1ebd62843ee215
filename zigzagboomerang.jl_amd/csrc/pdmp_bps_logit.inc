// pdmp_bps_logit.inc -- the speed-recorded Bouncy Particle (pdmp_bps_modern.inc's loop, src/not_fact_samplers.jl:151-384) on a Bayesian
// logistic-regression target, the reference's own application of that driver (turing/lr.jl:105-139, tilde/lr.jl:55-98).  Included by
// pdmp_bps.hip (inside namespace pdmp) after pdmp_bps_modern.inc.  With η = A x, ζ = A θ, p_i = inv(1 + exp(−η_i)):
//   ϕ(x)    = Σ_i [m_i log(1 + e^{η_i}) − y_i η_i] + (γ0/2)‖x‖²
//   ∇ϕ!(x)  = A'r + γ0 x,  r_i = m_i p_i − y_i
//   dϕ(x,θ) = (Σ_i r_i ζ_i + γ0 θ·x,  Σ_i m_i p_i (1 − p_i) ζ_i² + γ0 θ·θ)
// The loop, the draws, the tie rule, the statuses and the flow forms are bps_modern_run_kernel's; only dϕ and ∇ϕ! differ.  The Gaussian kernel
// is left as it is (DESIGN.md §4: it is sensitive to sharing); this one is built on its helpers (BpsModernOps: rebound, record_rate, normals)
// and on BpsWave.
// Layout: one chain per wavefront, x and θ in registers (element e = slot*64 + lane), and in LDS the [d] staging buffer followed by η[n]
// and ζ[n]; observation i belongs to lane i & 63.  A move costs d/64 register updates and n/64 LDS fused multiply-adds per lane, a bound
// n/64 pdmp_exp per lane and two wave sums; the O(nnz A) gathers happen only when θ changes (ζ), at a record (η) and inside an accepted
// bounce (A'r, with r staged in ζ's array: ζ is recomputed from the new θ straight afterwards).
// The arithmetic tests/ref/bps_logistic_ref.c fixes:
//   ζ_i  one idot of At[:, i] against θ, ascending coordinates; recomputed whenever θ changes (setup, refreshment, accepted bounce)
//   η_i  gathered from x the same way at setup and again at every record; between those points every move is η_i = fma(τ, ζ_i, η_i)
//   dϕ   per-lane partial sums over i = l, l + 64, ... of r_i ζ_i and of ((m_i w_i) ζ_i) ζ_i, the xor butterfly (wave_sum_f64), then
//        + γ0 · dot(θ, x) and + γ0 · dot(θ, θ)
//   ∇ϕ!  r[n] staged, one idot of A[:, e] against r per coordinate (ascending rows), then + γ0 x_e
// Chain state between launches: what bps_modern_run_kernel keeps, and η in BpsLogitParams::eta [nchains x n]: a launch can stop between two
// records, where an η gathered afresh from x is not the incrementally advanced one.  ζ is gathered from θ at the start of a launch (exact).

template <int NS>
struct BpsLogitOps {
    const BpsLogitParams& G;
    BpsWave<NS> wv;  // tmp: the [d] staging buffer
    double* eta;     // LDS [n]
    double* zeta;    // LDS [n]
    int lane;
    // out[i] = idot(At[:, i], v) for the lane's observations
    __device__ __forceinline__ void gather_obs(const double (&v)[NS], double* out) const {
        wv.stage(v, nullptr, false);
        for (int64_t i = lane; i < G.n; i += 64) out[i] = wv.idot(G.At_colptr, G.At_rowval, G.At_nzval, i);
        asm volatile("" ::: "memory");
    }
    __device__ __forceinline__ void moved(double tau) const {
        for (int64_t i = lane; i < G.n; i += 64) eta[i] = fma(tau, zeta[i], eta[i]);
    }
    __device__ __forceinline__ void dphi(const double (&x)[NS], const double (&th)[NS], double& d1, double& d2) const {
        double s1 = 0.0, s2 = 0.0;
        for (int64_t i = lane; i < G.n; i += 64) {
            double p, w;
            logit_link(eta[i], &p, &w);
            const double mi = G.m[i], z = zeta[i];
            s1 += (mi * p - G.y[i]) * z;
            s2 += ((mi * w) * z) * z;
        }
        d1 = wave_sum_f64(s1) + G.gamma0 * wv.dot(th, x);
        d2 = wave_sum_f64(s2) + G.gamma0 * wv.dot(th, th);
    }
    // g = ∇ϕ!(x); leaves r in ζ's array: theta_changed() follows
    __device__ __forceinline__ void grad(const double (&x)[NS], double (&g)[NS]) const {
        for (int64_t i = lane; i < G.n; i += 64) {
            double p, w;
            logit_link(eta[i], &p, &w);
            zeta[i] = G.m[i] * p - G.y[i];
        }
        asm volatile("" ::: "memory");
        const BpsWave<NS> rv{lane, wv.d, zeta};
        rv.gather(G.A_colptr, G.A_rowval, G.A_nzval, g);
#pragma unroll
        for (int s = 0; s < NS; ++s) g[s] = g[s] + G.gamma0 * x[s];
        asm volatile("" ::: "memory");
    }
};

template <int NS, bool UDIAG, bool OSCN>
__global__ __launch_bounds__(64) void bps_logit_run_kernel(BpsRunParams P, BpsModernParams Q, BpsLogitParams G) {
    const int lane = threadIdx.x;
    const int64_t chain = blockIdx.x;
    const int64_t d = P.d, n = G.n;
    extern __shared__ __align__(16) unsigned char smem[];
    double* tmp = reinterpret_cast<double*>(smem);  // [d] staging, then η[n], ζ[n]
    double* eta = tmp + d;
    double* zeta = eta + n;

    double* gx = P.x + chain * d;
    double* gth = P.th + chain * d;
    double* geta = G.eta + chain * n;
    double* sc = P.scal + chain * 8;    // {t, a, b, tp, -, c, -, -}
    double* ms = Q.mstate + chain * 4;  // {Δ, action, V, Δrec}
    DevChain* hdr = P.hdr + chain;

    uint32_t status = hdr->c.status;
    if (bps_chain_ended(status)) return;
    status = PDMP_CHAIN_OK;
    const uint64_t seed = hdr->seed;
    BpsCounters k;
    k.load(hdr);
    const uint64_t nm0 = k.nm;
    double t = sc[0], a = sc[1], b = sc[2], tp = sc[3], c = sc[5];
    double Delta = ms[0], V = ms[2], Drec = ms[3];
    int action = (int)ms[1];

    const BpsWave<NS> wv{lane, d, tmp};
    double x[NS], th[NS];
    wv.load_state(gx, gth, x, th);
    const double rho = P.rho, rhobar = sqrt(1 - rho * rho);
    const double T = P.T;
    const bool stop_before = (P.flags & PDMP_RUN_STOP_BEFORE) != 0;
    const bool has_mass = !UDIAG && !OSCN && P.Lcp != nullptr;
    const uint64_t nlimit = (uint64_t)Q.record_limit;
    const BpsModernOps<NS, UDIAG> mo{P, Q, tmp, lane, d, seed};
    const BpsLogitOps<NS> lg{G, wv, eta, zeta, lane};

    for (int64_t i = lane; i < n; i += 64) eta[i] = geta[i];  // carried, not gathered: see the header
    lg.gather_obs(th, zeta);

    auto move = [&](double tau) {
        t += tau;
#pragma unroll
        for (int s = 0; s < NS; ++s) x[s] += th[s] * tau;
    };

    bool running = (stop_before || (t < T)) && (nlimit == 0 || k.nevents < nlimit);  // :360
    while (running) {
        if (P.trace_cap > 0 && k.ntrace >= (uint64_t)P.trace_cap) {
            status = PDMP_CHAIN_TRACE_FULL;
            break;
        }
        if ((uint32_t)(k.nm - nm0) >= Q.count_limit) {
            status = PDMP_CHAIN_PAUSED;
            break;
        }
        const double trec = t + Drec / V;
        const bool is_rec = trec <= tp;  // :223
        if (stop_before && !((is_rec ? trec : tp) < T)) break;
        if (is_rec) {  // :224-236
            const double tau = Drec / V;
            move(tau);
            lg.gather_obs(x, eta);  // the record is where the sample is taken: η = A x afresh
            Drec = 1 / P.lambda_ref;
            double d1, d2;
            lg.dphi(x, th, d1, d2);
            const double lb = pos_part(a + b * tau);
            if (d1 > lb) {  // check bounds on recordings
                if (!P.adapt) {
                    status = PDMP_CHAIN_BOUND_VIOLATED;
                    break;
                }
                c *= P.factor;
            }
            mo.rebound(t, c, V, d1, d2, k.nm, a, b, Delta, tp, action);
            wv.emit_record(P, chain, k.ntrace, t, x, th);  // push!(Ξ, event(t, x, θ, flow)), :362
            k.ntrace += 1;
            k.nevents += 1;
            if (!stop_before && !(t < T)) running = false;
            if (nlimit != 0 && k.nevents >= nlimit) running = false;
            continue;
        }
        Drec = Drec - (tp - t) * V;  // :238
        if (!(Drec > 0.0)) {         // @assert Δrec > 0.0, :239
            status = PDMP_CHAIN_STALLED;
            break;
        }
        const double tau = tp - t;
        move(tau);
        lg.moved(tau);
        double d1, d2;
        if (action == 2) {  // :240-246
            mo.normals(k.nm);
            k.nm += normal_draws(d);
            if (has_mass) wv.solve_upper(P);  // L'\randn(rng, d), :177
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                th[s] *= rho;
                if (wv.has(s)) {
                    if constexpr (UDIAG) th[s] += (1.0 * rhobar) * (Q.su_diag[wv.elem(s)] * tmp[wv.elem(s)]);  // unwhiten(U, z) = √u .* z, :169
                    else th[s] += (1.0 * rhobar) * tmp[wv.elem(s)];
                }
            }
            asm volatile("" ::: "memory");
            V = mo.record_rate(th);
            k.nrefresh += 1;
            lg.gather_obs(th, zeta);
            lg.dphi(x, th, d1, d2);
        } else if (action == 1) {  // :247-252
            lg.dphi(x, th, d1, d2);
        } else {  // :253-281
            const double coin = pdmp_u01(seed, PDMP_STREAM_MAIN, k.nm);
            lg.dphi(x, th, d1, d2);
            const double lb = pos_part(a + b * tau);
            k.num += 1;
            k.nm += 1;
            if (coin * lb <= d1) {
                k.nacc += 1;
                if (d1 > lb) {
                    if (!P.adapt) {
                        status = PDMP_CHAIN_BOUND_VIOLATED;
                        break;
                    }
                    c *= P.factor;
                }
                double g[NS];
                lg.grad(x, g);         // ∇ϕ!, :265
                if constexpr (OSCN) {  // oscn!(rng, θ, ∇ϕx, ρ; normalize=false), src/oscn.jl
                    const double gg = wv.dot(g, g);
                    const double cp = wv.dot(th, g) / gg;
                    if (rho == 1) {
#pragma unroll
                        for (int s = 0; s < NS; ++s) th[s] = th[s] - 2 * (cp * g[s]);
                    } else {
                        mo.normals(k.nm);
                        k.nm += normal_draws(d);
                        const double sq = sqrt(1.0 - rho * rho);
                        double z[NS];
#pragma unroll
                        for (int s = 0; s < NS; ++s) z[s] = wv.has(s) ? tmp[wv.elem(s)] * sq : 0.0;
                        asm volatile("" ::: "memory");
                        const double cz = wv.dot(z, g) / gg;
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
                    for (int s = 0; s < NS; ++s) w[s] = wv.has(s) ? Q.u_diag[wv.elem(s)] * g[s] : 0.0;
                    const double coef = 2 * wv.dot(g, th) / wv.dot(g, w);
#pragma unroll
                    for (int s = 0; s < NS; ++s) th[s] -= coef * w[s];
                } else if (has_mass) {  // :161-164
                    const double gt = wv.dot(g, th);
                    wv.stage(g, nullptr, false);
                    wv.solve_lower(P);
#pragma unroll
                    for (int s = 0; s < NS; ++s) g[s] = wv.has(s) ? tmp[wv.elem(s)] : 0.0;
                    const double nrm = wv.dot(g, g);
                    wv.solve_upper(P);
                    const double coef = 2 * gt / nrm;
                    wv.each([&](int s, int64_t e) { th[s] -= coef * tmp[e]; });
                    asm volatile("" ::: "memory");
                } else {
                    const double coef = 2 * wv.dot(g, th) / wv.dot(g, g);
#pragma unroll
                    for (int s = 0; s < NS; ++s) th[s] -= coef * g[s];
                }
                V = mo.record_rate(th);
                lg.gather_obs(th, zeta);
                lg.dphi(x, th, d1, d2);
            }
        }
        mo.rebound(t, c, V, d1, d2, k.nm, a, b, Delta, tp, action);
    }

    wv.each([&](int s, int64_t e) {
        gx[e] = x[s];
        gth[e] = th[s];
    });
    asm volatile("" ::: "memory");
    for (int64_t i = lane; i < n; i += 64) geta[i] = eta[i];
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
        k.store(hdr, t, status);
    }
}

// The driver's head, :337-355, with η = A x0 and ζ = A θ0 gathered first; η goes to the chain's global row.
template <int NS, bool UDIAG>
__global__ __launch_bounds__(64) void bps_logit_init_kernel(BpsRunParams P, BpsModernParams Q, BpsLogitParams G, const uint64_t* seeds, double t0,
                                                            double c0) {
    const int lane = threadIdx.x;
    const int64_t chain = blockIdx.x;
    const int64_t d = P.d, n = G.n;
    extern __shared__ __align__(16) unsigned char smem[];
    double* tmp = reinterpret_cast<double*>(smem);
    double* eta = tmp + d;
    double* zeta = eta + n;
    const uint64_t seed = seeds[chain];
    const BpsWave<NS> wv{lane, d, tmp};
    double x[NS], th[NS];
    wv.load_state(P.x + chain * d, P.th + chain * d, x, th);
    const BpsModernOps<NS, UDIAG> mo{P, Q, tmp, lane, d, seed};
    const BpsLogitOps<NS> lg{G, wv, eta, zeta, lane};
    lg.gather_obs(x, eta);
    lg.gather_obs(th, zeta);
    const double V = mo.record_rate(th);
    double d1, d2, a, b, Delta, tp;
    int action;
    uint64_t nm = 0;
    lg.dphi(x, th, d1, d2);
    mo.rebound(t0, c0, V, d1, d2, nm, a, b, Delta, tp, action);
    double* geta = G.eta + chain * n;
    for (int64_t i = lane; i < n; i += 64) geta[i] = eta[i];
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

// a kernel that takes more than 64 KiB of dynamic LDS opts in first
template <class K, class... Args>
static int launch_logit_kernel(K kernel, size_t lds, int64_t nchains, void* stream, Args... args) {
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)nchains), dim3(64), lds, (hipStream_t)stream, args...);
    return (int)hipGetLastError();
}
template <int NS>
static int launch_logit_ns(const BpsRunParams& p, const BpsModernParams& q, const BpsLogitParams& g, int64_t nchains, bool init, const uint64_t* seeds,
                           double t0, double c0, void* stream) {
    const size_t lds = bps_logit_lds_bytes(p.d, g.n);
    if (lds > BPS_LOGIT_LDS_MAX) return (int)hipErrorInvalidValue;  // (set_state_bps refuses it first)
    const bool udiag = q.u_diag != nullptr;
    if (init) {
        if (udiag) return launch_logit_kernel(bps_logit_init_kernel<NS, true>, lds, nchains, stream, p, q, g, seeds, t0, c0);
        return launch_logit_kernel(bps_logit_init_kernel<NS, false>, lds, nchains, stream, p, q, g, seeds, t0, c0);
    }
    if (udiag) return launch_logit_kernel(bps_logit_run_kernel<NS, true, false>, lds, nchains, stream, p, q, g);
    if (q.oscn) return launch_logit_kernel(bps_logit_run_kernel<NS, false, true>, lds, nchains, stream, p, q, g);
    return launch_logit_kernel(bps_logit_run_kernel<NS, false, false>, lds, nchains, stream, p, q, g);
}
int launch_bps_logit_init(const BpsRunParams& p, const BpsModernParams& q, const BpsLogitParams& g, int64_t nchains, const uint64_t* seeds, double t0,
                          double c0, void* stream) {
    return bps_dispatch_ns<16>(p.d, [&](auto ns) { return launch_logit_ns<decltype(ns)::value>(p, q, g, nchains, true, seeds, t0, c0, stream); });
}
int launch_bps_logit_run(const BpsRunParams& p, const BpsModernParams& q, const BpsLogitParams& g, int64_t nchains, void* stream) {
    return bps_dispatch_ns<16>(p.d, [&](auto ns) { return launch_logit_ns<decltype(ns)::value>(p, q, g, nchains, false, nullptr, 0.0, 0.0, stream); });
}
