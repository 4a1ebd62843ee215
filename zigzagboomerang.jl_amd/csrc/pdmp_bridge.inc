// pdmp_bridge.inc -- the diffusion bridge in the Faber-Schauder basis (research/diffusion_bridge/diffbridge.jl, faberschauder.jl): the local
// ZigZag with a gradient that moves what it reads (SelfMoving / ExtendedForm, src/sfact.jl:57-68).  Included by pdmp_general.hip, inside
// namespace pdmp.
//
// spdmp_inner! (src/sfact.jl:73-145) under `while t′ < T′` (:199-208) with the flow ZigZag(I, 0): G[i] = G1[i] = {i}, G2[i] is empty, so a
// proposal of i moves i, evaluates ∇ϕmoving (faberschauder.jl:137-144) and re-bounds i alone, accepted or not.  No neighbourhood table exists:
// the gradient draws a time s in the support of basis function i and reads the L + 1 coefficients whose basis functions cover s, one per
// level, moving each to t′ first (dotψmoving, :37-46).  Mapping: one chain per wavefront, one proposal per iteration; lane lev = 0..L
// owns level lev: it computes its index j, gathers the record, moves it, writes (t, x) back and forms ξ[j] Λ(s, L − lev, T).  The terms are
// added in lev order by lane reads (the reference's summation order; no tree), after the end-point term.  Records and the two-level
// exact-minimum queue are the one-event kernel's (pdmp_engine.hpp, pdmp_device.hpp); the records stay in HBM.
// Draws: rand() of :141 is draw ng of PDMP_STREAM_GLOBAL; the thinning coin is draw nm and the re-bound draw nm + 1 of PDMP_STREAM_MAIN.
// The drift is b(x) = −βx + α sin(ωx) with its true derivatives.  A chain whose |ωx| leaves pdmp_sincos' range, or whose s is not below T
// (the reference then indexes ξ out of bounds), ends as PDMP_CHAIN_STALLED.  tests/ref/bridge_ref.c is the same arithmetic, sequentially.

__global__ __launch_bounds__(64) void zz_bridge_run_kernel(ZzRunParams P, ZzBridgeParams B) {
    const int lane = threadIdx.x;
    const int64_t chain = blockIdx.x;
    const int64_t d = P.d;
    const uint32_t nblk = P.nblk;  // <= 64 (L <= 10: 33 blocks): one block minimum per lane

    __shared__ double bk[64];    // block minima
    __shared__ uint32_t bi[64];  // block argmin (coordinate id)

    ZzRec* rec = P.rec + chain * d;
    double* keys = P.keys + chain * P.dk;
    DevChain* hdr = P.hdr + chain;
    pdmp_event* ev = P.ev ? P.ev + chain * P.trace_cap : nullptr;
    double* cmut = P.c_chain ? (P.c_chain + chain * d) : nullptr;
    const double* cvec = cmut ? cmut : P.tb.c_shared;

    uint32_t status = hdr->c.status;
    if (chain_ended(status)) return;
    const uint64_t seed = hdr->seed;
    const uint64_t nm0 = hdr->c.ndraw_main;
    uint64_t nm = nm0, ng = hdr->c.ndraw_global;
    uint64_t num = hdr->c.num, nacc = hdr->c.nacc, ntrace = hdr->c.ntrace, nevents = hdr->c.nevents;
    double t_last = hdr->c.t_last;
    double t_event = hdr->t_event;
    status = PDMP_CHAIN_OK;
    const double T = P.T;
    const bool stop_before = (P.flags & PDMP_RUN_STOP_BEFORE) != 0;
    const bool adapt = P.adapt != 0;

    const int L = B.L;
    const double Tb = B.T, sT = sqrt(Tb);
    const double aw = B.alpha * B.omega, aww = aw * B.omega;
    // what lane lev keeps of its level: 2^(L − lev), its square root, the index stride 2 << lev and offset 1 << lev (faberschauder.jl:6,41)
    const bool lev_on = lane <= L;
    const int lm = lev_on ? (L - lane) : 0;
    const double p2 = (double)(1u << lm), sq2 = sqrt(p2);
    const uint32_t jstride = lev_on ? (2u << lane) : 0u, joff = lev_on ? (1u << lane) : 0u;
    // the end points are fixed (θ = 0, c = 0: pdmp_ensemble_set_state checks it): never moved, never popped, read once
    const double x_first = rec[0].x, x_last = rec[d - 1].x;

    level1_build(bk, bi, keys, nblk, lane);  // (nblk <= 64 here: each lane scans one block)
    PDMP_LDS_ORDER();

    bool running = stop_before || (t_event < T);  // `while t′ < T′`, src/sfact.jl:199
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
        // ---------------- peek(Q), src/sfact.jl:77
        const double mk = ((uint32_t)lane < nblk) ? bk[lane] : PDMP_INF;
        const double tp = wave_min_f64(mk);
        if (!(tp < PDMP_INF)) {  // +Inf (or NaN): nothing can happen any more
            status = PDMP_CHAIN_STALLED;
            break;
        }
        if (stop_before && !(tp < T)) break;
        const uint64_t ball = __ballot(mk == tp);
        const uint32_t blk = (uint32_t)(__ffsll((unsigned long long)ball) - 1);  // exact ties: the lowest block, i.e. the lowest coordinate
        const uint32_t i = uniform_u32(bi[blk]);
        t_last = tp;
        if (i == 0u || i >= (uint32_t)(d - 1)) {  // (an end point's key is +Inf: unreachable; keeps every index below in bounds)
            status = PDMP_CHAIN_STALLED;
            break;
        }

        const ZzRec* ri = rec + i;
        const double x_i0 = ri->x, th_i = ri->th, t_i = ri->t;
        const double told_i = ri->t_old, a_i = ri->a, b_i = ri->b;
        const uint64_t acc_i = ri->acc;
        // ---------------- smove_forward!(G, i, t, x, θ, t′, F) with G[i] = {i}, src/sfact.jl:82
        double x_i = x_i0 + th_i * (tp - t_i);
        // ---------------- ∇ϕmoving, faberschauder.jl:137-144
        const int l = __builtin_ctz(i);                          // lvl(i, L) = lvl0(i − 1), :61-68,81-87 (0-based i)
        const uint32_t k = i >> (l + 1);                         // (i − 1) ÷ (2 << l), :139
        const double delta = Tb / (double)(1u << (L - l));       // :140
        const double s = delta * ((double)k + pdmp_u01(seed, PDMP_STREAM_GLOBAL, ng));  // :141
        ng += 1;
        if (!(s < Tb)) {
            if (lane == 63) {
                rec[i].x = x_i;
                rec[i].t = tp;
            }
            status = PDMP_CHAIN_STALLED;
            break;
        }
        const double sr = s / Tb;
        double r = s / sT * x_last + sT * (1 - sr) * x_first;  // :39
        double term = 0.0, lam = 0.0;
        if (lev_on) {  // dotψmoving, :40-44: lane lev moves ξ[j] to t′ and forms ξ[j] Λ(s, L − lev, T)
            uint32_t j = (uint32_t)(sr * p2) * jstride + joff;
            j = (j < (uint32_t)d) ? j : (uint32_t)(d - 1);
            ZzRec* rj = rec + j;
            const bool own = j == i;  // (level l: the proposal's own coordinate, moved above -- this move is by t′ − t′)
            const double xj = own ? x_i : rj->x, thj = own ? th_i : rj->th, tj = own ? tp : rj->t;
            const double xn = xj + thj * (tp - tj);  // smove_forward!(j, t, ξ, θ, t′, F), src/sfact.jl:13-16
            if (!own) {
                rj->x = xn;
                rj->t = tp;
            }
            const double f = fmod(s * p2, Tb);
            lam = (sT * 0.5 - fabs(f / sT - sT * 0.5)) / sq2;  // Λ(s, L − lev, T), :3-6
            term = xn * lam;
            if (own) x_i = xn;
        }
        x_i = readlane_f64(x_i, l);  // (lane l's copy carries the second move where its j is i; elsewhere it is the first move's value)
        if (lane == 63) {
            rec[i].x = x_i;
            rec[i].t = tp;
        }
        for (int lev = 0; lev <= L; ++lev) r += readlane_f64(term, lev);  // r += ξ[j]*Λ(s, L − lev, T) in lev order, :43
        const double lam_l = readlane_f64(lam, l);
        const double w = B.omega * r;
        if (!(fabs(w) <= PDMP_SINCOS_MAX)) {
            status = PDMP_CHAIN_STALLED;
            break;
        }
        double sn, cs;
        pdmp_sincos(w, &sn, &cs);
        const double b0 = -B.beta * r + B.alpha * sn;  // b(x)
        const double b1 = -B.beta + aw * cs;           // b′(x)
        const double b2 = -(aww * sn);                 // b″(x)
        const double g = 0.5 * delta * lam_l * (2 * b0 * b1 + b2) + x_i;  // :143

        const double l_rate = pos_part(g * th_i);                   // sλ, src/sfact.jl:69,119
        const double lbound = pos_part(a_i + b_i * (tp - told_i));  // sλ̄, :70,119
        num += 1;                                                   // :120
        const double ucoin = pdmp_u01(seed, PDMP_STREAM_MAIN, nm);
        nm += 1;
        const bool accept = (ucoin * lbound < l_rate);  // :121
        double cj = cvec[i];
        double th_new = th_i;
        if (accept) {
            nacc += 1;
            if (l_rate >= lbound) {  // :123
                if (!adapt) {        // error("Tuning parameter `c` too small."), :124 -> the chain's status word
                    status = PDMP_CHAIN_BOUND_VIOLATED;
                    break;
                }
                cj *= P.factor;  // adapt!(c, i, factor), :127
                if (lane == 63) cmut[i] = cj;
            }
            th_new = -th_i;  // reflect!, :130
        }
        // ---------------- b[i] = ab(G1, i, x, θ, c, F); t_old[i] = t[i]; Q[i] = t[i] + poisson_time(b[i], rand(rng)), :131-135 / :137-139
        const double gx = 0.0 + 1.0 * x_i, gt = 0.0 + 1.0 * th_new;  // idot(Γ, i, ·) with Γ = I, src/common.jl:16-24
        const double a = cj + (gx - 0.0) * th_new;                    // src/fact_samplers.jl:51
        const double b = cj / 100 + th_new * gt;                      // :52
        const double key = tp + poisson_time_L(a, b, pdmp_log(pdmp_u01(seed, PDMP_STREAM_MAIN, nm)));
        nm += 1;
        if (lane == 63) {
            ZzRec* wi = rec + i;
            wi->th = th_new;
            wi->t_old = tp;
            wi->a = a;
            wi->b = b;
            wi->acc = acc_i + (accept ? 1u : 0u);
            keys[i] = key;
        }
        level1_update(bk, bi, keys, lane, i, key);
        PDMP_LDS_ORDER();
        if (accept) {  // push!(Ξ, event(i, t, x, θ, F)), :143,202
            if (ev && lane == 0) {
                pdmp_event e;
                e.t = tp;
                e.i = (int64_t)i;
                e.x = x_i;
                e.theta = th_new;
                ev[ntrace] = e;
            }
            ntrace += 1;
            nevents += 1;
            t_event = tp;
            if (!stop_before && !(tp < T)) running = false;
        }
    }

    if (lane == 0) {
        hdr->c.t_last = t_last;
        hdr->t_event = t_event;
        hdr->c.num = num;
        hdr->c.nacc = nacc;
        hdr->c.ntrace = ntrace;
        hdr->c.nevents = nevents;
        hdr->c.ndraw_main = nm;
        hdr->c.ndraw_global = ng;
        hdr->c.status = status;
    }
}

int launch_zz_bridge_run(const ZzRunParams& p, const ZzBridgeParams& b, int64_t nchains, void* stream) {
    if (p.nblk > 64u || b.L < 0 || b.L > PDMP_BRIDGE_LMAX || p.d != ((int64_t)2 << b.L) + 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(zz_bridge_run_kernel, dim3((unsigned)nchains), dim3(64), 0, (hipStream_t)stream, p, b);
    return (int)hipGetLastError();
}
