// pdmp_precision.inc -- learning a sparse precision matrix through its Cholesky factor (casestudies/precision/precision.jl, research/newsticky/
// precision/precision4.jl): the sticky ZigZag on the lower triangle of L.  Included by pdmp_general.hip, inside namespace pdmp.
//
// sspdmp_inner! (src/ss_fact.jl:78-157) under `while t′ < T` (:202-211) with F = ZigZag(Γ̂, μ̂), Γ̂ diagonal: G1[i] = {i}, G[i] is the column of
// i, G2[i] is empty -- an event moves the column and re-bounds i alone.  The coordinates are L[r, c], r >= c, packed column by column:
// i = k0(c) + (r − c), k0(c) = c n − c (c − 1)/2, so the column is the contiguous run of records [k0, k0 + n − c) and
//   ∇ϕ_i = Σ_q YY[r, c + q] u[k0 + q] + (r == c ? −N/u_i + γ0 (u_i − 1) : γ0 u_i)            (precision.jl:42-53, precision4.jl:82-93)
// reads it and one contiguous row segment of YY.  Mapping: one chain per wavefront, one event per iteration; lane q < n − c owns member
// k0 + q: it moves its record to t′ (ssmove_forward!: not where θ = 0), writes (x, t) back and forms the one product YY[r, c + q] u[k0 + q]
// (0.0 in the other lanes); the 64 values are added by wave_sum_f64 and the diagonal or prior term is added to that sum.  No table of
// neighbourhoods exists.  Records and the two-level exact-minimum queue are the one-event kernel's (pdmp_engine.hpp, pdmp_device.hpp); rec.acc
// holds the flag f[i] as in every sticky kernel; the records and YY stay in HBM, YY shared by all chains.
// Draws (PDMP_STREAM_MAIN, the order of the sticky branch above and of orc_sspdmp_zigzag): a freeze takes one (the thaw time, :96), a thaw the
// reversible coin if asked for (:112) and the re-bound of i (:121), a proposal its coin (:130) and the re-bound of i (:144,150).
// A freeze popped for a DIAGONAL coordinate ends the chain as PDMP_CHAIN_STALLED before any state changes (the next gradient would be N/0), and
// so does a thaw that finds no saved speed (a coordinate started at x = 0 with θ = 0).  tests/ref/precision_ref.c is the same arithmetic, sequentially.

__global__ __launch_bounds__(64) void zz_precision_run_kernel(ZzRunParams P, ZzPrecisionParams B) {
    const int lane = threadIdx.x;
    const int64_t chain = blockIdx.x;
    const int64_t d = P.d;
    const uint32_t nblk = P.nblk;  // <= 64 (n <= 64: 33 blocks): one block minimum per lane

    __shared__ double bk[64];    // block minima
    __shared__ uint32_t bi[64];  // block argmin (coordinate id)

    ZzRec* rec = P.rec + chain * d;
    double* keys = P.keys + chain * P.dk;
    double* thf = P.thf + chain * d;
    DevChain* hdr = P.hdr + chain;
    pdmp_event* ev = P.ev ? P.ev + chain * P.trace_cap : nullptr;
    double* cmut = P.c_chain ? (P.c_chain + chain * d) : nullptr;
    const double* cvec = cmut ? cmut : P.tb.c_shared;

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
    const bool strong = P.strong_upperbounds != 0, reversible = P.reversible != 0;

    const uint32_t n = (uint32_t)B.n;
    // lane c keeps where column c begins: the column of i is the last one that begins at or before i
    const uint32_t myk0 = ((uint32_t)lane < n) ? ((uint32_t)lane * n - ((uint32_t)lane * ((uint32_t)lane - 1u)) / 2u) : 0xffffffffu;

    level1_build(bk, bi, keys, nblk, lane);
    PDMP_LDS_ORDER();

    bool running = stop_before || (t_event < T);  // `while t′ < T`, src/ss_fact.jl:202
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
        // ---------------- ii, t′ = peek(Q), src/ss_fact.jl:83
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
        if (i >= (uint32_t)d) {  // (the padding keys and the refresh slot are +Inf: unreachable; keeps every index below in bounds)
            status = PDMP_CHAIN_STALLED;
            break;
        }
        const uint32_t col = (uint32_t)__popcll(__ballot(myk0 <= i)) - 1u;
        const uint32_t k0 = col * n - (col * (col - 1u)) / 2u;
        const uint32_t len = n - col, qi = i - k0;  // the column [k0, k0 + len), i is its member qi: row r = col + qi
        const bool diag = qi == 0u;

        const ZzRec* ri = rec + i;
        const double x_i0 = ri->x, th_i0 = ri->th, t_i = ri->t;
        const double told_i = ri->t_old, a_i = ri->a, b_i = ri->b;
        const bool is_freeze = uniform_u32(ri->acc != 0 ? 1u : 0u) != 0;  // f[i]
        const bool is_thaw = !is_freeze && uniform_u32((x_i0 == 0 && th_i0 == 0) ? 1u : 0u) != 0;
        if (is_freeze && diag) {  // a diagonal of L at 0: the next gradient is N/0
            status = PDMP_CHAIN_STALLED;
            break;
        }
        t_last = tp;

        // what the case leaves in rec[i] and keys[i] (written once, by lane 63, below)
        double x_rec = x_i0, th_rec = th_i0, t_rec = tp, a_rec = a_i, b_rec = b_i, key = PDMP_INF;
        uint64_t f_rec = 0;
        bool emit = true, rebound = true;

        double thf_i = 0.0;
        double cj = cvec[i];
        if (is_freeze) {  // case 1) to be frozen, :87-107
            const double xs = x_i0 + th_i0 * (tp - t_i);  // smove_forward!(i, ...), :88
            if (fabs(xs) > 1e-8) {                        // :89-91
                status = PDMP_CHAIN_BOUND_VIOLATED;
                break;
            }
            x_rec = 0.0 * th_i0;  // x[i] = -0*θ[i], :92
            th_rec = 0.0;         // :93
            thf_i = th_i0;
            key = tp - pdmp_log(pdmp_u01(seed, PDMP_STREAM_MAIN, nm)) / P.kappa[i];  // :96
            nm += 1;
            rebound = false;  // G1[i] = {i} is frozen: no re-bound, :100-106
        } else if (is_thaw) {  // case 2) was frozen, :108-123
            double thn = thf[i];  // θ[i], θf[i] = θf[i], 0.0, :110
            if (thn == 0.0) {     // never frozen by this loop: nothing to restore
                status = PDMP_CHAIN_STALLED;
                break;
            }
            if (reversible) {  // :111-113
                thn *= (pdmp_u01(seed, PDMP_STREAM_MAIN, nm) < 0.5) ? -1.0 : 1.0;
                nm += 1;
            }
            th_rec = thn;
            x_rec = x_i0 + thn * (tp - tp);  // ssmove_forward!(G, i, ...) moves i too, by t′ − t′, :115: a −0.0 left by the freeze becomes +0.0 under θ > 0
        } else if (th_i0 != 0.0) {  // a proposal: i moves with its column, :125
            x_rec = x_i0 + th_i0 * (tp - t_i);
        } else {
            t_rec = t_i;  // (θ_i = 0 ≠ x_i: ssmove_forward! leaves the coordinate and its clock where they are)
        }

        // ---------------- ssmove_forward!(G, i, t, x, θ, t′, F), :98,115,125: lane q moves member k0 + q (i itself: above)
        const bool mine = (uint32_t)lane < len;
        const bool self = mine && (uint32_t)lane == qi;
        double xn = 0.0;
        if (mine && !self && !(is_freeze && strong)) {
            ZzRec* rj = rec + (k0 + (uint32_t)lane);
            const double xj = rj->x, thj = rj->th, tj = rj->t;
            xn = xj;
            if (thj != 0.0) {
                xn = xj + thj * (tp - tj);
                rj->x = xn;
                rj->t = tp;
            }
        }

        if (!is_freeze && !is_thaw) {  // a reflection time or an event time from the upper bound, :124-152
            // ---------------- ∇ϕ(u, i, YY, (𝕀, 𝕁), N), precision.jl:42-53
            const uint32_t r = col + qi;
            const double prod = mine ? (B.YY[(size_t)r * n + col + (uint32_t)lane] * (self ? x_rec : xn)) : 0.0;  // c += YY[c2] * u[j], :46
            const double s = wave_sum_f64(prod);
            const double term = diag ? (-B.N / x_rec + B.gamma0 * (x_rec - 1.0)) : (B.gamma0 * x_rec);  // :49-51, precision4.jl:88-92
            const double g = s + term;
            const double l_rate = pos_part(g * th_i0);                  // sλ, :128
            const double lbound = pos_part(a_i + b_i * (tp - told_i));  // sλ̄, :128
            num += 1;                                                   // :129
            const double coin = pdmp_u01(seed, PDMP_STREAM_MAIN, nm);
            nm += 1;
            if (coin * lbound < l_rate) {  // :130
                nacc += 1;
                if (l_rate > lbound) {  // :132
                    if (!adapt) {       // error("Tuning parameter `c` too small. ..."), :133 -> the chain's status word
                        if (lane == 63) {
                            rec[i].x = x_rec;
                            rec[i].t = t_rec;
                        }
                        status = PDMP_CHAIN_BOUND_VIOLATED;
                        break;
                    }
                    nacc = 0;  // acc = num = 0, :134
                    num = 0;
                    cj *= P.factor;  // adapt!(c, i, factor), :135
                    if (lane == 63) cmut[i] = cj;
                }
                th_rec = -th_i0;  // reflect!, :139
            } else {
                emit = false;  // :147-151
            }
        }

        if (rebound) {  // b[i] = ab(G1, i, x, θ, c, F); t_old[i] = t[i]; queue_time!(Q, t, x, θ, i, b, f, F), :119-121 / :142-144 / :148-150
            const double gam = P.tb.bval[i];                              // Γ̂ is diagonal: column i is its entry i
            const double gx = 0.0 + gam * x_rec, gt = 0.0 + gam * th_rec;  // idot(Γ̂, i, ·), src/common.jl:16-24
            a_rec = cj + (gx - P.tb.gmu_b[i]) * th_rec;                   // src/fact_samplers.jl:51
            b_rec = cj / 100 + th_rec * gt;                               // :52
            double dtn = poisson_time_L(a_rec, b_rec, pdmp_log(pdmp_u01(seed, PDMP_STREAM_MAIN, nm)));
            nm += 1;
            const double tfreeze = (th_rec * x_rec >= 0) ? PDMP_INF : (-x_rec / th_rec);  // freezing_time, src/ss_fact.jl:10-16
            const bool fz = tfreeze <= dtn;                                               // queue_time!, :54-65
            dtn = fz ? tfreeze : dtn;
            f_rec = fz ? 1u : 0u;
            key = tp + dtn;
        }
        if (lane == 63) {
            ZzRec* wi = rec + i;
            wi->x = x_rec;
            wi->th = th_rec;
            wi->t = t_rec;
            wi->t_old = tp;
            wi->a = a_rec;
            wi->b = b_rec;
            wi->acc = f_rec;
            keys[i] = key;
            if (is_freeze) thf[i] = thf_i;
            if (is_thaw) thf[i] = 0.0;
        }
        level1_update(bk, bi, keys, lane, i, key);
        PDMP_LDS_ORDER();
        if (emit) {  // push!(Ξ, event(i, t, x, θ, F)), :154
            if (ev && lane == 0) {
                pdmp_event e;
                e.t = tp;
                e.i = (int64_t)i;
                e.x = x_rec;
                e.theta = th_rec;
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
        hdr->c.status = status;
    }
}

int launch_zz_precision_run(const ZzRunParams& p, const ZzPrecisionParams& b, int64_t nchains, void* stream) {
    if (p.nblk > 64u || b.n < 1 || b.n > PDMP_PRECISION_NMAX || p.d != (int64_t)b.n * (b.n + 1) / 2 || !b.YY || !p.thf || !p.kappa) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(zz_precision_run_kernel, dim3((unsigned)nchains), dim3(64), 0, (hipStream_t)stream, p, b);
    return (int)hipGetLastError();
}
