/*
 * bridge_ref.c -- sequential restatement of the reference's diffusion-bridge sampler: the local ZigZag
 *   spdmp(∇ϕmoving, 0.0, ξ0, θ0, T′, c, ZigZag(sparse(I), 0), SelfMoving(), L, T; adapt)
 * of research/diffusion_bridge/diffbridge.jl:32-33 with the gradient of research/diffusion_bridge/faberschauder.jl:128-145 and the
 * loop of src/sfact.jl:73-145,162-212, line by line, for the tests to hold the device loop (csrc/pdmp_bridge.inc) to.  Test
 * infrastructure only: the product never loads it.  It shares include/pdmp_detmath.h with the kernels (Philox draws, log, sincos) and
 * restates everything else itself.  Written from reading the Julia; every block cites its lines.
 *
 * What the reference leaves open is fixed the way the engine fixes it everywhere:
 *   draws    rand() of the gradient (faberschauder.jl:141, the GLOBAL generator) is draw ng++ of PDMP_STREAM_GLOBAL, taken before the
 *            coin; the coin (src/sfact.jl:121) and the re-bound (:134, :139) are draws nm++ of PDMP_STREAM_MAIN in program order; the
 *            setup takes draws 0 .. d-1 of that stream (:185-187).
 *   queue    an exact minimum over all coordinates, lowest index on ties.
 *   drift    b(x) = −βx + α sin(ωx), b′(x) = −β + (αω) cos(ωx), b″(x) = −((αω)ω) sin(ωx): the TRUE derivatives (the script's b′ and b″
 *            carry a stray factor 2, diffbridge.jl:11-13).  sin / cos are pdmp_sincos, `%` is fmod, / and sqrt are IEEE.
 *   stalls   |ωx| > PDMP_SINCOS_MAX ends the chain as REF_STALLED, and so does a sampled time s that is not below T (δ(k + u) rounds up
 *            to T with probability ~2^-44: the reference's dotψmoving then indexes ξ out of bounds, faberschauder.jl:41).
 * Indices are 0-based: coordinate i here is ξ[i + 1] there.  The end points 0 and d − 1 have θ = 0 and c = 0: their bound is (0, 0), their
 * key +Inf, and they never pop (diffbridge.jl:23-26).
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pdmp_detmath.h"

#define REF_OK 0
#define REF_BOUND_VIOLATED 1 /* error("Tuning parameter `c` too small."), src/sfact.jl:124 */
#define REF_STALLED 2

#define REF_RUN_REFERENCE_TAIL 0 /* `while t′ < T′`: the event that crosses T′ is still returned, src/sfact.jl:199 */
#define REF_RUN_STOP_BEFORE 1    /* stop before the first proposal at or after T′ (the engine's sliced runs) */

typedef struct {
    int32_t L, adapt;
    double T, alpha, beta, omega, factor;
    uint64_t seed;
} ref_bridge_params;

/* everything a chain carries from one call to the next (the arrays t, x, θ, c, t_old, a, b, Q, acc are the caller's, [d] each) */
typedef struct {
    int64_t num, nacc, nevents, nadapt;
    uint64_t ndraw_main, ndraw_global;
    int32_t status, pad_;
    double t_event; /* t′ of the last returned event: the loop variable of `while t′ < T′` */
    double t_last;  /* the last popped time */
} ref_bridge_state;

/* pos(x) = max(zero(x), x), src/common.jl:8 */
static double pos(double x) { return x > 0 ? x : (x != x ? x : 0.0); }

/* poisson_time(a, b, u), src/poissontime.jl:8-30 */
static double poisson_time(double a, double b, double u) {
    const double L = pdmp_log(u);
    if (b > 0) {
        const double r = a / b;
        if (a < 0) return sqrt(-L * 2.0 / b) - r;
        return sqrt(r * r - L * 2.0 / b) - r;
    } else if (b == 0) {
        return (a > 0) ? (-L / a) : INFINITY;
    } else {
        if (a <= 0) return INFINITY;
        if (-L <= -(a * a) / b + (a * a) / (2 * b)) {
            const double r = a / b;
            return -sqrt(r * r - L * 2.0 / b) - r;
        }
        return INFINITY;
    }
}

/* Λ(t, T) = sqrt(T)*0.5 - abs((t % T)/sqrt(T) - sqrt(T)*0.5), faberschauder.jl:3 */
static double Lambda1(double t, double T) {
    const double sT = sqrt(T);
    return sT * 0.5 - fabs(fmod(t, T) / sT - sT * 0.5);
}
/* Λ(t, l⁻, T) = Λ(t*(1<<l⁻), T)/sqrt(1<<l⁻), faberschauder.jl:6 */
double ref_Lambda(double t, int32_t lm, double T) {
    const double p2 = (double)((int64_t)1 << lm);
    return Lambda1(t * p2, T) / sqrt(p2);
}

/* lvl(i, L), faberschauder.jl:81-87 with lvl0 (:61-68), 0-based i */
int32_t ref_lvl(int64_t i, int32_t L) {
    if (i == 0 || i == ((int64_t)2 << L)) return L;
    int32_t l = 0;
    while ((i & 1) == 0) {
        l += 1;
        i >>= 1;
    }
    return l;
}

/* j = floor(Int, s/T*(1 << (L - lev)))*(2 << lev) + (1 << lev) + 1, faberschauder.jl:20,41 (0-based: without the + 1) */
int64_t ref_index(double s, int32_t lev, int32_t L, double T) {
    const double q = s / T * (double)((int64_t)1 << (L - lev));
    return (int64_t)floor(q) * ((int64_t)2 << lev) + ((int64_t)1 << lev);
}

/* dotψ(ξ, s, L, T), faberschauder.jl:16-24 (NaN where the reference raises "out of bounds") */
double ref_dotpsi(const double* xi, double s, int32_t L, double T) {
    const int64_t d = ((int64_t)2 << L) + 1;
    if (!(0 <= s && s < T)) return NAN;
    double r = s / sqrt(T) * xi[d - 1] + sqrt(T) * (1 - s / T) * xi[0];
    for (int32_t lev = 0; lev <= L; ++lev) r += xi[ref_index(s, lev, L, T)] * ref_Lambda(s, L - lev, T);
    return r;
}

/* the drift and its derivatives at x: 2 b b′ + b″, formula (17); returns 0 where |ωx| is beyond pdmp_sincos */
static int drift_term(const ref_bridge_params* p, double x, double* out) {
    const double w = p->omega * x;
    if (!(fabs(w) <= PDMP_SINCOS_MAX)) return 0;
    double sn, cs;
    pdmp_sincos(w, &sn, &cs);
    const double aw = p->alpha * p->omega, aww = aw * p->omega;
    const double b0 = -p->beta * x + p->alpha * sn;
    const double b1 = -p->beta + aw * cs;
    const double b2 = -(aww * sn);
    *out = 2 * b0 * b1 + b2;
    return 1;
}

/* ∇ϕmoving(t, ξ, θ, i, t′, F, L, T) for an interior i, faberschauder.jl:137-144, with dotψmoving (:37-46) and
 * smove_forward!(j, t, ξ, θ, t′, F) (src/sfact.jl:13-16).  u01 is the reference's rand().  Returns REF_OK or REF_STALLED. */
int ref_bridge_grad(const ref_bridge_params* p, double* xi, double* t, const double* th, int64_t i, double tp, double u01, double* g) {
    const int32_t L = p->L;
    const double T = p->T;
    const int64_t d = ((int64_t)2 << L) + 1;
    const int32_t l = ref_lvl(i, L);                            /* :138 */
    const int64_t k = i / ((int64_t)2 << l);                    /* (i - 1) ÷ (2 << l), :139 */
    const double delta = T / (double)((int64_t)1 << (L - l));   /* :140 */
    const double s = delta * ((double)k + u01);                 /* :141 */
    if (!(s < T)) return REF_STALLED;
    double r = s / sqrt(T) * xi[d - 1] + sqrt(T) * (1 - s / T) * xi[0]; /* :39 */
    for (int32_t lev = 0; lev <= L; ++lev) {                    /* :40-44 */
        const int64_t j = ref_index(s, lev, L, T);
        xi[j] = xi[j] + th[j] * (tp - t[j]); /* t[i], x[i] = t′, x[i] + θ[i]*(t′ - t[i]), src/sfact.jl:14 */
        t[j] = tp;
        r += xi[j] * ref_Lambda(s, L - lev, T);
    }
    double dr;
    if (!drift_term(p, r, &dr)) return REF_STALLED;
    *g = 0.5 * delta * ref_Lambda(s, L - l, T) * dr + xi[i]; /* :143 */
    return REF_OK;
}

/* ab(G1, i, x, θ, c, Z::ZigZag), src/fact_samplers.jl:50-54, with Γ = I, μ = 0: idot(Γ, i, x) = 0.0 + 1.0*x[i] (src/common.jl:16-24) */
static void ab(int64_t i, const double* x, const double* th, const double* c, double* ba, double* bb) {
    const double gx = 0.0 + 1.0 * x[i], gt = 0.0 + 1.0 * th[i];
    ba[i] = c[i] + (gx - 0.0) * th[i];
    bb[i] = c[i] / 100 + th[i] * gt;
}

/* The setup of src/sfact.jl:164-190 (init != 0), then the loop `while t′ < T′` around spdmp_inner! (:199-208, :73-145) with G = G1 = {i} and
 * G2 empty.  x, th, c: in/out [d]; t, t_old, ba, bb, Q: state [d], written by the setup; acc [d].  Events beyond ev_cap are counted, not stored. */
int ref_bridge_run(const ref_bridge_params* p, int32_t init, double t0, double Tend, int32_t flags, double* x, double* th, double* t, double* c,
                   double* t_old, double* ba, double* bb, double* Q, int64_t* acc, double* ev_t, int64_t* ev_i, double* ev_x, double* ev_th,
                   int64_t ev_cap, ref_bridge_state* S) {
    const int64_t d = ((int64_t)2 << p->L) + 1;
    if (init) {
        memset(S, 0, sizeof *S);
        for (int64_t i = 0; i < d; ++i) { /* :168-169, :182 */
            t[i] = t0;
            t_old[i] = t0;
            acc[i] = 0;
        }
        for (int64_t i = 0; i < d; ++i) ab(i, x, th, c, ba, bb);                                                      /* :184 */
        for (int64_t i = 0; i < d; ++i) Q[i] = poisson_time(ba[i], bb[i], pdmp_u01(p->seed, PDMP_STREAM_MAIN, S->ndraw_main++)); /* :185-187 */
        S->t_event = t0;
        S->t_last = t0;
    }
    if (S->status != REF_OK) return 0;
    const int stop_before = (flags & REF_RUN_STOP_BEFORE) != 0;
    int running = stop_before || (S->t_event < Tend); /* :199 */
    while (running) {
        /* i, t′ = peek(Q), :77 */
        int64_t i = 0;
        for (int64_t j = 1; j < d; ++j)
            if (Q[j] < Q[i]) i = j;
        const double tp = Q[i];
        if (!(tp < INFINITY)) {
            S->status = REF_STALLED;
            break;
        }
        if (stop_before && !(tp < Tend)) break;
        S->t_last = tp;
        x[i] = x[i] + th[i] * (tp - t[i]); /* smove_forward!(G, i, ...) with G[i] = {i}, :82, :6-12 */
        t[i] = tp;
        double g;
        const double u = pdmp_u01(p->seed, PDMP_STREAM_GLOBAL, S->ndraw_global++);
        if (ref_bridge_grad(p, x, t, th, i, tp, u, &g) != REF_OK) { /* ∇ϕ_(∇ϕ, t, x, θ, i, t′, F, S::SelfMoving, args...), :68,118 */
            S->status = REF_STALLED;
            break;
        }
        const double l = pos(g * th[i]);                        /* sλ, :69,119; λ of the ZigZag, src/fact_samplers.jl:28-30 */
        const double lb = pos(ba[i] + bb[i] * (t[i] - t_old[i])); /* sλ̄, :70,119 */
        S->num += 1;                                            /* :120 */
        const double coin = pdmp_u01(p->seed, PDMP_STREAM_MAIN, S->ndraw_main++);
        if (coin * lb < l) { /* :121 */
            S->nacc += 1;
            if (l >= lb) { /* :123 */
                if (!p->adapt) {
                    S->status = REF_BOUND_VIOLATED; /* :124 */
                    break;
                }
                c[i] *= p->factor; /* adapt!(c, i, factor), :127, src/fact_samplers.jl:67-70 */
                S->nadapt += 1;
            }
            acc[i] += 1;     /* :122 */
            th[i] = -th[i];  /* reflect!, :130, src/dynamics.jl:46-49 */
            ab(i, x, th, c, ba, bb); /* :131-135 with G1[i] = {i} */
            t_old[i] = t[i];
            Q[i] = t[i] + poisson_time(ba[i], bb[i], pdmp_u01(p->seed, PDMP_STREAM_MAIN, S->ndraw_main++));
            /* push!(Ξ, event(i, t, x, θ, F)), :143,202 */
            if (S->nevents < ev_cap) {
                ev_t[S->nevents] = t[i];
                ev_i[S->nevents] = i;
                ev_x[S->nevents] = x[i];
                ev_th[S->nevents] = th[i];
            }
            S->nevents += 1;
            S->t_event = tp;
            if (!stop_before && !(tp < Tend)) running = 0;
        } else {
            ab(i, x, th, c, ba, bb); /* :137-139 */
            t_old[i] = t[i];
            Q[i] = t[i] + poisson_time(ba[i], bb[i], pdmp_u01(p->seed, PDMP_STREAM_MAIN, S->ndraw_main++));
        }
    }
    return 0;
}
