/*
 * precision_ref.c -- sequential restatement of the reference's precision case study: the sticky ZigZag
 *   sspdmp(∇ϕ, t0, x0, θ0, T, c, G, ZigZag(Γ̂, μ̂), κ, YY, (𝕀, 𝕁), N; adapt, reversible, strong_upperbounds)
 * of casestudies/precision/precision.jl:42-53,82 (γ0 = 0) and research/newsticky/precision/precision4.jl:82-93 (γ0 > 0) with the loop of
 * src/ss_fact.jl:78-215, line by line, for the tests to hold the device loop (csrc/pdmp_precision.inc) to.  Test infrastructure only: the
 * product never loads it.  It shares include/pdmp_detmath.h with the kernels (Philox draws, log) and restates everything else itself.
 * Written from reading the Julia; every block cites its lines.
 *
 * The model: N observations Y_k ~ N(0, (L Lᵀ)⁻¹) enter through YY = Σ Y_k Y_kᵀ (n x n, symmetric, row-major) and N.  The coordinates are the
 * lower triangle of L packed column by column (0-based): u[i] = L[r, c], i = k0(c) + (r − c), k0(c) = c n − c (c − 1)/2, len(c) = n − c.
 *   ϕ(u)  = ½ Σ_c L[:,c]ᵀ YY L[:,c] − N Σ_c log L[c,c] + (γ0/2)(Σ_{r>c} L[r,c]² + Σ_c (L[c,c] − 1)²)
 *   ∇ϕ_i  = Σ_{q<len} YY[r, c+q] u[k0+q] + (r == c ? −N/u_i + γ0 (u_i − 1) : γ0 u_i)
 *
 * What the reference leaves open is fixed the way the engine fixes it everywhere:
 *   sum      the len products are formed one per lane of a 64-lane wavefront (0.0 past len) and added in the order of wave_sum_f64
 *            (csrc/pdmp_bps_common.hpp; dot_wave64 of oracle/pdmp_oracle.c): the xor butterfly 1, 2, 4, 8, 16, 32.  The diagonal or prior
 *            term, formed on its own, is added to that sum.  Plain double, no fused multiply-add.
 *   draws    every rand() is draw nm++ of PDMP_STREAM_MAIN in program order (the order of orc_sspdmp_zigzag and of the sticky branch of
 *            pdmp_general.hip): the setup takes draws 0 .. d−1 (src/ss_fact.jl:178-188); a freeze takes one (the thaw time, :96), a thaw
 *            the reversible coin if asked for (:112) and the re-bound of i (:121), a proposal its coin (:130) and the re-bound of i (:144,150).
 *   queue    an exact minimum over all coordinates, lowest index on ties.
 *   flow     F = ZigZag(Γ̂, μ̂) with Γ̂ diagonal: G1[i] = {i}, G[i] = the column of i (what ∇ϕ_i reads), G2[i] = ∅.  ab (src/fact_samplers.jl:
 *            50-54) with idot's arithmetic (src/common.jl:16-24): a = c_i + ((0.0 + γ̂_i x_i) − (0.0 + γ̂_i μ̂_i)) θ_i, b = c_i/100 + θ_i (0.0 + γ̂_i θ_i).
 *   clocks   the re-bound of i after a proposal takes t′ as i's clock (t_old[i] = t′, Q[i] = t′ + τ).  The reference reads t[i], which
 *            ssmove_forward! leaves behind for a coordinate with θ_i = 0 ≠ x_i (a start nobody gives: its rate is 0 for ever).
 *   stalls   a freeze popped for a DIAGONAL coordinate ends the chain as REF_STALLED before any state changes: the reference would go on to
 *            evaluate N/0.  So does a thaw that restores the speed 0 (a coordinate started at x = 0 with θ = 0: the reference pops it for
 *            ever), and a queue whose minimum is not finite.
 *   :89-91   a freeze whose moved x_i is further than 1e-8 from 0 is the reference's error(...): REF_BOUND_VIOLATED, as orc_sspdmp_zigzag.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pdmp_detmath.h"

#define REF_OK 0
#define REF_BOUND_VIOLATED 1 /* error("Tuning parameter `c` too small. ..."), src/ss_fact.jl:133 (and :90) */
#define REF_STALLED 2

#define REF_RUN_REFERENCE_TAIL 0 /* `while t′ < T`: the event that crosses T is still returned, src/ss_fact.jl:202 */
#define REF_RUN_STOP_BEFORE 1    /* stop before the first pop at or after T (the engine's sliced runs) */

typedef struct {
    int32_t n, adapt, reversible, strong_upperbounds;
    double N, gamma0, factor;
    uint64_t seed;
    const double* YY;    /* [n x n] row-major */
    const double* gam;   /* [d] diagonal of Γ̂ */
    const double* mu;    /* [d] μ̂ */
    const double* kappa; /* [d] */
} ref_prec_params;

/* everything a chain carries from one call to the next (the arrays x, θ, t, c, t_old, a, b, Q, θf, f are the caller's, [d] each) */
typedef struct {
    int64_t num, nacc, nevents, nadapt;
    uint64_t ndraw_main;
    int32_t status, pad_;
    double t_event; /* t′ of the last returned event: the loop variable of `while t′ < T` */
    double t_last;  /* the last popped time that was acted on */
} ref_prec_state;

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

/* k0(c) = c n − c (c − 1)/2: where column c of the packed lower triangle begins */
int64_t ref_precision_k0(int32_t n, int32_t c) { return (int64_t)c * n - ((int64_t)c * (c - 1)) / 2; }

/* the column of coordinate i: the largest c with k0(c) <= i */
int32_t ref_precision_col(int32_t n, int64_t i) {
    int32_t c = 0;
    while (c + 1 < n && ref_precision_k0(n, c + 1) <= i) c += 1;
    return c;
}

/* ∇ϕ(u, i, YY, (𝕀, 𝕁), N), precision.jl:42-53 / precision4.jl:82-93, in the device's summation order */
double ref_precision_grad(int32_t n, const double* YY, double N, double gamma0, const double* u, int64_t i) {
    const int32_t c = ref_precision_col(n, i);
    const int64_t k0 = ref_precision_k0(n, c);
    const int32_t len = n - c, r = c + (int32_t)(i - k0);
    double part[64];
    for (int q = 0; q < 64; ++q) part[q] = (q < len) ? YY[(int64_t)r * n + c + q] * u[k0 + q] : 0.0; /* c += YY[c2] * u[j], :46 */
    for (int off = 1; off <= 32; off <<= 1) { /* wave_sum_f64 */
        double nxt[64];
        for (int l = 0; l < 64; ++l) nxt[l] = part[l] + part[l ^ off];
        memcpy(part, nxt, sizeof part);
    }
    const double ui = u[i];
    const double term = (r == c) ? (-N / ui + gamma0 * (ui - 1.0)) : (gamma0 * ui); /* :49-51 / precision4.jl:88-92 */
    return part[0] + term;
}

/* ab(G1, i, x, θ, c, Z::ZigZag), src/fact_samplers.jl:50-54, with Γ̂ diagonal */
static void ab(const ref_prec_params* p, int64_t i, const double* x, const double* th, const double* c, double* ba, double* bb) {
    const double gx = 0.0 + p->gam[i] * x[i], gt = 0.0 + p->gam[i] * th[i], gmu = 0.0 + p->gam[i] * p->mu[i];
    ba[i] = c[i] + (gx - gmu) * th[i];
    bb[i] = c[i] / 100 + th[i] * gt;
}

/* freezing_time, src/ss_fact.jl:10-16 */
static double freezing_time(double x, double th) { return (th * x >= 0) ? INFINITY : (-x / th); }

/* queue_time!, src/ss_fact.jl:54-65, with i's clock given */
static void queue_time(const ref_prec_params* p, ref_prec_state* S, double ti, const double* x, const double* th, int64_t i, const double* ba,
                       const double* bb, double* Q, uint8_t* f) {
    const double trefl = poisson_time(ba[i], bb[i], pdmp_u01(p->seed, PDMP_STREAM_MAIN, S->ndraw_main++));
    const double tfreeze = freezing_time(x[i], th[i]);
    if (tfreeze <= trefl) {
        f[i] = 1;
        Q[i] = ti + tfreeze;
    } else {
        f[i] = 0;
        Q[i] = ti + trefl;
    }
}

/* ssmove_forward!(G, i, t, x, θ, t′, Z), src/ss_fact.jl:38-45, with G[i] = the column of i */
static void move_column(int64_t k0, int32_t len, double* t, double* x, const double* th, double tp) {
    for (int32_t q = 0; q < len; ++q) {
        const int64_t j = k0 + q;
        if (th[j] != 0.0) {
            x[j] = x[j] + th[j] * (tp - t[j]);
            t[j] = tp;
        }
    }
}

/* The setup of src/ss_fact.jl:161-188 (init != 0), then `while t′ < T` around sspdmp_inner! (:202-211, :78-157).  x, th, c: in/out [d];
 * t, t_old, ba, bb, Q, thf, f: state [d], written by the setup.  Events beyond ev_cap are counted, not stored. */
int ref_precision_run(const ref_prec_params* p, int32_t init, double t0, double Tend, int32_t flags, double* x, double* th, double* t, double* c,
                      double* t_old, double* ba, double* bb, double* Q, double* thf, uint8_t* f, double* ev_t, int64_t* ev_i, double* ev_x,
                      double* ev_th, int64_t ev_cap, ref_prec_state* S) {
    const int32_t n = p->n;
    const int64_t d = (int64_t)n * (n + 1) / 2;
    if (init) {
        memset(S, 0, sizeof *S);
        for (int64_t i = 0; i < d; ++i) { /* :163-165, :174 */
            t[i] = t0;
            t_old[i] = t0;
            f[i] = 0;
            thf[i] = 0.0;
        }
        for (int64_t i = 0; i < d; ++i) ab(p, i, x, th, c, ba, bb); /* :177 */
        for (int64_t i = 0; i < d; ++i) {                            /* :178-188 */
            const double trefl = poisson_time(ba[i], bb[i], pdmp_u01(p->seed, PDMP_STREAM_MAIN, S->ndraw_main++));
            const double tfreez = freezing_time(x[i], th[i]);
            if (trefl > tfreez) {
                f[i] = 1;
                Q[i] = t0 + tfreez;
            } else {
                f[i] = 0;
                Q[i] = t0 + trefl;
            }
        }
        S->t_event = t0;
        S->t_last = t0;
    }
    if (S->status != REF_OK) return 0;
    const int stop_before = (flags & REF_RUN_STOP_BEFORE) != 0;
    int running = stop_before || (S->t_event < Tend); /* :202 */
    while (running) {
        /* ii, t′ = peek(Q), :83 */
        int64_t i = 0;
        for (int64_t j = 1; j < d; ++j)
            if (Q[j] < Q[i]) i = j;
        const double tp = Q[i];
        if (!(tp < INFINITY)) {
            S->status = REF_STALLED;
            break;
        }
        if (stop_before && !(tp < Tend)) break;
        const int32_t col = ref_precision_col(n, i);
        const int64_t k0 = ref_precision_k0(n, col);
        const int32_t len = n - col;
        const int diag = i == k0;
        if (f[i] && diag) { /* a diagonal of L at 0: the next gradient is N/0 */
            S->status = REF_STALLED;
            break;
        }
        S->t_last = tp;
        if (f[i]) { /* case 1) to be frozen, :87-107 */
            const double xs = x[i] + th[i] * (tp - t[i]); /* smove_forward!(i, ...), :88 */
            if (fabs(xs) > 1e-8) {                        /* :89-91 */
                S->status = REF_BOUND_VIOLATED;
                break;
            }
            t[i] = tp;
            x[i] = 0.0 * th[i]; /* x[i] = -0*θ[i], :92 (Int -0 == 0: the sign is θ's) */
            thf[i] = th[i];
            th[i] = 0.0; /* :93 */
            t_old[i] = tp;
            f[i] = 0;
            Q[i] = tp - pdmp_log(pdmp_u01(p->seed, PDMP_STREAM_MAIN, S->ndraw_main++)) / p->kappa[i]; /* :96 */
            if (!p->strong_upperbounds) move_column(k0, len, t, x, th, tp); /* :98; G2 is empty, and G1[i] = {i} is frozen: no re-bound, :100-106 */
        } else if (x[i] == 0 && th[i] == 0) { /* case 2) was frozen, :108-123 */
            if (thf[i] == 0.0) {              /* never frozen by this loop: nothing to restore */
                S->status = REF_STALLED;
                break;
            }
            t[i] = tp; /* :109 */
            th[i] = thf[i];
            thf[i] = 0.0; /* :110 */
            if (p->reversible) th[i] *= (pdmp_u01(p->seed, PDMP_STREAM_MAIN, S->ndraw_main++) < 0.5) ? -1.0 : 1.0; /* :111-113 */
            t_old[i] = tp;                                                                                          /* :114 */
            move_column(k0, len, t, x, th, tp);                                                                     /* :115 */
            ab(p, i, x, th, c, ba, bb);                                                                             /* :117-123 */
            queue_time(p, S, tp, x, th, i, ba, bb, Q, f);
        } else { /* a reflection time or an event time from the upper bound, :124-152 */
            move_column(k0, len, t, x, th, tp); /* :125 */
            const double g = ref_precision_grad(n, p->YY, p->N, p->gamma0, x, i); /* :127 */
            const double l = pos(g * th[i]);                                      /* sλ, :128 */
            const double lb = pos(ba[i] + bb[i] * (tp - t_old[i]));               /* sλ̄, :128 */
            S->num += 1;                                                          /* :129 */
            const double coin = pdmp_u01(p->seed, PDMP_STREAM_MAIN, S->ndraw_main++);
            if (coin * lb < l) { /* :130 */
                S->nacc += 1;
                if (l > lb) { /* :132 */
                    if (!p->adapt) {
                        S->status = REF_BOUND_VIOLATED; /* :133 */
                        break;
                    }
                    S->nacc = S->num = 0; /* :134 */
                    c[i] *= p->factor;    /* adapt!(c, i, factor), :135 */
                    S->nadapt += 1;
                }
                th[i] = -th[i]; /* reflect!, :139 */
                ab(p, i, x, th, c, ba, bb); /* :140-146 with G1[i] = {i} */
                t_old[i] = tp;
                queue_time(p, S, tp, x, th, i, ba, bb, Q, f);
            } else { /* :147-151 */
                ab(p, i, x, th, c, ba, bb);
                t_old[i] = tp;
                queue_time(p, S, tp, x, th, i, ba, bb, Q, f);
                continue;
            }
        }
        /* push!(Ξ, event(i, t, x, θ, F)), :154 */
        if (S->nevents < ev_cap) {
            ev_t[S->nevents] = tp;
            ev_i[S->nevents] = i;
            ev_x[S->nevents] = x[i];
            ev_th[S->nevents] = th[i];
        }
        S->nevents += 1;
        S->t_event = tp;
        if (!stop_before && !(tp < Tend)) running = 0;
    }
    return 0;
}
