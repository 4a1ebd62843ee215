/*
 * sticky_notfact_ref.c -- sequential restatement of the reference's non-factorised sticky sampler,
 *   sspdmp(∇ϕ!, t0, x0, θ0, T, c, Flow::Union{BouncyParticle, Boomerang}, κ, args...; strong_upperbounds, adapt, factor)
 * (src/ss_not_fact.jl:104-201), line by line, for the tests to hold the device loop (csrc/pdmp_bps_sticky.inc) to.  Test
 * infrastructure only: the product never loads it.  It shares include/pdmp_detmath.h with the kernels (Philox, log, sincos, atan) and
 * restates everything else itself (poisson_time, pos, idot, the freezing times, the loop).
 *
 * What the reference leaves open is fixed the way oracle/pdmp_oracle.c fixes it for the plain Bouncy Particle:
 *   draws   the reference calls the GLOBAL generator; in program order those calls are draws nm = 0, 1, 2, ... of PDMP_STREAM_MAIN.
 *           randn() x d of refresh_sticky_vel! -> element 128a + 64b + l is Box-Muller branch b of block nm + 64a + l, and
 *           ((d+127)>>7)<<6 draws are consumed (the BPS oracle's refresh).
 *   sums    dot / normsq / sdot / subnormsq in the 64-lane order of dot_wave64 (oracle/pdmp_oracle.c): per-lane partial sums over
 *           l, l+64, ..., then the xor butterfly; sdot / subnormsq SKIP elements with θ == 0 (:43-65), they do not add a zero product.
 *           Γ·v per output element in ascending index order (idot, src/common.jl:16-24).
 *   ties    findmin takes the first minimum: lowest index in tfrez; tref before tᶠ before t′.
 * Fixed DIFFERENTLY from the reference: a NaN clock never wins findmin here, while Julia's findmin returns the NaN.  A clock is NaN only
 * where a free coordinate has x = 0 and θ = 0 together (atan(0/0) in the Boomerang's freezing time), which no run reaches: a free
 * coordinate leaves 0 with θ ≠ 0.
 * Quirks of the reference that are kept: the trace begins with (t0, x0, θ0, all free) (:189); acc += 1 before the bound check
 * (:158-162); a rejected proposal recomputes ab in full (:169); reflect_sticky! updates the f[i] coordinates while its sums test
 * θ[i] == 0; x[i] = -0*θ[i] (:133: the integer 0 times θ[i] -- a zero with θ[i]'s sign); a freeze with |x[i]| > 1e-8 is error(...)
 * (:129-132), status REF_FROZE_AWAY here; tref of the driver does not add t0 (:190).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pdmp_detmath.h"

#define REF_OK 0
#define REF_BOUND_VIOLATED 1 /* error("Tuning parameter `c` too small."), :160 */
#define REF_FROZE_AWAY 2     /* error("x[i] = ... !≈ 0 at ..."), :131 */
#define REF_STALLED 3        /* every clock at +Inf: no next event */

typedef struct {
    int64_t d;
    int32_t flow_kind; /* 0 BouncyParticle, 1 Boomerang (L = I) */
    int32_t adapt, strong_upperbounds, pad_;
    /* BouncyParticle: the FLOW's Γ, μ (ab, src/not_fact_samplers.jl:26-28; also the target ∇ϕ!(y,x) = Γ(x-μ) unless t_* is given).
     * Boomerang: the TARGET's Γ, μ (the flow's Γ is I). */
    const int64_t* colptr;
    const int64_t* rowval;
    const double* nzval;
    const double* mu;
    /* BouncyParticle with a target of its own, else NULL */
    const int64_t* t_colptr;
    const int64_t* t_rowval;
    const double* t_nzval;
    const double* t_mu;
    const double* mu_flow; /* Boomerang: centre of rotation */
    const double* kappa;
    double lambda_ref, rho, c, factor;
    uint64_t seed;
} ref_params;

typedef struct {
    int64_t num, nacc, nrefresh, nevents;
    uint64_t ndraw_main;
    int32_t status, pad_;
    double t, c;
} ref_result;

double ref_atan(double x) { return pdmp_atan(x); }

/* pos(x) = max(zero(x), x), src/common.jl:8 */
static double pos(double x) { return x > 0 ? x : (x != x ? x : 0.0); }

/* poisson_time(a, b, u), src/poissontime.jl:8-30 */
static double poisson_time(double a, double b, double u) {
    const double L = pdmp_log(u);
    if (b > 0) {
        if (a < 0) return sqrt(-L * 2.0 / b) - a / b;
        return sqrt((a / b) * (a / b) - L * 2.0 / b) - a / b;
    } else if (b == 0) {
        if (a > 0) return -L / a;
        return INFINITY;
    } else {
        if (a <= 0) return INFINITY;
        if (-L <= -(a * a) / b + (a * a) / (2 * b)) return -sqrt((a / b) * (a / b) - L * 2.0 / b) - a / b;
        return INFINITY;
    }
}

/* freezing_time(x, θ, F::Union{BouncyParticle, ZigZag}), src/ss_fact.jl:10-16 */
double ref_freezing_time_linear(double x, double th) {
    if (th * x >= 0) return INFINITY;
    return -x / th;
}
/* freezing_time(x, θ, μ, F::Boomerang), src/ss_not_fact.jl:5-20 */
double ref_freezing_time_boomerang(double x, double th, double mu) {
    const double pi = 0x1.921fb54442d18p+1; /* Float64(π) */
    if (mu == 0) {
        if (th * x >= 0.0) return pi - pdmp_atan(x / th);
        return pdmp_atan(-x / th);
    } else {
        const double u = (x * x - (2 * mu) * x) + th * th; /* x^2 - 2μ*x + θ^2 */
        if (u < 0) return INFINITY;
        /* t1 = mod(2atan((sqrt(u) - θ)/(2μ - x)), 2pi); mod(v, 2pi) of v in [-π, π] is v >= 0 ? v : v + 2π */
        const double v1 = 2 * pdmp_atan((sqrt(u) - th) / (2 * mu - x));
        const double t1 = v1 >= 0 ? v1 : v1 + 6.283185307179586;
        /* t2 = mod(-2atan((sqrt(u) + θ)/(2μ - x)), 2pi) */
        const double v2 = -(2 * pdmp_atan((sqrt(u) + th) / (2 * mu - x)));
        const double t2 = v2 >= 0 ? v2 : v2 + 6.283185307179586;
        if (t1 != t1) return t1; /* Julia's min / max propagate NaN */
        if (t2 != t2) return t2;
        if (x == 0) return t1 > t2 ? t1 : t2;
        return t1 < t2 ? t1 : t2;
    }
}

/* Σ a[k] b[k] in the 64-lane order; skip != NULL: elements with skip[k] == 0 are left out (sdot / subnormsq, :43-65) */
static double dot64(const double* a, const double* b, const double* skip, int64_t d) {
    double part[64];
    for (int l = 0; l < 64; ++l) {
        double s = 0.0;
        for (int64_t k = l; k < d; k += 64) {
            if (skip && skip[k] == 0.0) continue;
            s += a[k] * b[k];
        }
        part[l] = s;
    }
    for (int off = 1; off <= 32; off <<= 1) {
        double nxt[64];
        for (int l = 0; l < 64; ++l) nxt[l] = part[l] + part[l ^ off];
        memcpy(part, nxt, sizeof part);
    }
    return part[0];
}

/* y = Γ (v - μ) (μ may be NULL): idot per output element, ascending row order (Γ symmetric: column gather = row product) */
static void gamma_mul(const int64_t* cp, const int64_t* rv, const double* nz, const double* mu, const double* v, double* tmp, double* y,
                      int64_t d) {
    for (int64_t k = 0; k < d; ++k) tmp[k] = mu ? v[k] - mu[k] : v[k];
    for (int64_t r = 0; r < d; ++r) {
        double s = 0.0;
        for (int64_t p = cp[r]; p < cp[r + 1]; ++p) s += nz[p] * tmp[rv[p]];
        y[r] = s;
    }
}

/* ab(x, θ, c, flow) = ab(x, θ, GlobalBound(c), nothing, nothing, flow), src/not_fact_samplers.jl:26-28,34-37 */
static void ab(const ref_params* p, double c, const double* x, const double* th, double* tmp, double* w, double* a, double* b) {
    const int64_t d = p->d;
    if (p->flow_kind == 0) {
        gamma_mul(p->colptr, p->rowval, p->nzval, p->mu, x, tmp, w, d);
        *a = c + dot64(th, w, NULL, d); /* C.c + θ'*(B.Γ*(x-B.μ)) */
        gamma_mul(p->colptr, p->rowval, p->nzval, NULL, th, tmp, w, d);
        *b = dot64(th, w, NULL, d); /* θ'*(B.Γ*θ) */
    } else {
        for (int64_t k = 0; k < d; ++k) tmp[k] = x[k] - p->mu_flow[k];
        *a = sqrt(dot64(th, th, NULL, d) + dot64(tmp, tmp, NULL, d)) * c; /* sqrt(normsq(θ) + normsq((x - B.μ)))*C.c */
        *b = 0.0;
    }
}

static double freezing_time(const ref_params* p, int64_t i, double x, double th) {
    /* freezing_time(x, θ, μ, F) = freezing_time(x, θ, F) unless F is a Boomerang, src/ss_not_fact.jl:4-5 */
    return p->flow_kind == 1 ? ref_freezing_time_boomerang(x, th, p->mu_flow[i]) : ref_freezing_time_linear(x, th);
}

/*
 * x, th [d]: in x0, θ0, out the final state.  thf, f [d]: out the final θf and free mask (1 = free).  Events (t, x, θ, f) are stored
 * while nevents <= ev_cap (the count goes on; pass NULL buffers with ev_cap = 0 to store none).  free_time [d] (may be NULL): total
 * time every coordinate was free over [t0, final t] -- a by-product for the statistical tests, not part of the sampler.
 */
int ref_sspdmp_notfact(const ref_params* p, double t0, double T, double* x, double* th, double* thf, uint8_t* f, double* t_ev, double* x_ev,
                       double* th_ev, uint8_t* f_ev, int64_t ev_cap, double* free_time, ref_result* res) {
    const int64_t d = p->d;
    const uint64_t seed = p->seed;
    uint64_t nm = 0;
    double* g = (double*)malloc((size_t)d * sizeof(double));
    double* tmp = (double*)malloc((size_t)d * sizeof(double));
    double* w = (double*)malloc((size_t)d * sizeof(double));
    double* tfrez = (double*)malloc((size_t)d * sizeof(double));
    if (!g || !tmp || !w || !tfrez) return -1;
    int64_t num = 0, acc = 0, nrefresh = 0, nev = 0;
    int status = REF_OK;
    double t = t0, told = t0, c = p->c; /* :184-185 */
    const double rho = p->rho, rhobar = sqrt(1 - rho * rho); /* :32 */
    for (int64_t k = 0; k < d; ++k) {
        thf[k] = 0 * th[k]; /* θf = 0*θ, :186 */
        f[k] = 1;           /* :187 */
        if (free_time) free_time[k] = 0.0;
    }
#define PUSH_EVENT()                                                          \
    do {                                                                      \
        if (nev < ev_cap) {                                                   \
            t_ev[nev] = t;                                                    \
            memcpy(x_ev + nev * d, x, (size_t)d * sizeof(double));            \
            memcpy(th_ev + nev * d, th, (size_t)d * sizeof(double));          \
            memcpy(f_ev + nev * d, f, (size_t)d);                             \
        }                                                                     \
        nev++;                                                                \
    } while (0)
    PUSH_EVENT();                                                                    /* push!(Ξ, sevent(t, x0, θ0, f, Flow)), :189 */
    double tref = -pdmp_log(pdmp_u01(seed, PDMP_STREAM_MAIN, nm++)) / p->lambda_ref; /* waiting_time_ref(Flow), :190 */
    for (int64_t k = 0; k < d; ++k) tfrez[k] = t0 + freezing_time(p, k, x[k], th[k]); /* :191-192 */
    double a, b;
    ab(p, c, x, th, tmp, w, &a, &b);                                                 /* :194 */
    double tp = t + poisson_time(a, b, pdmp_u01(seed, PDMP_STREAM_MAIN, nm++));      /* :195 */

    while (t < T && status == REF_OK) { /* :196 */
        for (;;) {                      /* sticky_pdmp_inner!, :109 */
            /* tᶠ, i = findmin(tfrez), :110 */
            int64_t i = 0;
            double tf = tfrez[0];
            for (int64_t k = 1; k < d; ++k)
                if (tfrez[k] < tf || (tf != tf && tfrez[k] == tfrez[k])) {
                    tf = tfrez[k];
                    i = k;
                }
            /* tt, j = findmin([tref, tᶠ, t′]), :111 */
            int j;
            double tt;
            if (tref <= tf && tref <= tp) j = 1, tt = tref;
            else if (tf <= tp) j = 2, tt = tf;
            else j = 3, tt = tp;
            if (!(tt < INFINITY)) {
                status = REF_STALLED;
                break;
            }
            const double tau = tt - t; /* :112 */
            /* smove_forward!(τ, t, x, θ, f, Flow), :78-97 */
            t += tau;
            if (p->flow_kind == 0) {
                for (int64_t k = 0; k < d; ++k)
                    if (f[k]) x[k] += th[k] * tau;
            } else {
                double sn, cs;
                pdmp_sincos(tau, &sn, &cs);
                for (int64_t k = 0; k < d; ++k)
                    if (f[k]) {
                        const double m = p->mu_flow[k];
                        const double xn = (x[k] - m) * cs + th[k] * sn + m;
                        const double tn = -(x[k] - m) * sn + th[k] * cs;
                        x[k] = xn;
                        th[k] = tn;
                    }
            }
            if (free_time)
                for (int64_t k = 0; k < d; ++k)
                    if (f[k]) free_time[k] += tau;
            if (j == 1) { /* refreshment of the velocities, :115-126 */
                /* refresh_sticky_vel!, :31-41 */
                for (int64_t k = 0; k < d; ++k) {
                    double z0, z1;
                    pdmp_randn2(seed, PDMP_STREAM_MAIN, nm + (uint64_t)(((k >> 7) << 6) + (k & 63)), &z0, &z1);
                    const double z = ((k >> 6) & 1) ? z1 : z0;
                    if (f[k]) {
                        th[k] = rho * th[k] + rhobar * z;
                    } else {
                        const double sg = thf[k] > 0 ? 1.0 : (thf[k] < 0 ? -1.0 : thf[k]); /* sign(θf[i]) */
                        thf[k] = fabs(rho * thf[k] + rhobar * z) * sg;
                    }
                }
                nm += (uint64_t)(((d + 127) >> 7) << 6);
                tref = t + (-pdmp_log(pdmp_u01(seed, PDMP_STREAM_MAIN, nm++)) / p->lambda_ref); /* :117 */
                ab(p, c, x, th, tmp, w, &a, &b);                                               /* :118 */
                told = t;                                                                      /* :119 */
                tp = t + poisson_time(a, b, pdmp_u01(seed, PDMP_STREAM_MAIN, nm++));           /* :120 */
                for (int64_t k = 0; k < d; ++k)
                    if (f[k]) tfrez[k] = t + freezing_time(p, k, x[k], th[k]); /* :121 */
                for (int64_t k = 0; k < d; ++k)                                /* :122-126 */
                    if (!f[k]) tfrez[k] = t - pdmp_log(pdmp_u01(seed, PDMP_STREAM_MAIN, nm++)) / (p->kappa[k] * fabs(thf[k]));
                nrefresh++;
            } else if (j == 2) { /* get frozen or unfrozen in i, :127-151 */
                if (f[i]) {
                    if (fabs(x[i]) > 1e-8) { /* :129-132 */
                        status = REF_FROZE_AWAY;
                        break;
                    }
                    x[i] = 0.0 * th[i]; /* x[i] = -0*θ[i], :133 */
                    thf[i] = th[i];     /* θf[i], θ[i] = θ[i], 0.0 */
                    th[i] = 0.0;
                    f[i] = 0;
                    tfrez[i] = t - pdmp_log(pdmp_u01(seed, PDMP_STREAM_MAIN, nm++)) / (p->kappa[i] * fabs(thf[i])); /* :136 */
                    if (!p->strong_upperbounds) {                                                                    /* :138-142 */
                        ab(p, c, x, th, tmp, w, &a, &b);
                        told = t;
                        tp = t + poisson_time(a, b, pdmp_u01(seed, PDMP_STREAM_MAIN, nm++));
                    }
                } else { /* :143-151 */
                    th[i] = thf[i];
                    thf[i] = 0.0;
                    f[i] = 1;
                    tfrez[i] = t + freezing_time(p, i, x[i], th[i]);
                    ab(p, c, x, th, tmp, w, &a, &b);
                    told = t;
                    tp = t + poisson_time(a, b, pdmp_u01(seed, PDMP_STREAM_MAIN, nm++));
                }
            } else { /* t′: the usual bouncy particle / boomerang step, :152-173 */
                /* ∇ϕx = ∇ϕ!(∇ϕx, x, args...); grad_correct!(∇ϕx, x, Flow): y .-= x - μ for the Boomerang with L = I */
                if (p->t_colptr) gamma_mul(p->t_colptr, p->t_rowval, p->t_nzval, p->t_mu, x, tmp, g, d);
                else gamma_mul(p->colptr, p->rowval, p->nzval, p->mu, x, tmp, g, d);
                if (p->flow_kind == 1)
                    for (int64_t k = 0; k < d; ++k) g[k] -= x[k] - p->mu_flow[k];
                const double l = pos(dot64(g, th, NULL, d)); /* λ(∇ϕx, θ, Flow), src/not_fact_samplers.jl:14 */
                const double lb = pos(a + b * (t - told));   /* sλ̄(b, t - told), src/sfact.jl:70 */
                num++;
                if (pdmp_u01(seed, PDMP_STREAM_MAIN, nm++) * lb <= l) { /* :157 */
                    acc++;
                    if (l > lb) {
                        if (!p->adapt) {
                            status = REF_BOUND_VIOLATED;
                            break;
                        }
                        c *= p->factor;
                    }
                    /* reflect_sticky!, :68-76 */
                    const double cc = 2 * dot64(g, th, th, d) / dot64(g, g, th, d);
                    for (int64_t k = 0; k < d; ++k)
                        if (f[k]) th[k] -= cc * g[k];
                    ab(p, c, x, th, tmp, w, &a, &b); /* :164 */
                    told = t;
                    tp = t + poisson_time(a, b, pdmp_u01(seed, PDMP_STREAM_MAIN, nm++));
                    for (int64_t k = 0; k < d; ++k)
                        if (f[k]) tfrez[k] = t + freezing_time(p, k, x[k], th[k]); /* :167 */
                } else { /* nothing happened, :168-172 */
                    ab(p, c, x, th, tmp, w, &a, &b);
                    told = t;
                    tp = t + poisson_time(a, b, pdmp_u01(seed, PDMP_STREAM_MAIN, nm++));
                    continue;
                }
            }
            PUSH_EVENT(); /* :175 */
            break;
        }
    }
#undef PUSH_EVENT
    res->num = num;
    res->nacc = acc;
    res->nrefresh = nrefresh;
    res->nevents = nev;
    res->ndraw_main = nm;
    res->status = status;
    res->pad_ = 0;
    res->t = t;
    res->c = c;
    free(g);
    free(tmp);
    free(w);
    free(tfrez);
    return 0;
}
