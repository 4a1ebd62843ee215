/*
 * modern_bps_ref.c -- sequential restatement of the reference's speed-recorded Bouncy Particle driver ("ModernBPS"),
 *   pdmp(dϕ, ∇ϕ!, t0, x0, θ0, T, c::LocalBound, flow::BouncyParticle; oscn, adapt, factor)
 * (src/not_fact_samplers.jl:151-283, 336-384, with oscn! of src/oscn.jl), one chain, for the tests to hold the device loop
 * (csrc/pdmp_bps_modern.inc) to.  Test infrastructure only: the product never loads it.  It shares include/pdmp_detmath.h with the kernels
 * (Philox, log, Box-Muller) and restates everything else itself.
 *
 * Target: Gaussian, dϕ(t, x, θ) = (θ'Γt(x − μt), θ'Γtθ) and ∇ϕ!(y, x) = Γt(x − μt), each one CSC product per output element in
 * ascending row order (idot) followed by one dot.
 *
 * What the reference leaves open is fixed here:
 *   draws   everything comes from PDMP_STREAM_MAIN in program order, nm = 0, 1, 2, ...   The draw table:
 *             next_event1   2: poisson_time(a, b, u) first, then randexp = -pdmp_log(u) of τrefresh   (setup, and after every record,
 *                              refreshment, expiry and proposal -- accepted or not)
 *             proposal      1: the thinning coin (:259), before the next_event1 that follows it
 *             refresh!      R = ((d+127)>>7)<<6 Box-Muller blocks: element 128a + 64b + l is branch b of block nm + 64a + l
 *             oscn!         R blocks in the same mapping, unless ρ == 1 (none)
 *           so ndraw = 2(1 + records + refreshments + expiries + num) + num + R(refreshments + oscn bounces with ρ != 1).
 *           There is no τref draw at setup: the modern driver has none.
 *   ties    findmin((τ, Δ, τrefresh)) takes the first minimum: bounce before expire before refresh.  A NaN never wins (Julia's findmin
 *           would return it); a NaN time ends the chain as STALLED through the Δrec assertion below.
 *   sums    dot / normsq / norm in the 64-lane order of wave_sum_f64: per-lane partial sums over l, l+64, ..., then the xor butterfly
 *           1, 2, 4, 8, 16, 32.  norm is the sqrt of such a sum.
 *   flow    L form (u_diag == NULL): reflect! :161-164, refresh! :173-180, V ≡ 1 (:198).  L is the identity (Lcp == NULL) or a lower
 *           triangular CSC factor with the diagonal stored first in each column; L\ and L'\ are the column-oriented substitutions of
 *           oracle/pdmp_oracle.c (tri_solve_lower / tri_solve_upper).
 *           Diagonal-U form (u_diag != NULL, L missing): the reference names PDMats, which it does not vendor.  These three definitions
 *           ARE the contract: reflect! (:156-160) with z = u .* ∇ϕx; refresh! (:165-172) with unwhiten(U, z) = sqrt.(u) .* z;
 *           V = record_rate(θ) = norm(θ ./ sqrt.(u)) (:197).
 *   oscn    src/oscn.jl with normalize = false; √(1.0f0 - ρ^2) is the double sqrt(1 - ρ·ρ); -vₚ + v⊥ + z is ((-vₚ) + v⊥) + z.
 * Kept as the reference has them: the record branch checks l > lb with τ = Δrec/V (:224-232); acc += 1 before the bound check (:260-264);
 * the coin is <=; c *= factor acts on LocalBound (src/types.jl:129); the trace does not begin with (t0, x0, θ0) -- the first stored element
 * is the first record; the driver loops `while T isa Int ? iter < T : t < T`, so the last record has t >= T.  Here both limits may be
 * given: the loop runs while t < T and (nrec_limit == 0 or records < nrec_limit).
 * Statuses: l > lb without adapt is the reference's error("Tuning parameter `c` too small.") -> REF_BOUND_VIOLATED (nothing is recorded
 * by the failing step); `@assert Δrec > 0` (:239) failing -> REF_STALLED.
 * Out of scope: adapt_mass, InvChol, :invalid re-entry, Boomerang, oscn with L != I (the reference asserts L == I, :267).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pdmp_detmath.h"

#define REF_OK 0
#define REF_BOUND_VIOLATED 1
#define REF_STALLED 2

typedef struct {
    int64_t d;
    int32_t adapt, oscn;
    const int64_t* t_colptr; /* target Γt, CSC, rows ascending */
    const int64_t* t_rowval;
    const double* t_nzval;
    const double* t_mu;      /* [d] or NULL */
    const int64_t* Lcp;      /* mass factor L (lower CSC, diagonal first) or NULL: identity */
    const int64_t* Lrv;
    const double* Lnz;
    const double* u_diag;    /* [d] > 0: the diagonal-U form, or NULL: the L form */
    double lambda_ref, rho, c, factor;
    uint64_t seed;
} mref_params;

typedef struct {
    int64_t num, nacc, nrefresh, nexpire, nevents, nviol, noscn_draws;
    uint64_t ndraw_main;
    int32_t status, pad_;
    double t, c, V;
} mref_result;

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

static double dot64(const double* a, const double* b, int64_t d) {
    double part[64];
    for (int l = 0; l < 64; ++l) {
        double s = 0.0;
        for (int64_t k = l; k < d; k += 64) s += a[k] * b[k];
        part[l] = s;
    }
    for (int off = 1; off <= 32; off <<= 1) {
        double nxt[64];
        for (int l = 0; l < 64; ++l) nxt[l] = part[l] + part[l ^ off];
        memcpy(part, nxt, sizeof part);
    }
    return part[0];
}

/* y = Γt (v − μ) (μ may be NULL) */
static void gamma_mul(const mref_params* p, const double* mu, const double* v, double* tmp, double* y) {
    const int64_t d = p->d;
    for (int64_t k = 0; k < d; ++k) tmp[k] = mu ? v[k] - mu[k] : v[k];
    for (int64_t r = 0; r < d; ++r) {
        double s = 0.0;
        for (int64_t q = p->t_colptr[r]; q < p->t_colptr[r + 1]; ++q) s += p->t_nzval[q] * tmp[p->t_rowval[q]];
        y[r] = s;
    }
}

typedef struct {
    int64_t d;
    const int64_t *cp, *rv;
    const double* nz;
    int64_t *tcp, *trv; /* L' as an upper CSC, diagonal last */
    double* tnz;
} tri;

static int tri_build(tri* F, const mref_params* p) {
    const int64_t d = p->d, nnz = p->Lcp[d];
    F->d = d, F->cp = p->Lcp, F->rv = p->Lrv, F->nz = p->Lnz;
    F->tcp = (int64_t*)calloc((size_t)d + 2, sizeof(int64_t));
    F->trv = (int64_t*)malloc((size_t)nnz * sizeof(int64_t));
    F->tnz = (double*)malloc((size_t)nnz * sizeof(double));
    if (!F->tcp || !F->trv || !F->tnz) return -1;
    for (int64_t q = 0; q < nnz; ++q) F->tcp[F->rv[q] + 2]++;
    for (int64_t j = 0; j < d; ++j) F->tcp[j + 2] += F->tcp[j + 1];
    for (int64_t j = 0; j < d; ++j)
        for (int64_t q = F->cp[j]; q < F->cp[j + 1]; ++q) {
            const int64_t s = F->tcp[F->rv[q] + 1]++;
            F->trv[s] = j;
            F->tnz[s] = F->nz[q];
        }
    return 0;
}
static void tri_free(tri* F) {
    free(F->tcp);
    free(F->trv);
    free(F->tnz);
}
/* b <- L \ b */
static void solve_lower(const tri* F, double* b) {
    for (int64_t j = 0; j < F->d; ++j) {
        const double yj = b[j] / F->nz[F->cp[j]];
        b[j] = yj;
        for (int64_t q = F->cp[j] + 1; q < F->cp[j + 1]; ++q) b[F->rv[q]] = b[F->rv[q]] - F->nz[q] * yj;
    }
}
/* y <- L' \ y */
static void solve_upper(const tri* F, double* y) {
    for (int64_t j = F->d - 1; j >= 0; --j) {
        const double zj = y[j] / F->tnz[F->tcp[j + 1] - 1];
        y[j] = zj;
        for (int64_t q = F->tcp[j]; q < F->tcp[j + 1] - 1; ++q) y[F->trv[q]] = y[F->trv[q]] - F->tnz[q] * zj;
    }
}

/* randn(rng, d) into z: R = ((d+127)>>7)<<6 blocks from draw nm on */
static uint64_t randn_vec(uint64_t seed, uint64_t nm, int64_t d, double* z) {
    for (int64_t k = 0; k < d; ++k) {
        double z0, z1;
        pdmp_randn2(seed, PDMP_STREAM_MAIN, nm + (uint64_t)(((k >> 7) << 6) + (k & 63)), &z0, &z1);
        z[k] = ((k >> 6) & 1) ? z1 : z0;
    }
    return nm + (uint64_t)(((d + 127) >> 7) << 6);
}

/* record_rate(θ, F), :197-198 */
static double record_rate(const mref_params* p, const double* th, double* tmp) {
    if (!p->u_diag) return 1.0;
    for (int64_t k = 0; k < p->d; ++k) tmp[k] = th[k] / sqrt(p->u_diag[k]);
    return sqrt(dot64(tmp, tmp, p->d));
}

/*
 * x, th [d]: in x0, θ0, out the final state.  Records (t, x, θ) are stored while their index < ev_cap (the count goes on).
 * Runs while t < T and (nrec_limit == 0 or records < nrec_limit).
 */
int mref_pdmp(const mref_params* p, double t0, double T, int64_t nrec_limit, double* x, double* th, double* t_ev, double* x_ev, double* th_ev,
              int64_t ev_cap, mref_result* res) {
    const int64_t d = p->d;
    const uint64_t seed = p->seed;
    uint64_t nm = 0;
    double* g = (double*)malloc((size_t)d * sizeof(double));
    double* tmp = (double*)malloc((size_t)d * sizeof(double));
    double* w = (double*)malloc((size_t)d * sizeof(double));
    double* z = (double*)malloc((size_t)d * sizeof(double));
    tri F;
    memset(&F, 0, sizeof F);
    if (!g || !tmp || !w || !z) return -1;
    if (p->Lcp && tri_build(&F, p) != 0) return -1;
    const int has_mass = p->Lcp != NULL;
    int64_t num = 0, acc = 0, nrefresh = 0, nexpire = 0, nrec = 0, nviol = 0, noscn = 0;
    int status = REF_OK;
    const double rho = p->rho, rhobar = sqrt(1 - rho * rho);
    double t = t0, c = p->c;
    double V = record_rate(p, th, tmp); /* :339 */
    double a, b, Delta, tp;
    int action; /* 0 bounce, 1 expire, 2 refresh */
    double th_dphi, v;

/* θdϕ, v = dϕ(t, x, θ, flow) */
#define DPHI()                                  \
    do {                                        \
        gamma_mul(p, p->t_mu, x, tmp, w);       \
        th_dphi = dot64(th, w, d);              \
        gamma_mul(p, NULL, th, tmp, w);         \
        v = dot64(th, w, d);                    \
    } while (0)
/* abc = ab(t, x, θ, V, c, θdϕ, v, flow) (:200-202); t′, action = next_event1(rng, (t, x, θ, V), abc, flow) (:204-211) */
#define REBOUND()                                                                                           \
    do {                                                                                                    \
        a = c + th_dphi;                                                                                    \
        b = v;                                                                                              \
        Delta = t + 2 * sqrt((double)d) / c / V;                                                            \
        const double tau_b = t + poisson_time(a, b, pdmp_u01(seed, PDMP_STREAM_MAIN, nm));                  \
        const double tau_r = t + (-pdmp_log(pdmp_u01(seed, PDMP_STREAM_MAIN, nm + 1)) / p->lambda_ref) / V; \
        nm += 2;                                                                                            \
        if (tau_b <= Delta && tau_b <= tau_r) action = 0, tp = tau_b;                                       \
        else if (Delta <= tau_r) action = 1, tp = Delta;                                                    \
        else action = 2, tp = tau_r;                                                                        \
    } while (0)
#define MOVE(tau)                                          \
    do {                                                   \
        t += (tau);                                        \
        for (int64_t k = 0; k < d; ++k) x[k] += th[k] * (tau); \
    } while (0)

    DPHI();                            /* :342 (∇ϕ! of :343 is recomputed before every use) */
    REBOUND();                         /* :346, :355 */
    double Drec = 1 / p->lambda_ref;   /* :354 */

    while (t < T && (nrec_limit == 0 || nrec < nrec_limit) && status == REF_OK) { /* :360 */
        for (;;) {                                                                /* pdmp_inner!, :222 */
            if (t + Drec / V <= tp) {                                             /* record, :223-237 */
                const double tau = Drec / V;
                MOVE(tau);
                Drec = 1 / p->lambda_ref;
                DPHI();
                const double l = th_dphi, lb = pos(a + b * tau);
                if (l > lb) {
                    nviol++;
                    if (!p->adapt) {
                        status = REF_BOUND_VIOLATED;
                        break;
                    }
                    c *= p->factor;
                }
                REBOUND();
                if (nrec < ev_cap) { /* push!(Ξ, event(t, x, θ, flow)), :362 */
                    t_ev[nrec] = t;
                    memcpy(x_ev + nrec * d, x, (size_t)d * sizeof(double));
                    memcpy(th_ev + nrec * d, th, (size_t)d * sizeof(double));
                }
                nrec++;
                break;
            }
            Drec = Drec - (tp - t) * V; /* :238 */
            if (!(Drec > 0.0)) {        /* @assert Δrec > 0.0, :239 */
                status = REF_STALLED;
                break;
            }
            const double tau = tp - t;
            MOVE(tau);
            if (action == 2) { /* :240-246 */
                nm = randn_vec(seed, nm, d, z);
                if (p->u_diag) {
                    for (int64_t k = 0; k < d; ++k) z[k] = sqrt(p->u_diag[k]) * z[k]; /* unwhiten */
                } else if (has_mass) {
                    solve_upper(&F, z); /* L'\randn */
                }
                for (int64_t k = 0; k < d; ++k) {
                    th[k] *= rho;
                    th[k] += (1.0 * rhobar) * z[k];
                }
                V = record_rate(p, th, tmp);
                nrefresh++;
                DPHI();
                REBOUND();
            } else if (action == 1) { /* :247-252 */
                nexpire++;
                DPHI();
                REBOUND();
            } else { /* :253-281 */
                DPHI();
                const double l = th_dphi, lb = pos(a + b * tau);
                num++;
                if (pdmp_u01(seed, PDMP_STREAM_MAIN, nm++) * lb <= l) {
                    acc++;
                    if (l > lb) {
                        nviol++;
                        if (!p->adapt) {
                            status = REF_BOUND_VIOLATED;
                            break;
                        }
                        c *= p->factor;
                    }
                    gamma_mul(p, p->t_mu, x, tmp, g); /* ∇ϕ!, :265 */
                    if (p->oscn) {                    /* oscn!(rng, θ, ∇ϕx, ρ), src/oscn.jl */
                        const double gg = dot64(g, g, d);
                        const double cp = dot64(th, g, d) / gg;
                        if (rho == 1) {
                            for (int64_t k = 0; k < d; ++k) th[k] = th[k] - 2 * (cp * g[k]);
                        } else {
                            nm = randn_vec(seed, nm, d, z);
                            noscn++;
                            const double sq = sqrt(1.0 - rho * rho);
                            for (int64_t k = 0; k < d; ++k) z[k] = z[k] * sq;
                            const double cz = dot64(z, g, d) / gg;
                            for (int64_t k = 0; k < d; ++k) {
                                const double vp = cp * g[k];
                                const double vperp = rho * (th[k] - vp);
                                th[k] = (-vp + vperp) + (z[k] - cz * g[k]);
                            }
                        }
                    } else if (p->u_diag) { /* :156-160 */
                        for (int64_t k = 0; k < d; ++k) w[k] = p->u_diag[k] * g[k];
                        const double coef = 2 * dot64(g, th, d) / dot64(g, w, d);
                        for (int64_t k = 0; k < d; ++k) th[k] -= coef * w[k];
                    } else if (has_mass) { /* :161-164 */
                        const double gt = dot64(g, th, d);
                        memcpy(w, g, (size_t)d * sizeof(double));
                        solve_lower(&F, w);
                        const double nrm = dot64(w, w, d);
                        solve_upper(&F, w);
                        const double coef = 2 * gt / nrm;
                        for (int64_t k = 0; k < d; ++k) th[k] -= coef * w[k];
                    } else {
                        const double coef = 2 * dot64(g, th, d) / dot64(g, g, d);
                        for (int64_t k = 0; k < d; ++k) th[k] -= coef * g[k];
                    }
                    V = record_rate(p, th, tmp);
                    DPHI();
                    REBOUND();
                } else {
                    REBOUND(); /* :278-279 with the θdϕ, v of :256 */
                }
            }
        }
    }
#undef DPHI
#undef REBOUND
#undef MOVE
    res->num = num;
    res->nacc = acc;
    res->nrefresh = nrefresh;
    res->nexpire = nexpire;
    res->nevents = nrec;
    res->nviol = nviol;
    res->noscn_draws = noscn;
    res->ndraw_main = nm;
    res->status = status;
    res->pad_ = 0;
    res->t = t;
    res->c = c;
    res->V = V;
    free(g);
    free(tmp);
    free(w);
    free(z);
    if (p->Lcp) tri_free(&F);
    return 0;
}

#ifdef MREF_MAIN
/* stand-alone driver for a sanitizer build: the d = 8 case of the tests on a tridiagonal target, both forms, oscn and a dense L */
#include <stdio.h>
int main(void) {
    enum { D = 8, N = 200 };
    int64_t cp[D + 1], rv[3 * D];
    double nz[3 * D];
    int64_t q = 0;
    for (int j = 0; j < D; ++j) {
        cp[j] = q;
        for (int r = j - 1; r <= j + 1; ++r)
            if (r >= 0 && r < D) rv[q] = r, nz[q] = (r == j) ? 2.0 : -0.5, ++q;
    }
    cp[D] = q;
    int64_t lcp[D + 1], lrv[D * (D + 1) / 2];
    double lnz[D * (D + 1) / 2], u[D];
    q = 0;
    for (int j = 0; j < D; ++j) {
        lcp[j] = q;
        for (int r = j; r < D; ++r) lrv[q] = r, lnz[q] = (r == j) ? 1.0 + 0.1 * j : 0.05 * (r - j), ++q;
        u[j] = 0.5 + 0.25 * j;
    }
    lcp[D] = q;
    int bad = 0;
    for (int form = 0; form < 4; ++form) {
        mref_params p;
        memset(&p, 0, sizeof p);
        p.d = D, p.t_colptr = cp, p.t_rowval = rv, p.t_nzval = nz;
        p.lambda_ref = 1.0, p.rho = 0.9, p.c = 20.0, p.factor = 2.0, p.seed = 7 + form;
        if (form == 1) p.u_diag = u;
        if (form == 2) p.Lcp = lcp, p.Lrv = lrv, p.Lnz = lnz;
        if (form == 3) p.oscn = 1;
        double x[D], th[D];
        for (int k = 0; k < D; ++k) x[k] = 0.1 * k - 0.3, th[k] = (k & 1) ? -1.0 : 0.7;
        double* te = (double*)malloc(N * sizeof(double));
        double* xe = (double*)malloc(N * D * sizeof(double));
        double* the = (double*)malloc(N * D * sizeof(double));
        mref_result r;
        if (mref_pdmp(&p, 0.0, INFINITY, N, x, th, te, xe, the, N, &r) != 0 || r.status != REF_OK || r.nevents != N) bad = 1;
        printf("form %d: status %d records %lld num %lld acc %lld draws %llu t %.6f\n", form, r.status, (long long)r.nevents, (long long)r.num,
               (long long)r.nacc, (unsigned long long)r.ndraw_main, r.t);
        free(te);
        free(xe);
        free(the);
    }
    return bad;
}
#endif
