/*
 * bps_logistic_ref.c -- sequential restatement of the speed-recorded Bouncy Particle driver on a Bayesian logistic-regression target, one
 * chain, for the tests to hold the device loop (csrc/pdmp_bps_logit.inc) to.  Test infrastructure only: the product never loads it.
 *
 * The loop, the draw table, the tie rule, the statuses and the flow forms (L = I, a lower CSC mass factor, diagonal U, oscn) are those of
 * modern_bps_ref.c, whose header states them; that file is included here for its helpers (poisson_time, dot64, the substitutions, randn_vec,
 * record_rate) and its parameter / result structs, and blref_pdmp below is mref_pdmp's text with three things exchanged: DPHI, MOVE and the
 * gradient of an accepted bounce.  (mref_params' t_colptr / t_rowval / t_nzval / t_mu go unread.)
 *
 * Target, with η = A x, ζ = A θ, p_i = 1 / (1 + pdmp_exp(−η_i)), w_i = p_i (1 − p_i):
 *   ϕ(x)    = Σ_i [ m_i log(1 + e^{η_i}) − y_i η_i ] + (γ0/2)‖x‖²
 *   ∇ϕ!(x)  = A'r + γ0 x,                    r_i = m_i p_i − y_i
 *   dϕ(x,θ) = ( Σ_i r_i ζ_i + γ0 θ·x ,  Σ_i m_i w_i ζ_i² + γ0 θ·θ )
 * A is n x d in CSC (column = coordinate, rows ascending, explicit zeros allowed), At its transpose in CSC (column = observation).
 *
 * This file FIXES the arithmetic the device must reproduce:
 *   η, ζ   are per-observation state.  ζ_i is a pure function of θ: one idot of At[:, i] against θ in ascending coordinate order (s = 0;
 *          s += At.nz[q] * θ[At.rv[q]]), recomputed whenever θ changes (setup, refreshment, accepted bounce).  η_i is gathered from x the
 *          same way at setup and AGAIN AT EVERY RECORD (this bounds the drift, and the record is where the sample is taken).  Between those
 *          points every move advances it incrementally, η_i = fma(τ, ζ_i, η_i): ONE rounding, a fused multiply-add.
 *   dϕ     the two data sums run over observations in the wave order of dot64: per-lane partials over i = l, l + 64, ... of
 *          (m_i p_i − y_i) ζ_i and of ((m_i w_i) ζ_i) ζ_i, then the xor butterfly 1, 2, 4, 8, 16, 32.  Each prior term is one dot64
 *          (θ·x, θ·θ) multiplied by γ0 and added after the data sum (also where γ0 == 0).
 *   ∇ϕ!    r[n] is staged, then one idot of A[:, e] against r per coordinate in ascending row order, then + γ0 x_e.
 * p and w: 1.0 / (1.0 + pdmp_exp(-η)) and p * (1.0 - p); past exp's range p is exactly 0 or 1 and w is 0.
 */
#include <math.h>

#include "modern_bps_ref.c"

typedef struct {
    mref_params base; /* d, adapt, oscn, Lcp / Lrv / Lnz, u_diag, lambda_ref, rho, c, factor, seed */
    int64_t n;
    const int64_t *A_colptr, *A_rowval;   /* [d + 1], [nnz] */
    const double* A_nzval;
    const int64_t *At_colptr, *At_rowval; /* [n + 1], [nnz] */
    const double* At_nzval;
    const double *y, *m;                  /* [n] */
    double gamma0;
} blref_params;

static void blref_link(double eta, double* p, double* w) {
    const double q = 1.0 / (1.0 + pdmp_exp(-eta));
    *p = q;
    *w = q * (1.0 - q);
}

/* out[i] = idot(At[:, i], v) */
static void blref_gather_obs(const blref_params* P, const double* v, double* out) {
    for (int64_t i = 0; i < P->n; ++i) {
        double s = 0.0;
        for (int64_t q = P->At_colptr[i]; q < P->At_colptr[i + 1]; ++q) s += P->At_nzval[q] * v[P->At_rowval[q]];
        out[i] = s;
    }
}

static double blref_sum64(const double* part_in) {
    double part[64];
    memcpy(part, part_in, sizeof part);
    for (int off = 1; off <= 32; off <<= 1) {
        double nxt[64];
        for (int l = 0; l < 64; ++l) nxt[l] = part[l] + part[l ^ off];
        memcpy(part, nxt, sizeof part);
    }
    return part[0];
}

/* dϕ from the carried η, ζ */
static void blref_dphi(const blref_params* P, const double* eta, const double* zeta, const double* x, const double* th, double* d1, double* d2) {
    double s1[64], s2[64];
    for (int l = 0; l < 64; ++l) {
        double a1 = 0.0, a2 = 0.0;
        for (int64_t i = l; i < P->n; i += 64) {
            double p, w;
            blref_link(eta[i], &p, &w);
            a1 += (P->m[i] * p - P->y[i]) * zeta[i];
            a2 += ((P->m[i] * w) * zeta[i]) * zeta[i];
        }
        s1[l] = a1, s2[l] = a2;
    }
    *d1 = blref_sum64(s1) + P->gamma0 * dot64(th, x, P->base.d);
    *d2 = blref_sum64(s2) + P->gamma0 * dot64(th, th, P->base.d);
}

/* g = ∇ϕ!(x) from the carried η; r [n] is scratch */
static void blref_grad(const blref_params* P, const double* eta, const double* x, double* r, double* g) {
    for (int64_t i = 0; i < P->n; ++i) {
        double p, w;
        blref_link(eta[i], &p, &w);
        r[i] = P->m[i] * p - P->y[i];
    }
    for (int64_t e = 0; e < P->base.d; ++e) {
        double s = 0.0;
        for (int64_t q = P->A_colptr[e]; q < P->A_colptr[e + 1]; ++q) s += P->A_nzval[q] * r[P->A_rowval[q]];
        g[e] = s + P->gamma0 * x[e];
    }
}

/* pointwise evaluator: dphi[2] and grad[d] at (x, θ), η and ζ gathered afresh */
int blref_eval(const blref_params* P, const double* x, const double* th, double* dphi, double* grad) {
    double* eta = (double*)malloc((size_t)P->n * sizeof(double));
    double* zeta = (double*)malloc((size_t)P->n * sizeof(double));
    double* r = (double*)malloc((size_t)P->n * sizeof(double));
    if (!eta || !zeta || !r) return -1;
    blref_gather_obs(P, x, eta);
    blref_gather_obs(P, th, zeta);
    blref_dphi(P, eta, zeta, x, th, &dphi[0], &dphi[1]);
    blref_grad(P, eta, x, r, grad);
    free(eta);
    free(zeta);
    free(r);
    return 0;
}

/* mref_pdmp on the logistic target: same arguments, same result struct */
int blref_pdmp(const blref_params* P, double t0, double T, int64_t nrec_limit, double* x, double* th, double* t_ev, double* x_ev, double* th_ev,
               int64_t ev_cap, mref_result* res) {
    const mref_params* p = &P->base;
    const int64_t d = p->d, n = P->n;
    const uint64_t seed = p->seed;
    uint64_t nm = 0;
    double* g = (double*)malloc((size_t)d * sizeof(double));
    double* tmp = (double*)malloc((size_t)d * sizeof(double));
    double* w = (double*)malloc((size_t)d * sizeof(double));
    double* z = (double*)malloc((size_t)d * sizeof(double));
    double* eta = (double*)malloc((size_t)n * sizeof(double));
    double* zeta = (double*)malloc((size_t)n * sizeof(double));
    double* r = (double*)malloc((size_t)n * sizeof(double));
    tri F;
    memset(&F, 0, sizeof F);
    if (!g || !tmp || !w || !z || !eta || !zeta || !r) return -1;
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

#define DPHI() blref_dphi(P, eta, zeta, x, th, &th_dphi, &v)
#define THETA_CHANGED() blref_gather_obs(P, th, zeta)
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
#define MOVE(tau)                                                         \
    do {                                                                  \
        t += (tau);                                                       \
        for (int64_t k = 0; k < d; ++k) x[k] += th[k] * (tau);            \
        for (int64_t i = 0; i < n; ++i) eta[i] = fma((tau), zeta[i], eta[i]); \
    } while (0)

    blref_gather_obs(P, x, eta);
    THETA_CHANGED();
    DPHI();                          /* :342 */
    REBOUND();                       /* :346, :355 */
    double Drec = 1 / p->lambda_ref; /* :354 */

    while (t < T && (nrec_limit == 0 || nrec < nrec_limit) && status == REF_OK) { /* :360 */
        for (;;) {                                                                /* pdmp_inner!, :222 */
            if (t + Drec / V <= tp) {                                             /* record, :223-237 */
                const double tau = Drec / V;
                MOVE(tau);
                blref_gather_obs(P, x, eta); /* η = A x afresh at every record */
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
                THETA_CHANGED();
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
                    blref_grad(P, eta, x, r, g); /* ∇ϕ!, :265 */
                    if (p->oscn) {               /* oscn!(rng, θ, ∇ϕx, ρ), src/oscn.jl */
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
                    THETA_CHANGED();
                    DPHI();
                    REBOUND();
                } else {
                    REBOUND(); /* :278-279 with the θdϕ, v of :256 */
                }
            }
        }
    }
#undef DPHI
#undef THETA_CHANGED
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
    free(eta);
    free(zeta);
    free(r);
    if (p->Lcp) tri_free(&F);
    return 0;
}

#ifdef BLREF_MAIN
/* stand-alone driver for a sanitizer build: d = 8, n = 100, a banded design with an empty column, every flow form, the pointwise evaluator */
#include <stdio.h>
int main(void) {
    enum { D = 8, NOBS = 100, N = 200 };
    int64_t acp[D + 1], arv[3 * NOBS], tcp[NOBS + 1], trv[3 * NOBS];
    double anz[3 * NOBS], tnz[3 * NOBS], y[NOBS], m[NOBS];
    int64_t q = 0;
    for (int j = 0; j < D; ++j) { /* observation i touches coordinates i % 7, (i + 2) % 7, (i + 3) % 7; coordinate 7 has no entry */
        acp[j] = q;
        for (int i = 0; i < NOBS; ++i)
            for (int s = 0; s < 3; ++s)
                if (j < 7 && (i + (s ? s + 1 : 0)) % 7 == j) arv[q] = i, anz[q] = 0.3 * (s + 1) - 0.1 * (i % 5), ++q;
    }
    acp[D] = q;
    int64_t fill[NOBS];
    for (int i = 0; i <= NOBS; ++i) tcp[i] = 0;
    for (int64_t k = 0; k < q; ++k) tcp[arv[k] + 1]++;
    for (int i = 0; i < NOBS; ++i) tcp[i + 1] += tcp[i], fill[i] = tcp[i];
    for (int j = 0; j < D; ++j)
        for (int64_t k = acp[j]; k < acp[j + 1]; ++k) trv[fill[arv[k]]] = j, tnz[fill[arv[k]]++] = anz[k];
    for (int i = 0; i < NOBS; ++i) m[i] = 1 + i % 3, y[i] = (i % 4 == 0) ? m[i] : (i % 2);
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
        blref_params P;
        memset(&P, 0, sizeof P);
        P.base.d = D, P.base.adapt = 1;
        P.base.lambda_ref = 1.0, P.base.rho = 0.9, P.base.c = 20.0, P.base.factor = 2.0, P.base.seed = 7 + form;
        P.n = NOBS, P.A_colptr = acp, P.A_rowval = arv, P.A_nzval = anz, P.At_colptr = tcp, P.At_rowval = trv, P.At_nzval = tnz;
        P.y = y, P.m = m, P.gamma0 = 0.7;
        if (form == 1) P.base.u_diag = u;
        if (form == 2) P.base.Lcp = lcp, P.base.Lrv = lrv, P.base.Lnz = lnz;
        if (form == 3) P.base.oscn = 1;
        double x[D], th[D], dphi[2], grad[D];
        for (int k = 0; k < D; ++k) x[k] = 0.1 * k - 0.3, th[k] = (k & 1) ? -1.0 : 0.7;
        if (blref_eval(&P, x, th, dphi, grad) != 0 || dphi[0] != dphi[0] || !(dphi[1] > 0)) bad = 1;
        double* te = (double*)malloc(N * sizeof(double));
        double* xe = (double*)malloc(N * D * sizeof(double));
        double* the = (double*)malloc(N * D * sizeof(double));
        mref_result r;
        if (blref_pdmp(&P, 0.0, INFINITY, N, x, th, te, xe, the, N, &r) != 0 || r.status != REF_OK || r.nevents != N) bad = 1;
        printf("form %d: status %d records %lld num %lld acc %lld draws %llu t %.6f dphi %.6f %.6f\n", form, r.status, (long long)r.nevents,
               (long long)r.num, (long long)r.nacc, (unsigned long long)r.ndraw_main, r.t, dphi[0], dphi[1]);
        free(te);
        free(xe);
        free(the);
    }
    return bad;
}
#endif
