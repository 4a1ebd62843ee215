/* condition_ref.c -- TEST INFRASTRUCTURE ONLY: the conditional trace (src/condition.jl, conditional_trace(Ξ, (p, n))), twice.
 *
 * ref_condition_fact / ref_condition_pdmp: the CONTRACT of the device consumers (DESIGN.md "Conditional trace"), one chain, the whole trace at
 * once, one event after the other.  Doubles throughout, no fused multiply-add (built with oracle/Makefile's flags); every dot product in the
 * order of dot_wave64 (oracle/pdmp_oracle.c): lane l sums elements l, l + 64, ... in order, then the xor butterfly 1, 2, 4, 8, 16, 32.
 *
 *   FactTrace.  S = the ascending indices with n_j != 0.  A piece opens at t_b (t0, afterwards the time of the latest event of a coordinate of
 *   S); with the cursors (t_c, x_c, θ_c) of S as of t_b:  xs_k = x_c + θ_c·(t_b − t_c),  g = Σ n_k·(p_k − xs_k),  h = Σ n_k·θ_c,k (list
 *   position = element index),  τ = g / h,  s = t_b + τ.  The piece has a candidate iff τ > 0.  It becomes a hit, once, when the next event of
 *   a coordinate of S arrives at t_e >= s, or when the last event time of the trace T_last >= s.  The row of a hit: x_c + θ_c·(s − t_c) for
 *   every j from j's last event with t < s (strictly), else from (t0, x0_j, θ0_j).
 *
 *   PDMPTrace.  For every event (t_k, x_k, θ_k[, f_k]) with the cursor (t_c, x_c, θ_c, f_c) before it:  g = dot_wave64(p − x_c, n),
 *   h = dot_wave64(θ_c, n),  τ = g / h;  a hit iff τ > 0 and t_c + τ < t_k, at t_c + τ, row_j = f_c,j ? x_c,j + θ_c,j·τ : x_c,j.
 *
 * ref_condition_fact_literal / ref_condition_pdmp_literal: src/condition.jl:35-76 line by line -- the state moved in place to every hit and
 * every event, τ recomputed from the point just put on the plane -- with plain left-to-right dot products and a cap on the hits of one event
 * segment behind its first (the reference itself never ends when t + τ == t).  They also return the event index each hit was found before.
 *
 * Every function returns the number of hits (it may exceed max_hits: the rows behind max_hits are not stored), -1 when out of memory.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    double t;
    int64_t i;
    double x, theta;
} cond_event;

static double dot_wave64(const double* a, const double* b, int64_t d) {
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

static double dot_plain(const double* a, const double* b, int64_t d) {
    double s = 0.0;
    for (int64_t k = 0; k < d; ++k) s += a[k] * b[k];
    return s;
}

/* ---------------------------------------------------------------------------------------------------------------- the contract */

typedef struct {
    int64_t d, n_ev, nS, q, nhits, max_hits;
    const cond_event* ev;
    const int64_t* idx;                 /* S */
    double *ct, *cx, *cth;              /* full cursors: the events [0, q) applied */
    double *st, *sx, *sth, *pn, *pp;    /* the cursors of S as of t_b; n and p over S */
    double *wa;                         /* [nS] */
    double t_b, s, h;
    int cand, done;
    double *out_t, *out_x, *out_h;
} fact_walk;

static void fact_open(fact_walk* w, double t_b) {
    for (int64_t k = 0; k < w->nS; ++k) {
        const double xs = w->sx[k] + w->sth[k] * (t_b - w->st[k]);
        w->wa[k] = w->pp[k] - xs;
    }
    const double g = dot_wave64(w->pn, w->wa, w->nS);
    const double h = dot_wave64(w->pn, w->sth, w->nS);
    const double tau = g / h;
    w->t_b = t_b;
    w->s = t_b + tau;
    w->h = h;
    w->cand = tau > 0;
    w->done = 0;
}

static void fact_emit(fact_walk* w) {
    const double s = w->s;
    while (w->q < w->n_ev && w->ev[w->q].t < s) {
        const cond_event* e = &w->ev[w->q];
        w->ct[e->i] = e->t;
        w->cx[e->i] = e->x;
        w->cth[e->i] = e->theta;
        w->q += 1;
    }
    if (w->nhits < w->max_hits) {
        if (w->out_t) w->out_t[w->nhits] = s;
        if (w->out_h) w->out_h[w->nhits] = w->h;
        if (w->out_x)
            for (int64_t j = 0; j < w->d; ++j) w->out_x[w->nhits * w->d + j] = w->cx[j] + w->cth[j] * (s - w->ct[j]);
    }
    w->nhits += 1;
    w->done = 1;
}

int64_t ref_condition_fact(int64_t d, int64_t n_ev, double t0, const double* x0, const double* th0, const cond_event* ev, const double* p,
                           const double* n, int64_t max_hits, double* out_t, double* out_x, double* out_h) {
    fact_walk w;
    memset(&w, 0, sizeof w);
    int64_t nS = 0;
    for (int64_t j = 0; j < d; ++j) nS += n[j] != 0.0;
    int64_t* idx = (int64_t*)malloc((size_t)(nS + 1) * sizeof(int64_t));
    int64_t* loc = (int64_t*)malloc((size_t)d * sizeof(int64_t));
    double* buf = (double*)malloc((size_t)(3 * d + 6 * (nS + 1)) * sizeof(double));
    if (!idx || !loc || !buf) {
        free(idx), free(loc), free(buf);
        return -1;
    }
    w.d = d, w.n_ev = n_ev, w.nS = nS, w.ev = ev, w.idx = idx, w.max_hits = max_hits;
    w.ct = buf, w.cx = buf + d, w.cth = buf + 2 * d;
    w.st = buf + 3 * d, w.sx = w.st + nS, w.sth = w.sx + nS, w.pn = w.sth + nS, w.pp = w.pn + nS, w.wa = w.pp + nS;
    w.out_t = out_t, w.out_x = out_x, w.out_h = out_h;
    int64_t k = 0;
    for (int64_t j = 0; j < d; ++j) {
        w.ct[j] = t0, w.cx[j] = x0[j], w.cth[j] = th0[j];
        loc[j] = -1;
        if (n[j] != 0.0) {
            idx[k] = j, loc[j] = k;
            w.st[k] = t0, w.sx[k] = x0[j], w.sth[k] = th0[j], w.pn[k] = n[j], w.pp[k] = p[j];
            k += 1;
        }
    }
    fact_open(&w, t0);
    for (int64_t e = 0; e < n_ev; ++e) {
        const int64_t l = loc[ev[e].i];
        if (l < 0) continue;
        if (!w.done && w.cand && ev[e].t >= w.s) fact_emit(&w);
        w.st[l] = ev[e].t, w.sx[l] = ev[e].x, w.sth[l] = ev[e].theta;
        fact_open(&w, ev[e].t);
    }
    if (n_ev > 0 && !w.done && w.cand && ev[n_ev - 1].t >= w.s) fact_emit(&w);
    free(idx), free(loc), free(buf);
    return w.nhits;
}

/* f0: [d] bytes or NULL (all free); f: [n x d] bytes (non-zero = free) or NULL */
int64_t ref_condition_pdmp(int64_t d, int64_t n_ev, double t0, const double* x0, const double* th0, const uint8_t* f0, const double* t,
                           const double* x, const double* th, const uint8_t* f, const double* p, const double* n, int64_t max_hits,
                           double* out_t, double* out_x, double* out_h) {
    double* wa = (double*)malloc((size_t)(d > 0 ? d : 1) * sizeof(double));
    if (!wa) return -1;
    int64_t nhits = 0;
    for (int64_t k = 0; k < n_ev; ++k) {
        const double t_c = k ? t[k - 1] : t0;
        const double* x_c = k ? x + (k - 1) * d : x0;
        const double* th_c = k ? th + (k - 1) * d : th0;
        const uint8_t* f_c = k ? (f ? f + (k - 1) * d : NULL) : f0;
        for (int64_t j = 0; j < d; ++j) wa[j] = p[j] - x_c[j];
        const double g = dot_wave64(wa, n, d);
        const double h = dot_wave64(th_c, n, d);
        const double tau = g / h;
        if (!(tau > 0 && t_c + tau < t[k])) continue;
        if (nhits < max_hits) {
            if (out_t) out_t[nhits] = t_c + tau;
            if (out_h) out_h[nhits] = h;
            if (out_x)
                for (int64_t j = 0; j < d; ++j) out_x[nhits * d + j] = (!f_c || f_c[j]) ? x_c[j] + th_c[j] * tau : x_c[j];
        }
        nhits += 1;
    }
    free(wa);
    return nhits;
}

/* ------------------------------------------------------------------------------------------------- src/condition.jl, line by line */

/* :35-53.  out_k: the index of the event each hit was found before (FT.events[k] of :41) */
int64_t ref_condition_fact_literal(int64_t d, int64_t n_ev, double t0, const double* x0, const double* th0, const cond_event* ev,
                                   const double* p, const double* n, int64_t max_rehits, int64_t max_hits, double* out_t, double* out_x,
                                   int64_t* out_k) {
    double* x = (double*)malloc((size_t)(3 * d + 1) * sizeof(double));
    if (!x) return -1;
    double *th = x + d, *pmx = x + 2 * d;
    memcpy(x, x0, (size_t)d * sizeof(double));
    memcpy(th, th0, (size_t)d * sizeof(double));
    double t = t0;
    int64_t k = 0, nhits = 0, here = 0;
    while (k < n_ev) {                                                   /* :39 */
        for (int64_t j = 0; j < d; ++j) pmx[j] = p[j] - x[j];
        const double tau = dot_plain(pmx, n, d) / dot_plain(th, n, d);   /* :40, :19 */
        const double ti = ev[k].t;                                       /* :41 */
        if (tau > 0 && t + tau <= ti && here <= max_rehits) {            /* :42 */
            t += tau;                                                    /* :43, src/dynamics.jl:11-15 */
            for (int64_t j = 0; j < d; ++j) x[j] += th[j] * tau;
            if (nhits < max_hits) {                                      /* :44 */
                if (out_t) out_t[nhits] = t;
                if (out_k) out_k[nhits] = k;
                if (out_x) memcpy(out_x + nhits * d, x, (size_t)d * sizeof(double));
            }
            nhits += 1;
            here += 1;
        } else {
            const double dt = ti - t;                                    /* :46 */
            t += dt;
            for (int64_t j = 0; j < d; ++j) x[j] += th[j] * dt;
            t = ti;                                                      /* :47 */
            x[ev[k].i] = ev[k].x;                                        /* :48 */
            th[ev[k].i] = ev[k].theta;                                   /* :49 */
            k += 1;                                                      /* :50 */
            here = 0;
        }
    }
    free(x);
    return nhits;
}

/* :56-76 with smove_forward! of src/ss_not_fact.jl:78-86 */
int64_t ref_condition_pdmp_literal(int64_t d, int64_t n_ev, double t0, const double* x0, const double* th0, const uint8_t* f0, const double* te,
                                   const double* xe, const double* the, const uint8_t* fe, const double* p, const double* n,
                                   int64_t max_rehits, int64_t max_hits, double* out_t, double* out_x, int64_t* out_k) {
    double* x = (double*)malloc((size_t)(3 * d + 1) * sizeof(double));
    uint8_t* f = (uint8_t*)malloc((size_t)(d > 0 ? d : 1));
    if (!x || !f) {
        free(x), free(f);
        return -1;
    }
    double *th = x + d, *pmx = x + 2 * d;
    memcpy(x, x0, (size_t)d * sizeof(double));
    memcpy(th, th0, (size_t)d * sizeof(double));
    for (int64_t j = 0; j < d; ++j) f[j] = f0 ? f0[j] : 1;
    double t = t0;
    int64_t k = 0, nhits = 0, here = 0;
    while (k < n_ev) {                                                   /* :60 */
        const double tn = te[k];                                         /* :61 */
        for (int64_t j = 0; j < d; ++j) pmx[j] = p[j] - x[j];
        const double tau = dot_plain(pmx, n, d) / dot_plain(th, n, d);   /* :62 */
        if (tau > 0 && t + tau < tn && here <= max_rehits) {             /* :63 */
            t += tau;                                                    /* :64 */
            for (int64_t j = 0; j < d; ++j)
                if (f[j]) x[j] += th[j] * tau;
            if (nhits < max_hits) {                                      /* :65 */
                if (out_t) out_t[nhits] = t;
                if (out_k) out_k[nhits] = k;
                if (out_x) memcpy(out_x + nhits * d, x, (size_t)d * sizeof(double));
            }
            nhits += 1;
            here += 1;
        } else {
            t = tn;                                                      /* :67-69: moved to tn, then replaced by the event */
            memcpy(x, xe + k * d, (size_t)d * sizeof(double));
            memcpy(th, the + k * d, (size_t)d * sizeof(double));
            if (fe) memcpy(f, fe + k * d, (size_t)d);                    /* :70-72 */
            k += 1;                                                      /* :73 */
            here = 0;
        }
    }
    free(x), free(f);
    return nhits;
}
