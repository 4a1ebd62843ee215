/* pairs_ref.c -- the contract of the pair consumers (pdmp_ensemble_[bps_]consume_pairs, DESIGN.md "Pair integrals"), stated once,
 * sequentially: S_k = ∫ (x_i − c_i)(x_j − c_j) dt of the pairs (i, j) = (pi[k], pj[k]) and J_i = ∫ (x_i − c_i) dt of every coordinate of one
 * chain's trace.  The device kernels and trace.pair_integrals follow it bit for bit.  TEST INFRASTRUCTURE ONLY.
 * Plain double arithmetic; compiled with -ffp-contract=off (no fused multiply-add), like the oracle. */
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    double t;
    int64_t i;
    double x, theta;
} ref_event;

/* A piece of the pair (i, j) over [s0, s0 + tau]: a, b the states at s0 minus the centre, vi, vj the velocities.  Symmetric in (i, j) bit
 * for bit: every product commutes, and so does the one sum of two products. */
static double pair_piece(double a, double b, double vi, double vj, double tau) {
    return tau * (a * b + tau * (0.5 * (a * vj + b * vi) + tau * ((vi * vj) / 3.0)));
}

/* a coordinate's own piece */
static double line_piece(double a, double vi, double tau) { return tau * (a + 0.5 * (vi * tau)); }

/* the piece of a pair from its two cursors (t, x, θ) to the time t1; tau is taken signed */
static double pair_close(double ti, double xi, double thi, double ci, double tj, double xj, double thj, double cj, double t1) {
    const double s0 = ti > tj ? ti : tj;
    const double a = (xi - ci) + thi * (s0 - ti);
    const double b = (xj - cj) + thj * (s0 - tj);
    return pair_piece(a, b, thi, thj, t1 - s0);
}

/* FactTrace: events in trace order.  A cursor (t, x, θ, J) per coordinate from (t0, x0, θ0, 0).  An event (t, i, x, θ): every listed pair
 * with i in it, in the order of the list, gets the piece [max(t_i, t_j), t]; then J_i gets [t_i, t] and i's cursor becomes (t, x, θ).  At the
 * end every pair is closed from max(t_i, t_j) and every J_i from t_i to T_last, the last event's time (t0 without an event).
 * center may be NULL (= 0).  Returns 0, or -1 without memory. */
int64_t ref_pairs_fact(int64_t d, int64_t nev, double t0, const double* x0, const double* th0, const ref_event* ev, int64_t npairs, const int64_t* pi,
                       const int64_t* pj, const double* center, double* S, double* J, double* T_last) {
    double* ct = (double*)malloc((size_t)(4 * d + 1) * sizeof(double));
    if (!ct) return -1;
    double *cx = ct + d, *cth = cx + d, *c = cth + d;
    for (int64_t j = 0; j < d; ++j) {
        ct[j] = t0;
        cx[j] = x0[j];
        cth[j] = th0[j];
        c[j] = center ? center[j] : 0.0;
        J[j] = 0.0;
    }
    for (int64_t k = 0; k < npairs; ++k) S[k] = 0.0;
    double T = t0;
    for (int64_t e = 0; e < nev; ++e) {
        const int64_t i = ev[e].i;
        const double t = ev[e].t;
        T = t;
        if (i < 0 || i >= d) continue;
        for (int64_t k = 0; k < npairs; ++k) { /* (i's OLD cursor, also for the pair (i, i)) */
            if (pi[k] != i && pj[k] != i) continue;
            const int64_t a = pi[k], b = pj[k];
            S[k] = S[k] + pair_close(ct[a], cx[a], cth[a], c[a], ct[b], cx[b], cth[b], c[b], t);
        }
        J[i] = J[i] + line_piece(cx[i] - c[i], cth[i], t - ct[i]);
        ct[i] = t;
        cx[i] = ev[e].x;
        cth[i] = ev[e].theta;
    }
    for (int64_t k = 0; k < npairs; ++k) {
        const int64_t a = pi[k], b = pj[k];
        S[k] = S[k] + pair_close(ct[a], cx[a], cth[a], c[a], ct[b], cx[b], cth[b], c[b], T);
    }
    for (int64_t j = 0; j < d; ++j) J[j] = J[j] + line_piece(cx[j] - c[j], cth[j], T - ct[j]);
    *T_last = T;
    free(ct);
    return 0;
}

/* PDMPTrace: events (t [nev], x and th [nev x d], f [nev x d] bytes or NULL = all free; f0 [d] or NULL = all free).  Per event k, with the
 * cursor (t_c, x_c, θ_c, f_c) before it, every pair gets the piece [t_c, t_k] with a = x_c,i − c_i and vi = f_c,i ? θ_c,i : 0 (a coordinate
 * that is not free keeps x), every coordinate its own piece.  Nothing behind the last event: the integrals are over [t0, T_last] exactly. */
int64_t ref_pairs_pdmp(int64_t d, int64_t nev, double t0, const double* x0, const double* th0, const uint8_t* f0, const double* t, const double* x,
                       const double* th, const uint8_t* f, int64_t npairs, const int64_t* pi, const int64_t* pj, const double* center, double* S,
                       double* J, double* T_last) {
    for (int64_t j = 0; j < d; ++j) J[j] = 0.0;
    for (int64_t k = 0; k < npairs; ++k) S[k] = 0.0;
    double tc = t0;
    const double *xc = x0, *thc = th0;
    const uint8_t* fc = f0;
    for (int64_t e = 0; e < nev; ++e) {
        const double tau = t[e] - tc;
        for (int64_t k = 0; k < npairs; ++k) {
            const int64_t a = pi[k], b = pj[k];
            const double va = (!fc || fc[a]) ? thc[a] : 0.0, vb = (!fc || fc[b]) ? thc[b] : 0.0;
            const double ca = center ? center[a] : 0.0, cb = center ? center[b] : 0.0;
            S[k] = S[k] + pair_piece(xc[a] - ca, xc[b] - cb, va, vb, tau);
        }
        for (int64_t j = 0; j < d; ++j) {
            const double v = (!fc || fc[j]) ? thc[j] : 0.0;
            J[j] = J[j] + line_piece(xc[j] - (center ? center[j] : 0.0), v, tau);
        }
        tc = t[e];
        xc = x + e * d;
        thc = th + e * d;
        fc = f ? f + e * d : NULL;
    }
    *T_last = tc;
    return 0;
}
