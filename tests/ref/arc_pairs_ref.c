/* arc_pairs_ref.c -- the contract of the arc pair consumer (pdmp_ensemble_bps_consume_arc_pairs, DESIGN.md "Pair integrals of arcs"), stated
 * once, sequentially: S_k = ∫ (x_i − z_i)(x_j − z_j) dt of the pairs (i, j) = (pi[k], pj[k]) and J_i = ∫ (x_i − z_i) dt of every coordinate of
 * one chain's PDMPTrace of a Boomerang (sticky or not), over [t0, T_last].  The device kernel and trace.arc_pair_integrals follow it bit for
 * bit.  TEST INFRASTRUCTURE ONLY.  Plain double arithmetic; compiled with -ffp-contract=off (no fused multiply-add), like the oracle;
 * pdmp_sincos is the one of include/pdmp_detmath.h, which the device compiles too. */
#include <stdint.h>
#include <stdlib.h>

#include "../../include/pdmp_detmath.h"

/* the five basis integrals of a piece of signed length tau: ∫cos², ∫sin², ∫sin·cos, ∫cos, ∫sin over [0, tau].  Is = 1 − cos τ is taken as
 * sin²/(1 + cos) where cos > 0: 1 − c cancels for small τ (at τ = 1e-9 it is 0 where the integral is 5e-19). */
typedef struct {
    double Icc, Iss, Isc, Ic, Is;
} arc_basis;

static arc_basis arc_basis_of(double tau, int exchanged) {
    double s, c;
    pdmp_sincos(tau, &s, &c);
    const double h = s * c;
    arc_basis b;
    b.Icc = 0.5 * (tau + h);
    b.Iss = 0.5 * (tau - h);
    b.Isc = 0.5 * (s * s);
    b.Ic = s;
    b.Is = c > 0 ? (s * s) / (1.0 + c) : 1.0 - c;
    if (exchanged) { /* NOT the contract: the wrong statement the tests hold the error bound against (a bound both forms pass proves nothing) */
        const double t = b.Icc;
        b.Icc = b.Iss;
        b.Iss = t;
    }
    return b;
}

/* x(s) − z = u·cos s + p·sin s + m on the piece.  Symmetric in (i, j) bit for bit: every product commutes, and each sum of two products is
 * one commutative addition.  Two frozen coordinates (u = p = 0): (mi·mj)·τ. */
static double arc_pair_piece(double ui, double pi, double mi, double uj, double pj, double mj, double tau, const arc_basis* b) {
    return (((ui * uj) * b->Icc + (pi * pj) * b->Iss) + (ui * pj + uj * pi) * b->Isc) +
           ((mi * (uj * b->Ic + pj * b->Is) + mj * (ui * b->Ic + pi * b->Is)) + (mi * mj) * tau);
}

static double arc_line_piece(double u, double p, double m, double tau, const arc_basis* b) { return (u * b->Ic + p * b->Is) + m * tau; }

/* events (t [nev], x and th [nev x d], f [nev x d] bytes or NULL = all free; f0 [d] or NULL = all free), mu [d] the Boomerang's centre, center
 * [d] or NULL (= 0) the z of the integrand.  Per event k, with the cursor (t_c, x_c, θ_c, f_c) before it, τ = t_k − t_c signed: a free coordinate
 * has u = x_c − μ, p = θ_c, m = μ − z; one that is not free (smove_forward! leaves it alone) u = 0, p = 0, m = x_c − z.  Nothing behind the last
 * event: the integrals are over [t0, T_last] exactly.  exchanged: 0 (the contract). */
int64_t ref_arc_pairs(int64_t d, int64_t nev, double t0, const double* x0, const double* th0, const uint8_t* f0, const double* t, const double* x,
                      const double* th, const uint8_t* f, const double* mu, int64_t npairs, const int64_t* pi, const int64_t* pj, const double* center,
                      int exchanged, double* S, double* J, double* T_last) {
    double* u = (double*)malloc((size_t)(3 * d + 1) * sizeof(double));
    if (!u) return -1;
    double *p = u + d, *m = p + d;
    for (int64_t j = 0; j < d; ++j) J[j] = 0.0;
    for (int64_t k = 0; k < npairs; ++k) S[k] = 0.0;
    double tc = t0;
    const double *xc = x0, *thc = th0;
    const uint8_t* fc = f0;
    for (int64_t e = 0; e < nev; ++e) {
        const double tau = t[e] - tc;
        const arc_basis b = arc_basis_of(tau, exchanged);
        for (int64_t j = 0; j < d; ++j) {
            const double z = center ? center[j] : 0.0;
            if (!fc || fc[j]) {
                u[j] = xc[j] - mu[j];
                p[j] = thc[j];
                m[j] = mu[j] - z;
            } else {
                u[j] = 0.0;
                p[j] = 0.0;
                m[j] = xc[j] - z;
            }
        }
        for (int64_t k = 0; k < npairs; ++k) {
            const int64_t a = pi[k], c = pj[k];
            S[k] = S[k] + arc_pair_piece(u[a], p[a], m[a], u[c], p[c], m[c], tau, &b);
        }
        for (int64_t j = 0; j < d; ++j) J[j] = J[j] + arc_line_piece(u[j], p[j], m[j], tau, &b);
        tc = t[e];
        xc = x + e * d;
        thc = th + e * d;
        fc = f ? f + e * d : NULL;
    }
    *T_last = tc;
    free(u);
    return 0;
}
