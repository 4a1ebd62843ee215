/* pdmp_trace_ref.c -- TEST INFRASTRUCTURE ONLY: a sequential restatement of the PDMPTrace consumers of the reference, src/trace.jl:129-150
 * (collect(discretize(Ξ, dt))) and :229-266 (mean, cummean), in the arithmetic the device consumers of csrc/pdmp_consume_bps.hip document, plus the
 * free-time fractions of a sticky trace (trace.py::inclusion_prob).  One chain, the whole trace at once, one event after the other, one coordinate
 * after the other: no cursor survives a call, no slice, no wavefront.  Doubles throughout, no fused multiply-add (built with oracle/Makefile's
 * flags); pdmp_sincos is the one of include/pdmp_detmath.h, which the device compiles too.
 *
 * Per event (t2, x2, θ2[, f2]):
 *   1. while g = t0 + (double)k·dt < t2: row k (if k < K) = x + θ·(g − t) -- Boomerang: (x − μ)·c + θ·s + μ, (s, c) = pdmp_sincos(g − t); a
 *      coordinate whose free bit is clear keeps x --, k += 1.  Rows at and behind K are counted, not stored.
 *   2. y += (x + x2)·(t2 − t); cummean row = y / (2·t2); free_time += free ? t2 − t : 0.
 *   3. x = x2, θ = θ2, free = f2, t = T_last = t2.
 * mean = y / T_last (the reference has no ½ there); inclusion = free_time / (T_last − t0), or the initial mask (all free) where T_last <= t0;
 * npoints = the number of k with t0 + k·dt < T_last, at least 1 -- row 0 is x0 whatever follows.  Rows at and behind npoints stay 0.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pdmp_detmath.h"

/* f: [n x d] bytes (non-zero = free) or NULL; mu: [d] (Boomerang) or NULL (linear flow); grid: [K x d] or NULL; cummean: [n x d] or NULL;
 * incl: [d] or NULL.  Returns npoints (a count that may exceed K), -1 when out of memory. */
int64_t ref_pdmp_trace(int64_t d, int64_t n, double t0, const double* x0, const double* th0, const double* t, const double* x, const double* th,
                       const uint8_t* f, const double* mu, double dt, int64_t K, double* grid, double* mean, double* cummean, double* incl,
                       double* T_last) {
    double* cx = (double*)malloc((size_t)d * sizeof(double));
    double* cth = (double*)malloc((size_t)d * sizeof(double));
    double* cy = (double*)malloc((size_t)d * sizeof(double));
    double* cft = (double*)malloc((size_t)d * sizeof(double));
    uint8_t* cf = (uint8_t*)malloc((size_t)d);
    if (!cx || !cth || !cy || !cft || !cf) {
        free(cx), free(cth), free(cy), free(cft), free(cf);
        return -1;
    }
    for (int64_t i = 0; i < d; ++i) {
        cx[i] = x0[i];
        cth[i] = th0[i];
        cy[i] = 0.0;
        cft[i] = 0.0;
        cf[i] = 1;
    }
    if (grid && K > 0) {
        memset(grid, 0, (size_t)(K * d) * sizeof(double));
        for (int64_t i = 0; i < d; ++i) grid[i] = x0[i];
    }
    double tc = t0, tl = t0;
    int64_t k = 0;
    const int want_grid = dt > 0.0;
    for (int64_t e = 0; e < n; ++e) {
        const double t2 = t[e];
        while (want_grid) {
            const double g = t0 + (double)k * dt;
            if (!(g < t2)) break;
            if (grid && k < K) {
                const double tau = g - tc;
                double s = 0.0, c = 0.0;
                if (mu) pdmp_sincos(tau, &s, &c);
                for (int64_t i = 0; i < d; ++i) {
                    double v = mu ? (cx[i] - mu[i]) * c + cth[i] * s + mu[i] : cx[i] + cth[i] * tau;
                    if (!cf[i]) v = cx[i];
                    grid[k * d + i] = v;
                }
            }
            k += 1;
        }
        const double dtau = t2 - tc;
        for (int64_t i = 0; i < d; ++i) {
            const double x2 = x[e * d + i];
            cy[i] = cy[i] + (cx[i] + x2) * dtau;
            if (cummean) cummean[e * d + i] = cy[i] / (2.0 * t2);
            cft[i] = cft[i] + (cf[i] ? dtau : 0.0);
            cx[i] = x2;
            cth[i] = th[e * d + i];
            if (f) cf[i] = f[e * d + i] != 0;
        }
        tc = tl = t2;
    }
    for (int64_t i = 0; i < d; ++i) {
        if (mean) mean[i] = cy[i] / tl;
        if (incl) incl[i] = (tl > t0) ? cft[i] / (tl - t0) : 1.0;
    }
    if (T_last) *T_last = tl;
    int64_t np = 0;
    if (want_grid)
        while (t0 + (double)np * dt < tl) np += 1;
    free(cx), free(cth), free(cy), free(cft), free(cf);
    return np > 0 ? np : 1;
}
