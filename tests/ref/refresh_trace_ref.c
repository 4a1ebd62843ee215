/* refresh_trace_ref.c -- TEST INFRASTRUCTURE ONLY: a sequential statement of the FactTrace consumers on a trace that is sorted within a coordinate
 * only -- a ZigZag with a refresh clock (λref > 0) or a FactBoomerang, whose refreshed coordinate is recorded at its own, stale clock
 * (src/sfact.jl:84-85,143) -- in the arithmetic the unordered walk of csrc/pdmp_consume.hip documents.  One chain, the whole
 * trace at once, one event after the other: no slice, no chunk, no wavefront.  Doubles throughout, no fused multiply-add (built with
 * oracle/Makefile's flags); pdmp_sincos is the one of include/pdmp_detmath.h, which the device compiles too.
 *
 * ref_refresh_trace -- the CLOSED FORM.  Cursor per coordinate (t, x, θ, y) from (t0, x0, θ0, 0); k = the first grid row not written yet.
 * Per event (t2, i, x2, θ2), in trace order:
 *   1. while g = t0 + (double)k·dt < t2 (this event is the first whose time exceeds g): row k (if k < K), for every coordinate j from ITS cursor,
 *      = x + θ·τ, τ = g − t_j -- FactBoomerang: (x − μ_j)·c + θ·s + μ_j, (s, c) = pdmp_sincos(τ) --, k += 1.
 *      A stale event (t2 <= g for the next unwritten row) opens no row: it is applied, and the next row shows it (src/trace.jl:111-121 takes the
 *      events in trace order and emits g as soon as the NEXT event is later than g).
 *   2. y_i += (x_i + x2)·(t2 − t_i); the cummean pair of this event = (t2, y_i / (2·t2)).
 *   3. (t_i, x_i, θ_i) = (t2, x2, θ2); T_last = t2; t_max = max(t_max, t2).
 * mean_j = y_j · (1 / (2·T_last)) -- T_last is the time of the LAST event in trace order (src/trace.jl:186), not the maximum; npoints = the number
 * of k with t0 + k·dt < t_max, at least 1 (a grid time is emitted while it lies before some event).  Row 0 is x0; the first event beyond t0
 * writes it again from the cursors.  Rows at and behind npoints stay 0.
 *
 * ref_refresh_steps -- the reference's own iterator, Base.iterate(::Discretize{<:FactTrace}) (src/trace.jl:106-125), restated step by step for
 * both flows: ALL coordinates are moved by every step -- move_forward! of src/dynamics.jl:11-15 (linear) or :29-36 (the rotation about μ, with
 * libm's sin / cos) --, backward steps (Δt < 0 at a stale event) included.  It is what the closed form is compared against.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pdmp_detmath.h"

/* mu: [d] (FactBoomerang) or NULL (linear flow); grid: [K x d] or NULL; cm_t, cm_y: [n] or NULL.  Returns npoints (a count that may exceed K),
 * -1 when out of memory. */
int64_t ref_refresh_trace(int64_t d, int64_t n, double t0, const double* x0, const double* th0, const double* et, const int64_t* ei, const double* ex,
                          const double* eth, const double* mu, double dt, int64_t K, double* grid, double* mean, double* cm_t, double* cm_y,
                          double* T_last, double* t_max) {
    double* ct = (double*)malloc((size_t)d * sizeof(double));
    double* cx = (double*)malloc((size_t)d * sizeof(double));
    double* cth = (double*)malloc((size_t)d * sizeof(double));
    double* cy = (double*)malloc((size_t)d * sizeof(double));
    if (!ct || !cx || !cth || !cy) {
        free(ct), free(cx), free(cth), free(cy);
        return -1;
    }
    for (int64_t j = 0; j < d; ++j) {
        ct[j] = t0;
        cx[j] = x0[j];
        cth[j] = th0[j];
        cy[j] = 0.0;
    }
    if (grid && K > 0) {
        memset(grid, 0, (size_t)(K * d) * sizeof(double));
        for (int64_t j = 0; j < d; ++j) grid[j] = x0[j];
    }
    double tl = t0, tm = t0;
    int64_t k = 0;
    const int want_grid = dt > 0.0;
    for (int64_t e = 0; e < n; ++e) {
        const double t2 = et[e];
        while (want_grid) {
            const double g = t0 + (double)k * dt;
            if (!(t2 > g)) break;
            if (grid && k < K)
                for (int64_t j = 0; j < d; ++j) {
                    const double tau = g - ct[j];
                    if (mu) {
                        double s, c;
                        pdmp_sincos(tau, &s, &c);
                        grid[k * d + j] = (cx[j] - mu[j]) * c + cth[j] * s + mu[j];
                    } else {
                        grid[k * d + j] = cx[j] + cth[j] * tau;
                    }
                }
            k += 1;
        }
        const int64_t i = ei[e];
        cy[i] = cy[i] + (cx[i] + ex[e]) * (t2 - ct[i]);
        ct[i] = t2;
        cx[i] = ex[e];
        cth[i] = eth[e];
        if (cm_t) cm_t[e] = t2;
        if (cm_y) cm_y[e] = cy[i] / (2.0 * t2);
        tl = t2;
        if (t2 > tm) tm = t2;
    }
    if (mean)
        for (int64_t j = 0; j < d; ++j) mean[j] = cy[j] * (1 / (2 * tl));
    if (T_last) *T_last = tl;
    if (t_max) *t_max = tm;
    int64_t np = 0;
    if (want_grid)
        while (t0 + (double)np * dt < tm) np += 1;
    free(ct), free(cx), free(cth), free(cy);
    return np > 0 ? np : 1;
}

/* The reference's iterator, step by step.  ts: [cap], xs: [cap x d], steps: [cap x d] or NULL -- steps[q·d + j] = the number of move_forward!
 * calls coordinate j's value of row q has been through since its own last event (or since t0).  Returns the number of rows the iterator emits
 * (a count that may exceed cap), -1 when out of memory. */
int64_t ref_refresh_steps(int64_t d, double t0, const double* x0, const double* th0, int64_t n, const double* et, const int64_t* ei, const double* ex,
                          const double* eth, const double* mu, double dt_grid, int64_t cap, double* ts, double* xs, int64_t* steps) {
    double* x = (double*)malloc((size_t)d * sizeof(double));
    double* th = (double*)malloc((size_t)d * sizeof(double));
    int64_t* st = (int64_t*)calloc((size_t)d, sizeof(int64_t));
    if (!x || !th || !st) {
        free(x), free(th), free(st);
        return -1;
    }
    memcpy(x, x0, (size_t)d * sizeof(double));
    memcpy(th, th0, (size_t)d * sizeof(double));
    double t = t0;
    int64_t k = 0, q = 0;
#define REF_EMIT()                                                                   \
    do {                                                                             \
        if (q < cap) {                                                               \
            ts[q] = t;                                                               \
            memcpy(xs + q * d, x, (size_t)d * sizeof(double));                       \
            if (steps) memcpy(steps + q * d, st, (size_t)d * sizeof(int64_t));       \
        }                                                                            \
        q += 1;                                                                      \
    } while (0)
#define REF_MOVE(tau)                                                                \
    do {                                                                             \
        const double tau_ = (tau);                                                   \
        const double s_ = sin(tau_), c_ = cos(tau_);                                 \
        for (int64_t j = 0; j < d; ++j) {                                            \
            if (mu) {                                                                \
                const double xn = (x[j] - mu[j]) * c_ + th[j] * s_ + mu[j];          \
                const double tn = -(x[j] - mu[j]) * s_ + th[j] * c_;                 \
                x[j] = xn;                                                           \
                th[j] = tn;                                                          \
            } else {                                                                 \
                x[j] = x[j] + th[j] * tau_;                                          \
            }                                                                        \
            st[j] += 1;                                                              \
        }                                                                            \
        t = t + tau_;                                                                \
    } while (0)
    REF_EMIT(); /* t0 => x0 */
    for (;;) {
        double dt = dt_grid;
        int produced = 0;
        for (;;) {
            if (k >= n) break; /* no event left: the iterator ends */
            const double ti = et[k];
            if (t + dt < ti) {
                REF_MOVE(dt);
                produced = 1;
                break;
            }
            const double del = ti - t; /* not further than the event; negative at a stale one */
            dt = dt - del;
            REF_MOVE(del);
            t = ti;
            x[ei[k]] = ex[k];
            th[ei[k]] = eth[k];
            st[ei[k]] = 0;
            k = k + 1;
        }
        if (!produced) break;
        REF_EMIT();
    }
#undef REF_EMIT
#undef REF_MOVE
    free(x), free(th), free(st);
    return q;
}
