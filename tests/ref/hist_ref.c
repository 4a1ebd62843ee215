/* hist_ref.c -- the contract of the histogram consumers (pdmp_ensemble_[bps_]consume_hist, DESIGN.md "Marginal histograms"), stated once,
 * sequentially: the time every listed coordinate of one chain's trace spends in each of B bins of its own range, below the range and at or
 * above it (occupation times: the exact histogram of a piecewise-linear path).  The device kernels follow it bit for bit, trace.marginal_histogram
 * to rounding.  TEST INFRASTRUCTURE ONLY.
 * Plain double arithmetic; compiled with -ffp-contract=off (no fused multiply-add), like the oracle. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    double t;
    int64_t i;
    double x, theta;
} ref_event;

/* the bins of one coordinate: B bins on [lo, hi), w = (hi − lo) / B */
typedef struct {
    double lo, hi, w;
    int64_t B;
} ref_bins;

static ref_bins bins_of(double lo, double hi, int64_t B) {
    ref_bins b;
    b.lo = lo;
    b.hi = hi;
    b.w = (hi - lo) / (double)B;
    b.B = B;
    return b;
}

/* e_k for k in −1 .. B + 1: e_−1 = −∞, e_0 = lo, e_k = lo + w·k, e_B = hi, e_B+1 = +∞ */
static double edge(const ref_bins* b, int64_t k) {
    if (k <= 0) return k < 0 ? -INFINITY : b->lo;
    if (k >= b->B) return k > b->B ? INFINITY : b->hi;
    return b->lo + b->w * (double)k;
}

/* the k in {−1, ..., B} with e_k <= x < e_k+1 against the computed edges: a floor, then one step where rounding put it on the wrong side.
 * −0.0 counts as 0 (every test is a comparison); a NaN goes below the range. */
static int64_t bin_of(const ref_bins* b, double x) {
    if (!(x >= b->lo)) return -1;
    if (x >= b->hi) return b->B;
    const double q = floor((x - b->lo) / b->w);
    int64_t k = q < (double)(b->B - 1) ? (int64_t)q : b->B - 1;
    if (x < edge(b, k)) k -= 1;
    else if (x >= edge(b, k + 1)) k += 1;
    return k;
}

/* A piece (a, v, tau) made ready: the ends of the interval it sweeps, the time per unit length r and the bins k0 .. k1 it touches.  A piece
 * at rest (v == 0, or b == a after rounding) has xl == xh, r = tau and one bin; tau <= 0 (or NaN) has no bin: k0 > k1. */
typedef struct {
    double xl, xh, r;
    int64_t k0, k1;
} ref_piece;

static ref_piece piece_of(const ref_bins* bn, double a, double v, double tau) {
    ref_piece p;
    p.xl = p.xh = a;
    p.r = tau;
    p.k0 = 0;
    p.k1 = -1;
    if (!(tau > 0.0)) return p;
    const double b = a + v * tau;
    if (v == 0.0 || b == a) {
        p.k0 = p.k1 = bin_of(bn, a);
        return p;
    }
    p.xl = a < b ? a : b;
    p.xh = a < b ? b : a;
    p.r = tau / (p.xh - p.xl);
    p.k0 = bin_of(bn, p.xl);
    p.k1 = bin_of(bn, p.xh);
    return p;
}

/* THE function of (piece, k): the time the piece spends in [e_k, e_k+1), k in −1 .. B.  The accumulation and the read both call it. */
static double piece_at(const ref_bins* bn, const ref_piece* p, int64_t k) {
    if (k < p->k0 || k > p->k1) return 0.0;
    if (p->xl == p->xh) return p->r;
    const double e0 = edge(bn, k), e1 = edge(bn, k + 1);
    const double o = (p->xh < e1 ? p->xh : e1) - (p->xl > e0 ? p->xl : e0);
    return o > 0.0 ? o * p->r : 0.0;
}

/* the rest time a piece adds to Z */
static double piece_rest(double v, double tau) { return (tau > 0.0 && v == 0.0) ? tau : 0.0; }

static void add_piece(const ref_bins* bn, double a, double v, double tau, double* H, double* Z) {
    const ref_piece p = piece_of(bn, a, v, tau);
    for (int64_t k = p.k0; k <= p.k1; ++k) H[k + 1] = H[k + 1] + piece_at(bn, &p, k);
    *Z = *Z + piece_rest(v, tau);
}

/* what the tests probe directly */
int64_t ref_hist_bin_of(double lo, double hi, int64_t B, double x) {
    const ref_bins b = bins_of(lo, hi, B);
    return bin_of(&b, x);
}
double ref_hist_edge(double lo, double hi, int64_t B, int64_t k) {
    const ref_bins b = bins_of(lo, hi, B);
    return edge(&b, k);
}
/* one piece into a row H [B + 2] and Z (both added to) */
void ref_hist_piece(double lo, double hi, int64_t B, double a, double v, double tau, double* H, double* Z) {
    const ref_bins b = bins_of(lo, hi, B);
    add_piece(&b, a, v, tau, H, Z);
}

/* FactTrace: events in trace order.  A cursor (t, x, θ) per listed coordinate from (t0, x0, θ0).  An event (t, i, x, θ) of a listed
 * coordinate adds the piece (x_c, θ_c, t − t_c), then the cursor becomes the event; other events only move T_last.  At the end every listed
 * coordinate's open piece is closed to T_last, the last event's time (t0 without an event).  H [m x (B + 2)], Z [m].
 * Returns the number of pieces with tau > 0 it added, or -1 without memory. */
int64_t ref_hist_fact(int64_t d, int64_t nev, double t0, const double* x0, const double* th0, const ref_event* ev, int64_t m, const int64_t* coords,
                      const double* lo, const double* hi, int64_t B, double* H, double* Z, double* T_last) {
    int64_t* slot = (int64_t*)malloc((size_t)d * sizeof(int64_t));
    double* ct = (double*)malloc((size_t)(3 * m) * sizeof(double));
    ref_bins* bn = (ref_bins*)malloc((size_t)m * sizeof(ref_bins));
    if (!slot || !ct || !bn) {
        free(slot), free(ct), free(bn);
        return -1;
    }
    double *cx = ct + m, *cth = cx + m;
    int64_t npieces = 0;
    for (int64_t j = 0; j < d; ++j) slot[j] = -1;
    for (int64_t s = 0; s < m; ++s) {
        slot[coords[s]] = s;
        ct[s] = t0;
        cx[s] = x0[coords[s]];
        cth[s] = th0[coords[s]];
        bn[s] = bins_of(lo[s], hi[s], B);
        Z[s] = 0.0;
        for (int64_t k = 0; k < B + 2; ++k) H[s * (B + 2) + k] = 0.0;
    }
    double T = t0;
    for (int64_t e = 0; e < nev; ++e) {
        const int64_t i = ev[e].i;
        T = ev[e].t;
        if (i < 0 || i >= d || slot[i] < 0) continue;
        const int64_t s = slot[i];
        add_piece(&bn[s], cx[s], cth[s], T - ct[s], H + s * (B + 2), Z + s);
        npieces += (T - ct[s] > 0.0);
        ct[s] = T;
        cx[s] = ev[e].x;
        cth[s] = ev[e].theta;
    }
    for (int64_t s = 0; s < m; ++s) {
        add_piece(&bn[s], cx[s], cth[s], T - ct[s], H + s * (B + 2), Z + s);
        npieces += (T - ct[s] > 0.0);
    }
    *T_last = T;
    free(slot), free(ct), free(bn);
    return npieces;
}

/* PDMPTrace: events (t [nev], x and th [nev x d], f [nev x d] bytes or NULL = all free; f0 [d] or NULL = all free).  Per event k, with the
 * cursor (t_c, x_c, θ_c, f_c) before it, every listed coordinate adds the piece (x_c,i, f_c,i ? θ_c,i : 0, t_k − t_c).  Nothing behind the
 * last event.  Returns the number of pieces with tau > 0. */
int64_t ref_hist_pdmp(int64_t d, int64_t nev, double t0, const double* x0, const double* th0, const uint8_t* f0, const double* t, const double* x,
                      const double* th, const uint8_t* f, int64_t m, const int64_t* coords, const double* lo, const double* hi, int64_t B, double* H,
                      double* Z, double* T_last) {
    int64_t npieces = 0;
    for (int64_t s = 0; s < m; ++s) {
        Z[s] = 0.0;
        for (int64_t k = 0; k < B + 2; ++k) H[s * (B + 2) + k] = 0.0;
    }
    double tc = t0;
    const double *xc = x0, *thc = th0;
    const uint8_t* fc = f0;
    for (int64_t e = 0; e < nev; ++e) {
        const double tau = t[e] - tc;
        for (int64_t s = 0; s < m; ++s) {
            const int64_t i = coords[s];
            const ref_bins bn = bins_of(lo[s], hi[s], B);
            const double v = (!fc || fc[i]) ? thc[i] : 0.0;
            add_piece(&bn, xc[i], v, tau, H + s * (B + 2), Z + s);
            npieces += (tau > 0.0);
        }
        tc = t[e];
        xc = x + e * d;
        thc = th + e * d;
        fc = f ? f + e * d : NULL;
    }
    *T_last = tc;
    return npieces;
}

/* the pooled read: the chains' rows summed in chain order, sequentially per entry, from 0.0.  rows [n x len] -> out [len] */
void ref_hist_pool(int64_t n, int64_t len, const double* rows, double* out) {
    for (int64_t k = 0; k < len; ++k) {
        double acc = 0.0;
        for (int64_t q = 0; q < n; ++q) acc = acc + rows[q * len + k];
        out[k] = acc;
    }
}
