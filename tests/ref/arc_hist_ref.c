/* arc_hist_ref.c -- the contract of the arc histogram consumer (pdmp_ensemble_bps_consume_arc_hist, DESIGN.md "Marginal histograms of arcs"),
 * stated once, sequentially: the time every listed coordinate of one chain's PDMPTrace of a Boomerang (sticky or not) spends in each of B bins of
 * its own range, below the range and at or above it -- the exact histogram of a path of arcs.  The device kernel follows it bit for bit,
 * trace.arc_marginal_histogram to rounding.  TEST INFRASTRUCTURE ONLY.  Plain double arithmetic; compiled with -ffp-contract=off (no fused
 * multiply-add), like the oracle; pdmp_acos / pdmp_atan2 are those of include/pdmp_detmath.h, which the device compiles too.
 * The bins, the edges, bin_of, the row layout (B + 2 slots) and the pooled read are those of hist_ref.c, included here so that they are stated
 * once. */
#include "hist_ref.c"

#include "../../include/pdmp_detmath.h"

#define ARC_TWO_PI 6.28318530717958623200e+00 /* 2π as ONE double constant */

/* A piece made ready.  From the cursor (x_c, θ_c, free) and τ: a coordinate that is not free, or one with R == 0, is AT REST (rest = 1, krest its
 * slot); every other one an arc  x(s) = μ + R·cos(ψ0 + s),  ψ0 = −atan2(p, u),  u = x_c − μ,  p = θ_c,  R = sqrt(u·u + p·p).  n and r split
 * ψ0 and ψ1 = ψ0 + τ into whole turns and a remainder once per piece.  τ <= 0 (or NaN) adds nothing: live = 0. */
typedef struct {
    double tau, mu, R, n0, r0, n1, r1;
    int live, rest;
    int64_t krest;
} arc_piece;

static arc_piece arc_piece_of(const ref_bins* bn, double xc, double thc, int is_free, double mu, double tau, int wrong) {
    arc_piece a;
    a.tau = tau;
    a.mu = mu;
    a.R = a.n0 = a.r0 = a.n1 = a.r1 = 0.0;
    a.live = tau > 0.0;
    a.rest = 1;
    a.krest = 0;
    if (!a.live) return a;
    const double u = xc - mu, p = thc;
    a.R = is_free ? PDMP_SQRT(u * u + p * p) : 0.0;
    if (a.R == 0.0) {
        a.krest = bin_of(bn, xc);
        return a;
    }
    a.rest = 0;
    /* wrong: NOT the contract -- ψ0 with the opposite sign, the wrong statement the tests hold the error bound against */
    const double psi0 = wrong ? pdmp_atan2(p, u) : -pdmp_atan2(p, u);
    const double psi1 = psi0 + tau;
    a.n0 = floor(psi0 / ARC_TWO_PI);
    a.r0 = psi0 - ARC_TWO_PI * a.n0;
    a.n1 = floor(psi1 / ARC_TWO_PI);
    a.r1 = psi1 - ARC_TWO_PI * a.n1;
    return a;
}

/* W(ψ) = n·L + clamp(r − α, 0, L): the time x < y up to the angle ψ = 2π·n + r, where x < y on (α, 2π − α) of every turn */
static double arc_w(double n, double r, double alpha, double L) {
    const double v = r - alpha;
    return n * L + (v < 0.0 ? 0.0 : (v > L ? L : v));
}

/* the time the arc spends below the level y */
static double arc_below(const arc_piece* a, double y) {
    const double z = (y - a->mu) / a->R;
    if (z >= 1.0) return a->tau;
    if (z <= -1.0) return 0.0;
    const double alpha = pdmp_acos(z);
    const double L = ARC_TWO_PI - 2.0 * alpha;
    return arc_w(a->n1, a->r1, alpha, L) - arc_w(a->n0, a->r0, alpha, L);
}

/* THE function of (piece, k): the time the piece spends in [e_k, e_k+1), k in −1 .. B.  Zero outside the bins of μ − R .. μ + R (both levels
 * saturate on the same side), so a walk may skip those bins. */
static double arc_piece_at(const ref_bins* bn, const arc_piece* a, int64_t k) {
    if (!a->live) return 0.0;
    if (a->rest) return k == a->krest ? a->tau : 0.0;
    const double o = arc_below(a, edge(bn, k + 1)) - arc_below(a, edge(bn, k));
    return o > 0.0 ? o : 0.0;
}

static void arc_add_piece(const ref_bins* bn, const arc_piece* a, double* H, double* Z) {
    for (int64_t k = -1; k <= bn->B; ++k) H[k + 1] = H[k + 1] + arc_piece_at(bn, a, k);
    *Z = *Z + ((a->live && a->rest) ? a->tau : 0.0);
}

/* what the tests probe directly */
double ref_arc_acos(double z) { return pdmp_acos(z); }
double ref_arc_atan2(double y, double x) { return pdmp_atan2(y, x); }
/* one piece into a row H [B + 2] and Z (both added to) */
void ref_arc_hist_piece(double lo, double hi, int64_t B, double xc, double thc, int is_free, double mu, double tau, int wrong, double* H, double* Z) {
    const ref_bins b = bins_of(lo, hi, B);
    const arc_piece a = arc_piece_of(&b, xc, thc, is_free, mu, tau, wrong);
    arc_add_piece(&b, &a, H, Z);
}

/* events (t [nev], x and th [nev x d], f [nev x d] bytes or NULL = all free; f0 [d] or NULL = all free), mu [d] the Boomerang's centre.  Per event
 * k, with the cursor (t_c, x_c, θ_c, f_c) before it, τ = t_k − t_c, every listed coordinate adds its piece.  Nothing behind the last event.
 * wrong: 0 (the contract).  Returns the number of pieces with tau > 0. */
int64_t ref_arc_hist(int64_t d, int64_t nev, double t0, const double* x0, const double* th0, const uint8_t* f0, const double* t, const double* x,
                     const double* th, const uint8_t* f, const double* mu, int64_t m, const int64_t* coords, const double* lo, const double* hi,
                     int64_t B, int wrong, double* H, double* Z, double* T_last) {
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
            const arc_piece a = arc_piece_of(&bn, xc[i], thc[i], !fc || fc[i], mu[i], tau, wrong);
            arc_add_piece(&bn, &a, H + s * (B + 2), Z + s);
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
