"""The occupation times of a Boomerang's PDMPTrace per bin with mpmath at 60 digits, and the error bound of the float64 statement of the contract
(tests/ref/arc_hist_ref.c), in the manner of tests/exact_arc_pairs.py.  TEST INFRASTRUCTURE ONLY.

The path is the one the trace's floats describe: every recorded number (t, x, θ, μ) and every computed edge e_k (a double: the bins are DEFINED
by the computed edges) is taken as the exact number it is.  On the piece of an event a free coordinate is x(s) = μ + R̂·cos(s − φ̂) with
û = x_c − μ, p̂ = θ_c, R̂ = sqrt(û² + p̂²), φ̂ = atan2(p̂, û), over s in [0, τ̂], τ̂ = t_k − t_c; it is below a level y on the intervals
(φ̂ + α̂ + 2πk, φ̂ + 2π − α̂ + 2πk), α̂ = acos((y − μ)/R̂).  THE EXACT OCCUPATION is evaluated as just that: the summed lengths of the
intersections of those intervals with [0, τ̂] -- no floor, no clamp, none of the statement's algebra.  At 60 digits its own error is below
1e-55.

THE BOUND is a running error analysis over the statement's operations, from the inputs alone; u = 2^-53.  A correctly rounded operation whose
operands carry the absolute errors e adds, to the propagated error P, the rounding u·(|exact result| + P) -- and NOTHING where P = 0 and the
exact result is a double (then the computed result IS the exact one).  That clause is what keeps the table's exact tangencies (μ = 0, û = 1,
p̂ = 0, edges ±1) exact; it is a property of the inputs, not of the code.

  1. τ = fl(t_k − t_c), û = fl(x_c − μ), d = fl(y − μ): one rounding each on the difference.  R = sqrt(fl(fl(û·û) + fl(p̂·p̂))): the products,
     the sum and the root one rounding each, the root's propagated error sqrt(s) − sqrt(s − e_s).
  2. ψ0 = −pdmp_atan2(p̂, û): the error the header states (x > 0: 3.5u|φ̂|, + 2^-1074 where 0 < |p̂/û| < 2^-1022; x < 0: 10u; x = 0: u), and the
     conditioning in û, at most e_û/(R̂ − e_û).  ψ1 = fl(ψ0 + τ).
  3. The turns.  c = 2π as the one double, δc = |c − 2π|.  n = floor(fl(ψ/c)), r = fl(ψ − fl(c·n)): r approximates ψ̂ − 2π·n with
     e_r = e_ψ + |n|·δc + u|c·n| + one rounding.  W(n, r) = n·L + clamp(r − α, 0, L) is the time below up to the angle 2πn + r whenever r lies
     in [0, 2π], and a computed n that differs from floor(ψ̂/2π) puts r outside that interval by no more than e_r + u·2π (W is continuous with
     slope at most 1): the split costs e_r + u·2π once more.  |n| <= |floor(ψ̂/2π)| + 1.
  4. THE LEVEL.  z = fl(d/R) with e_z = (e_d + |ẑ|·e_R)/(R̂ − e_R) + one rounding.  The time below a level near a turning point is ILL-CONDITIONED
     in the recorded data: dα/dz = −1/sqrt(1 − z²).  The bound takes it whole, as the width of the interval acos maps [ẑ − e_z, ẑ + e_z] (clipped
     to [−1, 1]) to -- |Δα| <= |Δz|/sqrt(1 − z²) away from ±1, of the order of sqrt(2·e_z) across a tangency that is not exact.  Where the whole
     interval lies at or beyond ±1 the statement saturates with certainty (below = τ or 0.0 exactly) and the term is 0.  On top, pdmp_acos's
     stated 5u·α.  L = fl(c − 2α): e_L = δc + 2e_α + one rounding.
  5. W: (|n| + 1)·e_L and the rounding of n·L; e_r + e_α and the rounding of r − α, at most u·2π; the split of 3.; the rounding of the sum.
     below = fl(W1 − W0), a bin fl(below(e_k+1) − below(e_k)) clipped at 0.0 (the exact value is >= 0: clipping only brings it nearer): one
     rounding each.  A piece at rest adds τ: e_τ.
  6. The accumulator adds the N pieces of a trace one after the other to 0.0: at most N·u·(the exact entry + the errors above), times 1 + 2^-40
     for the products of small quantities.

Nothing is picked, and nothing comes from the code under test."""
import numpy as np
from mpmath import mp, mpf

mp.dps = 60  # (as tests/exact_arc_pairs.py and tests/test_detmath_acos.py set it: the context is shared)
U = mpf(2) ** -53
TINY = mpf(2) ** -1074
C2PI = mpf(6.28318530717958623200e+00)
SLACK = 1 + mpf(2) ** -40
ZERO = mpf(0)


def M(v):
    return mpf(float(v))


def rnd(exact, prop):
    """the error of a correctly rounded operation: the propagated error and its rounding (none where the result is exactly a double)"""
    if prop == 0 and mpf(float(exact)) == exact:
        return ZERO
    return prop + U * (abs(exact) + prop)


def edges_of(lo, hi, bins):
    """the computed edges e_0 .. e_B of the contract, as the doubles they are"""
    import hist_ref_lib as HR
    return [HR.edge(lo, hi, bins, k) for k in range(bins + 1)]


class Piece:
    """one live arc: the exact quantities and the errors of the statement's, per ψ0 and ψ1"""

    def __init__(self, xc, p, mu, tau, e_tau):
        self.tau, self.e_tau, self.mu, self.p = tau, e_tau, mu, p
        u = xc - mu
        e_u = rnd(u, ZERO)
        uu, pp = u * u, p * p
        e_uu = rnd(uu, 2 * abs(u) * e_u + e_u * e_u)
        e_pp = rnd(pp, ZERO)
        s = uu + pp
        e_s = rnd(s, e_uu + e_pp)
        self.R = mp.sqrt(s)
        self.e_R = rnd(self.R, self.R - mp.sqrt(max(s - e_s, ZERO)))
        self.phi = mp.atan2(p, u)
        if u > 0:
            q = abs(p / u)
            e_at = mpf("3.5") * U * abs(self.phi) + (TINY if 0 < q < mpf(2) ** -1022 else ZERO)
        else:
            e_at = 10 * U if u < 0 else U
        e_psi0 = e_at + (e_u / (self.R - e_u) if e_u else ZERO)
        psi0 = -self.phi
        psi1 = psi0 + tau
        e_psi1 = rnd(psi1, e_psi0 + e_tau)
        dc = abs(C2PI - 2 * mp.pi)
        self.turn = []
        for psi, e_psi in ((psi0, e_psi0), (psi1, e_psi1)):
            n = abs(mp.floor(psi / (2 * mp.pi))) + 1
            e_r = rnd(psi - C2PI * mp.floor(psi / (2 * mp.pi)), e_psi + n * dc + U * C2PI * n)
            self.turn.append((n, e_r))
        self.dc = dc

    def level(self, y):
        """(ẑ, e_z) of a finite level"""
        d = y - self.mu
        z = d / self.R
        return z, rnd(z, (rnd(d, ZERO) + abs(z) * self.e_R) / (self.R - self.e_R))

    def below(self, y):
        """(the exact time below the level y, the error of the statement's)"""
        if mp.isinf(y):
            return (self.tau, self.e_tau) if y > 0 else (ZERO, ZERO)
        z, e_z = self.level(y)
        if z - e_z >= 1:
            return self.tau, self.e_tau
        if z + e_z <= -1:
            return ZERO, ZERO
        # the exact occupation: the intervals (φ + α + 2πk, φ + 2π − α + 2πk) against [0, τ]
        if z >= 1:
            exact = self.tau
        elif z <= -1:
            exact = ZERO
        else:
            alpha, tp = mp.acos(z), 2 * mp.pi
            exact = ZERO
            k = mp.floor((-self.phi - tp) / tp) - 1
            while self.phi + alpha + tp * k < self.tau:
                a, b = self.phi + alpha + tp * k, self.phi + tp - alpha + tp * k
                exact += max(ZERO, min(b, self.tau) - max(a, ZERO))
                k += 1
        # the bound
        zl, zh = max(mpf(-1), z - e_z), min(mpf(1), z + e_z)
        alpha_hi = mp.acos(zl)
        e_alpha = (alpha_hi - mp.acos(zh)) + 5 * U * alpha_hi
        L = 2 * mp.pi - 2 * mp.acos(max(mpf(-1), min(mpf(1), z)))
        e_L = (self.dc + 2 * e_alpha) * (1 + U) + U * L
        e = self.e_tau
        for n, e_r in self.turn:
            e_W = (n + 1) * e_L + U * (n + 1) * C2PI  # n·L
            e_W += e_r + e_alpha + U * C2PI  # clamp(r − α, 0, L)
            e_W += e_r + U * C2PI  # the split
            e_W += U * ((n + 2) * C2PI)  # the sum
            e += e_W
        e += U * (self.tau + e)  # W1 − W0
        return exact, e


def exact_hist(t0, x0, th0, t, x, th, mu, coords, lo, hi, bins, cuts, f0=None, f=None):
    """One chain's PDMPTrace.  Per prefix t[:b], b in cuts: (H [m][bins + 2], Z [m], bound_H [m][bins + 2], bound_Z [m]) as lists of mpf, and the number of
    pieces so far of a free coordinate with p̂ != 0 that cross an edge.
    Also returns the table's facts: (the smallest 1 − |ẑ| over the (piece, edge) with |ẑ| < 1 that are not exact tangencies, the number of exact
    tangencies -- ẑ = ±1 with e_z = 0 --, the number of pieces of a free coordinate with p̂ != 0 that cross an edge)."""
    import hist_ref_lib as HR
    m = len(coords)
    E = [edges_of(lo[s], hi[s], bins) for s in range(m)]
    Em = [[mpf("-inf")] + [M(v) for v in E[s]] + [mpf("inf")] for s in range(m)]
    H = [[ZERO] * (bins + 2) for _ in range(m)]
    EH = [[ZERO] * (bins + 2) for _ in range(m)]
    Z, EZ, N = [ZERO] * m, [ZERO] * m, 0
    gap, tangencies, crossing = mpf(1), 0, 0
    out = {}
    tc, xc, pc = M(t0), [M(v) for v in x0], [M(v) for v in th0]
    fc = None if (f is None or f0 is None) else [bool(v) for v in f0]

    def snapshot():
        g = N * U
        return ([[v for v in row] for row in H], list(Z),
                [[SLACK * (EH[s][k] + g * (H[s][k] + EH[s][k])) for k in range(bins + 2)] for s in range(m)],
                [SLACK * (EZ[s] + g * (Z[s] + EZ[s])) for s in range(m)], crossing)

    if 0 in cuts:
        out[0] = snapshot()
    for e in range(len(t)):
        tau = M(t[e]) - tc
        if tau > 0:
            N += 1
            e_tau = rnd(tau, ZERO)
            for s in range(m):
                i = int(coords[s])
                free = fc is None or fc[i]
                if not free or (xc[i] == M(mu[i]) and pc[i] == 0):
                    slot = HR.bin_of(lo[s], hi[s], bins, float(xc[i])) + 1  # (comparisons of doubles against the computed edges: exact)
                    H[s][slot] += tau
                    EH[s][slot] += e_tau
                    Z[s] += tau
                    EZ[s] += e_tau
                    continue
                P = Piece(xc[i], pc[i], M(mu[i]), tau, e_tau)
                prev, e_prev = ZERO, ZERO
                crossed = False
                for k in range(bins + 2):
                    y = Em[s][k + 1]
                    if not mp.isinf(y):
                        zz, e_zz = P.level(y)
                        if abs(zz) == 1 and e_zz == 0:
                            tangencies += 1
                        elif abs(zz) < 1:
                            gap = min(gap, 1 - abs(zz))
                            crossed = True
                        elif abs(zz) == 1:
                            gap = ZERO  # (a tangency that is not exact: the table has none)
                    b, e_b = P.below(y)
                    o = b - prev
                    H[s][k] += o
                    EH[s][k] += e_b + e_prev + U * (o + e_b + e_prev)
                    prev, e_prev = b, e_b
                crossing += crossed and P.p != 0
        tc, xc, pc = M(t[e]), [M(v) for v in x[e]], [M(v) for v in th[e]]
        fc = None if f is None else [bool(v) for v in f[e]]
        if e + 1 in cuts:
            out[e + 1] = snapshot()
    return out, (gap, tangencies, crossing)


def used(value, exact, bound):
    """the fraction of the bound a float uses (0 where both error and bound are 0)"""
    err = abs(mpf(float(value)) - exact)
    if bound == 0:
        assert err == 0, (value, exact)
        return 0.0
    return float(err / bound)
