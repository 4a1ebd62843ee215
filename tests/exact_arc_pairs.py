"""The pair integrals S_ij = ∫ (x_i − z_i)(x_j − z_j) dt and J_i = ∫ (x_i − z_i) dt of a Boomerang's PDMPTrace with mpmath at 60 digits, and the
error bound of the float64 statement of the contract (tests/ref/arc_pairs_ref.c), in the manner of tests/exact_pairs.py.  TEST
INFRASTRUCTURE ONLY.

The path is the one the trace's floats describe: every recorded number (t, x, θ, μ, the centre z) is taken as the exact number it is; on the
piece of an event a free coordinate is x(s) − z = û·cos s + p̂·sin s + m̂ with û = x_c − μ, p̂ = θ_c, m̂ = μ − z (not free: û = p̂ = 0,
m̂ = x_c − z), all exact, over s in [0, τ̂], τ̂ = t_k − t_c exact and signed.  The exact integral of a piece is the contract's expression in the
exact basis integrals  Îcc = (τ̂ + sin τ̂ cos τ̂)/2, Îss = (τ̂ − sin τ̂ cos τ̂)/2, Îsc = sin² τ̂/2, Îc = sin τ̂, Îs = 1 − cos τ̂.  At 60 digits the
reference's own error is below 1e-55 of the majorant B below: forty orders under the bound.

The bound.  u = 2^-53; every float operation returns the exact result times (1 + δ), |δ| <= u (no underflow: the tests' magnitudes are far
from it).  For an expression E built from exact leaves by +, −, ·, / write Ē for the same expression with every leaf and intermediate replaced
by its absolute value and k(E) for the largest number of roundings on a path from a leaf to the root; then |fl(E) − E| <= γ_k Ē,
γ_k = k u / (1 − k u) (Higham, Accuracy and Stability, Lemma 3.1 / 3.3): a product carries k1 + k2 + 1, a sum max(k1, k2) + 1 on the sum of
the absolute values; multiplying by 0.5 is exact.  Write A_i = |û_i| + |p̂_i| + |m̂_i| and, per piece, B_ij = |τ̂|·A_i·A_j: Σ_pieces B_ij is
the B of the contract's error statement.

  1. The leaves.  u = fl(x_c − μ), m = fl(μ − z) or fl(x_c − z), τ = fl(t_k − t_c): differences of exact leaves, one rounding each ON THE
     DIFFERENCE; p = θ_c: none.
  2. pdmp_sincos.  (s, c) = pdmp_sincos(τ) are sin τ and cos τ up to the absolute error ε = SINCOS_ABS = 2.5e-16 stated in
     include/pdmp_detmath.h and pinned by tests/test_detmath_accuracy.py, and |sin τ − sin τ̂| <= |τ − τ̂| <= u|τ̂| (cos alike): s = sin τ̂ + e_s,
     |e_s|, |e_c| <= η = ε + u|τ̂|.  To first order in η, with |s|, |c| <= 1 and 1 + c >= 1 on the branch c > 0:
         h = s·c: 2η | Icc, Iss = (τ ± h)/2: η | Isc = s²/2: η | Ic = s: η | Is = s²/(1 + c): 2η + η = 3η, or 1 − c: η.
     Both forms of Is are the same exact function, so the branch adds nothing.  The piece is linear in the five integrals with coefficients
     ûû, p̂p̂, (ûp̂ + ûp̂), m̂û, m̂p̂ (the term m̂m̂·τ has none of them), so the error of (s, c) moves a pair's piece by at most 3η·A_i·A_j and a
     coordinate's own by at most 3η·(|û| + |p̂|) <= 3η·A_i.  The u|τ̂| part of η is 3 more roundings on B_ij; the ε part stays absolute: a piece
     of any length, however short, may be off by 3ε·A_i·A_j.  This term is what the stated accuracy of pdmp_sincos costs; it has no |τ| in it.
  3. The roundings of one piece, with s and c now taken as leaves:
         h 1 | τ ± h 2 (Icc, Iss) | s·s 1 (Isc) | Ic 0 | 1 + c 1, s·s / (1 + c) 3 (Is; 1 − c: 1)
         (ui·uj)·Icc 3, 6 | (pi·pj)·Iss 1, 4 | + 7 | ui·pj + uj·pi 2, 3 | ·Isc 5 | + 8
         uj·Ic + pj·Is 2, 4, 5 | mi·(…) 7 | + 8 | (mi·mj)·τ 3, 5 | + 9 | the piece 10
         J: u·Ic + p·Is 2, 4, 5 | m·τ 3 | + 6
     The majorant: |sin|, |sin cos|, sin², 1 − cos <= |τ̂|, so every Ī <= |τ̂| -- except Īs on the branch 1 − c, where it is 1 + |c| <= 2 with
     |τ̂| >= π/2 (to ε), i.e. <= (4/π)|τ̂|.  The nine products of the piece are the nine terms of A_i·A_j: P̄ <= (4/π)·B_ij.
  4. The accumulator adds the N pieces of a trace one after the other to 0.0: at most N more roundings on any piece.

  Hence, with K_PAIR = 10 + 3 and K_LINE = 6 + 3,
      |S_float − S_exact| <= (1 + 2^-40)·[ (4/π)·γ_{N + K_PAIR}·Σ B_ij + 3ε·Σ A_i·A_j ]
      |J_float − J_exact| <= (1 + 2^-40)·[ (4/π)·γ_{N + K_LINE}·Σ |τ̂|·A_i + 3ε·Σ A_i ]
  the factor 1 + 2^-40 covering every product of two of the small quantities above (ε·γ, ε², η against ε in the majorants: each below 1e-30
  per unit of A_i·A_j, where the bracket holds at least 3ε = 7.5e-16 of it).  N, Σ B and Σ A·A are counted per pair from the trace; nothing is
  picked, and nothing comes from the code under test.
"""
from mpmath import mp, mpf

from test_detmath_accuracy import SINCOS_ABS

mp.dps = 60
U = mpf(2) ** -53
K_PAIR, K_LINE = 13, 9
EPS = mpf(SINCOS_ABS)
SLACK = 1 + mpf(2) ** -40


def gamma(k):
    return k * U / (1 - k * U)


def exact_arcs(t0, x0, th0, t, x, th, mu, pi, pj, center=None, f0=None, f=None):
    """(S, J, bound_S, bound_J): lists of mpf, per pair / per coordinate, of one chain's PDMPTrace (f: the free masks of a sticky trace, f0
    the initial one; None = all free)"""
    d = len(x0)
    z = [mpf(0)] * d if center is None else [mpf(float(v)) for v in center]
    mu = [mpf(float(v)) for v in mu]
    np_ = len(pi)
    S, SB, SA = [mpf(0)] * np_, [mpf(0)] * np_, [mpf(0)] * np_
    J, JB, JA = [mpf(0)] * d, [mpf(0)] * d, [mpf(0)] * d
    tc = mpf(float(t0))
    xc, pc = [mpf(float(v)) for v in x0], [mpf(float(v)) for v in th0]
    fc = None if (f is None or f0 is None) else [bool(v) for v in f0]
    n = len(t)
    for e in range(n):
        tau = mpf(float(t[e])) - tc
        s, c = mp.sin(tau), mp.cos(tau)
        Icc, Iss, Isc, Ic, Is = (tau + s * c) / 2, (tau - s * c) / 2, s * s / 2, s, 1 - c
        u, p, m = [None] * d, [None] * d, [None] * d
        for j in range(d):
            if fc is None or fc[j]:
                u[j], p[j], m[j] = xc[j] - mu[j], pc[j], mu[j] - z[j]
            else:
                u[j], p[j], m[j] = mpf(0), mpf(0), xc[j] - z[j]
        A = [abs(u[j]) + abs(p[j]) + abs(m[j]) for j in range(d)]
        g = [u[j] * Ic + p[j] * Is for j in range(d)]
        for k in range(np_):
            i, j = int(pi[k]), int(pj[k])
            S[k] += (u[i] * u[j]) * Icc + (p[i] * p[j]) * Iss + (u[i] * p[j] + u[j] * p[i]) * Isc + m[i] * g[j] + m[j] * g[i] + m[i] * m[j] * tau
            SB[k] += abs(tau) * A[i] * A[j]
            SA[k] += A[i] * A[j]
        for j in range(d):
            J[j] += g[j] + m[j] * tau
            JB[j] += abs(tau) * A[j]
            JA[j] += A[j]
        tc = mpf(float(t[e]))
        xc, pc = [mpf(float(v)) for v in x[e]], [mpf(float(v)) for v in th[e]]
        fc = None if f is None else [bool(v) for v in f[e]]
    q = 4 / mp.pi
    bS = [SLACK * (q * gamma(n + K_PAIR) * SB[k] + 3 * EPS * SA[k]) for k in range(np_)]
    bJ = [SLACK * (q * gamma(n + K_LINE) * JB[j] + 3 * EPS * JA[j]) for j in range(d)]
    return S, J, bS, bJ


def of_trace(tr, pi, pj, center=None):
    f = getattr(tr, "f", None)
    d = len(tr.x0)
    return exact_arcs(tr.t0, tr.x0, tr.θ0, tr.t, tr.x.reshape(-1, d), tr.θ.reshape(-1, d), tr.F.μ, pi, pj, center,
                      f0=(getattr(tr, "f0", None) if f is not None else None), f=None if f is None else f.reshape(-1, d))


def used(value, exact, bound):
    """the fraction of the bound a float uses (0 where both error and bound are 0)"""
    err = abs(mpf(float(value)) - exact)
    if bound == 0:
        assert err == 0
        return 0.0
    return float(err / bound)
