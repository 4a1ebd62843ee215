"""The pair integrals S_ij = ∫ (x_i − c_i)(x_j − c_j) dt and J_i = ∫ (x_i − c_i) dt of a trace in exact rational arithmetic, with the error bound
of the float64 statement of the contract (tests/ref/pairs_ref.c), in the manner of tests/exact_path.py.  TEST INFRASTRUCTURE ONLY.

The path is the one the trace's floats describe: every recorded number (t, x, θ, the centre c) is taken as the exact rational it is; a
FactTrace coordinate runs on the line from its last event (its cursor), a PDMPTrace state from the last event, frozen coordinates standing.
The pieces are the contract's pieces -- the exact integral of a piece is the polynomial the contract evaluates, so the exact S is the sum of
the exactly evaluated pieces and the only difference to the float64 statement is rounding.

The bound.  u = 2^-53; every float operation returns the exact result times (1 + δ), |δ| <= u (no underflow: the tests' magnitudes are far
from it).  For an expression E built from exact leaves by +, −, ·, / write Ē for the same expression with every leaf and every intermediate
replaced by its absolute value (so Ē >= |E|) and k(E) for the largest number of roundings on a path from a leaf to the root; then
|fl(E) − E| <= γ_k Ē with γ_k = k u / (1 − k u)  (Higham, Accuracy and Stability, Lemma 3.1 / 3.3): a product of two factors carrying k1 and
k2 roundings carries k1 + k2 + 1, a sum max(k1, k2) + 1 on the sum of the absolute values; multiplying by 0.5 is exact.
  FactTrace piece, a = (x_i − c_i) + θ_i·(s0 − t_i): x_i − c_i and s0 − t_i are differences of exact leaves, one rounding each ON THE
  DIFFERENCE (not on |x| + |c|: this is what a centre near the path buys); θ·(s0 − t_i): 2; the sum: 3, on ā = |x_i − c_i| + |θ_i||s0 − t_i|.
  τ = t − s0: 1.  Then
      a·b 7 | a·vj 4, + 5, ·0.5 5 | vi·vj 1, /3 2, τ·(…) 4 | (5, 4) + 6 | τ·(…) 8 | a·b + (…) 9 | τ·(…) 11
  so a piece P carries 11 roundings on  P̄ = |τ|(ā b̄ + |τ|(0.5(ā|vj| + b̄|vi|) + |τ||vi vj|/3)).
  PDMPTrace piece, a = x_i − c_i (1 rounding): a·b 3 | a·vj 2, + 3 | τ·(vi vj / 3) 4 | + 5 | τ· 7 | + 8 | τ· 10.
  J piece τ·(a + 0.5·(v·τ)), a = x − c: v·τ 2, + 3, τ· 5 (FactTrace and PDMPTrace alike).
  The accumulator adds the N pieces of a pair one after the other to 0.0, the read adds the closing piece: N + 1 additions at most on any
  piece.  Hence
      |S_float − S_exact| <= γ_{N + 1 + 11} · Σ P̄          |J_float − J_exact| <= γ_{M + 1 + 5} · Σ |τ|(|x − c| + 0.5|v||τ|)
  (PDMPTrace: 10 for 11 and no closing piece).  N, Σ P̄ are counted per pair from the trace; nothing is picked.
"""
from fractions import Fraction

U = Fraction(1, 2 ** 53)
K_FACT, K_PDMP, K_LINE = 11, 10, 5


def gamma(k):
    return k * U / (1 - k * U)


def _F(v):
    return Fraction(float(v))


def _piece(a, b, vi, vj, tau):
    return tau * (a * b + tau * (Fraction(1, 2) * (a * vj + b * vi) + tau * (vi * vj) / 3))


def _line(a, v, tau):
    return tau * (a + Fraction(1, 2) * v * tau)


def exact_fact(t0, x0, th0, events, pi, pj, center=None):
    """(S, J, bound_S, bound_J): lists of Fractions, per pair / per coordinate, of one chain's FactTrace"""
    d = len(x0)
    c = [Fraction(0)] * d if center is None else [_F(v) for v in center]
    ct, cx, cth = [_F(t0)] * d, [_F(v) for v in x0], [_F(v) for v in th0]
    np_ = len(pi)
    S, Sa, N = [Fraction(0)] * np_, [Fraction(0)] * np_, [0] * np_
    J, Ja, M = [Fraction(0)] * d, [Fraction(0)] * d, [0] * d
    of = [[] for _ in range(d)]
    for k in range(np_):
        of[int(pi[k])].append(k)
        if int(pj[k]) != int(pi[k]):
            of[int(pj[k])].append(k)

    def close(k, t):
        i, j = int(pi[k]), int(pj[k])
        s0 = max(ct[i], ct[j])
        a, b = (cx[i] - c[i]) + cth[i] * (s0 - ct[i]), (cx[j] - c[j]) + cth[j] * (s0 - ct[j])
        aa = abs(cx[i] - c[i]) + abs(cth[i]) * abs(s0 - ct[i])
        ba = abs(cx[j] - c[j]) + abs(cth[j]) * abs(s0 - ct[j])
        S[k] += _piece(a, b, cth[i], cth[j], t - s0)
        Sa[k] += _piece(aa, ba, abs(cth[i]), abs(cth[j]), abs(t - s0))
        N[k] += 1

    def line(i, t):
        J[i] += _line(cx[i] - c[i], cth[i], t - ct[i])
        Ja[i] += _line(abs(cx[i] - c[i]), abs(cth[i]), abs(t - ct[i]))
        M[i] += 1

    T = _F(t0)
    for e in events:
        i, t = int(e["i"]), _F(e["t"])
        T = t
        for k in of[i]:
            close(k, t)
        line(i, t)
        ct[i], cx[i], cth[i] = t, _F(e["x"]), _F(e["theta"])
    for k in range(np_):
        close(k, T)
    for i in range(d):
        line(i, T)
    return S, J, [gamma(N[k] + K_FACT) * Sa[k] for k in range(np_)], [gamma(M[i] + K_LINE) * Ja[i] for i in range(d)]


def exact_pdmp(t0, x0, th0, t, x, th, pi, pj, center=None, f0=None, f=None):
    """(S, J, bound_S, bound_J) of one chain's PDMPTrace (f: the free masks of a sticky trace, f0 the initial one; None = all free)"""
    d = len(x0)
    c = [Fraction(0)] * d if center is None else [_F(v) for v in center]
    np_ = len(pi)
    S, Sa = [Fraction(0)] * np_, [Fraction(0)] * np_
    J, Ja = [Fraction(0)] * d, [Fraction(0)] * d
    tc = _F(t0)
    xc = [_F(v) for v in x0]
    vc = [_F(v) if (f is None or f0 is None or f0[j]) else Fraction(0) for j, v in enumerate(th0)]
    n = len(t)
    for e in range(n):
        tau = _F(t[e]) - tc
        for k in range(np_):
            i, j = int(pi[k]), int(pj[k])
            S[k] += _piece(xc[i] - c[i], xc[j] - c[j], vc[i], vc[j], tau)
            Sa[k] += _piece(abs(xc[i] - c[i]), abs(xc[j] - c[j]), abs(vc[i]), abs(vc[j]), abs(tau))
        for j in range(d):
            J[j] += _line(xc[j] - c[j], vc[j], tau)
            Ja[j] += _line(abs(xc[j] - c[j]), abs(vc[j]), abs(tau))
        tc = _F(t[e])
        xc = [_F(v) for v in x[e]]
        vc = [_F(v) if (f is None or f[e][j]) else Fraction(0) for j, v in enumerate(th[e])]
    return S, J, [gamma(n + K_PDMP) * v for v in Sa], [gamma(n + K_LINE) * v for v in Ja]


def of_trace(tr, pi, pj, center=None):
    if hasattr(tr, "events"):
        return exact_fact(tr.t0, tr.x0, tr.θ0, tr.events, pi, pj, center)
    f = getattr(tr, "f", None)
    d = len(tr.x0)
    return exact_pdmp(tr.t0, tr.x0, tr.θ0, tr.t, tr.x.reshape(-1, d), tr.θ.reshape(-1, d), pi, pj, center,
                      f0=getattr(tr, "f0", None) if f is not None else None, f=None if f is None else f.reshape(-1, d))


def used(value, exact, bound):
    """the fraction of the bound a float uses (0 where both error and bound are 0)"""
    err = abs(Fraction(float(value)) - exact)
    if bound == 0:
        assert err == 0
        return 0.0
    return float(err / bound)
