"""The pair integrals of a Boomerang's arcs without a device: the sequential C statement of the contract (tests/ref/arc_pairs_ref.c), its host
mirror trace.arc_pair_integrals (bit for bit), the integrals with mpmath at 60 digits with the derived bound (tests/exact_arc_pairs.py) -- which
the statement keeps and a statement with ∫cos² and ∫sin² exchanged does not --, the three properties of the grouping, trace.path_moments, and
the refusals.

Used fraction of the derived bound, the C statement on every case (largest over pairs / coordinates), as printed by
test_statement_keeps_the_derived_bound: S 0.0196 (sticky130), J 0.0429 (boom_sticky); boom: 0.00671 and 0.0179.  A bound whose leading term is
the stated absolute error of pdmp_sincos, 2.5e-16, three times per piece, is wide for pieces whose sine and cosine are good to an ulp; the
statement with ∫cos² and ∫sin² exchanged is outside it on every case."""
import numpy as np
import pytest
import scipy.sparse as sp

import arc_pairs_cases as AC
import arc_pairs_ref_lib as AR
import exact_arc_pairs as EA


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def trace_of(pkg, c, k, upto=None):
    B = pkg.Boomerang(sp.identity(c.d, format="csc"), c.mu, 1.0)
    f = c.f[k][:upto] if c.sticky else None
    return pkg.PDMPTrace(B, c.t0, c.x0[k], c.th0[k], c.t[k][:upto], c.x[k][:upto], c.th[k][:upto], f0=None, f=f)


@pytest.fixture(scope="module")
def exact():
    """(exact S, exact J, bound S, bound J) per (name, chain): computed once, shared, read-only"""
    out = {}

    def get(pkg, name, k):
        if (name, k) not in out:
            c, pi, pj, cen = AC.listed(name)
            out[(name, k)] = EA.of_trace(trace_of(pkg, c, k), pi, pj, cen)
        return out[(name, k)]
    return get


@pytest.mark.parametrize("name", AC.NAMES)
def test_statement_keeps_the_derived_bound(pkg, exact, name, capsys):
    c, pi, pj, cen = AC.listed(name)
    for k in range(c.nchains):
        tr = trace_of(pkg, c, k)
        S, J, T = AC.reference(name, k, c.nseg - 1)
        assert T == (c.t[k][-1] if len(c.t[k]) else c.t0)
        eS, eJ, bS, bJ = exact(pkg, name, k)
        uS = max(EA.used(S[q], eS[q], bS[q]) for q in range(len(pi)))
        uJ = max(EA.used(J[j], eJ[j], bJ[j]) for j in range(c.d))
        with capsys.disabled():
            print("\n  %s chain %d: the statement uses %.3g of the bound on S, %.3g on J" % (name, k, uS, uJ), end="")
        assert uS < 1.0 and uJ < 1.0, (uS, uJ)
        # the same statement with ∫cos² and ∫sin² exchanged is outside it: the bound tells the two apart
        Sx, _, _ = AR.of_trace(tr, pi, pj, cen, exchanged=True)
        ux = max(EA.used(Sx[q], eS[q], bS[q]) for q in range(len(pi)))
        assert ux > 1.0, ux


@pytest.mark.parametrize("name", AC.NAMES)
def test_mirror_is_the_statement_bit_for_bit(pkg, name):
    c, pi, pj, cen = AC.listed(name)
    for k in range(c.nchains):
        for s in range(c.nseg):  # (every prefix the device test reads at)
            upto = c.cuts[k][s + 1]
            S, J, T = AC.reference(name, k, s)
            S2, J2, T2 = pkg.trace.arc_pair_integrals(trace_of(pkg, c, k, upto), pi, pj, cen)
            assert same_bits(S, S2) and same_bits(J, J2) and T == T2, (k, s)


def test_python_sincos_is_pdmp_sincos(pkg):
    import detmath_tables as T
    import oracle_lib as O
    x = np.concatenate([np.asarray(list(T.sincos_inputs()), dtype=np.float64), [0.0, -0.0, 1e-9, 27.0, np.nan, np.inf, 2.0 ** 30, np.nextafter(2.0 ** 30, np.inf)]])
    s, c = pkg.trace._pdmp_sincos(x)
    ref = np.array([O.sincos(float(v)) for v in x])
    ok = ~np.isnan(ref[:, 0])
    assert same_bits(s[ok], ref[ok, 0]) and same_bits(c[ok], ref[ok, 1])
    assert np.all(np.isnan(s[~ok])) and np.all(np.isnan(c[~ok])) and (~ok).sum() >= 3


@pytest.mark.parametrize("name", ["boom_sticky", "sticky130", "lists24_256", "edge"])
def test_symmetric_bit_for_bit(pkg, name):
    c, pi, pj, cen = AC.listed(name)
    tr = trace_of(pkg, c, 0)
    S, J, _ = AR.of_trace(tr, pi, pj, cen)
    S2, J2, _ = AR.of_trace(tr, pj, pi, cen)
    S3, J3, _ = pkg.trace.arc_pair_integrals(tr, pj, pi, cen)
    assert same_bits(S, S2) and same_bits(J, J2) and same_bits(S, S3) and same_bits(J, J3)
    perm = np.random.default_rng(0).permutation(len(pi))
    S4, J4, _ = AR.of_trace(tr, pi[perm], pj[perm], cen)
    assert same_bits(S[perm], S4) and same_bits(J, J4)


def test_all_frozen_piece_is_the_line_contracts(pkg):
    """two coordinates that are not free over a piece: (mi·mj)·τ, the bits of the line contract's τ·(a·b) with v = 0"""
    rng = np.random.default_rng(3)
    d = 3
    mu, cen = rng.uniform(-1, 1, d), rng.uniform(-1, 1, d)
    x0, th0 = mu + rng.standard_normal(d), rng.standard_normal(d)
    t = np.array([0.0, 0.0, 1.7])  # (t0, x0, θ0), then an event at the same time that freezes 0 and 1, then the piece
    x, th = np.vstack([x0, mu + rng.standard_normal((2, d))]), np.vstack([th0, rng.standard_normal((2, d))])
    f = np.array([[1, 1, 1], [0, 0, 1], [1, 1, 1]], dtype=bool)
    tr = pkg.PDMPTrace(pkg.Boomerang(sp.identity(d, format="csc"), mu, 1.0), 0.0, x0, th0, t, x, th, f0=None, f=f)
    pi, pj = np.array([0, 0, 1]), np.array([0, 1, 1])
    tau = t[2] - t[1]
    m = x[1] - cen
    want = [0.0 + (m[a] * m[b]) * tau for a, b in zip(pi, pj)]
    for S, J, T in (AR.of_trace(tr, pi, pj, cen), pkg.trace.arc_pair_integrals(tr, pi, pj, cen)):
        assert same_bits(S, want) and same_bits(J[:2], 0.0 + m[:2] * tau) and T == 1.7
    import pairs_ref_lib as PR
    lin = PR.pdmp(0.0, x0, th0, t, x, th, pi, pj, cen, f=f)  # the line contract on the same frozen piece: τ·(a·b)
    assert same_bits(lin[0], want)


def test_small_tau_does_not_cancel(pkg):
    """τ = 1e-9: 1 − cos τ rounds to 0 where ∫sin = 5e-19; the contract's Is keeps it"""
    d = 1
    B = pkg.Boomerang(sp.identity(d, format="csc"), np.zeros(d), 1.0)
    tr = pkg.PDMPTrace(B, 0.0, np.zeros(d), np.ones(d), np.array([1e-9]), np.zeros((1, d)), np.ones((1, d)))
    for S, J, _ in (AR.of_trace(tr, [0], [0]), pkg.trace.arc_pair_integrals(tr, [0], [0])):
        assert 1.0 - np.cos(1e-9) == 0.0 and abs(J[0] - 5e-19) < 1e-32  # x = sin s from (0, 1): J = 1 − cos τ = τ²/2, to a few ulps
        assert abs(S[0] - 1e-27 / 3) <= 2.0 ** -52 * 1e-9  # ∫ sin² = τ³/3 = (τ − sin τ cos τ)/2: good to u·|τ|·A², the B of the bound, no better


@pytest.mark.parametrize("name", ["boom", "d1", "lists24_255", "two"])
def test_against_path_moments(pkg, name):
    """centre 0: S_ii and J_i are trace.path_moments(Ξ, T_last), to the tolerance of tests/test_gpu_bps_moments.py (1e-9 of the scales s1, s2)"""
    c = AC.listed(name)[0]
    for k in range(c.nchains):
        tr = trace_of(pkg, c, k)
        S, J, T = pkg.trace.arc_pair_integrals(tr, np.arange(c.d), np.arange(c.d))
        h1, h2 = pkg.trace.path_moments(tr, T)
        s2 = np.abs(h2).max()
        s1 = np.sqrt((T - tr.t0) * s2)
        assert np.max(np.abs(J - h1)) <= 1e-9 * s1 and np.max(np.abs(S - h2)) <= 1e-9 * s2


def test_covariance_is_used_unchanged(pkg):
    c, pi, pj, cen = AC.listed("boom")
    tr = trace_of(pkg, c, 0)
    S, J, T = pkg.trace.arc_pair_integrals(tr, pi, pj, cen)
    cov, mean = pkg.trace.covariance(pi, pj, S, J, T - c.t0, center=cen)
    S0, J0, _ = pkg.trace.arc_pair_integrals(tr, pi, pj)
    cov0, mean0 = pkg.trace.covariance(pi, pj, S0, J0, T - c.t0)
    assert abs(cov - cov.T).max() == 0 and np.allclose(cov.toarray(), cov0.toarray(), rtol=0, atol=1e-12) and np.allclose(mean, mean0, rtol=0, atol=1e-13)


def test_mirror_refusals(pkg):
    d = 4
    G = sp.identity(d, format="csc")
    x0, th0 = np.zeros(d), np.ones(d)
    ev = np.array([(1.0, 0, 1.0, -1.0)], dtype=pkg._lib.EVENT_DTYPE)
    one = (np.array([1.0]), np.ones((1, d)), np.ones((1, d)))
    others = [pkg.FactTrace(pkg.FactBoomerang(G, np.zeros(d), 0.1), 0.0, x0, th0, ev), pkg.FactTrace(None, 0.0, x0, th0, ev),
              pkg.PDMPTrace(pkg.BouncyParticle(G, np.zeros(d), 1.0), 0.0, x0, th0, *one), pkg.PDMPTrace(None, 0.0, x0, th0, *one)]
    for tr in others:
        with pytest.raises(TypeError, match="Boomerang"):
            pkg.trace.arc_pair_integrals(tr, [0], [0])
    tr = pkg.PDMPTrace(pkg.Boomerang(G, np.zeros(d), 0.1), 0.0, x0, th0, *one)
    with pytest.raises(TypeError, match="Boomerang"):  # ... and the line mirror keeps refusing this one
        pkg.trace.pair_integrals(tr, [0], [0])
    for pi, pj, word in (([], [], "at least one"), ([0, 1], [0], "one entry each"), ([0], [d], "outside"), ([-1], [0], "outside"),
                         ([0, 1, 0], [1, 2, 1], "twice"), ([0, 1], [1, 0], "twice")):
        with pytest.raises(ValueError, match=word):
            pkg.trace.arc_pair_integrals(tr, pi, pj)
    for cen in (np.zeros(d + 1), np.array([0.0, np.inf, 0.0, 0.0]), np.array([np.nan, 0.0, 0.0, 0.0])):
        with pytest.raises(ValueError, match="centre"):
            pkg.trace.arc_pair_integrals(tr, [0], [1], cen)
    S, J, T = pkg.trace.arc_pair_integrals(pkg.PDMPTrace(tr.F, 0.0, x0, th0, np.empty(0), np.empty((0, d)), np.empty((0, d))), [0], [1])
    assert same_bits(S, [0.0]) and same_bits(J, np.zeros(d)) and T == 0.0  # no event: nothing to integrate
