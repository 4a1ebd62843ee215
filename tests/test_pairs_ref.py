"""The pair integrals S_ij = ∫ (x_i − c_i)(x_j − c_j) dt, J_i = ∫ (x_i − c_i) dt without a device: the sequential C statement of the contract
(tests/ref/pairs_ref.c), its host mirror trace.pair_integrals (bit for bit), the exact rational integrals with the derived rounding bound
(tests/exact_pairs.py), the covariance that follows (trace.covariance) against Γ⁻¹ inside the reference's own envelope, and the refusals."""
import numpy as np
import pytest
import scipy.sparse as sp

import consumer_cases as CC
import exact_pairs as EP
import oracle_lib as O
import pairs_ref_lib as PR
import pdmp_consumer_cases as PC


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check(pkg, tr, pi, pj, center=None):
    """C statement == host mirror bit for bit, both within the derived bound of the exact integrals; returns the largest used fractions"""
    S, J, T = PR.of_trace(tr, pi, pj, center)
    S2, J2, T2 = pkg.trace.pair_integrals(tr, pi, pj, center)
    assert same_bits(S, S2) and same_bits(J, J2) and T == T2
    eS, eJ, bS, bJ = EP.of_trace(tr, pi, pj, center)
    uS = max(EP.used(S[k], eS[k], bS[k]) for k in range(len(pi)))
    uJ = max(EP.used(J[j], eJ[j], bJ[j]) for j in range(len(J)))
    assert uS <= 1.0 and uJ <= 1.0, (uS, uJ)
    return uS, uJ, (S, J, T)


def fact_trace(pkg, c, k, upto=None):
    return pkg.FactTrace(None, c.t0, c.x0[k], c.th0[k], c.events[k][:upto])


def pdmp_trace(pkg, c, k):
    return pkg.PDMPTrace(None, c.t0, c.x0[k], c.th0[k], c.t[k], c.x[k], c.th[k], f0=None, f=c.f[k] if c.sticky else None)


# ---------------------------------------------------------------------------------------------- 1. the float64 statement against the exact integrals

@pytest.mark.parametrize("name", ["one", "few", "on_grid_end", "sticky"])
def test_dyadic_fact_traces(pkg, name, capsys):
    c = CC.case(name)
    pi, pj = np.triu_indices(c.d)
    for k in range(c.nchains):
        for center in (None, 0.25 + 0.125 * np.arange(c.d)):
            uS, uJ, _ = check(pkg, fact_trace(pkg, c, k), pi, pj, center)
            with capsys.disabled():
                print("\n  %s chain %d centre %s: the statement uses %.3g of the bound on S, %.3g on J" % (name, k, center is not None, uS, uJ), end="")
            assert uS < 0.5  # the bound has room: a dyadic trace rounds in the products of a piece only


@pytest.mark.parametrize("name", [n for n in PC.NAMES if not n.startswith("boom")])
def test_hand_made_pdmp_traces(pkg, name):
    c = PC.case(name)
    rng = np.random.default_rng(7)
    sel = np.sort(rng.choice(c.d, min(c.d, 5), replace=False))
    a, b = np.triu_indices(len(sel))
    for k in range(c.nchains):
        check(pkg, pdmp_trace(pkg, c, k), sel[a], sel[b], None if k == 0 else rng.standard_normal(c.d))


@pytest.fixture(scope="module")
def spdmp8(pkg):
    """test/maintest.jl:37-61: Γ = S S' at d = 8, flow 0.9 Γ, c = 0.7 column norms, T = 1000; 2 oracle chains, seed 2"""
    G = pkg.problems.maintest_precision(8)
    rng = np.random.default_rng(2)
    c = 0.7 * pkg.problems.column_norms(G)
    out = []
    for k in range(2):
        x0, th0 = rng.random(8), rng.choice([-1.0, 1.0], 8)
        r = O.spdmp_zigzag(sp.csc_matrix(0.9 * G), None, G, x0, th0, c, 1000.0, seed=2 + k)
        out.append(pkg.FactTrace(None, 0.0, x0, th0, r["events"]))
    return G, out


@pytest.fixture(scope="module")
def bps16(pkg):
    G = pkg.problems.gmrf_precision(4)
    rng = np.random.default_rng(3)
    x0, th0 = rng.standard_normal(16), rng.standard_normal(16)
    r = O.pdmp_bps(G, None, x0, th0, 10.0, 30.0, ev_cap=4096, seed=3)
    assert 50 < len(r["t_ev"]) < 4096
    return pkg.PDMPTrace(None, 0.0, x0, th0, r["t_ev"], r["x_ev"], r["theta_ev"])


def test_oracle_traces(pkg, spdmp8, bps16):
    pi, pj = np.tril_indices(8)
    tr = spdmp8[1][0]
    short = pkg.FactTrace(None, tr.t0, tr.x0, tr.θ0, tr.events[:600])  # (the exact sums are slow; the bound is per piece)
    check(pkg, short, pi, pj)
    check(pkg, short, pi, pj, np.linspace(-1, 1, 8))
    a, b = np.tril_indices(8)
    pi16, pj16 = np.concatenate([np.arange(16), a[a != b] + 4]), np.concatenate([np.arange(16), b[a != b] + 4])
    short = pkg.PDMPTrace(None, 0.0, bps16.x0, bps16.θ0, bps16.t[:150], bps16.x[:150], bps16.θ[:150])
    check(pkg, short, pi16, pj16)
    S, J, T = PR.of_trace(bps16, pi16, pj16)  # ... and the whole trace, C against the mirror
    S2, J2, T2 = pkg.trace.pair_integrals(bps16, pi16, pj16)
    assert same_bits(S, S2) and same_bits(J, J2) and T == T2 == bps16.t[-1]


# ---------------------------------------------------------------------------------------------- 2. slicing changes nothing

class Stream:
    """The FactTrace contract as a streaming consumer states it: cursors and accumulators carried from slice to slice, a read closes the open
    pieces WITHOUT touching them (floats throughout, the arithmetic of trace._pair_piece).  A statement of the CONTRACT's property, written
    here: the package has no streaming path on the host -- trace.pair_integrals takes a whole trace -- and the product code that slices is
    the device's, which tests/test_gpu_pairs.py cuts one-shot, in five and at a seventh of the buffer, with a read after every slice."""

    def __init__(self, trace_mod, t0, x0, th0, pi, pj, c):
        self.m, self.pi, self.pj, self.c = trace_mod, pi, pj, c
        self.t, self.x, self.th = np.full(len(x0), float(t0)), np.array(x0, dtype=np.float64), np.array(th0, dtype=np.float64)
        self.S, self.J, self.T = np.zeros(len(pi)), np.zeros(len(x0)), float(t0)
        self.of = [[k for k in range(len(pi)) if i in (pi[k], pj[k])] for i in range(len(x0))]

    def piece(self, k, t):
        i, j = self.pi[k], self.pj[k]
        s0 = max(self.t[i], self.t[j])
        a = (self.x[i] - self.c[i]) + self.th[i] * (s0 - self.t[i])
        b = (self.x[j] - self.c[j]) + self.th[j] * (s0 - self.t[j])
        return self.m._pair_piece(a, b, self.th[i], self.th[j], t - s0)

    def feed(self, events):
        for e in events:
            i, t = int(e["i"]), np.float64(e["t"])
            for k in self.of[i]:
                self.S[k] = self.S[k] + self.piece(k, t)
            self.J[i] = self.J[i] + self.m._line_piece(self.x[i] - self.c[i], self.th[i], t - self.t[i])
            self.t[i], self.x[i], self.th[i], self.T = t, e["x"], e["theta"], float(t)

    def read(self):
        S = np.array([self.S[k] + self.piece(k, np.float64(self.T)) for k in range(len(self.pi))])
        J = np.array([self.J[i] + self.m._line_piece(self.x[i] - self.c[i], self.th[i], np.float64(self.T) - self.t[i]) for i in range(len(self.J))])
        return S, J, self.T


@pytest.mark.parametrize("name", ["few", "on_grid_end", "sticky"])
def test_slicing_and_reading_midway_change_nothing(pkg, name):
    c = CC.case(name)
    pi, pj = np.triu_indices(c.d)
    cen = 0.5 * np.ones(c.d)
    rng = np.random.default_rng(11)
    ev = c.events[0]
    whole = PR.fact(c.t0, c.x0[0], c.th0[0], ev, pi, pj, cen)
    for _ in range(3):
        cuts = np.concatenate([[0], np.sort(rng.integers(0, len(ev) + 1, 6)), [len(ev)]])
        st = Stream(pkg.trace, c.t0, c.x0[0], c.th0[0], pi, pj, cen)
        for a, b in zip(cuts[:-1], cuts[1:]):
            st.feed(ev[a:b])
            S, J, T = st.read()  # a read after every slice: the prefix's integrals, and nothing is disturbed
            ref = PR.fact(c.t0, c.x0[0], c.th0[0], ev[:b], pi, pj, cen)
            assert same_bits(S, ref[0]) and same_bits(J, ref[1]) and T == ref[2]
        again = st.read()
        assert same_bits(again[0], whole[0]) and same_bits(again[1], whole[1]) and again[2] == whole[2]


def test_orientation_and_order_of_the_list(pkg, spdmp8):
    tr = spdmp8[1][1]
    pi, pj = np.tril_indices(8)
    S, J, _ = PR.of_trace(tr, pi, pj)
    S2, J2, _ = PR.of_trace(tr, pj, pi)  # (i, j) and (j, i): the same bits
    perm = np.random.default_rng(0).permutation(len(pi))
    S3, J3, _ = pkg.trace.pair_integrals(tr, pi[perm], pj[perm])
    assert same_bits(S, S2) and same_bits(J, J2) and same_bits(S[perm], S3) and same_bits(J, J3)


# ---------------------------------------------------------------------------------------------- 3. the covariance against Γ⁻¹

def envelope(T):
    return 2.5 / np.sqrt(T)  # test/maintest.jl:33,60


def test_covariance_of_the_oracle_chains_at_d8(pkg, spdmp8):
    """mean|cov − Γ⁻¹| < 2.5/√T = 0.0791 (test/maintest.jl:60), dense pair set, the test's own T = 1000 and c = 0.7 ‖Γ[:, i]‖; 2 oracle chains of
    seed 2 pooled: observed 0.0133 (one chain alone: 0.0195), |mean| 0.0153 < 2/√T."""
    G, traces = spdmp8
    pi, pj = np.tril_indices(8)
    res = [pkg.trace.pair_integrals(tr, pi, pj) for tr in traces]
    S, J, L = (np.array([r[q] for r in res]) for q in range(3))
    cov, mean = pkg.trace.covariance(pi, pj, S, J, L)
    inv = np.linalg.inv(G.toarray())
    dev = np.mean(np.abs(cov.toarray() - inv))
    print("d = 8: mean|cov - inv| = %.4g (envelope %.4g), mean|mean| = %.4g" % (dev, envelope(1000.0), np.mean(np.abs(mean))))
    assert dev < envelope(1000.0) and np.mean(np.abs(mean)) < 2 / np.sqrt(1000.0)
    assert abs(cov - cov.T).max() == 0
    one = pkg.trace.covariance(pi, pj, S, J, L, pooled=False)
    assert len(one) == 2 and np.mean(np.abs(one[0][0].toarray() - inv)) < envelope(1000.0)
    # a centre changes the integrals, not the covariance (to rounding) -- and the mean is shifted back
    cen = np.linspace(-2, 2, 8)
    res = [pkg.trace.pair_integrals(tr, pi, pj, cen) for tr in traces]
    cov2, mean2 = pkg.trace.covariance(pi, pj, *(np.array([r[q] for r in res]) for q in range(3)), center=cen)
    assert np.allclose(cov2.toarray(), cov.toarray(), rtol=0, atol=1e-11) and np.allclose(mean2, mean, rtol=0, atol=1e-12)


def test_variances_of_a_12x12_lattice(pkg):
    """The diagonal of the pooled covariance against diag(Γ⁻¹) of gmrf_precision(12) (mean 1.365), pair set = the pattern of Γ (lower triangle +
    diagonal, 408 pairs), T = 1000, c = ‖Γ[:, i]‖, 8 oracle chains of seed 5 started in stationarity (the lattice's slow modes do not forget a start
    at rand(d) in T = 1000): observed mean|cov_ii − (Γ⁻¹)_ii| = 0.0334 < 2.5/√T = 0.0791."""
    G = pkg.problems.gmrf_precision(12)
    A = sp.coo_matrix(G)
    low = A.row >= A.col
    pi, pj = A.row[low].astype(np.int64), A.col[low].astype(np.int64)
    assert len(pi) == 144 + 2 * 12 * 11
    rng = np.random.default_rng(5)
    c = pkg.problems.column_norms(G)
    X0 = pkg.problems.gmrf_stationary_sample(12, 8, rng)
    S, J, L = [], [], []
    for k in range(8):
        th0 = rng.choice([-1.0, 1.0], 144)
        r = O.spdmp_zigzag(G, None, G, X0[k], th0, c, 1000.0, seed=5 + k)
        s, j, t = pkg.trace.pair_integrals(pkg.FactTrace(None, 0.0, X0[k], th0, r["events"]), pi, pj)
        S.append(s), J.append(j), L.append(t)
    cov, _ = pkg.trace.covariance(pi, pj, np.array(S), np.array(J), np.array(L))
    dev = np.mean(np.abs(cov.diagonal() - np.diag(np.linalg.inv(G.toarray()))))
    print("12 x 12: mean|cov_ii - inv_ii| = %.4g (envelope %.4g)" % (dev, envelope(1000.0)))
    assert dev < envelope(1000.0)
    assert cov.nnz == 144 + 4 * 12 * 11  # symmetric, on the pattern of Γ


# ---------------------------------------------------------------------------------------------- 4. a large centre kills the cancellation

def test_large_centre(pkg, spdmp8):
    """The target shifted by μ = 10^6.  The positions are first rounded to multiples of 2^-30, so that x + μ is exact and the shifted trace IS the
    shift of the unshifted one.  With center = μ every x − c is the unshifted x exactly: S, J and the covariance are the unshifted run's bit for
    bit (so certainly within its bound).  With center = 0 the statement still keeps its own bound -- which is 10^12 times wider: the covariance
    computed from it has lost the digits that S/L − (J/L)² cancels."""
    tr0 = spdmp8[1][0]
    mu, q = 1.0e6, 2.0 ** -30
    ev = tr0.events[:400].copy()
    ev["x"] = np.round(ev["x"] / q) * q
    x0 = np.round(tr0.x0 / q) * q
    base = pkg.FactTrace(None, 0.0, x0, tr0.θ0, ev)
    evs = ev.copy()
    evs["x"] = ev["x"] + mu
    assert np.array_equal(evs["x"] - mu, ev["x"])
    shifted = pkg.FactTrace(None, 0.0, x0 + mu, tr0.θ0, evs)
    pi, pj = np.tril_indices(8)
    _, _, (S0, J0, T) = check(pkg, base, pi, pj)
    _, _, (S1, J1, _) = check(pkg, shifted, pi, pj, np.full(8, mu))  # within its own bound ...
    assert same_bits(S0, S1) and same_bits(J0, J1)  # ... and the unshifted run's bits
    uS, uJ, (S2, J2, _) = check(pkg, shifted, pi, pj, None)  # centre 0: within ITS bound
    cov0 = pkg.trace.covariance(pi, pj, S0, J0, T)[0].toarray()
    cov1, mean1 = pkg.trace.covariance(pi, pj, S1, J1, T, center=np.full(8, mu))
    cov2 = pkg.trace.covariance(pi, pj, S2, J2, T)[0].toarray()
    assert np.array_equal(cov1.toarray(), cov0) and np.allclose(mean1 - mu, J0 / T, rtol=0, atol=1e-9)
    lost = np.abs(cov2 - cov0).max()
    print("centre 0 at mu = 1e6: the covariance is off by %.3g (entries of size %.3g)" % (lost, np.abs(cov0).max()))
    assert lost > 1e6 * np.abs(cov1.toarray() - cov0).max() and lost > 1e-7


# ---------------------------------------------------------------------------------------------- 5. refusals

def test_host_refusals(pkg):
    d = 4
    G = sp.identity(d, format="csc")
    x0, th0 = np.zeros(d), np.ones(d)
    ev = np.array([(1.0, 0, 1.0, -1.0)], dtype=CC.EVENT_DTYPE)
    fb = pkg.FactTrace(pkg.FactBoomerang(G, np.zeros(d), 0.1), 0.0, x0, th0, ev)
    bo = pkg.PDMPTrace(pkg.Boomerang(G, np.zeros(d), 0.1), 0.0, x0, th0, np.array([1.0]), np.ones((1, d)), np.ones((1, d)))
    for tr in (fb, bo):
        with pytest.raises(TypeError, match="Boomerang"):
            pkg.trace.pair_integrals(tr, [0], [0])
    tr = pkg.FactTrace(None, 0.0, x0, th0, ev)
    for pi, pj, word in (([], [], "at least one"), ([0, 1], [0], "one entry each"), ([0], [d], "outside"), ([-1], [0], "outside"),
                         ([0, 1, 0], [1, 2, 1], "twice"), ([0, 1], [1, 0], "twice")):
        with pytest.raises(ValueError, match=word):
            pkg.trace.pair_integrals(tr, pi, pj)
    for cen in (np.zeros(d + 1), np.array([0.0, np.inf, 0.0, 0.0]), np.array([np.nan, 0.0, 0.0, 0.0])):
        with pytest.raises(ValueError, match="centre"):
            pkg.trace.pair_integrals(tr, [0], [1], cen)
    S, J, T = pkg.trace.pair_integrals(tr, [0, 0], [0, 1])  # a trace the contract can be read off: x_0 = t on [0, 1], x_1 = t
    assert same_bits(S, [1 / 3.0, 1 / 3.0]) and same_bits(J, [0.5, 0.5, 0.5, 0.5]) and T == 1.0
