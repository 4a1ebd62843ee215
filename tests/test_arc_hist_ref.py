"""The marginal histograms of a Boomerang's arcs without a device: the sequential C statement of the contract (tests/ref/arc_hist_ref.c), the
exact occupation with mpmath and the bound derived from the inputs alone (tests/exact_arc_hist.py) -- which the statement keeps on every prefix
the device test reads at, and a statement with ψ0 of the opposite sign does not --, the host mirror trace.arc_marginal_histogram inside the same
bound, the invariants, the rest piece's bits against the line contract, the table's distance from tangencies, and the mirror's refusals.

Used fraction of the derived bound, the C statement on every entry (largest over chains, prefixes, coordinates and slots), as printed by
test_statement_keeps_the_derived_bound: boom_62 0.00975, boom_sticky_63 0.0901, d1_1 0.0027, d1_2 0.00218, d1_4096 0.00774, sticky130_all 0.0369,
sticky130_126 0.0235, edge_127 0.0138, sticky130_127 0.0235, sticky130_4096 0.0165, rest0_127 0.15, two_63 0.0175, d1_inside 0.00177, edge_never 0, d1_onebin 0, rest0 0.15, tangent 0.0173.  The bounds
themselves are between 9e-15 and 1.1e-11 per slot; the statement with ψ0 of the opposite sign is 1e11 to 1e13 bounds away on every prefix in
which a moving coordinate with p != 0 has crossed an edge."""
import numpy as np
import pytest
import scipy.sparse as sp
from mpmath import mp, mpf

import arc_hist_cases as HC
import arc_hist_ref_lib as AH
import exact_arc_hist as EX
import hist_ref_lib as HR


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def trace_of(pkg, c, k, upto=None):
    B = pkg.Boomerang(sp.identity(c.d, format="csc"), c.mu, 1.0)
    f = c.f[k][:upto] if c.sticky else None
    return pkg.PDMPTrace(B, c.t0, c.x0[k], c.th0[k], c.t[k][:upto], c.x[k][:upto], c.th[k][:upto], f0=None, f=f)


_exact = {}


def exact(name, k):
    """({prefix length: (H, Z, bound_H, bound_Z)}, the table's facts) of chain k of an entry: computed once, shared, read-only"""
    if (name, k) not in _exact:
        c, coords, lo, hi, bins = HC.listed(name)
        cuts = set(c.cuts[k][s + 1] for s in range(c.nseg))
        _exact[(name, k)] = EX.exact_hist(c.t0, c.x0[k], c.th0[k], c.t[k], c.x[k], c.th[k], c.mu, coords, lo, hi, bins, cuts,
                                          f=c.f[k] if c.sticky else None)
    return _exact[(name, k)]


def worst_used(H, Z, ex):
    eH, eZ, bH, bZ = ex[:4]
    return max(max(EX.used(H[a, q], eH[a][q], bH[a][q]) for a in range(H.shape[0]) for q in range(H.shape[1])),
               max(EX.used(Z[a], eZ[a], bZ[a]) for a in range(H.shape[0])))


@pytest.mark.parametrize("name", HC.NAMES)
def test_statement_keeps_the_derived_bound(name, capsys):
    c, coords, lo, hi, bins = HC.listed(name)
    worst = 0.0
    for k in range(c.nchains):
        out, (gap, tangencies, crossing) = exact(name, k)
        for s in range(c.nseg):
            H, Z, T = HC.reference(name, k, s)
            upto = c.cuts[k][s + 1]
            assert T == (c.t[k][upto - 1] if upto else c.t0)
            worst = max(worst, worst_used(H, Z, out[upto]))
            # the same statement with ψ0 of the opposite sign is outside it, on every prefix, wherever the sign can matter -- a free coordinate
            # with p != 0 has crossed an edge --: the bound tells the two apart; elsewhere (no edge crossed yet, or p = 0 where ψ0 = ∓0) the two
            # statements are the same function of the inputs and return the same bits, which shows nothing about the sign
            t, x, th, f = c.so_far(k, s)
            Hw, Zw, _ = AH.arcs(c.t0, c.x0[k], c.th0[k], t, x, th, c.mu, coords, lo, hi, bins, f=f, wrong=True)
            if out[upto][4]:
                assert worst_used(Hw, Zw, out[upto]) > 1.0, (k, s)
            else:
                assert same_bits(Hw, H), (k, s)
    with capsys.disabled():
        print("\n  %s: the statement uses %.3g of the bound" % (name, worst), end="")
    assert worst < 1.0, worst


@pytest.mark.parametrize("name", HC.NAMES)
def test_table_keeps_clear_of_tangencies(name):
    """a property of the inputs: apart from the exact tangencies of `tangent` every (piece, edge) has 1 − |ẑ| >= 2^-20 or |ẑ| > 1, so the
    conditioning term of the bound stays small and the bound can tell a right form from a wrong one"""
    c = HC.listed(name)[0]
    for k in range(c.nchains):
        gap, tangencies, crossing = exact(name, k)[1]
        assert gap >= mpf(2) ** -20, float(gap)
        assert tangencies == (2 if name == "tangent" else 0)  # (the edges −1.0 and 1.0 of its one piece)


def test_tangent_slots_by_hand():
    """μ = 0, u = 1, p = 0 over a quarter, a half and a whole turn, 4 bins on [−1, 1): multiples of π/6 (up to τ̂ being the double next to π/2, π
    and 2π: within 2^-51 of them, and the slots move by no more than that)"""
    c = HC.case("tangent")
    for k in range(3):
        eH = exact("tangent", k)[0][1][0][0]
        H = HC.reference("tangent", k, 0)[0][0]
        for q in range(6):
            assert abs(eH[q] - HC.TANGENT_SLOTS[k][q] * mp.pi / 6) <= mpf(2) ** -51
            assert (H[q] == 0.0) == (HC.TANGENT_SLOTS[k][q] == 0)  # (nothing outside [−1, 1): the tangencies are exact)


@pytest.mark.parametrize("name", HC.NAMES)
def test_invariants(name):
    """Σ_k H[k] = the summed positive τ (T_last − t0 where the times increase: every entry but `edge`'s) within the summed bounds; Z <= Σ_k H[k]"""
    c, coords, lo, hi, bins = HC.listed(name)
    for k in range(c.nchains):
        out = exact(name, k)[0]
        for s in range(c.nseg):
            H, Z, T = HC.reference(name, k, s)
            upto = c.cuts[k][s + 1]
            eH, eZ, bH, bZ = out[upto][:4]
            ts = np.concatenate([[c.t0], c.t[k][:upto]])
            total = sum((mpf(float(b)) - mpf(float(a)) for a, b in zip(ts[:-1], ts[1:]) if b > a), mpf(0))
            if not c.name.startswith("edge"):
                assert total == mpf(float(T)) - mpf(float(c.t0))
            for a in range(len(coords)):
                assert abs(sum(mpf(float(v)) for v in H[a]) - total) <= sum(bH[a])
                assert Z[a] <= H[a].sum() * (1 + (bins + 2) * 2.0 ** -53)  # (the sum here rounds at most bins + 2 times)
                assert abs(sum(eH[a]) - total) < mpf(10) ** -30


def test_rest_piece_has_the_bits_of_the_line_contracts():
    rng = np.random.default_rng(5)
    for lo, hi, bins in ((-1.0, 1.5, 1), (-2.0, 2.0, 7), (0.1, 0.7, 64), (-3.0, 3.0, 4096)):
        H0, Z0 = rng.uniform(0, 3, bins + 2), 0.37
        for a in list(rng.uniform(lo - 1, hi + 1, 12)) + [lo, hi, -0.0, HR.edge(lo, hi, bins, bins // 2)]:
            for tau in (1.7, 1e-9, 0.0, -0.3, float("nan")):
                want = HR.piece(lo, hi, bins, a, 0.0, tau, H=H0, Z=Z0)
                got = AH.piece(lo, hi, bins, a, rng.standard_normal(), False, 0.3, tau, H=H0, Z=Z0)  # not free: whatever θ and μ are
                got2 = AH.piece(lo, hi, bins, a, 0.0, True, a, tau, H=H0, Z=Z0)  # free with u = p = 0
                assert same_bits(got[0], want[0]) and got[1] == want[1] and same_bits(got2[0], want[0]) and got2[1] == want[1]


@pytest.mark.parametrize("name", HC.NAMES)
def test_mirror_inside_the_bound(pkg, name):
    """trace.arc_marginal_histogram (numpy's arctan2 and arccos: within the header's stated errors) on every prefix the device test reads at"""
    c, coords, lo, hi, bins = HC.listed(name)
    for k in range(c.nchains):
        out = exact(name, k)[0]
        for s in range(c.nseg):
            upto = c.cuts[k][s + 1]
            H, Z, T = pkg.trace.arc_marginal_histogram(trace_of(pkg, c, k, upto), coords, lo, hi, bins)
            assert T == HC.reference(name, k, s)[2] and worst_used(H, Z, out[upto]) < 1.0


def test_mean_from_the_histogram_and_from_the_pair_integrals(pkg):
    """with the range covering the path and nothing in the outer slots, each bin's mass sits within w/2 of its midpoint:
    |Σ_k mid_k·H[k] − ∫ x_i dt| <= (w/2)·Σ_k H[k], and with the floats' own bounds on both sides
    |Σ_k mid_k·H[k] − J_i| <= Σ_k (w_k/2)·Ĥ[k] + Σ_k |mid_k|·bound_H[k] + bound_J[i]   (J_i from trace.arc_pair_integrals, centre 0).
    A derived inequality, not a tolerance."""
    import exact_arc_pairs as EA
    c = HC.case("two")
    coords, bins = np.arange(c.d), 63
    lo, hi = np.full(c.d, -7.0), np.full(c.d, 7.0)
    E = [EX.edges_of(lo[0], hi[0], bins)] * c.d
    for k in range(c.nchains):
        tr = trace_of(pkg, c, k)
        H, Z, T = AH.of_trace(tr, coords, lo, hi, bins)
        assert np.all(H[:, 0] == 0) and np.all(H[:, -1] == 0)
        n = len(c.t[k])
        eH, eZ, bH, bZ = EX.exact_hist(c.t0, c.x0[k], c.th0[k], c.t[k], c.x[k], c.th[k], c.mu, coords, lo, hi, bins, {n})[0][n][:4]
        S, J, _ = pkg.trace.arc_pair_integrals(tr, [0], [0])
        bJ = EA.of_trace(tr, [0], [0])[3]
        for i in range(c.d):
            mid = [(mpf(E[i][q]) + mpf(E[i][q + 1])) / 2 for q in range(bins)]
            lhs = abs(sum(mid[q] * mpf(float(H[i, q + 1])) for q in range(bins)) - mpf(float(J[i])))
            half = [(mpf(E[i][q + 1]) - mpf(E[i][q])) / 2 for q in range(bins)]  # (w/2 of each bin, from the computed edges)
            rhs = sum(half[q] * eH[i][q + 1] for q in range(bins)) + sum(abs(mid[q]) * bH[i][q + 1] for q in range(bins)) + bJ[i]
            assert lhs <= rhs, (i, float(lhs), float(rhs))


def test_mirror_refusals_and_arguments(pkg):
    d = 3
    G = sp.identity(d, format="csc")
    x0, th0 = np.zeros(d), np.ones(d)
    ev = np.array([(1.0, 0, 1.0, -1.0)], dtype=pkg._lib.EVENT_DTYPE)
    one = (np.array([1.0]), np.ones((1, d)), np.ones((1, d)))
    others = [pkg.FactTrace(pkg.FactBoomerang(G, np.zeros(d), 0.1), 0.0, x0, th0, ev), pkg.FactTrace(None, 0.0, x0, th0, ev),
              pkg.FactTrace(pkg.ZigZag(G, np.zeros(d)), 0.0, x0, th0, ev),
              pkg.PDMPTrace(pkg.BouncyParticle(G, np.zeros(d), 1.0), 0.0, x0, th0, *one), pkg.PDMPTrace(None, 0.0, x0, th0, *one)]
    for tr in others:
        with pytest.raises(TypeError, match="Boomerang"):
            pkg.trace.arc_marginal_histogram(tr, [0], 0.0, 1.0, 4)
    tr = pkg.PDMPTrace(pkg.Boomerang(G, np.zeros(d), 0.1), 0.0, x0, th0, *one)
    with pytest.raises(TypeError, match="arc"):  # ... and the line mirror keeps refusing this one
        pkg.trace.marginal_histogram(tr, [0], 0.0, 1.0, 4)
    for args, word in ((([], 0.0, 1.0, 4), "at least one"), (([d], 0.0, 1.0, 4), "at least one"), (([0, 0], 0.0, 1.0, 4), "each once"),
                       (([0], 0.0, 1.0, 0), "4096"), (([0], 0.0, 1.0, 4097), "4096"), (([0], 1.0, 1.0, 4), "lo < hi"),
                       (([0], 0.0, np.inf, 4), "finite")):
        with pytest.raises(ValueError, match=word):
            pkg.trace.arc_marginal_histogram(tr, *args)
    H, Z, T = pkg.trace.arc_marginal_histogram(pkg.PDMPTrace(tr.F, 0.0, x0, th0, np.empty(0), np.empty((0, d)), np.empty((0, d))), None, 0.0, 1.0, 4)
    assert same_bits(H, np.zeros((d, 6))) and same_bits(Z, np.zeros(d)) and T == 0.0  # no event: nothing to count
    Q = pkg.trace.histogram_quantiles(pkg.trace.arc_marginal_histogram(tr, None, -2.0, 2.0, 8)[0], -2.0, 2.0, 0.5)  # used unchanged
    assert Q.shape == (d,) and np.all(np.isfinite(Q))
