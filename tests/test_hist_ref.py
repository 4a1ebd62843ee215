"""The marginal histograms (occupation times per bin) without a device: the sequential C statement of the contract (tests/ref/hist_ref.c) on
values worked out by hand, its invariant Σ_k H[k] = T_last − t0 on the hand-made traces of the three case tables, the host mirror
trace.marginal_histogram against it, and trace.histogram_quantiles on a hand-made H."""
import numpy as np
import pytest
import scipy.sparse as sp

import barrier_consumer_cases as BC
import consumer_cases as CC
import hist_ref_lib as HR
import pdmp_consumer_cases as PC

EV = HR.EVENT_DTYPE


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------------------------------------- 1. hand values

def test_a_unit_line_over_four_bins():
    """x = t on [0, 1], 4 bins on [0, 1]: 0.25 each, nothing outside (the end x = 1 = hi touches the upper slot for no time)"""
    ev = np.array([(1.0, 0, 1.0, -1.0)], dtype=EV)
    H, Z, T = HR.fact(0.0, [0.0], [1.0], ev, [0], 0.0, 1.0, 4)
    assert same_bits(H, [[0.0, 0.25, 0.25, 0.25, 0.25, 0.0]]) and same_bits(Z, [0.0]) and T == 1.0
    H, Z, T = HR.pdmp(0.0, [0.0], [1.0], [1.0], [[1.0]], [[-1.0]], [0], 0.0, 1.0, 4)
    assert same_bits(H, [[0.0, 0.25, 0.25, 0.25, 0.25, 0.0]]) and same_bits(Z, [0.0]) and T == 1.0


def test_a_piece_that_leaves_through_both_outer_slots():
    """x from −1 to 3 in 4 time units (speed 1), 2 bins on [0, 2]: 1 below, 1 in each bin, 1 above; and the same piece travelled downwards"""
    H, Z = HR.piece(0.0, 2.0, 2, -1.0, 1.0, 4.0)
    assert same_bits(H, [1.0, 1.0, 1.0, 1.0]) and Z == 0.0
    H, Z = HR.piece(0.0, 2.0, 2, 3.0, -1.0, 4.0)
    assert same_bits(H, [1.0, 1.0, 1.0, 1.0]) and Z == 0.0
    H, Z = HR.piece(0.0, 2.0, 2, -1.0, 2.0, 2.0)  # twice the speed: half the time everywhere
    assert same_bits(H, [0.5, 0.5, 0.5, 0.5])


def test_rest_pieces_on_the_edges():
    """at rest at x == lo: bin 0; at x == hi: the upper slot; at −0.0 with lo = 0: bin 0 (−0.0 counts as 0); θ = 0 adds to Z, b == a alone not"""
    assert same_bits(HR.piece(0.0, 1.0, 4, 0.0, 0.0, 2.0)[0], [0, 2.0, 0, 0, 0, 0]) and HR.piece(0.0, 1.0, 4, 0.0, 0.0, 2.0)[1] == 2.0
    assert same_bits(HR.piece(0.0, 1.0, 4, 1.0, 0.0, 2.0)[0], [0, 0, 0, 0, 0, 2.0])
    assert same_bits(HR.piece(0.0, 1.0, 4, -0.0, 0.0, 2.0)[0], [0, 2.0, 0, 0, 0, 0])
    assert same_bits(HR.piece(0.0, 1.0, 4, -0.0, -0.0, 2.0)[0], [0, 2.0, 0, 0, 0, 0]) and HR.piece(0.0, 1.0, 4, -0.0, -0.0, 2.0)[1] == 2.0
    assert same_bits(HR.piece(-1.0, 1.0, 4, -0.0, 0.0, 2.0)[0], [0, 0, 0, 2.0, 0, 0])  # an inner edge: the bin above it
    H, Z = HR.piece(0.0, 1.0, 4, 0.5, 1e-300, 1.0)  # moves, but a + v·τ == a after rounding: at rest for the bins, not for Z
    assert same_bits(H, [0, 0, 0, 1.0, 0, 0]) and Z == 0.0
    for tau in (0.0, -1.0, float("nan")):  # τ <= 0 adds nothing
        H, Z = HR.piece(0.0, 1.0, 4, 0.5, 1.0, tau)
        assert same_bits(H, np.zeros(6)) and Z == 0.0


def test_a_piece_ending_exactly_on_an_edge():
    """x from 0.125 to 0.5 = e_2 of 4 bins on [0, 1]: bins 0 and 1 only (bin 2 is touched for no time); downwards from the edge the same"""
    H, _ = HR.piece(0.0, 1.0, 4, 0.125, 0.375, 1.0)
    assert same_bits(H, [0, 0.125 / 0.375, 0.25 / 0.375, 0, 0, 0])
    H, _ = HR.piece(0.0, 1.0, 4, 0.5, -0.375, 1.0)
    assert same_bits(H, [0, 0.125 / 0.375, 0.25 / 0.375, 0, 0, 0])
    H, _ = HR.piece(0.0, 1.0, 4, 0.5, 0.5, 1.0)  # from the edge e_2 up to hi
    assert same_bits(H, [0, 0, 0, 0.5, 0.5, 0])


def test_one_bin():
    H, Z = HR.piece(-1.0, 1.0, 1, -2.0, 1.0, 4.0)
    assert same_bits(H, [1.0, 2.0, 1.0])
    assert [HR.bin_of(-1.0, 1.0, 1, x) for x in (-1.5, -1.0, 0.0, 1.0, 2.0)] == [-1, 0, 0, 1, 1]


@pytest.mark.parametrize("B", [1, 3, 63, 64, 65, 4096])
def test_bin_of_against_the_computed_edges(B):
    """e_k <= x < e_k+1 for points on, just below and just above every edge, for ranges whose width is no dyadic number"""
    for lo, hi in ((0.0, 1.0), (-0.7, 0.3), (0.1, 3.7e5), (-1e-3, 2e-3)):
        E = np.array([HR.edge(lo, hi, B, k) for k in range(B + 1)])
        assert E[0] == lo and E[-1] == hi and np.all(np.diff(E) > 0)
        step = max(1, B // 97)
        for k in list(range(0, B + 1, step)) + [B]:
            for x in (np.nextafter(E[k], -np.inf), E[k], np.nextafter(E[k], np.inf)):
                j = HR.bin_of(lo, hi, B, x)
                assert -1 <= j <= B
                assert (j == -1 or HR.edge(lo, hi, B, j) <= x) and (j == B or x < HR.edge(lo, hi, B, j + 1)), (lo, hi, k, x, j)
    assert HR.edge(0.0, 1.0, B, -1) == -np.inf and HR.edge(0.0, 1.0, B, B + 1) == np.inf


# ---------------------------------------------------------------------------------------------- 2. the invariant and the host mirror on the case tables

def fact_trace(pkg, c, k):
    return pkg.FactTrace(None, c.t0, c.x0[k], c.th0[k], c.events[k])


def pdmp_trace(pkg, c, k):
    return pkg.PDMPTrace(None, c.t0, c.x0[k], c.th0[k], c.t[k], c.x[k], c.th[k], f0=None, f=c.f[k] if c.sticky else None)


def check(pkg, tr, coords, lo, hi, B):
    """Σ_k H[k] = T_last − t0 within 1e-12·(T_last − t0)·(number of pieces), Z <= Σ_k H[k]; trace.marginal_histogram within the same bound"""
    H, Z, T, npieces = HR.of_trace(tr, coords, lo, hi, B, pieces=True)
    L = T - tr.t0
    tol = 1e-12 * L * max(npieces, 1)
    assert np.all(H >= 0) and np.all(np.abs(H.sum(axis=1) - L) <= tol), (np.abs(H.sum(axis=1) - L).max(), tol)
    assert np.all(Z <= H.sum(axis=1) + tol) and np.all(Z >= 0)
    H2, Z2, T2 = pkg.trace.marginal_histogram(tr, coords, lo, hi, B)
    assert T2 == T and np.all(np.abs(H2 - H) <= tol) and np.all(np.abs(Z2 - Z) <= tol)
    return H, Z, T


def spread(values, margin):
    """a range that keeps everything inside (margin > 0) or cuts both tails off (margin < 0)"""
    a, b = float(np.min(values)), float(np.max(values))
    w = max(b - a, 1.0)
    return a - margin * w, b + margin * w


@pytest.mark.parametrize("name", CC.NAMES)
def test_fact_case_table(pkg, name):
    c = CC.case(name)
    rng = np.random.default_rng(3)
    coords = rng.permutation(c.d)[:min(c.d, 12)]
    for k in range(c.nchains):
        tr = fact_trace(pkg, c, k)
        allx = np.concatenate([c.x0[k], c.events[k]["x"]])
        for B, margin in ((1, 0.1), (7, -0.2), (64, 0.1), (65, -0.3)):
            lo, hi = spread(allx, margin)
            H, Z, _ = check(pkg, tr, coords, lo, hi, B)
        if name == "sticky":
            assert Z.max() > 0  # θ = 0 pieces


@pytest.mark.parametrize("name", [n for n in PC.NAMES if not n.startswith("boom")])
def test_pdmp_case_table(pkg, name):
    c = PC.case(name)
    rng = np.random.default_rng(4)
    coords = rng.permutation(c.d)[:min(c.d, 9)]
    for k in range(c.nchains):
        tr = pdmp_trace(pkg, c, k)
        allx = np.concatenate([c.x0[k], np.asarray(c.x[k]).reshape(-1)]) if len(c.t[k]) else c.x0[k]
        for B, margin in ((1, 0.1), (63, -0.2), (65, 0.1)):
            lo, hi = spread(allx, margin)
            check(pkg, tr, coords, lo, hi, B)


def test_barrier_case_table(pkg):
    """the barrier ZigZag's table from the start (t0, x0, θ_eff): the frozen times written out by hand there are the rest times Z, and a frozen
    coordinate's time lies in the bin of its barrier"""
    lo, hi = np.array([-1.0, -0.5, 0.0, -1.0]), np.array([2.0, 1.5, 1.0, 1.0])
    for k in range(BC.NCHAINS):
        th_eff, _ = pkg.trace.barrier_start(BC.X0[k], BC.TH0[k], BC.BARRIERS)
        assert np.array_equal(th_eff, BC.TH_EFF[k])
        tr = pkg.FactTrace(None, BC.T0, BC.X0[k], th_eff, BC.EVENTS[k])
        H, Z, T = check(pkg, tr, None, lo, hi, 4)
        assert T == BC.T_LAST[k] and same_bits(Z, BC.FROZEN_LO[k] + BC.FROZEN_HI[k])
        if k == 0:  # coordinate 1 starts frozen on its upper barrier 1.5 = hi for 1.5 time units: the slot at or above hi; 3 sits on −1 = lo: bin 0
            assert H[1, 5] >= 1.5 and H[3, 1] >= 2.75 and H[3, 0] == 0


def test_reading_midway_is_the_contract_on_the_trace_so_far(pkg):
    """the accumulated pieces plus the open one: a prefix of the trace is a trace"""
    c = CC.case("few")
    lo, hi = spread(np.concatenate([c.x0[0], c.events[0]["x"]]), -0.1)
    for upto in range(len(c.events[0]) + 1):
        tr = pkg.FactTrace(None, c.t0, c.x0[0], c.th0[0], c.events[0][:upto])
        check(pkg, tr, None, lo, hi, 5)


def test_pool_is_the_chain_ordered_sum():
    rows = np.array([[0.1, 1e16], [0.2, -1e16], [0.3, 1.0]])
    assert same_bits(HR.pool(rows), [(0.0 + 0.1 + 0.2) + 0.3, ((0.0 + 1e16) - 1e16) + 1.0])


# ---------------------------------------------------------------------------------------------- 3. quantiles, refusals of the host mirror

def test_histogram_quantiles_on_a_hand_made_H(pkg):
    q = pkg.trace.histogram_quantiles
    H = np.array([0.0, 1.0, 1.0, 2.0, 0.0, 0.0])  # 4 bins on [0, 4): mass 1, 1, 2, 0
    assert q(H, 0.0, 4.0, 0.5) == 2.0 and q(H, 0.0, 4.0, 0.25) == 1.0 and q(H, 0.0, 4.0, 0.75) == 2.5 and q(H, 0.0, 4.0, 0.125) == 0.5
    assert np.array_equal(q(H, 0.0, 4.0, [0.0, 1.0]), [0.0, 3.0])
    Hout = np.array([1.0, 1.0, 0.0, 0.0, 0.0, 2.0])  # a quarter below lo, half at or above hi
    r = q(Hout, 0.0, 4.0, [0.1, 0.25, 0.375, 0.5, 0.9])
    assert np.isnan(r[0]) and r[1] == 0.0 and r[2] == 0.5 and r[3] == 1.0 and np.isnan(r[4])
    two = q(np.stack([H, Hout]), [0.0, 0.0], [4.0, 4.0], [0.5])  # one row per coordinate
    assert two.shape == (2, 1) and two[0, 0] == 2.0 and two[1, 0] == 1.0
    chains = q(np.stack([np.stack([H, Hout])] * 3), 0.0, 4.0, 0.5)  # [chains x m x (B + 2)]
    assert chains.shape == (3, 2) and np.array_equal(chains[:, 0], [2.0] * 3)
    assert np.isnan(q(np.zeros(6), 0.0, 4.0, 0.5))
    assert np.array_equal(pkg.trace.histogram_edges([0.0, -1.0], [4.0, 1.0], 4), [[0, 1, 2, 3, 4], [-1, -0.5, 0, 0.5, 1]])


def test_the_median_of_a_symmetric_path(pkg):
    """a triangle wave between −1 and 1: the median is 0, the quartiles ∓0.5, whatever the bin count"""
    t = np.arange(1, 9, dtype=np.float64) * 2.0
    ev = np.array([(tk, 0, 1.0 if k % 2 == 0 else -1.0, -1.0 if k % 2 == 0 else 1.0) for k, tk in enumerate(t)], dtype=EV)
    tr = pkg.FactTrace(None, 0.0, np.array([-1.0]), np.array([1.0]), ev)
    for B in (2, 7, 64):
        H, Z, T = pkg.trace.marginal_histogram(tr, [0], -1.0, 1.0, B)
        assert np.allclose(pkg.trace.histogram_quantiles(H, -1.0, 1.0, [0.25, 0.5, 0.75]), [[-0.5, 0.0, 0.5]], atol=1e-12)


def test_host_refusals(pkg):
    d = 3
    G = sp.identity(d, format="csc")
    x0, th0 = np.zeros(d), np.ones(d)
    ev = np.array([(1.0, 0, 1.0, -1.0)], dtype=EV)
    fb = pkg.FactTrace(pkg.FactBoomerang(G, np.zeros(d), 0.1), 0.0, x0, th0, ev)
    bo = pkg.PDMPTrace(pkg.Boomerang(G, np.zeros(d), 0.1), 0.0, x0, th0, np.array([1.0]), np.ones((1, d)), np.ones((1, d)))
    for tr in (fb, bo):
        with pytest.raises(TypeError, match="arc"):
            pkg.trace.marginal_histogram(tr, [0], 0.0, 1.0, 4)
    tr = pkg.FactTrace(None, 0.0, x0, th0, ev)
    for bad in (([0, 0], 0.0, 1.0, 4), ([3], 0.0, 1.0, 4), ([], 0.0, 1.0, 4), ([0], 1.0, 1.0, 4), ([0], 0.0, np.inf, 4), ([0], 0.0, 1.0, 0),
                ([0], 0.0, 1.0, 4097)):
        with pytest.raises(ValueError):
            pkg.trace.marginal_histogram(tr, *bad)
