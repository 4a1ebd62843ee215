"""The marginal histograms of a Boomerang's arcs on the device (pdmp_ensemble_bps_consume_arc_hist, read by pdmp_ensemble_bps_consume_histogram;
bps_arc_hist_kernel of csrc/pdmp_consume_bps.hip; -m gpu) against the sequential statement of their contract, tests/ref/arc_hist_ref.c, BIT FOR
BIT (H, Z and T_last, per chain and pooled):

  1. every entry of tests/arc_hist_cases.py through pdmp_debug_bps_trace_append, segment by segment with a bps_consume() and a read after each --
     rows of 3, 4, 64, 65, 128 (registers), 129 and 4098 (global memory; sticky and not, with pieces at rest) slots, m = 1, 5 and all of d = 130, trace buffers smaller than the trace,
     a segment grown in place, a chain without events in a slice --, each run twice and equal to itself;
  2. the ordinary consumers and the arc pairs of an ensemble with the list return the bytes they return without it;
  3. every refusal, by status and by the word in the message; both old refusals (bps_consume_hist, trace.marginal_histogram) still in place;
  4. pdmp / sspdmp on a Boomerang at d = 8 with consume=dict(hist=...): a buffer for the whole run and one of 48 events give identical bytes,
     equal to the C statement on the returned trace;
  5. the pooled median of a standard-normal target lies in the bin of 0."""
import numpy as np
import pytest
import scipy.sparse as sp

import arc_hist_cases as HC
import arc_hist_ref_lib as AH
import hist_ref_lib as HR

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def open_case(pkg, c):
    """A Boomerang ensemble in the state of case c, bps_consume_begin done (a sticky one holds the event its set_state_bps wrote)"""
    L = pkg._lib
    G = sp.identity(c.d, format="csc")
    ens = pkg.Ensemble(c.nchains, c.d, sampler=L.SAMPLER_BPS, factor=2.0, trace_capacity=c.trace_capacity)
    ens.set_flow_boomerang(pkg.GaussianTarget(G, c.mu), pkg.Boomerang(G, c.mu, 1.0))
    if c.sticky:
        ens.set_bps_sticky(np.full(c.d, 0.8))
    ens.set_state_bps(c.t0, c.x0, c.th0, 10.0, np.arange(c.nchains, dtype=np.uint64) + 1)
    ens.bps_consume_begin(c.dt, c.K)
    return ens


def walk(pkg, name, with_hist, with_pairs=True):
    """the entry fed segment by segment; returns (the reads of the histogram after every segment, what the other consumers returned)"""
    c, coords, lo, hi, bins = HC.listed(name)
    reads, got = [], []
    with open_case(pkg, c) as ens:
        ens.bps_consume_cummean(True)
        if with_pairs:
            ens.bps_consume_arc_pairs(*(([0], [0]) if c.d == 1 else ([0, c.d - 1], [0, 0])))
        if with_hist:
            ens.bps_consume_arc_hist(coords, lo, hi, bins)
        held = [0] * c.nchains
        for s in range(c.nseg):
            for k in range(c.nchains):
                t, x, th, f = c.segment(k, s)
                if not (c.sticky and s == 0):  # (a sticky ensemble holds the event its set_state_bps wrote: the case's first segment)
                    ens.debug_bps_trace_append(k, t, x, th, f)
            ens.bps_consume()
            if with_hist:
                reads.append((ens.bps_consume_histogram(), ens.bps_consume_histogram(pooled=True)))
                assert all(same_bits(a, b) for a, b in zip(ens.bps_consume_histogram(), reads[-1][0]))  # (a read disturbs nothing)
            for k in range(c.nchains):
                n = c.cuts[k][s + 1] - c.cuts[k][s]
                if n:
                    got.append(ens.bps_consume_cummean_rows(k, n, first=held[k]))
            if s in c.grow:
                held = [held[k] + c.cuts[k][s + 1] - c.cuts[k][s] for k in range(c.nchains)]
            else:
                ens.trace_reset()
                held = [0] * c.nchains
        got.append(ens.bps_consume_mean()[0])
        if with_pairs:
            got += list(ens.bps_consume_pair_integrals())
        if c.sticky:
            got.append(ens.bps_consume_inclusion()[0])
        if c.K > 0:
            got += [ens.bps_consume_discretized(k)[1] for k in range(c.nchains)]
    return reads, got


@pytest.mark.parametrize("name", HC.NAMES)
def test_hand_made_traces(gpu_pkg, name):
    """after every segment H, Z and T_last are the contract's on the trace so far, per chain and pooled; a second run returns the same bytes;
    mean, cummean, the grid, the free-time fractions and the arc pairs are byte for byte those of an ensemble without the list"""
    pkg = gpu_pkg
    c, coords, lo, hi, bins = HC.listed(name)
    reads, got = walk(pkg, name, True)
    assert len(reads) == c.nseg
    for s, ((H, Z, T), (Hp, Zp, Tp)) in enumerate(reads):
        assert H.shape == (c.nchains, len(coords), bins + 2)
        for k in range(c.nchains):
            ref = HC.reference(name, k, s)
            assert same_bits(H[k], ref[0]), (s, k, np.argwhere(H[k] != ref[0])[:4])
            assert same_bits(Z[k], ref[1]) and T[k] == ref[2], (s, k)
        assert same_bits(Hp, HR.pool(H)) and same_bits(Zp, HR.pool(Z)) and same_bits(Tp, T)
    again, got2 = walk(pkg, name, True)
    assert all(same_bits(a, b) for ra, rb in zip(reads, again) for pa, pb in zip(ra, rb) for a, b in zip(pa, pb))
    _, plain = walk(pkg, name, False)
    assert len(got) == len(plain) == len(got2) and all(same_bits(a, b) for a, b in zip(got, plain)) and all(same_bits(a, b) for a, b in zip(got, got2))


def refused(L, code, word, call, *a):
    with pytest.raises(L.PdmpError) as ei:
        call(*a)
    assert ei.value.code == code and word in str(ei.value), str(ei.value)


def test_refusals(gpu_pkg):
    pkg = gpu_pkg
    L = pkg._lib
    INV, UNS = L.PDMP_ERR_INVALID, L.PDMP_ERR_UNSUPPORTED
    d = 8
    G = sp.identity(d, format="csc")
    one = np.zeros(1, dtype=np.int64)
    lo1, hi1 = np.zeros(1), np.ones(1)

    def bps(flow="boom", begin=True, subsample=False):
        ens = pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, factor=2.0, trace_capacity=8)
        if flow == "boom":
            ens.set_flow_boomerang(pkg.GaussianTarget(G, np.zeros(d)), pkg.Boomerang(G, np.zeros(d), 1.0))
        elif flow == "modern":
            ens.set_flow_bps_modern(1.0)
            ens.set_target(pkg.GaussianTarget(G, np.zeros(d)))
        else:
            ens.set_flow_bps(pkg.BouncyParticle(G, np.zeros(d), 1.0))
        if subsample:
            ens.set_bps_options(False, True)
        ens.set_state_bps(0.0, np.zeros((1, d)), np.ones((1, d)), 10.0, np.array([1], dtype=np.uint64))
        if begin:
            ens.bps_consume_begin()
        return ens

    with bps() as ens:
        h, raw, raw_read = ens._h, ens._L.pdmp_ensemble_bps_consume_arc_hist, ens._L.pdmp_ensemble_bps_consume_histogram
        err = lambda: L.load().pdmp_last_error().decode()
        hist = ens.bps_consume_arc_hist
        p1, pl, ph = one.ctypes.data, lo1.ctypes.data, hi1.ctypes.data
        assert raw(h, 0, p1, pl, ph, 4) == INV and "m = 0" in err()
        assert raw(h, 1, None, pl, ph, 4) == INV and "null" in err()
        assert raw(h, 1, p1, None, ph, 4) == INV and "null" in err()
        assert raw(h, 1, p1, pl, None, 4) == INV and "null" in err()
        assert raw(h, 1 << 40, p1, pl, ph, 4096) == INV and "GiB" in err()  # refused before the lists are read
        assert raw(h, 1 << 26, p1, pl, ph, 4) == INV and "wavefronts" in err()  # (3 GiB of rows, but more wavefronts than one launch holds)
        refused(L, INV, "outside", hist, [d], 0.0, 1.0, 4)
        refused(L, INV, "outside", hist, [-1], 0.0, 1.0, 4)
        refused(L, INV, "twice", hist, [0, 1, 0], 0.0, 1.0, 4)
        refused(L, INV, "lo < hi", hist, [0], 1.0, 1.0, 4)
        refused(L, INV, "finite", hist, [0], 0.0, np.inf, 4)
        refused(L, INV, "finite", hist, [0], np.nan, 1.0, 4)
        refused(L, INV, "4096", hist, [0], 0.0, 1.0, 0)
        refused(L, INV, "4096", hist, [0], 0.0, 1.0, 4097)
        refused(L, INV, "bps_consume_hist first", ens.bps_consume_histogram)
        refused(L, UNS, "arc", ens.bps_consume_hist, [0], 0.0, 1.0, 4)  # the line call keeps refusing, and names this one
        refused(L, UNS, "bps_consume_arc_hist", ens.bps_consume_hist, [0], 0.0, 1.0, 4)
        hist([1, 0], 0.0, 1.0, 4)
        refused(L, UNS, "already", hist, [0], 0.0, 1.0, 4)  # a second list on one ensemble
        for pooled in (0, 1):
            assert raw_read(h, 0, 2, pooled, None, None, None, None) == INV and "chain range" in err()
            assert raw_read(h, 0, 1, pooled, None, None, None, None) == 0  # any output may be NULL
        ens.bps_consume()
        refused(L, INV, "first bps_consume", hist, [0], 0.0, 1.0, 4)
        H, Z, T = ens.bps_consume_histogram()
        assert same_bits(H, np.zeros((1, 2, 6))) and same_bits(Z, np.zeros((1, 2))) and T[0] == 0.0  # no event yet
    with bps(begin=False) as ens:
        refused(L, INV, "bps_consume_begin", ens.bps_consume_arc_hist, [0], 0.0, 1.0, 4)
    with bps(flow="bps") as ens:
        refused(L, UNS, "bps_consume_hist", ens.bps_consume_arc_hist, [0], 0.0, 1.0, 4)
        ens.bps_consume_hist([0], 0.0, 1.0, 4)  # ... which serves it as before
    with bps(flow="modern") as ens:
        refused(L, UNS, "speed-recorded", ens.bps_consume_arc_hist, [0], 0.0, 1.0, 4)
    with bps(subsample=True) as ens:
        refused(L, UNS, "subsample", ens.bps_consume_arc_hist, [0], 0.0, 1.0, 4)
    with pkg.Ensemble(1, d, trace_capacity=8) as ens:  # the other family's ensemble
        ens.set_flow(pkg.ZigZag(G, np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_state(0.0, np.zeros((1, d)), np.ones((1, d)), np.ones(d), np.array([1], dtype=np.uint64))
        ens.consume_begin()
        refused(L, INV, "PDMP_SAMPLER_BPS", ens.bps_consume_arc_hist, [0], 0.0, 1.0, 4)


def sampler(pkg, sticky, d=8, seed=21):
    rng = np.random.default_rng(seed)
    G = sp.identity(d, format="csc")
    mu = rng.uniform(0.1, 0.6, d)
    x0, th0 = mu + rng.standard_normal((2, d)), rng.standard_normal((2, d))
    B = pkg.Boomerang(G, mu, 0.5)
    target = pkg.GaussianTarget(sp.csc_matrix(1.2 * G), mu)
    if sticky:
        return lambda cap, **k: pkg.sspdmp(target, 0.0, x0, th0, 60.0, 10.0, B, 1.5, trace_capacity=cap, seed=5, adapt=True, **k)
    return lambda cap, **k: pkg.pdmp(target, 0.0, x0, th0, 200.0, 3.0, B, trace_capacity=cap, seed=5, adapt=True, **k)


@pytest.mark.parametrize("sticky", [False, True])
def test_sampler_runs(gpu_pkg, sticky):
    """pdmp on a Boomerang(Γ, μ ≠ 0, λref = 0.5) at d = 8 and its sticky twin through sspdmp, with consume=dict(hist=...): a buffer for the whole
    run and one of 48 events give identical bytes, equal to the C statement on the returned trace; the old TypeError stays"""
    pkg = gpu_pkg
    run = sampler(pkg, sticky)
    coords = np.array([5, 0, 3, 7, 1, 2])
    hist = dict(coords=coords, lo=-2.6 + 0.02 * np.arange(6), hi=3.4, bins=64)
    args = (coords, hist["lo"], 3.4, 64)
    big, small = run(4096, consume=dict(hist=hist)), run(48, consume=dict(hist=hist))
    for k in range(2):
        assert 48 < len(big[0][k].t) < 4096 and same_bits(big[0][k].t, small[0][k].t)  # (several slices of the small buffer)
        assert (big[0][k].f is not None and not big[0][k].f.all()) == sticky
    for res in (big, small):
        for k, tr in enumerate(res[0]):
            ref = AH.of_trace(tr, *args)
            assert same_bits(res[-1]["hist_H"][k], ref[0]) and same_bits(res[-1]["hist_Z"][k], ref[1]) and res[-1]["T"][k] == ref[2], k
        assert np.array_equal(res[-1]["hist_coords"], coords) and res[-1]["hist_edges"].shape == (6, 65)
    assert same_bits(big[-1]["hist_H"], small[-1]["hist_H"]) and same_bits(big[-1]["hist_Z"], small[-1]["hist_Z"])
    assert (big[-1]["hist_Z"].sum() > 0) == sticky
    H, T = big[-1]["hist_H"], big[-1]["T"]
    n = max(len(tr.t) for tr in big[0])  # Σ_k H[k] = T_last − t0 to rounding: n pieces of at most 66 additions into a row, each within 2^-53
    assert np.allclose(H.sum(axis=2), T[:, None], rtol=n * 66 * 2.0 ** -53, atol=0)
    plain = run(48, consume=dict())
    assert set(small[-1]) - set(plain[-1]) == {"hist_coords", "hist_edges", "hist_H", "hist_Z"} and same_bits(small[-1]["mean"], plain[-1]["mean"])
    tr = big[0][0]
    assert pkg.trace.arc_marginal_histogram(tr, *args)[2] == T[0]  # (the host mirror; tests/test_arc_hist_ref.py holds it to the derived bound)
    with pytest.raises(TypeError, match="arc"):
        pkg.trace.marginal_histogram(tr, *args)
    med = pkg.trace.histogram_quantiles(H, hist["lo"], 3.4, 0.5)  # used unchanged
    assert med.shape == (2, 6) and np.all(np.isfinite(med))


def test_pooled_median_of_a_standard_normal(gpu_pkg):
    """4 chains of a Boomerang on N(0, I_4) for T = 64 each, 9 bins of width 1 on [−4.5, 4.5): the pooled median of every coordinate lies in the
    bin of 0, [−0.5, 0.5).  The run length is the reference's own envelope (test/maintest.jl asks |mean| < 2/√T of its runs): 2/√64 = 0.25 is
    inside the half width 0.5 of that bin -- the bin is chosen from the envelope, no new tolerance is set."""
    pkg = gpu_pkg
    d, nch, T = 4, 4, 64.0
    rng = np.random.default_rng(3)
    G = sp.identity(d, format="csc")
    x0, th0 = rng.standard_normal((nch, d)), rng.standard_normal((nch, d))
    assert 2.0 / np.sqrt(T) <= 0.5
    res = pkg.pdmp(pkg.GaussianTarget(G, np.zeros(d)), 0.0, x0, th0, T, 3.0, pkg.Boomerang(G, np.zeros(d), 0.5), seed=7, adapt=True,
                   trace_capacity=256, consume=dict(hist=dict(coords=None, lo=-4.5, hi=4.5, bins=9)))
    H = res[-1]["hist_H"]
    med = pkg.trace.histogram_quantiles(HR.pool(H), -4.5, 4.5, 0.5)
    print("pooled medians:", med)
    assert med.shape == (d,) and all(HR.bin_of(-4.5, 4.5, 9, v) == HR.bin_of(-4.5, 4.5, 9, 0.0) == 4 for v in med)
