"""The pair integrals of a Boomerang's arcs on the device (pdmp_ensemble_bps_consume_arc_pairs, read by pdmp_ensemble_bps_consume_pair_integrals;
bps_pairs_kernel<ARC = true> of csrc/pdmp_consume_bps.hip; -m gpu) against the sequential statement of their contract, tests/ref/arc_pairs_ref.c, BIT
FOR BIT (S, J and T_last):

  1. the hand-made traces of tests/arc_pairs_cases.py (boom and boom_sticky of tests/pdmp_consumer_cases.py among them) through
     pdmp_debug_bps_trace_append, segment by segment with a bps_consume() and a read after each -- trace buffers smaller than the trace, a
     segment grown in place, a chain without events in a slice, pair lists on both sides of one workgroup per chain;
  2. the ordinary consumers of an ensemble with the list return the bytes they return without it;
  3. every refusal, by status and by the word in the message;
  4. pdmp / sspdmp on a Boomerang with consume=dict(cov=...): the device's integrals are trace.arc_pair_integrals of the returned trace, with a
     buffer for the whole run and with one of 48 events."""
import numpy as np
import pytest
import scipy.sparse as sp

import arc_pairs_cases as AC

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


@pytest.mark.parametrize("name", AC.NAMES)
def test_hand_made_traces(gpu_pkg, name):
    """after every segment S, J and T_last are the contract's on the trace so far, and a second read returns the same bytes (reading midway
    disturbs nothing: the later segments are checked in the same way); mean, cummean, the grid and the free-time fractions are byte for byte
    those of an ensemble without the list"""
    pkg = gpu_pkg
    c, pi, pj, cen = AC.listed(name)
    assert max(len(t) for t in c.t) > 0
    plain = []
    for with_pairs in (False, True):
        got = []
        with open_case(pkg, c) as ens:
            ens.bps_consume_cummean(True)
            if with_pairs:
                ens.bps_consume_arc_pairs(pi, pj, cen)
            held = [0] * c.nchains
            for s in range(c.nseg):
                for k in range(c.nchains):
                    t, x, th, f = c.segment(k, s)
                    if not (c.sticky and s == 0):  # (a sticky ensemble holds the event its set_state_bps wrote: the case's first segment)
                        ens.debug_bps_trace_append(k, t, x, th, f)
                ens.bps_consume()
                assert ens.last_consume_ms() >= 0.0
                if with_pairs:
                    S, J, T = ens.bps_consume_pair_integrals()
                    for k in range(c.nchains):
                        ref = AC.reference(name, k, s)
                        assert same_bits(S[k], ref[0]) and same_bits(J[k], ref[1]) and T[k] == ref[2], (s, k)
                    assert all(same_bits(a, b) for a, b in zip(ens.bps_consume_pair_integrals(), (S, J, T)))
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
            if c.sticky:
                got.append(ens.bps_consume_inclusion()[0])
            if c.K > 0:
                got += [ens.bps_consume_discretized(k)[1] for k in range(c.nchains)]
        plain.append(got)
    assert len(plain[0]) == len(plain[1]) and all(same_bits(a, b) for a, b in zip(*plain))


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
        h, raw, raw_read = ens._h, ens._L.pdmp_ensemble_bps_consume_arc_pairs, ens._L.pdmp_ensemble_bps_consume_pair_integrals
        err = lambda: L.load().pdmp_last_error().decode()
        assert raw(h, 0, one.ctypes.data, one.ctypes.data, None) == INV and "npairs" in err()
        assert raw(h, 1, None, one.ctypes.data, None) == INV and "null" in err()
        assert raw(h, 1, one.ctypes.data, None, None) == INV and "null" in err()
        assert raw(h, 1 << 40, one.ctypes.data, one.ctypes.data, None) == INV and "GiB" in err()  # refused before the list is read
        refused(L, INV, "outside", ens.bps_consume_arc_pairs, [0], [d])
        refused(L, INV, "outside", ens.bps_consume_arc_pairs, [-1], [0])
        refused(L, INV, "twice", ens.bps_consume_arc_pairs, [0, 1, 0], [1, 2, 1])
        refused(L, INV, "twice", ens.bps_consume_arc_pairs, [0, 1], [1, 0])  # either orientation
        refused(L, INV, "finite", ens.bps_consume_arc_pairs, [0], [1], np.array([0.0, np.nan] + [0.0] * (d - 2)))
        refused(L, INV, "bps_consume_pairs first", ens.bps_consume_pair_integrals)
        refused(L, UNS, "Boomerang", ens.bps_consume_pairs, [0], [0])  # the line call keeps refusing, and names this one
        refused(L, UNS, "bps_consume_arc_pairs", ens.bps_consume_pairs, [0], [0])
        ens.bps_consume_arc_pairs([0, 1], [1, 1])
        refused(L, UNS, "already", ens.bps_consume_arc_pairs, [0], [0])  # a second list on one ensemble
        assert raw_read(h, 0, 2, None, None, None, None) == INV and raw_read(h, -1, 1, None, None, None, None) == INV  # the chain range
        assert raw_read(h, 0, 1, None, None, None, None) == 0  # any output may be NULL
        ens.bps_consume()
        refused(L, INV, "first bps_consume", ens.bps_consume_arc_pairs, [0], [0])
        S, J, T = ens.bps_consume_pair_integrals()
        assert same_bits(S, np.zeros((1, 2))) and same_bits(J, np.zeros((1, d))) and T[0] == 0.0  # no event yet
    with bps(begin=False) as ens:
        refused(L, INV, "bps_consume_begin", ens.bps_consume_arc_pairs, [0], [0])
    with bps(flow="bps") as ens:
        refused(L, UNS, "bps_consume_pairs", ens.bps_consume_arc_pairs, [0], [0])
        ens.bps_consume_pairs([0], [0])  # ... which serves it as before
    with bps(flow="modern") as ens:
        refused(L, UNS, "speed-recorded", ens.bps_consume_arc_pairs, [0], [0])
    with bps(subsample=True) as ens:
        refused(L, UNS, "subsample", ens.bps_consume_arc_pairs, [0], [0])
    with pkg.Ensemble(1, d, trace_capacity=8) as ens:  # the other family's ensemble
        ens.set_flow(pkg.ZigZag(G, np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_state(0.0, np.zeros((1, d)), np.ones((1, d)), np.ones(d), np.array([1], dtype=np.uint64))
        ens.consume_begin()
        refused(L, INV, "PDMP_SAMPLER_BPS", ens.bps_consume_arc_pairs, [0], [0])


@pytest.mark.parametrize("sticky", [False, True])
def test_sampler_runs(gpu_pkg, sticky):
    """pdmp on a Boomerang(Γ, μ ≠ 0, λref = 0.5) at d = 8 and its sticky twin through sspdmp, with consume=dict(cov=..., center=...): a buffer
    for the whole run and one of 48 events give identical bits, equal to trace.arc_pair_integrals of the returned trace"""
    pkg = gpu_pkg
    d = 8
    rng = np.random.default_rng(21)
    G = sp.identity(d, format="csc")
    mu = rng.uniform(0.1, 0.6, d)
    x0, th0 = mu + rng.standard_normal((2, d)), rng.standard_normal((2, d))
    B = pkg.Boomerang(G, mu, 0.5)
    pi, pj = np.tril_indices(d)
    cen = 0.1 * rng.standard_normal(d)
    kw = dict(seed=5, adapt=True, consume=dict(cov=(pi, pj), center=cen))
    target = pkg.GaussianTarget(sp.csc_matrix(1.2 * G), mu)
    run = (lambda cap, **k: pkg.sspdmp(target, 0.0, x0, th0, 60.0, 10.0, B, 1.5, trace_capacity=cap, **{**kw, **k})) if sticky \
        else (lambda cap, **k: pkg.pdmp(target, 0.0, x0, th0, 200.0, 3.0, B, trace_capacity=cap, **{**kw, **k}))
    big, small = run(4096), run(48)
    for k in range(2):
        assert 48 < len(big[0][k].t) < 4096 and same_bits(big[0][k].t, small[0][k].t)  # (several slices of the small buffer)
        assert (big[0][k].f is not None and not big[0][k].f.all()) == sticky
    for res in (big, small):
        for k, tr in enumerate(res[0]):
            S, J, T = pkg.trace.arc_pair_integrals(tr, pi, pj, cen)
            assert same_bits(res[-1]["pair_S"][k], S) and same_bits(res[-1]["pair_J"][k], J) and res[-1]["T"][k] == T, k
        assert res[-1]["pairs"][0] is not None and same_bits(res[-1]["pairs"][0], pi) and same_bits(res[-1]["pairs"][1], pj)
    assert same_bits(big[-1]["pair_S"], small[-1]["pair_S"]) and same_bits(big[-1]["pair_J"], small[-1]["pair_J"])
    plain = run(48, consume=dict())
    assert set(small[-1]) - set(plain[-1]) == {"pairs", "pair_S", "pair_J"} and same_bits(small[-1]["mean"], plain[-1]["mean"])
    cov, mean = pkg.trace.covariance(pi, pj, small[-1]["pair_S"], small[-1]["pair_J"], small[-1]["T"], center=cen)  # used unchanged
    assert abs(cov - cov.T).max() == 0 and np.all(cov.diagonal() > 0) and np.all(np.isfinite(mean))
