"""The edges of the event walk every trace consumer of the Bouncy Particle family shares (bps_walk of csrc/pdmp_consume_bps.hip; -m gpu): the groups
of BC_AHEAD = 4 events, the last group that is not full, the clamped loads behind a segment, segments shorter than one group.

One hand-made trace of 13 events per case (plain d = 3, sticky d = 65 = two strips and two mask words; line flow and Boomerang flow) through
pdmp_debug_bps_trace_append, beside a second chain without events (a sticky one holds the event its set_state_bps wrote), with the consumers
driven beside each other -- mean + cummean + grid, pairs or arc pairs, hist or arc hist with 8 bins, and the arc hist once more with 130 bins
(the rows in global memory) -- under three slicings, each slice followed by trace_reset as a run does:

    13              3·4 + 1: the last group holds one event
    1 + 2 + 3 + 7   segments below BC_AHEAD, then 4 + 3
    4 + 4 + 5       whole groups, then 4 + 1

Every result has the same bits under the three slicings and the same bits as the sequential statements the consumers' own tests use
(tests/ref/pdmp_trace_ref.c, pairs_ref.c, arc_pairs_ref.c, hist_ref.c, arc_hist_ref.c).  trace.py's mean, cummean and discretize are held to the same
bits where they are the same arithmetic (everything but a Boomerang's grid rows: numpy adds the 13 rows in order, so the sums are the sequential
ones); a Boomerang's rows rotate with libm's sin / cos there and are held to the bound tests/test_pdmp_consumer_cases_ref.py derives for that.
The chain without events keeps its initial values."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import arc_hist_ref_lib as AH
import arc_pairs_ref_lib as AP
import hist_ref_lib as HR
import pairs_ref_lib as PR
import pdmp_trace_ref_lib as R
from test_detmath_accuracy import SINCOS_ABS

pytestmark = pytest.mark.gpu

N = 13
SLICINGS = {"whole": (13,), "short": (1, 2, 3, 7), "groups": (4, 4, 5)}
T0, DT, K = 0.5, 0.11, 64
LO, HI = -2.0, 2.5
CASES = [(False, False), (False, True), (True, False), (True, True)]  # (sticky, boom)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def case(sticky, boom):
    """The two chains' traces: chain 0 with 13 events, chain 1 with none of its own"""
    rng = np.random.default_rng(100 + 2 * sticky + boom)
    d = 65 if sticky else 3
    c = dict(sticky=sticky, boom=boom, d=d, mu=rng.uniform(-0.5, 0.5, d) if boom else None)
    c["x0"], c["th0"] = rng.standard_normal((2, d)), rng.standard_normal((2, d))
    t = T0 + np.cumsum(rng.uniform(0.05, 0.4, N))
    x, th = rng.standard_normal((N, d)), rng.standard_normal((N, d))
    f = None
    if sticky:  # event 0 is the one set_state_bps writes: (t0, x0, θ0, all free)
        t[0], x[0], th[0] = T0, c["x0"][0], c["th0"][0]
        f = rng.random((N, d)) < 0.7
        f[0] = True
        f[5, [3, 63, 64]], f[6, [3, 63, 64]] = False, True
        assert all(np.any(np.diff(f[:, q].astype(int)) != 0) for q in (3, 63, 64))  # free bits change in both strips (both mask words)
    c["t"], c["x"], c["th"], c["f"] = t, x, th, f
    c["pairs"] = ([0, 0, 1, 2], [0, 1, 2, 2]) if d == 3 else ([0, 0, 3, 64, 63], [0, 64, 63, 64, 5])
    c["coords"] = [2, 0] if d == 3 else [64, 3, 0, 63]
    return c


def chain_trace(c, k):
    """(t, x, θ, f) of chain k as the reference statements take it"""
    d = c["d"]
    if k == 0:
        return c["t"], c["x"], c["th"], c["f"]
    if c["sticky"]:
        return np.array([T0]), c["x0"][1][None], c["th0"][1][None], np.ones((1, d), dtype=bool)
    return np.empty(0), np.empty((0, d)), np.empty((0, d)), None


@functools.lru_cache(maxsize=None)
def reference(sticky, boom, k, bins):
    c = case(sticky, boom)
    t, x, th, f = chain_trace(c, k)
    x0, th0 = c["x0"][k], c["th0"][k]
    f0 = np.ones(c["d"], dtype=bool) if sticky else None
    r = R.consume(T0, x0, th0, t, x, th, f=f, mu=c["mu"], dt=DT, K=K)
    pi, pj = c["pairs"]
    if boom:
        r["S"], r["J"], _ = AP.arcs(T0, x0, th0, t, x, th, c["mu"], pi, pj, f0=f0, f=f)
        r["H"], r["Z"], _ = AH.arcs(T0, x0, th0, t, x, th, c["mu"], c["coords"], LO, HI, bins, f0=f0, f=f)
    else:
        r["S"], r["J"], _ = PR.pdmp(T0, x0, th0, t, x, th, pi, pj, f0=f0, f=f)
        r["H"], r["Z"], _ = HR.pdmp(T0, x0, th0, t, x, th, c["coords"], LO, HI, bins, f0=f0, f=f)
    return r


def mirror(pkg, c):
    """trace.py's mean, cummean and discretize of chain 0"""
    F = pkg.Boomerang(np.eye(c["d"]), c["mu"], 1.0) if c["boom"] else None
    tr = pkg.PDMPTrace(F, T0, c["x0"][0], c["th0"][0], c["t"], c["x"], c["th"])
    if c["sticky"]:
        tr.f0, tr.f = np.ones(c["d"], dtype=bool), c["f"]
    return pkg.trace.mean(tr), pkg.trace.cummean(tr), pkg.trace.discretize(tr, DT)


def drive(pkg, c, cuts, bins):
    """The consumers beside each other over chain 0's trace cut into `cuts`; every result by name"""
    L = pkg._lib
    d, sticky, boom = c["d"], c["sticky"], c["boom"]
    G = sp.identity(d, format="csc")
    with pkg.Ensemble(2, d, sampler=L.SAMPLER_BPS, factor=2.0, trace_capacity=16) as ens:
        if boom:
            ens.set_flow_boomerang(pkg.GaussianTarget(G, c["mu"]), pkg.Boomerang(G, c["mu"], 1.0))
        else:
            ens.set_flow_bps(pkg.BouncyParticle(G, np.zeros(d), 1.0))
        if sticky:
            ens.set_bps_sticky(np.full(d, 0.8))
        ens.set_state_bps(T0, c["x0"], c["th0"], 10.0, np.array([1, 2], dtype=np.uint64))
        ens.bps_consume_begin(DT, K)
        ens.bps_consume_cummean(True)
        (ens.bps_consume_arc_pairs if boom else ens.bps_consume_pairs)(*c["pairs"])
        (ens.bps_consume_arc_hist if boom else ens.bps_consume_hist)(c["coords"], LO, HI, bins)
        a, cm = 0, []
        for n in cuts:
            b = a + n
            lo = max(a, 1) if sticky else a  # (a sticky chain holds event 0 already)
            if b > lo:
                ens.debug_bps_trace_append(0, c["t"][lo:b], c["x"][lo:b], c["th"][lo:b], c["f"][lo:b] if sticky else None)
            ens.bps_consume()
            assert ens.counters()["ntrace"][0] == n
            cm.append(ens.bps_consume_cummean_rows(0, n))
            ens.trace_reset()
            a = b
        assert a == N
        out = dict(cummean=np.vstack(cm))
        out["mean"], out["T"] = ens.bps_consume_mean()
        if sticky:
            out["inclusion"] = ens.bps_consume_inclusion()[0]
        grids = [ens.bps_consume_discretized(k) for k in range(2)]
        out["grid_t0"], out["grid0"], out["grid_t1"], out["grid1"] = grids[0][0], grids[0][1], grids[1][0], grids[1][1]
        out["S"], out["J"], out["T_pairs"] = ens.bps_consume_pair_integrals()
        out["H"], out["Z"], out["T_hist"] = ens.bps_consume_histogram()
    return out


@pytest.mark.parametrize("sticky,boom", CASES)
def test_the_walk_under_three_slicings(gpu_pkg, sticky, boom):
    pkg = gpu_pkg
    c = case(sticky, boom)
    for bins in (8, 130) if boom else (8,):
        runs = {name: drive(pkg, c, cuts, bins) for name, cuts in SLICINGS.items()}
        whole = runs["whole"]
        for name, got in runs.items():  # the slicing does not show in a single bit
            assert got.keys() == whole.keys()
            for key in whole:
                assert same_bits(got[key], whole[key]), (bins, name, key)
        ref = [reference(sticky, boom, k, bins) for k in range(2)]
        for k in range(2):  # the sequential statements, bit for bit
            r = ref[k]
            assert same_bits(whole["T"][k], r["T"]) and same_bits(whole["T_pairs"][k], r["T"]) and same_bits(whole["T_hist"][k], r["T"])
            assert same_bits(whole["mean"][k], r["mean"]), k
            assert same_bits(whole["S"][k], r["S"]) and same_bits(whole["J"][k], r["J"]), k
            assert same_bits(whole["H"][k], r["H"]) and same_bits(whole["Z"][k], r["Z"]), (bins, k)
            assert r["npoints"] <= K and same_bits(whole["grid_t%d" % k], r["grid_t"]) and same_bits(whole["grid%d" % k], r["grid"][:r["npoints"]]), k
            if sticky:
                assert same_bits(whole["inclusion"][k], r["inclusion"]), k
        assert same_bits(whole["cummean"], ref[0]["cummean"])
        assert ref[0]["npoints"] > 13 and np.any(whole["H"][0][:, 1:-1] > 0) and np.all(whole["S"][0] != 0)  # (the trace reaches every consumer)
        # trace.py's statements of chain 0
        m, cmr, (gt, gx) = mirror(pkg, c)
        # (a sticky trace's event 0 lies at t0: its term (x0 + x0)·0 is −0.0 where x0 < 0, which numpy's cumsum keeps and y = 0.0 + term does not)
        assert same_bits(whole["cummean"][int(sticky):], cmr[int(sticky):]) and np.array_equal(whole["cummean"][:1], cmr[:1])
        assert same_bits(whole["mean"][0], m) and same_bits(whole["grid_t0"], gt)
        if boom:
            X = np.vstack([c["x0"][0][None], c["x"][:-1]])  # (the states the rows flow from: nothing flows from the last event)
            TH = np.vstack([c["th0"][0][None], c["th"][:-1]])
            mag = (np.abs(X - c["mu"]) + np.abs(TH)).max()
            assert np.abs(whole["grid0"] - gx).max() <= SINCOS_ABS * mag
        else:
            assert same_bits(whole["grid0"], gx)
        # the chain without events keeps its initial values
        assert whole["T"][1] == T0 and not np.any(whole["mean"][1]) and len(whole["grid_t1"]) == 1 and same_bits(whole["grid1"][0], c["x0"][1])
        for key in ("S", "J", "H", "Z"):
            assert not np.ascontiguousarray(whole[key][1]).view(np.uint64).any(), key
        if sticky:
            assert np.all(whole["inclusion"][1] == 1.0)
