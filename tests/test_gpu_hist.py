"""The marginal histograms on the device (pdmp_ensemble_[bps_]consume_hist / _consume_histogram; csrc/pdmp_consume.hip, csrc/pdmp_consume_bps.hip;
-m gpu) against the sequential statement of their contract, tests/ref/hist_ref.c, BIT FOR BIT (H, Z and T_last):

  1. hand-made traces (tests/consumer_cases.py, tests/barrier_consumer_cases.py, tests/pdmp_consumer_cases.py) through pdmp_debug_trace_append /
     pdmp_debug_bps_trace_append, segment by segment with a consume() and two reads after each, the `grow` segments included, at 1, 63, 64 and 65
     bins (one short of a wavefront's stride, exactly one, one past it), on ranges that make pieces cross every bin and both outer slots;
  2. sampler runs of both families, one-shot, in five slices with a read after each, and with a trace buffer of a seventh of the events:
     identical bits, equal to the contract on the returned trace; the consume= keyword;
  3. the other consumers of an ensemble with hist return the bytes they return without; the mean and the pooled read derived from H; every
     refusal, by status and by a word of the message."""
import numpy as np
import pytest
import scipy.sparse as sp

import barrier_consumer_cases as BC
import consumer_cases as CC
import hist_ref_lib as HR
import pdmp_consumer_cases as PC
import stickyzz_cases as K
import stickyzz_ref_lib as R

pytestmark = pytest.mark.gpu

EV = HR.EVENT_DTYPE
BINS = [1, 63, 64, 65]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def cut_range(values, frac):
    """a range that cuts `frac` of the spread off either end: some pieces cross every bin and end in both outer slots"""
    a, b = float(np.min(values)), float(np.max(values))
    w = max(b - a, 1.0)
    return a + frac * w, b - frac * w


def reads_match(read, ref_of, nchains, where):
    """a read equals the contract per chain, the pooled read is its chain-ordered sum, and a second read returns the same bytes"""
    H, Z, T = read()
    for k in range(nchains):
        ref = ref_of(k)
        assert same_bits(H[k], ref[0]) and same_bits(Z[k], ref[1]) and T[k] == ref[2], (where, k)
    assert all(same_bits(a, b) for a, b in zip(read(), (H, Z, T))), where
    Hp, Zp, Tp = read(pooled=True)
    assert same_bits(Hp, HR.pool(H)) and same_bits(Zp, HR.pool(Z)) and same_bits(Tp, T), where
    if nchains > 1:  # a range of chains
        H1, Z1, T1 = read(1, nchains - 1)
        assert same_bits(H1, H[1:]) and same_bits(Z1, Z[1:]) and same_bits(T1, T[1:]), where
    return H, Z, T


# ------------------------------------------------------------------------------------------------------------------- hand-made traces, factorised

def open_fact(pkg, c):
    L = pkg._lib
    G = sp.identity(c.d, format="csc")
    kw = dict(sampler=L.SAMPLER_STICKY_ZIGZAG, factor=1.5) if c.sticky else {}
    ens = pkg.Ensemble(c.nchains, c.d, trace_capacity=c.trace_capacity, **kw)
    ens.set_flow(pkg.ZigZag(G, np.zeros(c.d)))
    ens.set_target(pkg.GaussianTarget(G))
    if c.sticky:
        ens.set_sticky(np.full(c.d, 0.8))
    ens.set_state(c.t0, c.x0, c.th0, np.ones(c.d), np.arange(c.nchains, dtype=np.uint64) + 1)
    ens.consume_begin(c.dt, c.K)
    return ens


def fact_coords(c):
    """a permuted subset: listed coordinates that never fire, unlisted ones that do, and (clash) both clashing coordinates"""
    rng = np.random.default_rng(23)
    if c.d <= 4:
        return rng.permutation(c.d)
    coords = rng.permutation(c.d)[:40]
    if c.name == "clash":
        coords = np.unique(np.concatenate([coords, np.asarray(c.pair)]))[::-1].copy()
    return coords


@pytest.mark.parametrize("B", BINS)
@pytest.mark.parametrize("name", ["one", "few", "sticky", "sparse", "clash", "on_grid_end"])
def test_hand_made_fact_traces(gpu_pkg, name, B):
    """d = 1 (256 events of one coordinate in a row), d = 3 with t0 = −1.5 and a segment grown without a reset, d = 4 sticky (θ = 0 pieces, ±0.0
    positions), d = 300 sparse (coordinates that never fire, a chain with no event in a segment), d = 5000 clash (two events of one coordinate in a
    chunk): after every segment the read equals the contract on the trace so far, twice; the ordinary consumers return what they return without"""
    pkg = gpu_pkg
    c = CC.case(name)
    coords = fact_coords(c)
    allx = np.concatenate([c.x0.reshape(-1)] + [e["x"] for e in c.events])
    lo, hi = cut_range(allx, 0.2)
    lo = lo + 0.01 * np.arange(len(coords))  # (a range per coordinate)
    plain = []
    for with_hist in (False, True):
        with open_fact(pkg, c) as ens:
            if with_hist:
                ens.consume_hist(coords, lo, hi, B)
            for s in range(c.nseg):
                for k in range(c.nchains):
                    ens.debug_trace_append(k, c.segment(k, s))
                ens.consume()
                if with_hist:
                    H, _, _ = reads_match(ens.consume_histogram, lambda k: HR.fact(c.t0, c.x0[k], c.th0[k], c.so_far(k, s), coords, lo, hi, B), c.nchains,
                                          (name, s))
                if s not in c.grow:
                    ens.trace_reset()
            if with_hist and all(len(e) for e in c.events):
                assert np.all(H[:, :, 0].sum(axis=1) > 0) and np.all(H[:, :, B + 1].sum(axis=1) > 0)  # both outer slots were reached
            if all(len(e) for e in c.events):
                plain.append([ens.consume_mean()[0]] + [ens.consume_discretized(k)[1] for k in range(c.nchains)])
    assert len(plain) != 2 or all(same_bits(a, b) for a, b in zip(*plain))


def test_two_events_of_one_coordinate_in_a_chunk_and_a_long_row(gpu_pkg):
    """d = 2: coordinate 1 fires 200 times in a row inside chunks of 64 with pieces that sweep all 65 bins and both outer slots (every lane of the
    wavefront and the second round), coordinate 0 is not listed; one slice and three give the same bits"""
    pkg = gpu_pkg
    rng = np.random.default_rng(2)
    n, d = 200, 2
    t = np.cumsum(rng.uniform(0.5, 3.0, n))
    x0, th0 = np.array([[0.1, -2.0]]), np.array([[1.0, 1.0]])
    ev = np.empty(n, dtype=EV)
    x, th, tc = x0[0].copy(), th0[0].copy(), np.zeros(d)
    for k in range(n):
        i = 1 if k % 5 else 0
        x[i] = x[i] + th[i] * (t[k] - tc[i])
        tc[i], th[i] = t[k], -th[i]
        ev[k] = (t[k], i, x[i], th[i])
    G = sp.identity(d, format="csc")
    out = []
    for cuts in ([0, n], [0, 63, 129, n]):
        with pkg.Ensemble(1, d, trace_capacity=n) as ens:
            ens.set_flow(pkg.ZigZag(G, np.zeros(d)))
            ens.set_target(pkg.GaussianTarget(G))
            ens.set_state(0.0, x0, th0, np.ones(d), np.array([1], dtype=np.uint64))
            ens.consume_begin()
            ens.consume_hist([1], -1.0, 1.0, 65)
            for a, b in zip(cuts[:-1], cuts[1:]):
                ens.debug_trace_append(0, ev[a:b])
                ens.consume()
                ens.trace_reset()
            out.append(ens.consume_histogram())
    ref = HR.fact(0.0, x0[0], th0[0], ev, [1], -1.0, 1.0, 65)
    assert same_bits(out[0][0][0], ref[0]) and same_bits(out[0][1][0], ref[1]) and out[0][2][0] == ref[2]
    assert all(same_bits(a, b) for a, b in zip(*out)) and np.all(ref[0] > 0)


def test_barrier_table_with_a_frozen_start(gpu_pkg):
    """tests/barrier_consumer_cases.py through barrier_consume_begin: a coordinate that starts frozen starts with θ = 0 (the contract on the
    θ_eff-started trace), fed in the table's two segments; the rest times are the frozen times written out by hand there"""
    pkg = gpu_pkg
    L = pkg._lib
    G = sp.identity(BC.D, format="csc")
    lo, hi = np.array([-0.5, -0.25, 0.0, -1.0]), np.array([1.5, 1.5, 1.0, 1.0])
    for B in (4, 64):
        with pkg.Ensemble(BC.NCHAINS, BC.D, sampler=L.SAMPLER_BARRIER_ZIGZAG, factor=1.5, trace_capacity=BC.TRACE_CAPACITY) as ens:
            ens.set_flow(pkg.ZigZag(G, np.zeros(BC.D)))
            ens.set_target(pkg.GaussianTarget(G, None))
            ens.set_barriers(*R.barrier_table(BC.BARRIERS, BC.D))
            ens.set_state(BC.T0, BC.X0, BC.TH0, np.ones(BC.D), np.arange(BC.NCHAINS, dtype=np.uint64) + 1)
            ens.barrier_consume_begin(BC.DT, BC.K)
            ens.consume_hist(None, lo, hi, B)
            for s in range(BC.NSEG):
                for k in range(BC.NCHAINS):
                    ens.debug_trace_append(k, BC.segment(k, s))
                ens.consume()
                H, Z, T = reads_match(ens.consume_histogram, lambda k: HR.fact(BC.T0, BC.X0[k], BC.TH_EFF[k], BC.so_far(k, s), None, lo, hi, B),
                                      BC.NCHAINS, s)
                ens.trace_reset()
            assert same_bits(Z, BC.FROZEN_LO + BC.FROZEN_HI) and same_bits(T, BC.T_LAST)
            zl, zh = ens.barrier_consume_occupation()[:2]
            assert same_bits(zl, BC.FROZEN_LO) and same_bits(zh, BC.FROZEN_HI)  # (the occupation beside it is untouched)


# ------------------------------------------------------------------------------------------------------------------- hand-made traces, Bouncy Particle family

def open_bps(pkg, c):
    L = pkg._lib
    G = sp.identity(c.d, format="csc")
    ens = pkg.Ensemble(c.nchains, c.d, sampler=L.SAMPLER_BPS, factor=2.0, trace_capacity=c.trace_capacity)
    ens.set_flow_bps(pkg.BouncyParticle(G, np.zeros(c.d), 1.0))
    if c.sticky:
        ens.set_bps_sticky(np.full(c.d, 0.8))
    ens.set_state_bps(c.t0, c.x0, c.th0, 10.0, np.arange(c.nchains, dtype=np.uint64) + 1)
    ens.bps_consume_begin(c.dt, c.K)
    return ens


def pdmp_coords(c):
    """both sides of a 64-lane strip and of a mask-word boundary, the first and the last coordinate, in no order"""
    want = [c.d - 1, 0, 63, 64, 65, 127, 128, 129, 1, 62]
    return np.array([j for j in dict.fromkeys(want) if 0 <= j < c.d], dtype=np.int64)


@pytest.mark.parametrize("B", [1, 64, 65])
@pytest.mark.parametrize("name", ["one", "neg", "d63", "d65", "sparse", "sticky130", "c1024"])
def test_hand_made_pdmp_traces(gpu_pkg, name, B):
    """d = 1, t0 < 0, 63 and 65 coordinates, two chains with a segment that gives one of them nothing, a sticky trace over three mask words,
    d = 1024: after every segment H, Z and T_last are the contract's on the trace so far, twice; mean and the grid are unchanged"""
    pkg = gpu_pkg
    c = PC.case(name)
    coords = pdmp_coords(c)
    allx = np.concatenate([c.x0.reshape(-1)] + [np.asarray(x).reshape(-1) for x in c.x])
    lo, hi = cut_range(allx, 0.3)
    hi = hi + 0.01 * np.arange(len(coords))
    plain = []
    for with_hist in (False, True):
        with open_bps(pkg, c) as ens:
            if with_hist:
                ens.bps_consume_hist(coords, lo, hi, B)
            for s in range(c.nseg):
                for k in range(c.nchains):
                    t, x, th, f = c.segment(k, s)
                    if not (c.sticky and s == 0):  # (a sticky ensemble holds the event its set_state_bps wrote: the case's first segment)
                        ens.debug_bps_trace_append(k, t, x, th, f)
                ens.bps_consume()
                if with_hist:
                    def ref_of(k):
                        t, x, th, f = c.so_far(k, s)
                        return HR.pdmp(c.t0, c.x0[k], c.th0[k], t, x, th, coords, lo, hi, B, f=f)
                    reads_match(ens.bps_consume_histogram, ref_of, c.nchains, (name, s))
                if s not in c.grow:
                    ens.trace_reset()
            plain.append([ens.bps_consume_mean()[0]] + [ens.bps_consume_discretized(k)[1] for k in range(c.nchains)])
    assert all(same_bits(a, b) for a, b in zip(*plain))


# ------------------------------------------------------------------------------------------------------------------- sampler runs, factorised

def direct_zigzag(pkg, setup, x0, th0, c, T_slices, seed, cap, hist, barrier=False):
    """the loop of spdmp / stickyzz on an ensemble: per slice run -> consume -> drain, a read after every slice; the last slice runs with the
    reference's tail, the earlier ones pause before their end time, so however T is cut the trace is that of a single run to T.  Returns
    (events per chain, (H, Z, T_last), reads after each slice with the number of events each chain had then)."""
    L = pkg._lib
    nch, d = x0.shape
    reads = []
    with setup(cap) as ens:
        ens.set_state(0.0, x0, th0, c, np.uint64(seed) + np.arange(nch, dtype=np.uint64))
        (ens.barrier_consume_begin if barrier else ens.consume_begin)()
        ens.consume_hist(*hist)
        evs = [[] for _ in range(nch)]
        for s, Tk in enumerate(T_slices):
            while True:
                ens.run(Tk, L.RUN_REFERENCE_TAIL if s == len(T_slices) - 1 else L.RUN_STOP_BEFORE)
                cnt = ens.counters()
                assert not np.any(cnt["status"] == L.CHAIN_BOUND_VIOLATED)
                ens.consume()
                for k in range(nch):
                    evs[k].append(ens.trace(k, counters=cnt))
                ens.trace_reset()
                if not L.needs_rerun(cnt["status"]):
                    break
            reads.append((ens.consume_histogram(), [sum(len(e) for e in evs[k]) for k in range(nch)]))
        out = ens.consume_histogram()
    return [np.concatenate(e) for e in evs], out, reads


def three_ways(pkg, setup, x0, th0, th_start, c, T, seed, hist, min_events=100, barrier=False):
    """One shot with room for the whole trace, five slices with a read after each, a trace buffer of a seventh of the events: the same trace
    bytes and the same bits of H, Z, T_last, equal to the contract on the trace; every read midway is the contract on the events until then"""
    big = 1 << 14
    ev1, out1, _ = direct_zigzag(pkg, setup, x0, th0, c, [T], seed, big, hist, barrier)
    nch = len(ev1)
    for k in range(nch):
        ref = HR.fact(0.0, x0[k], th_start[k], ev1[k], *hist)
        assert same_bits(out1[0][k], ref[0]) and same_bits(out1[1][k], ref[1]) and out1[2][k] == ref[2], k
    n = max(len(e) for e in ev1)
    assert min_events < n < big, n
    ev5, out5, reads = direct_zigzag(pkg, setup, x0, th0, c, [0.2 * T, 0.4 * T, 0.6 * T, 0.8 * T, T], seed, big, hist, barrier)
    ev7, out7, _ = direct_zigzag(pkg, setup, x0, th0, c, [T], seed, n // 7, hist, barrier)
    for ev, out in ((ev5, out5), (ev7, out7)):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ev1, ev))
        assert all(same_bits(a, b) for a, b in zip(out1, out))
    assert len(reads) == 5 and 0 < reads[0][1][0] < reads[2][1][0] < reads[4][1][0]
    for (H, Z, Tl), upto in reads:
        for k in range(nch):
            ref = HR.fact(0.0, x0[k], th_start[k], ev5[k][:upto[k]], *hist)
            assert same_bits(H[k], ref[0]) and same_bits(Z[k], ref[1]) and Tl[k] == ref[2]
    return ev1, out1


def test_spdmp_d8(gpu_pkg):
    """test/maintest.jl's problem at d = 8, 3 chains, 6 listed coordinates in no order, 64 bins on ranges that cut the tails"""
    pkg = gpu_pkg
    G = pkg.problems.maintest_precision(8)
    rng = np.random.default_rng(4)
    x0, th0 = rng.random((3, 8)), rng.choice([-1.0, 1.0], (3, 8))
    c = 0.7 * pkg.problems.column_norms(G)
    flow = pkg.ZigZag(sp.csc_matrix(0.9 * G), np.zeros(8))
    hist = (np.array([5, 0, 7, 2, 3, 6]), -0.3 - 0.05 * np.arange(6), 0.4, 64)

    def setup(cap):
        ens = pkg.Ensemble(3, 8, trace_capacity=cap, factor=1.8)
        ens.set_flow(flow)
        ens.set_target(pkg.GaussianTarget(G))
        return ens

    ev1, out1 = three_ways(pkg, setup, x0, th0, th0, c, 60.0, 3, hist, min_events=200)
    assert np.all(out1[0][:, :, 0] > 0) and np.all(out1[0][:, :, -1] > 0)
    res = pkg.spdmp(pkg.GaussianTarget(G), 0.0, x0, th0, 60.0, c, flow, seed=3, trace_capacity=100,
                    consume=dict(hist=dict(coords=hist[0], lo=hist[1], hi=hist[2], bins=64)))
    extra = res[-1]
    assert all(a.tobytes() == b.events.tobytes() for a, b in zip(ev1, res[0]))
    assert same_bits(extra["hist_H"], out1[0]) and same_bits(extra["hist_Z"], out1[1]) and same_bits(extra["T"], out1[2])
    assert np.array_equal(extra["hist_coords"], hist[0]) and same_bits(extra["hist_edges"], pkg.trace.histogram_edges(hist[1], np.full(6, 0.4), 64))


def test_sspdmp_d8(gpu_pkg):
    """the sticky ZigZag at d = 8 (freezes: θ = 0 pieces at 0, an inner edge of the bins), all coordinates, 65 bins"""
    pkg = gpu_pkg
    G = pkg.problems.maintest_precision(8)
    rng = np.random.default_rng(12)
    x0, th0 = rng.standard_normal((2, 8)), rng.choice([-1.0, 1.0], (2, 8))
    c = pkg.problems.column_norms(G)
    kappa = np.full(8, 0.8)
    flow = pkg.ZigZag(G, np.zeros(8))
    hist = (np.arange(8), -0.65, 0.65, 65)

    def setup(cap):
        ens = pkg.Ensemble(2, 8, trace_capacity=cap, sampler=pkg._lib.SAMPLER_STICKY_ZIGZAG, factor=1.5)
        ens.set_flow(flow)
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_sticky(kappa)
        return ens

    ev1, out1 = three_ways(pkg, setup, x0, th0, th0, c, 40.0, 9, hist)
    assert any(np.any(e["theta"] == 0) for e in ev1) and np.all(out1[1].sum(axis=1) > 0)
    res = pkg.sspdmp(pkg.GaussianTarget(G), 0.0, x0, th0, 40.0, c, flow, kappa, seed=9, trace_capacity=4096,
                     consume=dict(hist=dict(lo=-0.65, hi=0.65, bins=65)))  # coords=None: all of d; scalars broadcast
    assert all(a.tobytes() == b.events.tobytes() for a, b in zip(ev1, res[0]))
    assert same_bits(res[-1]["hist_H"], out1[0]) and same_bits(res[-1]["hist_Z"], out1[1]) and np.array_equal(res[-1]["hist_coords"], np.arange(8))


def box_problem(pkg):
    G = pkg.problems.maintest_precision(8)
    rng = np.random.default_rng(21)
    x0 = rng.uniform(-0.4, 0.4, (2, 8))
    th0 = rng.choice([-1.0, 1.0], (2, 8))
    x0[:, 4] = np.where(th0[:, 4] > 0, 0.5, -0.5)  # coordinate 4 starts frozen on the barrier of its direction
    bar = [((-0.5, 0.5), ("sticky", "sticky"), (1.0, 1.0))] * 8
    return G, x0, th0, bar


def test_stickyzz_in_a_box_d8(gpu_pkg):
    """the barrier ZigZag in the box [−0.5, 0.5]^8 with sticky walls, one coordinate frozen at the start: 63 bins on a range inside the box, so
    the time on a wall lies in an outer slot"""
    pkg = gpu_pkg
    G, x0, th0, bar = box_problem(pkg)
    c = 2.0 * pkg.problems.column_norms(G)
    flow = pkg.ZigZag(sp.csc_matrix(G), np.zeros(8))
    th_eff, _ = pkg.trace.barrier_start(x0, th0, bar)
    assert np.all(th_eff[:, 4] == 0)
    hist = (np.array([4, 1, 7, 0]), -0.45, 0.45, 63)

    def setup(cap):
        ens = pkg.Ensemble(2, 8, trace_capacity=cap, sampler=pkg._lib.SAMPLER_BARRIER_ZIGZAG, factor=1.5)
        ens.set_flow(flow)
        ens.set_target(pkg.GaussianTarget(G, None))
        ens.set_barriers(*R.barrier_table(bar, 8))
        return ens

    ev1, out1 = three_ways(pkg, setup, x0, th0, th_eff, c, 40.0, 6, hist, barrier=True)
    assert np.all(out1[0][:, :, 0] > 0) and np.all(out1[0][:, :, -1] > 0) and np.all(out1[1] > 0)
    res = pkg.stickyzz(pkg.GaussianTarget(G, None), 0.0, x0, th0, 40.0, c, flow, K.barriers_for(pkg, bar, 8), seed=6, trace_capacity=4096,
                       consume=dict(hist=dict(coords=hist[0], lo=-0.45, hi=0.45, bins=63)))
    assert same_bits(res[-1]["hist_H"], out1[0]) and same_bits(res[-1]["hist_Z"], out1[1]) and same_bits(res[-1]["T"], out1[2])


# ------------------------------------------------------------------------------------------------------------------- sampler runs, Bouncy Particle family

def direct_bps(pkg, d, x0, th0, sticky, T_slices, cap, hist):
    """pdmp / sspdmp's loop on an ensemble (their factors and c), slice by slice with a read after each: the earlier slices pause before their
    end time, the last runs with the reference's tail"""
    L = pkg._lib
    nch = x0.shape[0]
    B = pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0)
    reads = []
    with pkg.Ensemble(nch, d, sampler=L.SAMPLER_BPS, factor=2.0 if sticky else 1.8, trace_capacity=cap) as ens:
        ens.set_flow_bps(B)
        if sticky:
            ens.set_bps_sticky(1.5, False)
        ens.set_state_bps(0.0, x0, th0, 0.5 if sticky else 1e-3, np.uint64(5) + np.arange(nch, dtype=np.uint64))
        ens.bps_consume_begin()
        ens.bps_consume_hist(*hist)
        for s, Tk in enumerate(T_slices):
            while True:
                ens.run(Tk, L.RUN_REFERENCE_TAIL if s == len(T_slices) - 1 else L.RUN_STOP_BEFORE)
                cnt = ens.counters()
                assert not np.any(cnt["status"] == L.CHAIN_BOUND_VIOLATED)
                ens.bps_consume()
                ens.trace_reset()
                if not L.needs_rerun(cnt["status"]):
                    break
            reads.append(ens.bps_consume_histogram())
        return ens.bps_consume_histogram(), reads


@pytest.mark.parametrize("d,sticky", [(16, False), (8, True)])
def test_bps_sampler_runs(gpu_pkg, d, sticky):
    """pdmp on a BouncyParticle at d = 16 and its sticky form through sspdmp at d = 8 with consume=dict(hist=...): a buffer for the whole run, one
    of a seventh of the events and five slices of the direct calls with a read after each give identical bits, equal to the contract on the trace"""
    pkg = gpu_pkg
    rng = np.random.default_rng(9 + d)
    x0, th0 = rng.standard_normal((2, d)), rng.standard_normal((2, d))
    B = pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0)
    coords = rng.permutation(d)[:6]
    hist = dict(coords=coords, lo=-0.8 + 0.02 * np.arange(6), hi=0.9, bins=64)
    args = (coords, hist["lo"], 0.9, 64)
    run = (lambda cap: pkg.sspdmp(None, 0.0, x0, th0, 60.0, 0.5, B, 1.5, seed=5, trace_capacity=cap, consume=dict(hist=hist))) if sticky \
        else (lambda cap: pkg.pdmp(None, 0.0, x0, th0, 60.0, 1e-3, B, seed=5, trace_capacity=cap, consume=dict(hist=hist)))
    big = run(4096)
    n = max(len(tr.t) for tr in big[0])
    assert 100 < n < 4096
    small = run(n // 7)
    for k in range(2):
        assert same_bits(big[0][k].t, small[0][k].t)
        assert (big[0][k].f is not None and not big[0][k].f.all()) == sticky
    for res in (big, small):
        for k, tr in enumerate(res[0]):
            ref = HR.of_trace(tr, *args)
            assert same_bits(res[-1]["hist_H"][k], ref[0]) and same_bits(res[-1]["hist_Z"][k], ref[1]) and res[-1]["T"][k] == ref[2]
    assert same_bits(big[-1]["hist_H"], small[-1]["hist_H"]) and same_bits(big[-1]["hist_Z"], small[-1]["hist_Z"])
    assert np.all(big[-1]["hist_H"][:, :, 0] > 0) and np.all(big[-1]["hist_H"][:, :, -1] > 0)
    assert (big[-1]["hist_Z"].sum() > 0) == sticky
    plain = (pkg.sspdmp(None, 0.0, x0, th0, 60.0, 0.5, B, 1.5, seed=5, trace_capacity=n // 7, consume=dict())) if sticky \
        else pkg.pdmp(None, 0.0, x0, th0, 60.0, 1e-3, B, seed=5, trace_capacity=n // 7, consume=dict())
    assert set(small[-1]) - set(plain[-1]) == {"hist_coords", "hist_edges", "hist_H", "hist_Z"} and same_bits(small[-1]["mean"], plain[-1]["mean"])
    # five slices of the direct calls, a read after each: the reads grow, the last one is the keyword's
    out5, reads = direct_bps(pkg, d, x0, th0, sticky, [12.0, 24.0, 36.0, 48.0, 60.0], 4096, args)
    assert same_bits(out5[0], big[-1]["hist_H"]) and same_bits(out5[1], big[-1]["hist_Z"]) and same_bits(out5[2], big[-1]["T"])
    sums = [r[0].sum() for r in reads]
    assert len(reads) == 5 and all(a < b for a, b in zip(sums[:-1], sums[1:]))
    for H, Z, T in reads:
        assert np.allclose(H.sum(axis=2), T[:, None], rtol=1e-10, atol=0)  # Σ_k H[k] = T_last − t0 at every read


# ------------------------------------------------------------------------------------------------------------------- coexistence, derived checks, refusals

def test_hist_beside_pairs_condition_and_cummean(gpu_pkg):
    """one ensemble with a condition, cummean, pairs and hist: mean, the grid, the hits, the cummean pairs, S and J are byte for byte those of
    the same run without hist"""
    pkg = gpu_pkg
    c = CC.case("few")
    a, b = np.triu_indices(c.d)
    p, n = np.zeros(c.d), np.zeros(c.d)
    p[1], n[1] = 1.0, 1.0
    got = []
    for with_hist in (False, True):
        with open_fact(pkg, c) as ens:
            ens.consume_cummean(True)
            ens.consume_condition(p, n, 64)
            ens.consume_pairs(a, b)
            if with_hist:
                ens.consume_hist(None, -0.5, 0.5, 64)
            cm = []
            held = 0
            for s in range(c.nseg):
                seg = c.segment(0, s)
                ens.debug_trace_append(0, seg)
                ens.consume()
                if len(seg):
                    cm.extend(ens.consume_cummean_pairs(0, len(seg), first=held))
                if s in c.grow:
                    held += len(seg)
                else:
                    ens.trace_reset()
                    held = 0
            ht, hx, nh = ens.consume_conditioned(0)
            S, J, T = ens.consume_pair_integrals()
            assert nh > 0
            got.append([ens.consume_mean()[0], ens.consume_discretized(0)[1], ht, hx, S, J, T] + cm)
            if with_hist:
                H, Z, Th = ens.consume_histogram()
                ref = HR.fact(c.t0, c.x0[0], c.th0[0], c.events[0], None, -0.5, 0.5, 64)
                assert same_bits(H[0], ref[0]) and same_bits(Z[0], ref[1]) and same_bits(Th, T)
    assert len(got[0]) == len(got[1]) and all(same_bits(x, y) for x, y in zip(*got))
    # ... and the Bouncy Particle family: pairs and a condition beside hist
    c = PC.case("d65")
    got = []
    for with_hist in (False, True):
        with open_bps(pkg, c) as ens:
            ens.bps_consume_pairs([0, 64], [64, 3])
            if with_hist:
                ens.bps_consume_hist([64, 0], -0.5, 0.5, 65)
            for s in range(c.nseg):
                for k in range(c.nchains):
                    ens.debug_bps_trace_append(k, *c.segment(k, s))
                ens.bps_consume()
                if s not in c.grow:
                    ens.trace_reset()
            got.append(list(ens.bps_consume_pair_integrals()) + [ens.bps_consume_mean()[0]])
    assert all(same_bits(x, y) for x, y in zip(*got))


def test_mean_and_pool_derived_from_the_histogram(gpu_pkg):
    """a run with no mass in the outer slots: |Σ_k H_k·mid_k / L − consume_mean| <= w / 2 per coordinate (each bin's mass sits within w / 2 of its
    midpoint); the pooled read is the chain-ordered sum of the per-chain read; the sup distance of the pooled CDF to the Gaussian marginal's is
    printed, not asserted"""
    from math import erf, sqrt
    pkg = gpu_pkg
    G = pkg.problems.maintest_precision(8)
    rng = np.random.default_rng(2)
    nch, Bn = 8, 64
    x0, th0 = rng.random((nch, 8)), rng.choice([-1.0, 1.0], (nch, 8))
    sd = np.sqrt(np.diag(np.linalg.inv(G.toarray())))
    lo, hi = -12.0 * sd - 1.0, 12.0 * sd + 1.0
    L = pkg._lib
    with pkg.Ensemble(nch, 8, trace_capacity=2048, factor=1.8) as ens:
        ens.set_flow(pkg.ZigZag(sp.csc_matrix(0.9 * G), np.zeros(8)))
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_state(0.0, x0, th0, 0.7 * pkg.problems.column_norms(G), np.uint64(2) + np.arange(nch, dtype=np.uint64))
        ens.consume_begin()
        ens.consume_hist(None, lo, hi, Bn)
        while True:
            ens.run(300.0, L.RUN_REFERENCE_TAIL)
            cnt = ens.counters()
            ens.consume()
            ens.trace_reset()
            if not L.needs_rerun(cnt["status"]):
                break
        H, Z, T = ens.consume_histogram()
        Hp, Zp, Tp = ens.consume_histogram(pooled=True)
        Hr, _, _ = ens.consume_histogram(2, 5, pooled=True)
        mean, Tm = ens.consume_mean()
    assert np.all(H[:, :, 0] == 0) and np.all(H[:, :, -1] == 0) and same_bits(T, Tm) and np.all(Z == 0)
    E = pkg.trace.histogram_edges(lo, hi, Bn)
    mid, w = 0.5 * (E[:, :-1] + E[:, 1:]), (hi - lo) / Bn
    est = (H[:, :, 1:-1] * mid[None]).sum(axis=2) / T[:, None]
    err = np.abs(est - mean)
    print("max |Σ H mid / L − mean| / (w / 2) = %.3g" % (err / (0.5 * w[None])).max())
    assert np.all(err <= 0.5 * w[None])
    assert same_bits(Hp, HR.pool(H)) and same_bits(Zp, HR.pool(Z)) and same_bits(Tp, T) and same_bits(Hr, HR.pool(H[2:7]))
    cdf = np.cumsum(Hp[:, 1:-1], axis=1) / Hp.sum(axis=1)[:, None]
    gauss = np.array([[0.5 * (1 + erf(e / (s * sqrt(2)))) for e in E[j, 1:]] for j, s in enumerate(sd)])
    print("sup |pooled CDF − Gaussian CDF| at the edges = %.3g" % np.abs(cdf - gauss).max())
    med = pkg.trace.histogram_quantiles(Hp, lo, hi, 0.5)
    assert med.shape == (8,) and np.all(np.isfinite(med))


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
    ev = np.array([(1.0, 0, 1.0, -1.0)], dtype=EV)

    def fact(begin=True, flow=None, refresh=None):
        ens = pkg.Ensemble(1, d, trace_capacity=8)
        ens.set_flow(flow or pkg.ZigZag(G, np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_state(0.0, np.zeros((1, d)), np.ones((1, d)), np.ones(d), np.array([1], dtype=np.uint64))
        if begin:
            ens.consume_begin()
        return ens

    def bps(flow="bps", begin=True, subsample=False):
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

    def common(ens, hist, histogram, raw, raw_read, first_word):
        h = ens._h
        err = lambda: L.load().pdmp_last_error().decode()
        p1, pl, ph = one.ctypes.data, lo1.ctypes.data, hi1.ctypes.data
        assert raw(h, 0, p1, pl, ph, 4) == INV and "m = 0" in err()
        assert raw(h, 1, None, pl, ph, 4) == INV and "null" in err()
        assert raw(h, 1, p1, None, ph, 4) == INV and "null" in err()
        assert raw(h, 1, p1, pl, None, 4) == INV and "null" in err()
        assert raw(h, 1 << 40, p1, pl, ph, 4096) == INV and "GiB" in err()  # refused before the lists are read
        refused(L, INV, "outside", hist, [d], 0.0, 1.0, 4)
        refused(L, INV, "outside", hist, [-1], 0.0, 1.0, 4)
        refused(L, INV, "twice", hist, [0, 1, 0], 0.0, 1.0, 4)
        refused(L, INV, "twice", hist, list(range(d)) + [0], 0.0, 1.0, 4)
        refused(L, INV, "lo < hi", hist, [0], 1.0, 1.0, 4)
        refused(L, INV, "lo < hi", hist, [0, 1], [0.0, 2.0], [1.0, 1.0], 4)
        refused(L, INV, "finite", hist, [0], 0.0, np.inf, 4)
        refused(L, INV, "finite", hist, [0], np.nan, 1.0, 4)
        refused(L, INV, "4096", hist, [0], 0.0, 1.0, 0)
        refused(L, INV, "4096", hist, [0], 0.0, 1.0, 4097)
        refused(L, INV, first_word, histogram)
        hist([1, 0], 0.0, 1.0, 4)
        for pooled in (0, 1):
            assert raw_read(h, 0, 2, pooled, None, None, None, None) == INV and "chain range" in err()
            assert raw_read(h, -1, 1, pooled, None, None, None, None) == INV
            assert raw_read(h, 0, 1, pooled, None, None, None, None) == 0  # any output may be NULL
            assert raw_read(h, 1, 0, pooled, None, None, None, None) == 0

    with fact() as ens:
        common(ens, ens.consume_hist, ens.consume_histogram, ens._L.pdmp_ensemble_consume_hist, ens._L.pdmp_ensemble_consume_histogram,
               "consume_hist first")
        refused(L, INV, "PDMP_SAMPLER_BPS", ens.bps_consume_hist, [0], 0.0, 1.0, 4)  # the other family's call
        refused(L, INV, "PDMP_SAMPLER_BPS", ens.bps_consume_histogram)
        refused(L, UNS, "synchronous", ens.consume_async)
        ens.debug_trace_append(0, ev)
        ens.consume()
        refused(L, INV, "first consume", ens.consume_hist, [0], 0.0, 1.0, 4)
        H, Z, T = ens.consume_histogram()  # x_0 = x_1 = t on [0, 1]: a quarter in each of the 4 bins
        assert same_bits(H, [[[0, 0.25, 0.25, 0.25, 0.25, 0]] * 2]) and same_bits(Z, [[0.0, 0.0]]) and T[0] == 1.0
    with fact(begin=False) as ens:
        refused(L, INV, "consume_begin", ens.consume_hist, [0], 0.0, 1.0, 4)
    with fact(begin=False, flow=pkg.FactBoomerang(G, np.zeros(d), 0.1)) as ens:  # what consume_begin refuses stays refused there
        refused(L, UNS, "piecewise-linear", ens.consume_begin)
        refused(L, INV, "consume_begin", ens.consume_hist, [0], 0.0, 1.0, 4)
    with bps() as ens:
        common(ens, ens.bps_consume_hist, ens.bps_consume_histogram, ens._L.pdmp_ensemble_bps_consume_hist, ens._L.pdmp_ensemble_bps_consume_histogram,
               "bps_consume_hist first")
        refused(L, INV, "PDMP_SAMPLER_BPS", ens.consume_hist, [0], 0.0, 1.0, 4)
        ens.bps_consume()
        refused(L, INV, "first bps_consume", ens.bps_consume_hist, [0], 0.0, 1.0, 4)
    with bps(begin=False) as ens:
        refused(L, INV, "bps_consume_begin", ens.bps_consume_hist, [0], 0.0, 1.0, 4)
    with bps(flow="boom") as ens:
        refused(L, UNS, "arc", ens.bps_consume_hist, [0], 0.0, 1.0, 4)
    with bps(flow="modern") as ens:
        refused(L, UNS, "speed-recorded", ens.bps_consume_hist, [0], 0.0, 1.0, 4)
    with bps(subsample=True) as ens:
        refused(L, UNS, "subsample", ens.bps_consume_hist, [0], 0.0, 1.0, 4)
    B = pkg.BouncyParticle(G, np.zeros(d), 1.0)
    with pytest.raises(TypeError, match="consume=dict"):
        pkg.pdmp(None, 0.0, np.zeros(d), np.ones(d), 1.0, 1e-3, B, consume=dict(histo=dict(lo=0.0, hi=1.0, bins=4)))
    with pytest.raises(TypeError, match="consume=dict"):
        pkg.pdmp(None, 0.0, np.zeros(d), np.ones(d), 1.0, 1e-3, B, consume=dict(hist=dict(lo=0.0, hi=1.0)))
