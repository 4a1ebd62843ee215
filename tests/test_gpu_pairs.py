"""The pair integrals on the device (pdmp_ensemble_[bps_]consume_pairs / _consume_pair_integrals; csrc/pdmp_consume.hip, csrc/pdmp_consume_bps.hip;
-m gpu) against the sequential statement of their contract, tests/ref/pairs_ref.c, BIT FOR BIT (S, J and T_last):

  1. hand-made traces (tests/consumer_cases.py, tests/pdmp_consumer_cases.py) through pdmp_debug_trace_append / pdmp_debug_bps_trace_append,
     segment by segment with a consume() and a read after each, the `grow` segments that start mid-buffer included;
  2. partner lists of 63, 64 and 128 entries (both sides of the wavefront's stride), a coordinate in no pair, both orientations of a pair;
  3. sampler runs of both families, one-shot, sliced and with a trace buffer of a seventh of the events: identical bits;
  4. the ordinary consumers of an ensemble with pairs return the bytes they return without; reading twice; the consume= keyword; the covariance
     of the device's own chains inside the reference's envelope; every refusal, by status and by the word in the message."""
import numpy as np
import pytest
import scipy.sparse as sp

import consumer_cases as CC
import pairs_ref_lib as PR
import pdmp_consumer_cases as PC

pytestmark = pytest.mark.gpu

EV = PR.EVENT_DTYPE


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def dense(idx):
    idx = np.asarray(idx, dtype=np.int64)
    a, b = np.triu_indices(len(idx))
    return idx[a], idx[b]


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


def fact_pairs(c):
    rng = np.random.default_rng(17)
    if c.name == "sparse":  # 300 random pairs, the diagonal of 40 coordinates; many coordinates in no pair, many that never fire
        key = rng.choice(c.d * c.d, 300, replace=False)
        i, j = key // c.d, key % c.d
        key = np.unique(np.minimum(i, j) * c.d + np.maximum(i, j))
        off = key[key // c.d != key % c.d]
        dg = rng.choice(c.d, 40, replace=False)
        swap = rng.random(len(off)) < 0.5  # either orientation
        return np.concatenate([np.where(swap, off % c.d, off // c.d), dg]), np.concatenate([np.where(swap, off // c.d, off % c.d), dg])
    if c.name == "clash":  # only the two clashing coordinates and a few unrelated ones are paired
        i, j = c.pair
        seen = np.unique(c.events[0]["i"])
        other = [int(v) for v in seen if v not in (i, j)][:4]
        return np.array([i, j, i, other[0], other[1], other[2], j]), np.array([j, j, i, other[1], other[1], i, other[3]])
    return dense(np.arange(c.d))


@pytest.mark.parametrize("name", ["one", "few", "sticky", "sparse", "clash", "on_grid_end"])
def test_hand_made_fact_traces(gpu_pkg, name):
    """d = 1 (only the pair (0, 0); 256 events of one coordinate in a row), d = 3 with t0 = −1.5 and a segment grown without a reset, d = 4 sticky
    (θ = 0, ±0.0 positions), d = 300 sparse (coordinates that never fire, a chain with no event in a segment), d = 5000 clash: after every
    segment the read equals the contract on the trace so far; the ordinary consumers' results are those of a run without pairs"""
    pkg = gpu_pkg
    c = CC.case(name)
    pi, pj = fact_pairs(c)
    cen = None if name == "one" else 0.25 + 0.125 * (np.arange(c.d) % 7)
    plain = []
    for with_pairs in (False, True):
        with open_fact(pkg, c) as ens:
            if with_pairs:
                ens.consume_pairs(pi, pj, cen)
            for s in range(c.nseg):
                for k in range(c.nchains):
                    ens.debug_trace_append(k, c.segment(k, s))
                ens.consume()
                if with_pairs:
                    S, J, T = ens.consume_pair_integrals()
                    for k in range(c.nchains):
                        ref = PR.fact(c.t0, c.x0[k], c.th0[k], c.so_far(k, s), pi, pj, cen)
                        assert same_bits(S[k], ref[0]) and same_bits(J[k], ref[1]) and T[k] == ref[2], (s, k)
                    assert all(same_bits(a, b) for a, b in zip(ens.consume_pair_integrals(), (S, J, T)))  # a second read: the same bytes
                if s not in c.grow:
                    ens.trace_reset()
            if all(len(e) for e in c.events):
                out = [ens.consume_mean()[0]] + [ens.consume_discretized(k)[1] for k in range(c.nchains) if name != "short_grid"]
                plain.append(out)
    assert len(plain) != 2 or all(same_bits(a, b) for a, b in zip(*plain))


# ------------------------------------------------------------------------------------------------------------------- partner lists

def busy_trace(rng, d, K, x0, th0, hot, t0=0.0):
    """K events of a continuous path; every third event belongs to a coordinate of `hot`, and runs of one coordinate and of partners occur"""
    t, x, th, tc = t0, x0.copy(), th0.copy(), np.full(d, t0)
    out = np.empty(K, dtype=EV)
    prev = 0
    for k in range(K):
        t = t + rng.uniform(0.01, 0.2)
        r = rng.random()
        i = prev if r < 0.15 else (int(rng.choice(hot)) if r < 0.5 else int(rng.integers(d)))
        x[i] = x[i] + th[i] * (t - tc[i])
        tc[i], th[i], prev = t, -th[i], i
        out[k] = (t, i, x[i], th[i])
    return out


def run_events(pkg, x0, th0, evs, pi, pj, cen=None, cuts=None, t0=0.0):
    nch, d = x0.shape
    cuts = cuts or [[0, len(e)] for e in evs]
    G = sp.identity(d, format="csc")
    with pkg.Ensemble(nch, d, trace_capacity=max(max(len(e) for e in evs), 1)) as ens:
        ens.set_flow(pkg.ZigZag(G, np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_state(t0, x0, th0, np.ones(d), np.arange(nch, dtype=np.uint64) + 1)
        ens.consume_begin()
        ens.consume_pairs(pi, pj, cen)
        for s in range(len(cuts[0]) - 1):
            for k in range(nch):
                ens.debug_trace_append(k, evs[k][cuts[k][s]:cuts[k][s + 1]])
            ens.consume()
            ens.trace_reset()
        return ens.consume_pair_integrals()


@pytest.mark.parametrize("d", [64, 65, 129])
def test_arrow_pattern(gpu_pkg, d):
    """coordinate 0 paired with every other: 63, 64 and 128 partners -- one round of the wavefront short of a lane, exactly one, and two rounds
    and more; 700 events per chain, a third of them of coordinate 0, in one slice and in three; both orientations"""
    pkg = gpu_pkg
    rng = np.random.default_rng(d)
    x0, th0 = 0.3 * rng.standard_normal((2, d)), rng.choice([-1.0, 1.0], (2, d))
    evs = [busy_trace(rng, d, 700, x0[k], th0[k], [0]) for k in range(2)]
    pi, pj = np.zeros(d - 1, dtype=np.int64), np.arange(1, d, dtype=np.int64)
    cen = 0.1 * rng.standard_normal(d)
    S, J, T = run_events(pkg, x0, th0, evs, pi, pj, cen)
    for k in range(2):
        ref = PR.fact(0.0, x0[k], th0[k], evs[k], pi, pj, cen)
        assert same_bits(S[k], ref[0]) and same_bits(J[k], ref[1]) and T[k] == ref[2]
    S3, J3, T3 = run_events(pkg, x0, th0, evs, pi, pj, cen, cuts=[[0, 63, 64, 700], [0, 300, 301, 700]])
    assert same_bits(S3, S) and same_bits(J3, J) and same_bits(T3, T)
    Sr, Jr, _ = run_events(pkg, x0, th0, evs, pj, pi, cen)  # (i, j) with i > j
    assert same_bits(Sr, S) and same_bits(Jr, J)
    both = d == 65  # ... and with (0, 0) and the partners' own diagonals in the list: rows of 65 and 2
    if both:
        pi2, pj2 = np.concatenate([pi, np.arange(d)]), np.concatenate([pj, np.arange(d)])
        S2, J2, _ = run_events(pkg, x0, th0, evs, pi2, pj2, cen)
        for k in range(2):
            ref = PR.fact(0.0, x0[k], th0[k], evs[k], pi2, pj2, cen)
            assert same_bits(S2[k], ref[0]) and same_bits(J2[k], ref[1])
        assert same_bits(S2[:, :d - 1], S)


def test_a_coordinate_in_no_pair_still_gets_its_J(gpu_pkg):
    pkg = gpu_pkg
    d = 6
    rng = np.random.default_rng(1)
    x0, th0 = rng.standard_normal((2, d)), rng.choice([-1.0, 1.0], (2, d))
    evs = [busy_trace(rng, d, 200, x0[k], th0[k], [2, 3]) for k in range(2)]
    S, J, T = run_events(pkg, x0, th0, evs, [0], [1])
    for k in range(2):
        ref = PR.fact(0.0, x0[k], th0[k], evs[k], [0], [1])
        assert same_bits(S[k], ref[0]) and same_bits(J[k], ref[1]) and np.all(J[k] != 0)


# ------------------------------------------------------------------------------------------------------------------- sampler runs, factorised

def direct_spdmp(pkg, target, flow, x0, th0, c, T_slices, seed, cap, pi, pj, cen=None, adapt=False, sticky=None):
    """the loop of spdmp on an ensemble: per slice run -> consume -> drain, a read after every slice.  The last slice runs as spdmp does (the
    reference's tail: `while t′ < T`), the earlier ones pause before their end time (resumable, exact): however T is cut, the trace is the one
    of a single run to T.  Returns (traces, (S, J, T_last), reads after each slice with the number of events each chain had then)."""
    L = pkg._lib
    nch, d = x0.shape
    kw = dict(sampler=L.SAMPLER_STICKY_ZIGZAG, factor=1.5) if sticky is not None else dict(factor=1.8)
    reads = []
    with pkg.Ensemble(nch, d, trace_capacity=cap, adapt=adapt, **kw) as ens:
        ens.set_flow(flow)
        ens.set_target(target)
        if sticky is not None:
            ens.set_sticky(sticky)
        ens.set_state(0.0, x0, th0, c, np.uint64(seed) + np.arange(nch, dtype=np.uint64))
        ens.consume_begin()
        ens.consume_pairs(pi, pj, cen)
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
            reads.append((ens.consume_pair_integrals(), [sum(len(e) for e in evs[k]) for k in range(nch)]))
        out = ens.consume_pair_integrals()
    return [pkg.FactTrace(None, 0.0, x0[k], th0[k], np.concatenate(evs[k])) for k in range(nch)], out, reads


def against_ref(traces, out, pi, pj, cen=None):
    for k, tr in enumerate(traces):
        ref = PR.of_trace(tr, pi, pj, cen)
        assert same_bits(out[0][k], ref[0]) and same_bits(out[1][k], ref[1]) and out[2][k] == ref[2], k


def three_ways(pkg, target, flow, x0, th0, c, T, seed, pi, pj, cen=None, min_events=200, **kw):
    """One shot with room for the whole trace, five slices with a read after each, and a trace buffer of a seventh of the events: the same
    trace bytes and the same bits of S, J, T_last, equal to the contract on the trace; every read midway is the contract on the events
    consumed until then.  Returns the one-shot run's (traces, (S, J, T_last))."""
    args = (pkg, target, flow, x0, th0, c)
    big = 1 << 14
    tr1, out1, _ = direct_spdmp(*args, [T], seed, big, pi, pj, cen, **kw)
    against_ref(tr1, out1, pi, pj, cen)
    n = max(len(t.events) for t in tr1)
    assert min_events < n < big, n
    tr5, out5, reads = direct_spdmp(*args, [0.2 * T, 0.4 * T, 0.6 * T, 0.8 * T, T], seed, big, pi, pj, cen, **kw)
    tr7, out7, _ = direct_spdmp(*args, [T], seed, n // 7, pi, pj, cen, **kw)
    for tr, out in ((tr5, out5), (tr7, out7)):
        assert all(a.events.tobytes() == b.events.tobytes() for a, b in zip(tr1, tr))
        assert all(same_bits(a, b) for a, b in zip(out1, out))
    assert len(reads) == 5 and 0 < reads[0][1][0] < reads[2][1][0] < reads[4][1][0]
    for (S, J, Tl), upto in reads:
        for k in range(len(tr5)):
            ref = PR.fact(0.0, x0[k], th0[k], tr5[k].events[:upto[k]], pi, pj, cen)
            assert same_bits(S[k], ref[0]) and same_bits(J[k], ref[1]) and Tl[k] == ref[2]
    return tr1, out1


@pytest.mark.parametrize("adapt", [False, True])
def test_spdmp_d8_dense(gpu_pkg, adapt):
    """test/maintest.jl's problem, dense pairs, 3 chains, with and without adapt: one shot, five slices, a buffer of a seventh of the events"""
    pkg = gpu_pkg
    G = pkg.problems.maintest_precision(8)
    rng = np.random.default_rng(4)
    x0, th0 = rng.random((3, 8)), rng.choice([-1.0, 1.0], (3, 8))
    c = (0.2 if adapt else 0.7) * pkg.problems.column_norms(G)
    pi, pj = np.tril_indices(8)
    cen = np.linspace(-0.5, 0.5, 8)
    flow = pkg.ZigZag(sp.csc_matrix(0.9 * G), np.zeros(8))
    tr1, out1 = three_ways(pkg, pkg.GaussianTarget(G), flow, x0, th0, c, 60.0, 3, pi, pj, cen, adapt=adapt)
    # the consume= keyword of spdmp returns the arrays of the direct calls
    res = pkg.spdmp(pkg.GaussianTarget(G), 0.0, x0, th0, 60.0, c, flow, seed=3, adapt=adapt, trace_capacity=100, consume=dict(cov=(pi, pj), center=cen))
    extra = res[-1]
    assert all(a.events.tobytes() == b.events.tobytes() for a, b in zip(tr1, res[0]))
    assert same_bits(extra["pair_S"], out1[0]) and same_bits(extra["pair_J"], out1[1]) and same_bits(extra["T"], out1[2])
    assert np.array_equal(extra["pairs"][0], pi) and np.array_equal(extra["pairs"][1], pj)


def test_lattice_gamma_pattern(gpu_pkg):
    """A 12 x 12 lattice with the pattern of Γ as the pair set (consume=dict(cov=Γ) builds the same list): one shot, five slices with a read after
    each, a buffer of a seventh -- identical bits; the reads midway are the contract on the trace so far"""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(12)
    A = sp.coo_matrix(sp.tril(G, -1))
    key = np.unique(A.row.astype(np.int64) * 144 + A.col)
    pi, pj = np.concatenate([np.arange(144), key // 144]), np.concatenate([np.arange(144), key % 144])
    rng = np.random.default_rng(8)
    x0, th0 = pkg.problems.gmrf_stationary_sample(12, 2, rng), rng.choice([-1.0, 1.0], (2, 144))
    c = pkg.problems.column_norms(G)
    flow = pkg.ZigZag(G, np.zeros(144))
    tr1, out1 = three_ways(pkg, pkg.GaussianTarget(G), flow, x0, th0, c, 10.0, 5, pi, pj, min_events=700)
    res = pkg.spdmp(pkg.GaussianTarget(G), 0.0, x0, th0, 10.0, c, flow, seed=5, trace_capacity=8192, consume=dict(cov=G))
    assert np.array_equal(res[-1]["pairs"][0], pi) and np.array_equal(res[-1]["pairs"][1], pj)
    assert same_bits(res[-1]["pair_S"], out1[0]) and same_bits(res[-1]["pair_J"], out1[1])


def test_sspdmp_d8(gpu_pkg):
    """the sticky ZigZag at d = 8 (freezes: θ = 0 pieces): one shot, five slices, a buffer of a seventh; and through sspdmp(consume=dict(cov="diag"))"""
    pkg = gpu_pkg
    G = pkg.problems.maintest_precision(8)
    rng = np.random.default_rng(12)
    x0, th0 = rng.standard_normal((2, 8)), rng.choice([-1.0, 1.0], (2, 8))
    c = pkg.problems.column_norms(G)
    kappa = np.full(8, 0.8)
    pi, pj = np.tril_indices(8)
    flow = pkg.ZigZag(G, np.zeros(8))
    tr1, out1 = three_ways(pkg, pkg.GaussianTarget(G), flow, x0, th0, c, 40.0, 9, pi, pj, min_events=100, sticky=kappa)
    assert any(np.any(t.events["theta"] == 0) for t in tr1)
    res = pkg.sspdmp(pkg.GaussianTarget(G), 0.0, x0, th0, 40.0, c, flow, kappa, seed=9, trace_capacity=4096, consume=dict(cov="diag"))
    dg = np.flatnonzero(pi == pj)
    assert all(a.events.tobytes() == b.events.tobytes() for a, b in zip(tr1, res[0]))
    assert same_bits(res[-1]["pair_S"], out1[0][:, dg]) and same_bits(res[-1]["pair_J"], out1[1])


def test_bridge_neighbouring_coefficients(gpu_pkg):
    """the diffusion bridge at L = 3 (self-moving gradient, adapt), pairs of neighbouring coefficients and the diagonal: one shot, five slices,
    a buffer of a seventh; and through spdmp(consume=dict(cov=...))"""
    pkg = gpu_pkg
    L_, T = 3, 2.0
    xi0, th0, c = pkg.problems.diffusion_bridge_problem(L_, T, 0.0, 0.0, nchains=2, rng=np.random.default_rng(3))
    d = xi0.shape[1]
    pi, pj = np.concatenate([np.arange(d), np.arange(d - 1)]), np.concatenate([np.arange(d), np.arange(1, d)])
    flow = pkg.ZigZag(sp.identity(d, format="csc"), np.zeros(d))
    tr1, out1 = three_ways(pkg, pkg.DiffusionBridgeTarget(L_, T), flow, xi0, th0, c, 60.0, 11, pi, pj, min_events=600, adapt=True)
    res = pkg.spdmp(pkg.DiffusionBridgeTarget(L_, T), 0.0, xi0, th0, 60.0, c, flow, adapt=True, seed=11, trace_capacity=300, consume=dict(cov=(pi, pj)))
    assert all(a.events.tobytes() == b.events.tobytes() for a, b in zip(tr1, res[0]))
    assert same_bits(res[-1]["pair_S"], out1[0]) and same_bits(res[-1]["pair_J"], out1[1]) and same_bits(res[-1]["T"], out1[2])


# ------------------------------------------------------------------------------------------------------------------- the Bouncy Particle family

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


@pytest.mark.parametrize("name", ["one", "neg", "d63", "d65", "sparse", "sticky130", "c1024"])
def test_hand_made_pdmp_traces(gpu_pkg, name):
    """d = 1, t0 < 0, 63 and 65 coordinates (one strip and past it), two chains with a segment that gives one of them nothing, a sticky trace over
    three mask words, d = 1024: after every segment S, J and T_last are the contract's on the trace so far; mean and the grid are unchanged"""
    pkg = gpu_pkg
    c = PC.case(name)
    rng = np.random.default_rng(5)
    sel = np.sort(rng.choice(c.d, min(c.d, 9), replace=False))
    pi, pj = dense(sel)
    if c.d > 64:  # ... and a pair across two strips / mask words, in the other orientation
        pi, pj = np.concatenate([pi, [c.d - 1]]), np.concatenate([pj, [0]])
        keep = ~((pi[:-1] == 0) & (pj[:-1] == c.d - 1))
        pi, pj = np.concatenate([pi[:-1][keep], pi[-1:]]), np.concatenate([pj[:-1][keep], pj[-1:]])
    cen = None if name == "one" else rng.standard_normal(c.d)
    plain = []
    for with_pairs in (False, True):
        with open_bps(pkg, c) as ens:
            if with_pairs:
                ens.bps_consume_pairs(pi, pj, cen)
            for s in range(c.nseg):
                for k in range(c.nchains):
                    t, x, th, f = c.segment(k, s)
                    if not (c.sticky and s == 0):  # (a sticky ensemble holds the event its set_state_bps wrote: the case's first segment)
                        ens.debug_bps_trace_append(k, t, x, th, f)
                ens.bps_consume()
                assert ens.last_consume_ms() >= 0.0  # (the slice's consumers are timed by the same pair of device events, with pairs as without)
                if with_pairs:
                    S, J, T = ens.bps_consume_pair_integrals()
                    for k in range(c.nchains):
                        t, x, th, f = c.so_far(k, s)
                        ref = PR.pdmp(c.t0, c.x0[k], c.th0[k], t, x, th, pi, pj, cen, f=f)
                        assert same_bits(S[k], ref[0]) and same_bits(J[k], ref[1]) and T[k] == ref[2], (s, k)
                    assert all(same_bits(a, b) for a, b in zip(ens.bps_consume_pair_integrals(), (S, J, T)))
                if s not in c.grow:
                    ens.trace_reset()
            plain.append([ens.bps_consume_mean()[0]] + ([ens.bps_consume_discretized(k)[1] for k in range(c.nchains)] if name != "short_grid" else []))
    assert all(same_bits(a, b) for a, b in zip(*plain))


@pytest.mark.parametrize("d,sticky", [(16, False), (1, False), (65, False), (8, True)])
def test_bps_sampler_runs(gpu_pkg, d, sticky):
    """pdmp on a BouncyParticle (d = 16: the diagonal and a dense 8 x 8 block; d = 1; d = 65: past one strip) and its sticky form through sspdmp
    (d = 8), with consume=dict(cov=...): a buffer for the whole run and one of 48 events give identical bits, equal to the contract on the trace"""
    pkg = gpu_pkg
    rng = np.random.default_rng(9 + d)
    x0, th0 = rng.standard_normal((2, d)), rng.standard_normal((2, d))
    B = pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0)
    if d == 16:
        a, b = np.tril_indices(8, -1)
        pi, pj = np.concatenate([np.arange(16), a + 4]), np.concatenate([np.arange(16), b + 4])
    elif d == 65:
        pi, pj = np.concatenate([np.arange(65), [64, 0, 63]]), np.concatenate([np.arange(65), [0, 63, 64]])
    else:
        pi, pj = np.tril_indices(d)
    cen = 0.1 * rng.standard_normal(d)
    run = (lambda cap: pkg.sspdmp(None, 0.0, x0, th0, 60.0, 0.5, B, 1.5, seed=5, trace_capacity=cap, consume=dict(cov=(pi, pj), center=cen))) if sticky \
        else (lambda cap: pkg.pdmp(None, 0.0, x0, th0, 60.0, 1e-3, B, seed=5, trace_capacity=cap, consume=dict(cov=(pi, pj), center=cen)))
    big, small = run(4096), run(48)
    for k in range(2):
        assert 48 < len(big[0][k].t) < 4096 and same_bits(big[0][k].t, small[0][k].t)  # (several slices of the small buffer)
        assert (big[0][k].f is not None and not big[0][k].f.all()) == sticky
    for res in (big, small):
        against_ref(res[0], (res[-1]["pair_S"], res[-1]["pair_J"], res[-1]["T"]), pi, pj, cen)
    assert same_bits(big[-1]["pair_S"], small[-1]["pair_S"]) and same_bits(big[-1]["pair_J"], small[-1]["pair_J"])
    plain = (pkg.sspdmp(None, 0.0, x0, th0, 60.0, 0.5, B, 1.5, seed=5, trace_capacity=48, consume=dict())) if sticky \
        else pkg.pdmp(None, 0.0, x0, th0, 60.0, 1e-3, B, seed=5, trace_capacity=48, consume=dict())
    assert set(small[-1]) - set(plain[-1]) == {"pairs", "pair_S", "pair_J"} and same_bits(small[-1]["mean"], plain[-1]["mean"])


# ------------------------------------------------------------------------------------------------------------------- coexistence, covariance, refusals

def test_pairs_beside_condition_and_cummean(gpu_pkg):
    """one ensemble with a condition, cummean and pairs: mean, the grid, the cummean pairs and the hits are byte for byte those of the same run
    without pairs, and last_consume_ms is produced by the same calls"""
    pkg = gpu_pkg
    c = CC.case("few")
    pi, pj = dense(np.arange(c.d))
    p, n = np.zeros(c.d), np.zeros(c.d)
    p[1], n[1] = 1.0, 1.0
    got = []
    for with_pairs in (False, True):
        with open_fact(pkg, c) as ens:
            ens.consume_cummean(True)
            ens.consume_condition(p, n, 64)
            if with_pairs:
                ens.consume_pairs(pi, pj)
            cm = []
            held = 0
            for s in range(c.nseg):
                seg = c.segment(0, s)
                ens.debug_trace_append(0, seg)
                ens.consume()
                with pytest.raises(pkg._lib.PdmpError, match="no asynchronous consumer"):  # (the synchronous consumer keeps no timing: with pairs as without)
                    ens.last_consume_ms()
                if len(seg):
                    cm.extend(ens.consume_cummean_pairs(0, len(seg), first=held))
                if s in c.grow:
                    held += len(seg)
                else:
                    ens.trace_reset()
                    held = 0
            ht, hx, nh = ens.consume_conditioned(0)
            assert nh > 0
            got.append([ens.consume_mean()[0], ens.consume_discretized(0)[1], ht, hx] + cm)
            if with_pairs:
                S, J, T = ens.consume_pair_integrals()
                ref = PR.fact(c.t0, c.x0[0], c.th0[0], c.events[0], pi, pj)
                assert same_bits(S[0], ref[0]) and same_bits(J[0], ref[1])
    assert len(got[0]) == len(got[1]) and all(same_bits(a, b) for a, b in zip(*got))


def test_covariance_of_the_device_chains(gpu_pkg):
    """trace.covariance on the device's own integrals, test/maintest.jl's problem, T = 1000 and c = 0.7 ‖Γ[:, i]‖, 16 chains pooled: inside the
    reference's envelope mean|cov − Γ⁻¹| < 2.5/√T = 0.0791 (observed on the MI355X: 0.0043); the chains alone too (pooled=False)"""
    pkg = gpu_pkg
    G = pkg.problems.maintest_precision(8)
    rng = np.random.default_rng(2)
    x0, th0 = rng.random((16, 8)), rng.choice([-1.0, 1.0], (16, 8))
    pi, pj = np.tril_indices(8)
    res = pkg.spdmp(pkg.GaussianTarget(G), 0.0, x0, th0, 1000.0, 0.7 * pkg.problems.column_norms(G), pkg.ZigZag(sp.csc_matrix(0.9 * G), np.zeros(8)),
                    seed=2, trace=False, trace_capacity=2048, consume=dict(cov=(pi, pj)))
    extra = res[-1]
    inv = np.linalg.inv(G.toarray())
    cov, mean = pkg.trace.covariance(pi, pj, extra["pair_S"], extra["pair_J"], extra["T"])
    dev = np.mean(np.abs(cov.toarray() - inv))
    print("16 device chains: mean|cov - inv| = %.4g, envelope %.4g" % (dev, 2.5 / np.sqrt(1000.0)))
    assert dev < 2.5 / np.sqrt(1000.0) and np.mean(np.abs(mean)) < 2 / np.sqrt(1000.0)
    each = pkg.trace.covariance(pi, pj, extra["pair_S"], extra["pair_J"], extra["T"], pooled=False)
    assert np.mean([np.mean(np.abs(cv.toarray() - inv)) for cv, _ in each]) < 2.5 / np.sqrt(1000.0)


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
    ev = np.array([(1.0, 0, 1.0, -1.0)], dtype=EV)

    def fact(begin=True):
        ens = pkg.Ensemble(1, d, trace_capacity=8)
        ens.set_flow(pkg.ZigZag(G, np.zeros(d)))
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

    def common(ens, pairs, integrals, raw, raw_read, first_word):
        h = ens._h
        err = lambda: L.load().pdmp_last_error().decode()
        assert raw(h, 0, one.ctypes.data, one.ctypes.data, None) == INV and "npairs" in err()
        assert raw(h, 1, None, one.ctypes.data, None) == INV and "null" in err()
        assert raw(h, 1, one.ctypes.data, None, None) == INV and "null" in err()
        assert raw(h, 1 << 40, one.ctypes.data, one.ctypes.data, None) == INV and "GiB" in err()  # refused before the list is read
        refused(L, INV, "outside", pairs, [0], [d])
        refused(L, INV, "outside", pairs, [-1], [0])
        refused(L, INV, "twice", pairs, [0, 1, 0], [1, 2, 1])
        refused(L, INV, "twice", pairs, [0, 1], [1, 0])  # either orientation
        refused(L, INV, "finite", pairs, [0], [1], np.array([0.0, np.nan] + [0.0] * (d - 2)))
        refused(L, INV, first_word, integrals)
        pairs([0, 1], [1, 1])
        assert raw_read(h, 0, 2, None, None, None, None) == INV and raw_read(h, -1, 1, None, None, None, None) == INV  # the chain range
        assert raw_read(h, 0, 1, None, None, None, None) == 0  # any output may be NULL

    with fact() as ens:
        common(ens, ens.consume_pairs, ens.consume_pair_integrals, ens._L.pdmp_ensemble_consume_pairs, ens._L.pdmp_ensemble_consume_pair_integrals,
               "consume_pairs first")
        refused(L, INV, "PDMP_SAMPLER_BPS", ens.bps_consume_pairs, [0], [0])  # the other family's call
        refused(L, UNS, "synchronous", ens.consume_async)
        ens.debug_trace_append(0, ev)
        ens.consume()
        refused(L, INV, "first consume", ens.consume_pairs, [0], [0])
        S, J, T = ens.consume_pair_integrals()
        assert same_bits(S, [[1 / 3.0, 1 / 3.0]]) and same_bits(J[0, :2], [0.5, 0.5]) and T[0] == 1.0  # x_0 = x_1 = t on [0, 1]: ∫ t² = 1/3
    with fact(begin=False) as ens:
        refused(L, INV, "consume_begin", ens.consume_pairs, [0], [0])
    with bps() as ens:
        common(ens, ens.bps_consume_pairs, ens.bps_consume_pair_integrals, ens._L.pdmp_ensemble_bps_consume_pairs,
               ens._L.pdmp_ensemble_bps_consume_pair_integrals, "bps_consume_pairs first")
        refused(L, INV, "PDMP_SAMPLER_BPS", ens.consume_pairs, [0], [0])
        ens.bps_consume()
        refused(L, INV, "first bps_consume", ens.bps_consume_pairs, [0], [0])
    with bps(begin=False) as ens:
        refused(L, INV, "bps_consume_begin", ens.bps_consume_pairs, [0], [0])
    with bps(flow="boom") as ens:
        refused(L, UNS, "Boomerang", ens.bps_consume_pairs, [0], [0])
    with bps(flow="modern") as ens:
        refused(L, UNS, "speed-recorded", ens.bps_consume_pairs, [0], [0])
    with bps(subsample=True) as ens:
        refused(L, UNS, "subsample", ens.bps_consume_pairs, [0], [0])
    with pytest.raises(TypeError, match="cov=P"):
        pkg.pdmp(None, 0.0, np.zeros(d), np.ones(d), 1.0, 1e-3, pkg.BouncyParticle(G, np.zeros(d), 1.0), consume=dict(center=np.zeros(d)))
    with pytest.raises(TypeError, match="consume=dict"):
        pkg.pdmp(None, 0.0, np.zeros(d), np.ones(d), 1.0, 1e-3, pkg.BouncyParticle(G, np.zeros(d), 1.0), consume=dict(cove="diag"))
