"""The conditional trace on the device (pdmp_ensemble_[bps_]consume_condition / _conditioned; csrc/pdmp_consume.hip, csrc/pdmp_consume_bps.hip;
-m gpu) against the sequential statement of its contract, tests/ref/condition_ref.c, BIT FOR BIT:

  1. hand-made traces through pdmp_debug_trace_append / pdmp_debug_bps_trace_append, two chains with different traces: every way a piece can
     end (a hit inside it, h = 0 with g = 0 and g != 0, τ < 0, a hit exactly at the closing event, the T_last rule), one piece spread over three
     slices, events of S at slots 255 and 256 of a 600-event slice, two events of a coordinate outside S around a hit, more hits than rows; the
     ordinary consumers of the same ensemble unchanged;
  2. end to end: the device's hits equal trace.conditional_trace of the trace the same run returned;
  3. every refusal, by status and by the word in the message."""
import numpy as np
import pytest
import scipy.sparse as sp

import condition_ref_lib as CR

pytestmark = pytest.mark.gpu

EV = CR.EVENT_DTYPE


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def events(rows):
    return np.array(rows, dtype=EV)


# ------------------------------------------------------------------------------------------------------------------- factorised

def flip_trace(rng, d, K, x0, th0, only=None, t0=0.0):
    """K events of a continuous path that stays near 0: at every event the coordinate that runs away from 0 fastest turns round (with noise, so
    that chains differ).  only: the coordinates that may have events."""
    t, x, th, tc = t0, x0.copy(), th0.copy(), np.full(d, t0)
    who = np.arange(d) if only is None else np.asarray(only)
    out = np.empty(K, dtype=EV)
    for k in range(K):
        t = t + rng.uniform(0.01, 0.2)
        pos = x[who] + th[who] * (t - tc[who])
        i = who[np.argmax(pos * th[who] + 0.3 * rng.standard_normal(len(who)))]
        x[i] = x[i] + th[i] * (t - tc[i])
        tc[i] = t
        th[i] = -th[i] if th[i] != 0 else 1.0
        out[k] = (t, i, x[i], th[i])
    return out


def run_fact(pkg, x0, th0, evs, p, n, max_hits, cuts=None, t0=0.0, cap=None, condition=True, grid=(0.25, 64)):
    """begin, [condition,] then per slice append -> consume -> trace_reset.  evs: one event array per chain; cuts: slice boundaries per chain.
    Returns (per chain (t, x, nhits), mean, per chain grid rows)."""
    nch, d = x0.shape
    cuts = cuts or [[0, len(e)] for e in evs]
    cap = cap or max(max(len(e) for e in evs), 1)
    G = sp.identity(d, format="csc")
    with pkg.Ensemble(nch, d, trace_capacity=cap) as ens:
        ens.set_flow(pkg.ZigZag(G, np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_state(t0, x0, th0, np.ones(d), np.arange(nch, dtype=np.uint64) + 1)
        ens.consume_begin(*grid)
        if condition:
            ens.consume_condition(p, n, max_hits)
        for s in range(len(cuts[0]) - 1):
            for k in range(nch):
                ens.debug_trace_append(k, evs[k][cuts[k][s]:cuts[k][s + 1]])
            ens.consume()
            ens.trace_reset()
        hits = [ens.consume_conditioned(k) for k in range(nch)] if condition else None
        raw = None
        if condition:  # every reserved row, through the C entry point: rows behind the hits still hold the zeros condition put there
            raw = []
            for k in range(nch):
                t, x = np.empty(max_hits), np.empty((max_hits, d))
                assert ens._L.pdmp_ensemble_consume_conditioned(ens._h, k, 0, max_hits, t.ctypes.data, x.ctypes.data, None, None) == 0
                raw.append((t, x))
        mean = ens.consume_mean()[0]
        rows = []
        for k in range(nch):
            out = np.empty((grid[1], d))
            assert ens._L.pdmp_ensemble_consume_discretized(ens._h, k, 0, grid[1], out.ctypes.data, None, None) == 0
            rows.append(out)
    return hits, mean, rows, raw


def check_fact(pkg, x0, th0, evs, p, n, max_hits, min_hits, t0=0.0, **kw):
    hits, mean, rows, raw = run_fact(pkg, x0, th0, evs, p, n, max_hits, t0=t0, **kw)
    refs = []
    for k in range(len(evs)):
        ref = CR.fact(t0, x0[k], th0[k], evs[k], p, n, max_hits=max_hits)
        t, x, nh = hits[k]
        assert nh == ref["nhits"] >= min_hits, (k, nh, ref["nhits"])
        assert same_bits(t, ref["t"]) and same_bits(x, ref["x"]), k
        m = len(ref["t"])
        assert same_bits(raw[k][0][:m], ref["t"]) and not raw[k][0][m:].view(np.uint64).any() and not raw[k][1][m:].view(np.uint64).any()
        tr = pkg.FactTrace(None, t0, x0[k], th0[k], evs[k])  # ... and the host mirror on the same trace
        ht, hx = pkg.trace.conditional_trace(tr, p, n)
        assert same_bits(ht[:max_hits], ref["t"]) and same_bits(hx[:max_hits], ref["x"])
        refs.append(ref)
    return refs, mean, rows


def test_every_way_a_piece_ends(gpu_pkg):
    """d = 5, S = {2}, p_2 = 0.5, exactly representable numbers.  Chain 0, the events of coordinate 2:
         t = 1    from (0, 0, +1): τ = 0.5, a hit INSIDE the piece at 0.5 -- between the two events of coordinate 0 at 0.25 and 0.75: row_0 comes
                  from the event at 0.25
         t = 1.5  from (1, 1, −1): τ = 0.5, s = 1.5 = t_e: a hit exactly AT the closing event (inclusive)
         t = 2    from (1.5, 0.5, +1): g = 0, τ = 0: no candidate
         t = 2.5  from (2, 1, 0): h = 0, g != 0: τ = −Inf
         t = 3    from (2.5, 0.5, 0): h = 0, g = 0: NaN
         t = 4    from (3, 0.25, −1): τ = −0.25 < 0
         then from (4, 0, +1): s = 4.5 behind the last event of S; an event of coordinate 0 at 4.25 (before s) and one at 5 (T_last >= s): a hit.
       Chain 1: the same, but its last event lies at 4.375 < s: no hit beyond T_last."""
    pkg = gpu_pkg
    d = 5
    x0, th0 = np.zeros((2, d)), np.ones((2, d))
    head = [(0.25, 0, 0.25, -1.0), (0.5, 4, 0.5, -1.0), (0.75, 0, -0.25, 1.0), (1.0, 2, 1.0, -1.0), (1.25, 1, 1.25, -1.0), (1.5, 2, 0.5, 1.0),
            (2.0, 2, 1.0, 0.0), (2.25, 3, 2.25, -1.0), (2.5, 2, 0.5, 0.0), (3.0, 2, 0.25, -1.0), (4.0, 2, 0.0, 1.0), (4.25, 0, 3.25, -1.0)]
    evs = [events(head + [(5.0, 0, 2.5, 1.0)]), events(head + [(4.375, 1, -1.875, 1.0)])]
    p, n = np.zeros(d), np.zeros(d)
    p[2], n[2] = 0.5, 1.0
    refs, _, _ = check_fact(pkg, x0, th0, evs, p, n, 8, 2)
    assert same_bits(refs[0]["t"], [0.5, 1.5, 4.5]) and same_bits(refs[1]["t"], [0.5, 1.5])
    assert same_bits(refs[0]["x"][0], [0.0, 0.5, 0.5, 0.5, 0.5])  # row_0 from the event at 0.25, row_4 from (t0, x0, θ0): its event lies AT s


@pytest.mark.parametrize("d,S", [(5, [1, 3]), (70, list(range(3, 68))), (130, list(range(130)))])
def test_random_traces_whole_and_in_three_slices(gpu_pkg, d, S):
    """|S| = 2, 65 (a second list slot per lane) and 130 (dense), 300 or 1200 events per chain -- several chunks; sliced in three, the hits are
    those of the unsliced call, and     mean / discretize of the same ensemble are what they are without a condition"""
    pkg = gpu_pkg
    rng = np.random.default_rng(d)
    x0, th0 = 0.2 * rng.standard_normal((2, d)), rng.choice([-1.0, 1.0], (2, d))
    K = 300 if d == 5 else 1200
    evs = [flip_trace(rng, d, K, x0[k], th0[k]) for k in range(2)]
    n = np.zeros(d)
    n[S] = rng.standard_normal(len(S))
    p = 0.02 * rng.standard_normal(d)
    refs, mean, rows = check_fact(pkg, x0, th0, evs, p, n, 400, 8)
    cuts = [[0, 90, K - 89, K], [0, 130, 131, K]]
    refs3, mean3, rows3 = check_fact(pkg, x0, th0, evs, p, n, 400, 8, cuts=cuts, cap=K)
    _, mean0, rows0, _ = run_fact(pkg, x0, th0, evs, p, n, 400, cuts=cuts, cap=K, condition=False)
    assert same_bits(mean3, mean0) and all(same_bits(a, b) for a, b in zip(rows3, rows0))  # coexistence: the ordinary consumers are unchanged


def test_one_piece_over_three_slices(gpu_pkg):
    """S = {2}: an event of S at 0.5 opens a piece with s = 4.5; the slices end at 2.5, 6.5 and 10.5: the hit is found at the end of the second
    slice (T_last >= s), its row from the events before 4.5 -- part of them in that slice --, and the event of S at 10.5 does not find it again"""
    pkg = gpu_pkg
    d = 5
    rng = np.random.default_rng(2)
    x0, th0 = np.zeros((2, d)), np.ones((2, d))
    evs, cuts = [], []
    for k in range(2):
        other = flip_trace(rng, d, 40, x0[k], th0[k], only=[0, 1, 3, 4])
        other["t"] = 1.0 + 0.25 * np.arange(40) + 0.0625 * k  # 1.0 ... 10.75
        ev = np.concatenate([events([(0.5, 2, -1.0, 1.0)]), other[other["t"] < 10.5], events([(10.5, 2, 9.0, -1.0)])])
        evs.append(ev)
        cuts.append([0, int(np.sum(ev["t"] <= 2.5)), int(np.sum(ev["t"] <= 6.5)), len(ev)])
    p, n = np.zeros(d), np.zeros(d)
    p[2], n[2] = 3.0, 2.0
    refs, _, _ = check_fact(pkg, x0, th0, evs, p, n, 4, 1, cuts=cuts, cap=64)
    assert same_bits(refs[0]["t"], [4.5]) and same_bits(refs[1]["t"], [4.5])
    check_fact(pkg, x0, th0, evs, p, n, 4, 1)  # ... as in one slice


def test_events_of_S_at_the_chunk_boundary(gpu_pkg):
    """600 events in one slice, the events of S = {2} at slots 255 and 256 (the last of one 256-event chunk, the first of the next) and 500"""
    pkg = gpu_pkg
    d = 5
    rng = np.random.default_rng(4)
    x0, th0 = 0.1 * rng.standard_normal((2, d)), rng.choice([-1.0, 1.0], (2, d))
    th0[:, 2] = 1.0  # coordinate 2 climbs from about 0 to about 27 (slot 255), turns for one step, climbs on to about 52 (slot 500) and comes back
    evs = []
    for k in range(2):
        ev = flip_trace(rng, d, 600, x0[k], th0[k], only=[0, 1, 3, 4])
        x2, th2, tc = x0[k, 2], th0[k, 2], 0.0
        for slot in (255, 256, 500):
            t = ev["t"][slot]
            x2, tc, th2 = x2 + th2 * (t - tc), t, -th2
            ev[slot] = (t, 2, x2, th2)
        evs.append(ev)
    p, n = np.zeros(d), np.zeros(d)
    n[2] = 1.0
    for level in (5.0, 40.0):  # crossed by both chains: in the piece that ends at slot 255, and in the piece from slot 256 to slot 500
        p[2] = level
        check_fact(pkg, x0, th0, evs, p, n, 8, 1)
    p[2] = 0.5 * (evs[0]["x"][255] + evs[0]["x"][256])  # between the positions at slots 255 and 256: chain 0 crosses it in that piece
    refs, _, _ = check_fact(pkg, x0, th0, evs, p, n, 8, 0)
    assert np.any((refs[0]["t"] > evs[0]["t"][255]) & (refs[0]["t"] <= evs[0]["t"][256]))


def test_more_hits_than_rows(gpu_pkg):
    """coordinate 0 runs between −1 and 1 and crosses 0 five times; max_hits = 2: nhits == 5 and two rows"""
    pkg = gpu_pkg
    d = 5
    x0, th0 = np.zeros((2, d)), np.ones((2, d))
    zig = [(1.0, 0, 1.0, -1.0), (3.0, 0, -1.0, 1.0), (5.0, 0, 1.0, -1.0), (7.0, 0, -1.0, 1.0), (9.0, 0, 1.0, -1.0), (11.0, 0, -1.0, 1.0)]
    evs = [events(zig), events(zig[:4] + [(7.5, 3, 7.5, -1.0)])]
    p, n = np.zeros(d), np.zeros(d)
    n[0] = -3.0
    refs, _, _ = check_fact(pkg, x0, th0, evs, p, n, 2, 3)
    assert refs[0]["nhits"] == 5 and same_bits(refs[0]["t"], [2.0, 4.0]) and refs[1]["nhits"] == 3


# ------------------------------------------------------------------------------------------------------------------- Bouncy Particle family

def bps_trace(rng, d, K, x0, th0, t0=0.0, sticky=False):
    """K events of a continuous path pulled towards 0 (θ = −x + noise after every event); sticky: random free masks, frozen coordinates keep x"""
    t, x, th, f = t0, x0.copy(), th0.copy(), np.ones(d, dtype=bool)
    ts, xs, ths, fs = np.empty(K), np.empty((K, d)), np.empty((K, d)), np.ones((K, d), dtype=bool)
    for k in range(K):
        dt = rng.uniform(0.05, 0.6)
        t = t + dt
        x = np.where(f, x + th * dt, x)
        th = -x + 0.5 * rng.standard_normal(d)
        if sticky:
            f = rng.random(d) < 0.7
        ts[k], xs[k], ths[k], fs[k] = t, x, th, f
    return ts, xs, ths, fs


def run_bps(pkg, x0, th0, tr, p, n, max_hits, cuts=None, t0=0.0, sticky=False, cap=None):
    """tr: per chain (t, x, θ, f).  A sticky ensemble's buffer already holds the event set_state_bps wrote: (t0, x0, θ0, all free)."""
    nch, d = x0.shape
    cuts = cuts or [[0, len(c[0])] for c in tr]
    cap = cap or max(len(c[0]) for c in tr) + 1
    G = sp.identity(d, format="csc")
    with pkg.Ensemble(nch, d, sampler=pkg._lib.SAMPLER_BPS, factor=2.0, trace_capacity=cap) as ens:
        ens.set_flow_bps(pkg.BouncyParticle(G, np.zeros(d), 1.0))
        if sticky:
            ens.set_bps_sticky(np.full(d, 0.8))
        ens.set_state_bps(t0, x0, th0, 10.0, np.arange(nch, dtype=np.uint64) + 1)
        ens.bps_consume_begin(0.5, 16)
        ens.bps_consume_condition(p, n, max_hits)
        for s in range(len(cuts[0]) - 1):
            for k in range(nch):
                a, b = cuts[k][s], cuts[k][s + 1]
                t, x, th, f = tr[k]
                ens.debug_bps_trace_append(k, t[a:b], x[a:b], th[a:b], f[a:b] if sticky else None)
            ens.bps_consume()
            ens.trace_reset()
        return [ens.bps_consume_conditioned(k) for k in range(nch)]


def check_bps(pkg, x0, th0, tr, p, n, max_hits, min_hits, t0=0.0, sticky=False, **kw):
    hits = run_bps(pkg, x0, th0, tr, p, n, max_hits, t0=t0, sticky=sticky, **kw)
    refs = []
    for k in range(len(tr)):
        t, x, th, f = tr[k]
        if sticky:  # with the event set_state_bps wrote in front
            t, x, th, f = np.concatenate([[t0], t]), np.vstack([x0[k][None], x]), np.vstack([th0[k][None], th]), np.vstack([np.ones((1, len(x0[k])), dtype=bool), f])
        ref = CR.pdmp(t0, x0[k], th0[k], t, x, th, p, n, f=f if sticky else None, max_hits=max_hits)
        ht, hx, nh = hits[k]
        assert nh == ref["nhits"] >= min_hits, (k, nh, ref["nhits"])
        assert same_bits(ht, ref["t"]) and same_bits(hx, ref["x"]), k
        host = pkg.PDMPTrace(None, t0, x0[k], th0[k], t, x, th)
        if sticky:
            host.f0, host.f = np.ones(len(x0[k]), dtype=bool), f
        mt, mx = pkg.trace.conditional_trace(host, p, n)
        assert same_bits(mt[:max_hits], ref["t"]) and same_bits(mx[:max_hits], ref["x"])
        refs.append(ref)
    return refs


@pytest.mark.parametrize("d", [3, 64, 65, 130])
def test_bps_random_traces_whole_and_in_three_slices(gpu_pkg, d):
    pkg = gpu_pkg
    rng = np.random.default_rng(100 + d)
    x0, th0 = 0.3 * rng.standard_normal((2, d)), rng.standard_normal((2, d))
    tr = [bps_trace(rng, d, 70, x0[k], th0[k]) for k in range(2)]
    p, n = 0.02 * rng.standard_normal(d), rng.standard_normal(d)
    a = check_bps(pkg, x0, th0, tr, p, n, 100, 5)
    b = check_bps(pkg, x0, th0, tr, p, n, 100, 5, cuts=[[0, 20, 21, 70], [0, 33, 60, 70]], cap=64)
    assert all(same_bits(u["t"], v["t"]) for u, v in zip(a, b))
    c = check_bps(pkg, x0, th0, tr, p, n, 3, 5)  # more hits than rows
    assert all(len(u["t"]) == 3 and u["nhits"] > 3 for u in c)


def test_bps_sticky_mask_with_a_frozen_coordinate_in_the_support(gpu_pkg):
    pkg = gpu_pkg
    d = 8
    rng = np.random.default_rng(8)
    x0, th0 = 0.3 * rng.standard_normal((2, d)), rng.standard_normal((2, d))
    tr = [bps_trace(rng, d, 60, x0[k], th0[k], sticky=True) for k in range(2)]
    p, n = 0.02 * rng.standard_normal(d), rng.standard_normal(d)
    refs = check_bps(pkg, x0, th0, tr, p, n, 100, 5, sticky=True)
    assert not tr[0][3].all() and np.all(n != 0)  # frozen coordinates, all of them inside supp n
    for k in range(2):  # ... and some hit's row keeps a frozen coordinate where its cursor has it
        t, x, th, f = tr[k]
        seg = np.searchsorted(t, refs[k]["t"], side="right") - 1  # the event before each hit (−1: the initial state, all free)
        assert np.any(~f[seg[seg >= 0]])
    check_bps(pkg, x0, th0, tr, p, n, 100, 5, sticky=True, cuts=[[0, 7, 40, 60], [0, 1, 2, 60]], cap=64)


def test_bps_strict_end_first_segment_and_order(gpu_pkg):
    """d = 3, n = e_0, p_0 = 1, exactly representable.  Chain 0: from (0, 0, +1) the crossing lies exactly AT the first event (t = 1): no hit;
    then three hits in one slice, in order.  Chain 1: the first segment, from (t0, x0, θ0), holds a hit."""
    pkg = gpu_pkg
    d = 3
    x0, th0 = np.zeros((2, d)), np.tile([1.0, 0.0, 0.0], (2, 1))
    z, v = [0.0, 0.5, -0.5], [1.0, 0.0, 0.0]
    tr = [(np.array([1.0, 2.5, 4.0, 5.25, 6.0]), np.array([z] * 5), np.array([v] * 5), None),
          (np.array([1.5, 2.0, 4.0]), np.array([z] * 3), np.array([v] * 3), None)]
    p, n = np.array([1.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])
    refs = check_bps(pkg, x0, th0, tr, p, n, 8, 1)
    assert same_bits(refs[0]["t"], [2.0, 3.5, 5.0]) and same_bits(refs[1]["t"], [1.0, 3.0])
    assert same_bits(refs[0]["x"][0], [1.0, 0.5, -0.5]) and same_bits(refs[1]["x"][0], [1.0, 0.0, 0.0])


# ------------------------------------------------------------------------------------------------------------------- end to end

def run_ensemble(pkg, ens, T, trace_of):
    L = pkg._lib
    evs = [[] for _ in range(ens.nchains)]
    while True:
        ens.run(T, L.RUN_REFERENCE_TAIL)
        cnt = ens.counters()
        assert not np.any(cnt["status"] == L.CHAIN_BOUND_VIOLATED)
        ens.consume()
        for k in range(ens.nchains):
            evs[k].append(trace_of(k, cnt))
        ens.trace_reset()
        if not L.needs_rerun(cnt["status"]):
            return evs


@pytest.mark.parametrize("sticky", [False, True])
def test_spdmp_and_sspdmp_through_the_ensemble(gpu_pkg, sticky):
    """spdmp on the 8 x 8 GMRF, T = 50, conditioned on x_3 = x_12 (and the sticky ZigZag on the same field), the trace buffer far smaller than
    the trace: the device's hits are trace.conditional_trace of the trace the run returned"""
    pkg = gpu_pkg
    L = pkg._lib
    G = pkg.problems.gmrf_precision(8, 0.5 if sticky else 0.01)
    d, nch = 64, 2
    rng = np.random.default_rng(6)
    x0, th0 = pkg.problems.gmrf_stationary_sample(8, nch, rng, 0.5 if sticky else 0.01), rng.choice([-1.0, 1.0], (nch, d))
    p, n = np.zeros(d), np.zeros(d)
    n[3], n[12] = 1.0, -1.0
    kw = dict(sampler=L.SAMPLER_STICKY_ZIGZAG, factor=1.5) if sticky else {}
    with pkg.Ensemble(nch, d, trace_capacity=700, **kw) as ens:
        ens.set_flow(pkg.ZigZag(G, np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(G))
        if sticky:
            ens.set_sticky(np.full(d, 0.8))
        ens.set_state(0.0, x0, th0, 2.0 * pkg.problems.column_norms(G), np.arange(nch, dtype=np.uint64) + 40)
        ens.consume_begin()
        ens.consume_condition(p, n, 512)
        evs = run_ensemble(pkg, ens, 50.0, lambda k, cnt: ens.trace(k, counters=cnt))
        assert min(len(e) for e in evs) >= 3  # several slices
        for k in range(nch):
            tr = pkg.FactTrace(None, 0.0, x0[k], th0[k], np.concatenate(evs[k]))
            t, X = pkg.trace.conditional_trace(tr, p, n)
            ht, hx, nh = ens.consume_conditioned(k)
            assert nh == len(t) >= 10 and same_bits(ht, t) and same_bits(hx, X)
            assert np.allclose(hx[:, 3], hx[:, 12], rtol=0, atol=1e-12)


@pytest.mark.parametrize("sticky", [False, True])
def test_pdmp_and_sspdmp_bps_through_the_consume_keyword(gpu_pkg, sticky):
    """pdmp on a BouncyParticle at d = 16, and its sticky form through sspdmp, with consume=dict(..., condition=(p, n), hits=K), in several slices"""
    pkg = gpu_pkg
    d = 16
    rng = np.random.default_rng(9)
    x0, th0 = rng.standard_normal((2, d)), rng.standard_normal((2, d))
    B = pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0)
    p, n = 0.05 * rng.standard_normal(d), rng.standard_normal(d)
    run = (lambda **kw: pkg.sspdmp(None, 0.0, x0, th0, 60.0, 0.5, B, 1.5, seed=5, trace_capacity=48, **kw)) if sticky else \
          (lambda **kw: pkg.pdmp(None, 0.0, x0, th0, 60.0, 1e-3, B, seed=5, trace_capacity=48, **kw))
    out = run(consume=dict(dt=0.5, points=200, condition=(p, n), hits=256))
    traces, extra = out[0], out[-1]
    plain = run(consume=dict(dt=0.5, points=200))
    assert set(extra) - set(plain[-1]) == {"hit_t", "hit_x", "nhits"} and same_bits(extra["mean"], plain[-1]["mean"])
    for k in range(2):
        assert len(traces[k].t) > 3 * 48 and same_bits(traces[k].t, plain[0][k].t)
        assert (traces[k].f is not None and not traces[k].f.all()) == sticky
        t, X = pkg.trace.conditional_trace(traces[k], p, n)
        assert extra["nhits"][k] == len(t) >= 10 and same_bits(extra["hit_t"][k], t) and same_bits(extra["hit_x"][k], X)


def test_the_bridge_through_a_point(gpu_pkg):
    """spdmp with a DiffusionBridgeTarget at L = 3 and consume=dict(condition=bridge_point_condition(L, T, s, a)): every row is a bridge with X_s = a"""
    pkg = gpu_pkg
    L_, T, s, a = 3, 2.0, 0.7, 0.1
    xi0, th0, c = pkg.problems.diffusion_bridge_problem(L_, T, 0.0, 0.0, nchains=2, rng=np.random.default_rng(3))
    p, n = pkg.problems.bridge_point_condition(L_, T, s, a)
    target = pkg.DiffusionBridgeTarget(L_, T)
    d = xi0.shape[1]
    out = pkg.spdmp(target, 0.0, xi0, th0, 200.0, c, pkg.ZigZag(sp.identity(d, format="csc"), np.zeros(d)), adapt=True, seed=11, trace_capacity=400,
                    consume=dict(condition=(p, n), hits=8192))
    traces, extra = out[0], out[-1]
    for k in range(2):
        t, X = pkg.trace.conditional_trace(traces[k], p, n)
        assert extra["nhits"][k] == len(t) >= 10 and same_bits(extra["hit_t"][k], t) and same_bits(extra["hit_x"][k], X)
        assert np.allclose(pkg.trace.faber_schauder_path(extra["hit_x"][k], s, L_, T), a, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------- refusals

def refused(L, code, word, call, *a):
    with pytest.raises(L.PdmpError) as ei:
        call(*a)
    assert ei.value.code == code and word in str(ei.value), str(ei.value)


def test_refusals(gpu_pkg):
    pkg = gpu_pkg
    L = pkg._lib
    INV, UNS = L.PDMP_ERR_INVALID, L.PDMP_ERR_UNSUPPORTED
    d = 1100
    G = sp.identity(d, format="csc")
    p, n = np.zeros(d), np.zeros(d)
    n[0] = 1.0
    bad = n.copy()
    bad[5] = np.nan
    ev = events([(1.0, 0, 1.0, -1.0)])

    def fact(flow=None, begin=True):
        ens = pkg.Ensemble(1, d, trace_capacity=8)
        ens.set_flow(flow or pkg.ZigZag(G, np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_state(0.0, np.zeros((1, d)), np.ones((1, d)), np.ones(d), np.array([1], dtype=np.uint64))
        if begin:
            ens.consume_begin()
        return ens

    def bps(flow="bps", begin=True, subsample=False):
        ens = pkg.Ensemble(1, 8, sampler=L.SAMPLER_BPS, factor=2.0, trace_capacity=8)
        I8 = sp.identity(8, format="csc")
        if flow == "boom":
            ens.set_flow_boomerang(pkg.GaussianTarget(I8, np.zeros(8)), pkg.Boomerang(I8, np.zeros(8), 1.0))
        elif flow == "modern":
            ens.set_flow_bps_modern(1.0)
            ens.set_target(pkg.GaussianTarget(I8, np.zeros(8)))
        else:
            ens.set_flow_bps(pkg.BouncyParticle(I8, np.zeros(8), 1.0))
        if subsample:
            ens.set_bps_options(False, True)
        ens.set_state_bps(0.0, np.zeros((1, 8)), np.ones((1, 8)), 10.0, np.array([1], dtype=np.uint64))
        if begin:
            ens.bps_consume_begin()
        return ens

    p8, n8 = np.zeros(8), np.ones(8)
    with fact() as ens:
        h = ens._h
        assert ens._L.pdmp_ensemble_consume_condition(h, None, n.ctypes.data, 4) == INV and "null" in L.load().pdmp_last_error().decode()
        assert ens._L.pdmp_ensemble_consume_condition(h, p.ctypes.data, None, 4) == INV
        refused(L, INV, "finite", ens.consume_condition, bad, n, 4)
        refused(L, INV, "finite", ens.consume_condition, p, bad, 4)
        refused(L, INV, "zero", ens.consume_condition, p, np.zeros(d), 4)
        refused(L, INV, "max_hits", ens.consume_condition, p, n, 0)
        refused(L, INV, "GiB", ens.consume_condition, p, n, 1 << 40)  # rows beyond what a device holds: refused before any product is taken
        refused(L, INV, "GiB", ens.consume_condition, p, n, (1 << 63) - 1)
        refused(L, UNS, "1024", ens.consume_condition, p, np.ones(d), 4)  # |S| = 1100
        refused(L, INV, "consume_condition first", ens.consume_conditioned, 0)
        refused(L, INV, "PDMP_SAMPLER_BPS", ens.bps_consume_condition, p, n, 4)  # the other family's call
        ens.consume_condition(p, n, 4)
        refused(L, UNS, "synchronous", ens.consume_async)
        assert ens._L.pdmp_ensemble_consume_conditioned(h, 0, 0, 5, None, None, None, None) == INV  # first + count > max_hits
        assert ens._L.pdmp_ensemble_consume_conditioned(h, 1, 0, 1, None, None, None, None) == INV  # a bad chain
        assert ens._L.pdmp_ensemble_consume_conditioned(h, 0, 0, 4, None, None, None, None) == 0    # any output may be NULL
        ens.debug_trace_append(0, ev)
        ens.consume()
        refused(L, INV, "first consume", ens.consume_condition, p, n, 4)
    with fact(begin=False) as ens:
        refused(L, INV, "consume_begin", ens.consume_condition, p, n, 4)
    with fact(flow=pkg.FactBoomerang(G, np.zeros(d), 0.1), begin=False) as ens:
        refused(L, UNS, "Boomerang", ens.consume_condition, p, n, 4)
    with bps() as ens:
        refused(L, INV, "finite", ens.bps_consume_condition, np.full(8, np.inf), n8, 4)
        refused(L, INV, "zero", ens.bps_consume_condition, p8, np.zeros(8), 4)
        refused(L, INV, "max_hits", ens.bps_consume_condition, p8, n8, -1)
        refused(L, INV, "GiB", ens.bps_consume_condition, p8, n8, (1 << 63) - 1)
        refused(L, INV, "bps_consume_condition first", ens.bps_consume_conditioned, 0)
        refused(L, INV, "PDMP_SAMPLER_BPS", ens.consume_condition, p8, n8, 4)  # the other family's call
        assert ens._L.pdmp_ensemble_bps_consume_condition(ens._h, None, None, 4) == INV
        ens.bps_consume_condition(p8, n8, 4)
        ens.bps_consume()
        refused(L, INV, "first bps_consume", ens.bps_consume_condition, p8, n8, 4)
    with bps(begin=False) as ens:
        refused(L, INV, "bps_consume_begin", ens.bps_consume_condition, p8, n8, 4)
    with bps(flow="boom") as ens:
        refused(L, UNS, "Boomerang", ens.bps_consume_condition, p8, n8, 4)
    with bps(flow="modern") as ens:
        refused(L, UNS, "speed-recorded", ens.bps_consume_condition, p8, n8, 4)
    with bps(subsample=True) as ens:
        refused(L, UNS, "subsample", ens.bps_consume_condition, p8, n8, 4)
