"""The device trace consumers (csrc/pdmp_consume.hip) on the hand-made traces of tests/consumer_cases.py (-m gpu): events exactly at grid times,
256-long chains of one coordinate in one chunk, a forced clash in the per-chunk hash table, rows of 255 / 256 / 257 coordinates, many grid rows
between two events, a grid that runs out, a segment grown without a reset, t0 < 0, events sharing a time, −0.0 freezes, subtrace at every size.
A sampler cannot produce any of these; pdmp_debug_trace_append (include/pdmp_debug.h) puts them in front of the consumers through the C ABI:
consume_begin, then per segment append -> consume() -> checks against the trace SO FAR -> trace_reset().

References: trace.py (the device's grid t0 + k·dt, bit for bit) everywhere; oracle/trace_oracle.c bit for bit too where the case is dyadic
(tests/test_consumer_cases_ref.py holds the two to each other there, and shows that they part on the row* cases); for mean(Ξ) a host loop in the
kernel's documented arithmetic (bit for bit) and the exact rational mean of the same floats (within the sequential-summation bound).  Rows of the
grid buffer at and behind npoints are never written (a point is emitted while it lies BEFORE the last event, src/trace.jl:111): they must still
hold the zeros consume_begin put there -- an event that ends a segment exactly on a grid time does not emit that row."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import consumer_cases as CC
import oracle_lib as O

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-12, atol=1e-15)  # the project's tolerance for mean / inclusion_prob against trace.py and the oracle


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_events(a, b):
    return len(a) == len(b) and np.array_equal(a["i"], b["i"]) and all(same_bits(a[f], b[f]) for f in ("t", "x", "theta"))


def open_case(pkg, c, grid=True):
    """An ensemble in the state of case c, consume_begin done: nothing has run, the trace is empty"""
    L = pkg._lib
    assert CC.EVENT_DTYPE == L.EVENT_DTYPE
    G = sp.identity(c.d, format="csc")
    kw = dict(sampler=L.SAMPLER_STICKY_ZIGZAG, factor=1.5) if c.sticky else {}
    ens = pkg.Ensemble(c.nchains, c.d, trace_capacity=c.trace_capacity, **kw)
    ens.set_flow(pkg.ZigZag(G, np.zeros(c.d)))
    ens.set_target(pkg.GaussianTarget(G))
    if c.sticky:
        ens.set_sticky(np.full(c.d, 0.8))
    ens.set_state(c.t0, c.x0, c.th0, np.ones(c.d), np.arange(c.nchains, dtype=np.uint64) + 1)
    if grid:
        ens.consume_begin(c.dt, c.K)
    return ens


def all_rows(ens, chain, K):
    """The K rows of the grid buffer and npoints, through the C entry point (the wrapper raises where npoints > K)"""
    out = np.empty((K, ens.d))
    npts = C.c_int64()
    st = ens._L.pdmp_ensemble_consume_discretized(ens._h, int(chain), 0, int(K), out.ctypes.data, C.byref(npts), None)
    assert st == 0
    return out, int(npts.value)


def check_grid(pkg, ens, c, k, ev, prev):
    """consume_discretized of chain k against the references on the trace so far; returns the rows for the next segment's look back"""
    tr = pkg.FactTrace(None, c.t0, c.x0[k], c.th0[k], ev)
    grid, X = pkg.trace.discretize(tr, c.dt)
    rows, npts = all_rows(ens, k, c.K)
    assert npts == len(grid)
    n = min(npts, c.K)
    if c.name == "short_grid":
        assert npts > c.K  # the run went past the grid: reported, unclamped, with the reference's count -- and the wrapper says so
        with pytest.raises(ValueError, match="consume_begin was given %d points" % c.K):
            ens.consume_discretized(k)
    else:
        assert npts <= c.K
        gt, got = ens.consume_discretized(k)
        assert same_bits(gt, grid) and same_bits(got, X)
    assert same_bits(rows[:n], X[:n])
    assert not rows[n:].view(np.uint64).any()  # rows at and behind npoints were never written
    if prev is not None:
        assert same_bits(rows[:len(prev)], prev)  # rows flushed earlier come back with the same values
    if c.dyadic and len(ev):
        ts, xs = O.trace_discretize(c.t0, c.x0[k], c.th0[k], ev, c.dt)
        assert len(ts) == npts and same_bits(ts[:n], grid[:n]) and same_bits(rows[:n], xs[:n])
    return rows[:n].copy()


def check_mean(pkg, c, k, ev, m, T):
    """mean(Ξ) of chain k: the kernel's arithmetic bit for bit, and the exact rational mean within the sequential-summation bound"""
    assert T == ev["t"][-1]
    loop, cnt = CC.mean_loop(c.t0, c.x0[k], ev)
    assert same_bits(m, loop)
    exact, absum = CC.mean_exact(c.t0, c.x0[k], ev)
    u = Fraction(1, 2 ** 53)
    for j in range(c.d):
        assert abs(Fraction(float(m[j])) - exact[j]) <= (int(cnt[j]) + 3) * u * absum[j], (j, m[j], float(exact[j]))
    tr = pkg.FactTrace(None, c.t0, c.x0[k], c.th0[k], ev)
    assert np.allclose(m, pkg.trace.mean(tr), **TOL) and np.allclose(m, O.trace_mean(c.t0, c.x0[k], ev), **TOL)


def check_inclusion(pkg, c, k, ev, p, T):
    tr = pkg.FactTrace(None, c.t0, c.x0[k], c.th0[k], ev)
    assert T == ev["t"][-1]
    assert np.allclose(p, pkg.trace.inclusion_prob(tr), **TOL) and np.allclose(p, O.trace_inclusion_prob(c.t0, c.x0[k], ev), **TOL)


@pytest.mark.parametrize("name", CC.NAMES)
def test_consumers_on_a_hand_made_trace(gpu_pkg, name):
    pkg = gpu_pkg
    c = CC.case(name)
    with open_case(pkg, c) as ens:
        ens.consume_cummean(True)
        assert np.all(ens.counters()["ntrace"] == 0)
        prev = [None] * c.nchains
        held = [0] * c.nchains  # events in the buffer in front of this segment (a segment grown without a reset)
        cm_t, cm_y = [[] for _ in range(c.nchains)], [[] for _ in range(c.nchains)]
        for s in range(c.nseg):
            for k in range(c.nchains):
                ens.debug_trace_append(k, c.segment(k, s))
            ens.consume()
            cnt = ens.counters()
            have = [len(c.so_far(k, s)) > 0 for k in range(c.nchains)]
            if all(have):
                m, T = ens.consume_mean()
                p, Tp = ens.consume_inclusion()
            for k in range(c.nchains):
                seg, ev = c.segment(k, s), c.so_far(k, s)
                assert cnt["ntrace"][k] == held[k] + len(seg) and cnt["nevents"][k] == len(ev)
                assert same_events(ens.trace(k, counters=cnt), ev[len(ev) - held[k] - len(seg):])  # the buffer holds what was appended
                prev[k] = check_grid(pkg, ens, c, k, ev, prev[k])
                if all(have):
                    check_mean(pkg, c, k, ev, m[k], T[k])
                    check_inclusion(pkg, c, k, ev, p[k], Tp[k])
                if len(seg):  # the pairs beside the NEW slots (those of a grown segment's first part were read after its own consume)
                    t, y = ens.consume_cummean_pairs(k, len(seg), first=held[k])
                    cm_t[k].append(t)
                    cm_y[k].append(y)
                ot, oy = O.trace_cummean(c.t0, c.x0[k], ev)
                assert same_bits(np.concatenate(cm_t[k] or [np.empty(0)]), ot) and same_bits(np.concatenate(cm_y[k] or [np.empty(0)]), oy)
            if s in c.grow:
                held = [held[k] + len(c.segment(k, s)) for k in range(c.nchains)]
            else:
                ens.trace_reset()
                held = [0] * c.nchains
        if c.sticky:  # a stretch between a 0.0 and a −0.0 counts as stuck: coordinates do spend time at 0
            assert 0.05 < p.min() and p.max() < 0.95


def test_subtrace_at_every_segment_length(gpu_pkg):
    """subtrace_copy on segments of 0, 1, 255, 256, 257 and 600 events with J = [], 0..d−1 and a strict subset: the oracle's events with the
    oracle's new coordinates; n_out is the full count also where out_cap is smaller, and nothing is written behind out_cap."""
    pkg = gpu_pkg
    c = CC.case("sub")
    L = pkg._lib.load()
    with open_case(pkg, c) as ens:
        for s in range(c.nseg):
            seg = c.segment(0, s)
            ens.debug_trace_append(0, seg)
            for J in c.J:
                ok, oi = O.trace_subtrace(J, seg)
                want = seg[ok].copy()
                want["i"] = oi
                assert same_events(ens.subtrace(0, J), want)
                if len(J) == c.d:
                    assert len(want) == len(seg)
                Ja = np.ascontiguousarray(J, dtype=np.int64)
                for cap in sorted({0, len(want) // 2, max(len(want) - 1, 0)}):
                    buf = np.empty(len(seg) + 8, dtype=CC.EVENT_DTYPE)
                    buf.view(np.uint8)[:] = 0xA5  # the sentinel
                    n = C.c_int64(-1)
                    st = L.pdmp_ensemble_subtrace_copy(ens._h, 0, Ja.ctypes.data, len(J), buf.ctypes.data, cap, C.byref(n))
                    assert st == 0 and n.value == len(want)
                    assert same_events(buf[:min(cap, len(want))], want[:cap])
                    assert np.all(buf[min(cap, len(want)):].view(np.uint8) == 0xA5)
            ens.trace_reset()


@pytest.mark.parametrize("name", ["few", "sparse"])
def test_asynchronous_consumer_on_a_hand_made_trace(gpu_pkg, name):
    """consume_async() after every append, no reset and no run between: mean, T and every grid come out bit for bit as with consume() +
    trace_reset(); every call hands the segments back empty (and the next append lands in the OTHER trace buffer)."""
    pkg = gpu_pkg
    c = CC.case(name)
    res = []
    for mode in ("sync", "async"):
        with open_case(pkg, c) as ens:
            for s in range(c.nseg):
                for k in range(c.nchains):
                    ens.debug_trace_append(k, c.segment(k, s))
                if mode == "sync":
                    ens.consume()
                    ens.trace_reset()
                else:
                    ens.consume_async()
                    if name == "few":  # (sparse: the consumer stays deferred until the next append waits for the device)
                        assert np.all(ens.counters()["ntrace"] == 0)
            m, T = ens.consume_mean()
            grids = [all_rows(ens, k, c.K) for k in range(c.nchains)]
            res.append((m, T, grids, ens.counters()["nevents"].copy()))
    (m0, T0, g0, n0), (m1, T1, g1, n1) = res
    assert np.array_equal(n0, [len(e) for e in c.events]) and np.array_equal(n0, n1)
    assert same_bits(T0, T1) and same_bits(m0, m1)
    for k in range(c.nchains):
        assert g0[k][1] == g1[k][1] and same_bits(g0[k][0], g1[k][0])
        grid, X = pkg.trace.discretize(pkg.FactTrace(None, c.t0, c.x0[k], c.th0[k], c.events[k]), c.dt)
        assert g1[k][1] == len(grid) and same_bits(g1[k][0][:len(grid)], X)
        check_mean(pkg, c, k, c.events[k], m1[k], T1[k])


def test_the_hook_refuses_what_it_must(gpu_pkg):
    pkg = gpu_pkg
    L = pkg._lib
    c = CC.case("few")
    ev = c.events[0]

    def refused(call, *a):
        with pytest.raises(L.PdmpError) as ei:
            call(*a)
        assert ei.value.code == L.PDMP_ERR_INVALID

    with open_case(pkg, c, grid=False) as ens:
        refused(ens.debug_trace_append, 0, ev[:1])  # before consume_begin
    with open_case(pkg, c) as ens:
        refused(ens.debug_trace_append, 1, ev[:1])  # a bad chain
        refused(ens.debug_trace_append, -1, ev[:1])
        assert L.load().pdmp_debug_trace_append(ens._h, 0, ev.ctypes.data, -1) == L.PDMP_ERR_INVALID  # n < 0
        refused(ens.debug_trace_append, 0, ev[:c.trace_capacity + 1])  # over capacity: nothing is written
        assert ens.counters()["ntrace"][0] == 0
        ens.debug_trace_append(0, ev[:c.trace_capacity])
        refused(ens.debug_trace_append, 0, ev[:1])  # ... nor behind a full segment
        ens.debug_trace_append(0, ev[:0])           # (an empty append fits)
        cn = ens.counters()
        assert cn["ntrace"][0] == cn["nevents"][0] == c.trace_capacity
        refused(ens.run, 5.0, L.RUN_STOP_BEFORE)    # the records no longer match the trace
        assert same_events(ens.trace(0), ev[:c.trace_capacity])
    d = 4
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, trace_capacity=16) as ens:  # a non-factorised ensemble
        refused(ens.debug_trace_append, 0, ev[:1])
