"""tests/consumer_cases.py on the hosts alone (no device): the table holds what its docstring says, and the two host references of the trace
consumers -- zigzagboomerang.jl_amd/trace.py (closed forms on the grid t0 + k·dt, the device's arithmetic) and oracle/trace_oracle.c (src/trace.jl
restated event by event, t += dt) -- agree on every case with dyadic times: bit for bit for discretize, cummean and subtrace, to rounding for
mean and inclusion_prob.  On the row* cases, whose events sit an ulp beside t0 + k·dt, they DIFFER, which is why tests/test_gpu_consumers_synthetic.py
holds the device to trace.py alone there.  The floors below are what the generators yield (deterministic from their seeds)."""
import numpy as np
import pytest

import consumer_cases as CC
import oracle_lib as O


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def test_event_layout(pkg):
    assert CC.EVENT_DTYPE == pkg._lib.EVENT_DTYPE


@pytest.mark.parametrize("name", CC.NAMES)
def test_case_is_well_formed(name):
    c = CC.case(name)
    assert c.nchains in (1, 2) and c.x0.shape == c.th0.shape == (c.nchains, c.d) and (name in CC.DYADIC) == c.dyadic
    for k in range(c.nchains):
        ev, cuts = c.events[k], c.cuts[k]
        assert ev.dtype == CC.EVENT_DTYPE and cuts[0] == 0 and cuts[-1] == len(ev) and np.all(np.diff(cuts) >= 0) and len(cuts) == c.nseg + 1
        assert np.all(np.diff(ev["t"]) >= 0) and ev["t"][0] > c.t0 and not np.any(ev["t"] == 0.0)  # sorted; 1/(2T), y/(2t) finite
        assert ev["i"].min() >= 0 and ev["i"].max() < c.d and np.all(np.isin(ev["theta"], [-1.0, 0.0, 1.0]))
        nz = ev["x"][ev["x"] != 0.0]
        assert nz.min() >= 0.5 and nz.max() <= 2.0 and (c.sticky or len(nz) == len(ev))
        if c.dyadic:
            assert np.all(ev["t"] * 8 == np.round(ev["t"] * 8)) and np.all(ev["x"] * 2 ** 20 == np.round(ev["x"] * 2 ** 20)) and c.dt == 0.25
        # the buffer holds every stretch between two resets
        held = 0
        for s in range(c.nseg):
            held += cuts[s + 1] - cuts[s]
            assert held <= c.trace_capacity
            if s not in c.grow:
                held = 0
        # the grid is long enough (short_grid: it is not, and says so)
        npts = int((CC.grid_times(c, 4 * c.K + 4000) < ev["t"][-1]).sum())
        assert (npts > c.K) if name == "short_grid" else (1 <= npts <= c.K)
    assert case_is_cached(name)


def case_is_cached(name):
    return CC.case(name) is CC.case(name)  # (one table for every test: nobody regenerates or changes it)


def test_the_table_holds_what_its_docstring_says():
    one, few, short = CC.case("one"), CC.case("few"), CC.case("short_grid")
    # events exactly at a grid time, events sharing a time
    assert CC.grid_hits(one, 0) >= 600 and CC.same_time_events(one, 0) >= 800
    assert CC.grid_hits(few, 0) >= 300 and CC.same_time_events(few, 0) >= 300
    assert [b - a for a, b in zip(one.cuts[0], one.cuts[0][1:])] == [256, 257, 1, 255, 331]
    assert few.t0 == -1.5 and few.events[0]["t"][0] < 0 < few.events[0]["t"][-1] and few.grow == {1}
    # d = 1: a chunk of 256 events is a dependency chain of 256 -- in the chunks the CONSUMER takes (between grid rows), in both cases
    assert CC.longest_chain(one, 0) == 256 and CC.longest_chain(short, 0) == 256
    assert (256, 512) in CC.consumer_chunks(one, 0) and (512, 513) in CC.consumer_chunks(one, 0)
    t = one.events[0]["t"]
    assert t[239] < t[240] == t[511] < t[512] and t[511] in CC.grid_times(one, one.K)  # the chain's last event decides the row behind the chunk
    assert sum(b - a == 256 for a, b in CC.consumer_chunks(short, 0)) >= 2
    assert CC.longest_chain(few, 0) >= 3
    for d in (255, 256, 257):
        c = CC.case("row%d" % d)
        t = c.events[0]["t"]
        g = CC.grid_times(c, c.K)
        on = np.isin(t, g)
        below, above = np.isin(t, np.nextafter(g, -np.inf)), np.isin(t, np.nextafter(g, np.inf))
        assert on.sum() >= 140 and below.sum() >= 140 and above.sum() >= 140 and (on | below | above).all()
        assert CC.same_time_events(c, 0) >= 100
        i = c.events[0]["i"]
        assert (i == d - 1).sum() >= 3 and (i == 0).any() and (d < 257 or (i >= 256).any())
    sp = CC.case("sparse")
    for k in range(2):
        assert CC.empty_rows(sp, k) >= 900 and CC.never_hit(sp, k) >= 100
    segs = [[sp.cuts[k][s + 1] - sp.cuts[k][s] for s in range(sp.nseg)] for k in range(2)]
    assert any(a > 0 and b == 0 for a, b in zip(*segs))  # chain 0 gets events, chain 1 none
    # the forced clash: i ≠ j in one slot, i three times and j twice in a chunk; thread 255 (whose id is the "contested" mark) and thread 0 in a group
    cl = CC.case("clash")
    a, b = cl.pair
    assert a != b and CC.hash_slot(a) == CC.hash_slot(b)
    assert CC.consumer_chunks(cl, 0) == [(0, 256), (256, 512), (512, 768)]
    i = cl.events[0]["i"]
    assert (0, 251) in cl.groups and (1, 0) in cl.groups
    for ch, s in cl.groups:
        assert list(i[ch * 256 + s:ch * 256 + s + 5]) == [a, b, a, b, a]
        chunk = i[ch * 256:(ch + 1) * 256]
        assert (chunk == a).sum() == 3 and (chunk == b).sum() == 2
        assert sum(CC.hash_slot(q) == CC.hash_slot(a) for q in chunk) == 5  # (nobody else in that slot)
    assert CC.longest_chain(cl, 0) == 3
    # a segment's last event ON a grid time, the next segment's first event at the same time
    og = CC.case("on_grid_end")
    t = og.events[0]["t"]
    for cpt in og.cuts[0][1:]:
        assert t[cpt - 1] in CC.grid_times(og, og.K) and (cpt == len(t) or (t[cpt] == t[cpt - 1] and og.events[0]["i"][cpt] != og.events[0]["i"][cpt - 1]))
    # sticky: freezes with both zeros, a stuck stretch between a 0.0 and a −0.0, long stretches of the rare coordinate
    st = CC.case("sticky")
    ev = st.events[0]
    z = ev["x"] == 0.0
    neg = np.signbit(ev["x"]) & z
    assert (z & (ev["theta"] == 0)).sum() >= 60 and neg.sum() >= 40 and (z & ~neg).sum() >= 40 and (z & (ev["theta"] != 0)).sum() >= 60
    mixed = 0
    for j in range(st.d):
        own = ev[ev["i"] == j]
        zz = (own["x"][1:] == 0.0) & (own["x"][:-1] == 0.0)
        mixed += int((zz & (np.signbit(own["x"][1:]) != np.signbit(own["x"][:-1]))).sum())
    assert mixed >= 10
    own3 = ev["t"][ev["i"] == 3]
    assert 3 <= len(own3) <= 40 and np.diff(own3).max() >= 20 * st.dt
    sub = CC.case("sub")
    assert [b - a for a, b in zip(sub.cuts[0], sub.cuts[0][1:])] == [0, 1, 255, 256, 257, 600]
    assert sub.J[0] == [] and sub.J[1] == list(range(sub.d)) and 0 < len(sub.J[2]) < sub.d


def _trace(pkg, c, k, ev=None):
    return pkg.FactTrace(None, c.t0, c.x0[k], c.th0[k], c.events[k] if ev is None else ev)


@pytest.mark.parametrize("name", CC.DYADIC)
def test_the_two_references_agree_on_dyadic_cases(pkg, name):
    c = CC.case(name)
    T = pkg.trace
    for k in range(c.nchains):
        for s in range(c.nseg):  # every prefix the device test checks against
            ev = c.so_far(k, s)
            if len(ev) == 0:
                continue
            tr = _trace(pkg, c, k, ev)
            grid, X = T.discretize(tr, c.dt)
            ts, xs = O.trace_discretize(c.t0, c.x0[k], c.th0[k], ev, c.dt)
            assert same_bits(grid, ts) and same_bits(X, xs)
            assert np.allclose(T.mean(tr), O.trace_mean(c.t0, c.x0[k], ev), rtol=1e-12, atol=1e-15)
            assert np.allclose(T.inclusion_prob(tr), O.trace_inclusion_prob(c.t0, c.x0[k], ev), rtol=1e-12, atol=1e-15)
            m, cnt = CC.mean_loop(c.t0, c.x0[k], ev)
            assert np.allclose(m, T.mean(tr), rtol=1e-12, atol=1e-15) and cnt.sum() == len(ev)
        ev = c.events[k]
        ot, oy = O.trace_cummean(c.t0, c.x0[k], ev)
        cm = T.cummean(_trace(pkg, c, k))
        for j in range(c.d):
            own = ev["i"] == j
            assert same_bits(cm[j][0][1:], ot[own]) and same_bits(cm[j][1][1:], oy[own])
        for J in (c.J or [[], list(range(c.d)), list(range(0, c.d, 2))]):
            ok, oi = O.trace_subtrace(J, ev)
            sub = T.subtrace(_trace(pkg, c, k), np.array(J, dtype=np.int64)).events
            assert len(sub) == len(ok) and np.array_equal(sub["i"], oi)
            for f in ("t", "x", "theta"):
                assert same_bits(sub[f], ev[f][ok])
    if c.sticky:  # a stretch between a 0.0 and a −0.0 counts as stuck: the inclusion probabilities stay well inside (0, 1)
        p = T.inclusion_prob(_trace(pkg, c, 0))
        assert 0.05 < p.min() and p.max() < 0.95


@pytest.mark.parametrize("d", [255, 256, 257])
def test_the_two_references_differ_beside_the_grid(pkg, d):
    """The oracle steps t += dt like the reference; trace.py and the device take t0 + k·dt.  An event an ulp beside such a time falls on different
    sides of the row: the oracle is no reference for the row* cases."""
    c = CC.case("row%d" % d)
    tr = _trace(pkg, c, 0)
    grid, X = pkg.trace.discretize(tr, c.dt)
    ts, xs = O.trace_discretize(c.t0, c.x0[0], c.th0[0], c.events[0], c.dt)
    n = min(len(grid), len(ts))
    assert n > 200 and not same_bits(grid[:n], ts[:n])  # the grids themselves part after a few steps
    assert int((np.abs(X[:n] - xs[:n]) > 0.1).sum()) >= 20  # ... and events land on the other side of a row: O(1), not rounding
    # mean and cummean do not look at the grid: there the oracle stays a reference
    assert np.allclose(pkg.trace.mean(tr), O.trace_mean(c.t0, c.x0[0], c.events[0]), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("name", ["row256", "clash", "sparse"])
def test_mean_references_bracket_each_other(name):
    """mean_loop (the device's arithmetic) lies within the sequential-summation bound of the exact rational mean"""
    c = CC.case(name)
    for k in range(c.nchains):
        m, cnt = CC.mean_loop(c.t0, c.x0[k], c.events[k])
        ex, ab = CC.mean_exact(c.t0, c.x0[k], c.events[k])
        for j in range(c.d):
            assert abs(CC.Fraction(float(m[j])) - ex[j]) <= (int(cnt[j]) + 3) * CC.Fraction(1, 2 ** 53) * ab[j]
