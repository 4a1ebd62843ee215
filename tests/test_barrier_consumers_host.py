"""trace.barrier_start and trace.barrier_occupation -- the host mirrors of the barrier ensembles' device consumers (DESIGN.md "Barrier
occupation") -- on the hand-made table of tests/barrier_consumer_cases.py (values written out by hand, exact dyadic numbers) and on traces of
the sequential restatement of stickyzz (tests/stickyzz_ref_lib.py): there the time frozen must equal the time with θ = 0 of the path, computed
independently, and the hits the number of θ = 0 events.  No device."""
import numpy as np
import pytest

import barrier_consumer_cases as B
import stickyzz_cases as K
import stickyzz_ref_lib as R


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def test_barrier_start_on_the_case_table(pkg):
    th_eff, side0 = pkg.trace.barrier_start(B.X0, B.TH0, B.BARRIERS)
    assert same_bits(th_eff, B.TH_EFF) and np.array_equal(side0, B.SIDE0)
    for k in range(B.NCHAINS):  # one chain at a time, and StickyBarriers objects instead of plain triples
        th1, s1 = pkg.trace.barrier_start(B.X0[k], B.TH0[k], K.barriers_for(pkg, B.BARRIERS, B.D))
        assert same_bits(th1, B.TH_EFF[k]) and np.array_equal(s1, B.SIDE0[k])
    # one barrier for all coordinates; −0.0 lies ON a barrier at 0.0; a start on the barrier BEHIND the direction of travel is not frozen
    th, side = pkg.trace.barrier_start([0.0, -0.0, 0.0, 1.0], [1.0, -2.0, -1.0, -1.0], ((0.0, 1.0), ("sticky", "sticky"), (1.0, 1.0)))
    assert same_bits(th, [1.0, 0.0, 0.0, -1.0]) and np.array_equal(side, [1, 0, 0, 0])


@pytest.mark.parametrize("k", range(B.NCHAINS))
def test_occupation_on_the_case_table(pkg, k):
    zl, zh, nl, nh, T = pkg.trace.barrier_occupation(B.EVENTS[k], B.T0, B.X0[k], B.TH0[k], B.BARRIERS)
    assert same_bits(zl, B.FROZEN_LO[k]) and same_bits(zh, B.FROZEN_HI[k])
    assert nl.dtype == nh.dtype == np.uint64 and np.array_equal(nl, B.HITS_LO[k]) and np.array_equal(nh, B.HITS_HI[k])
    assert T == B.T_LAST[k]
    tr = pkg.FactTrace(None, B.T0, B.X0[k], B.TH0[k], B.EVENTS[k])  # (a FactTrace is taken like its events)
    again = pkg.trace.barrier_occupation(tr, B.T0, B.X0[k], B.TH0[k], B.BARRIERS)
    assert all(np.array_equal(a, b) for a, b in zip(again[:4], (zl, zh, nl, nh)))
    # no event at all: a frozen start has been frozen for no time yet
    zl0, zh0, nl0, nh0, T0 = pkg.trace.barrier_occupation(B.EVENTS[k][:0], B.T0, B.X0[k], B.TH0[k], B.BARRIERS)
    assert not zl0.any() and not zh0.any() and not nl0.any() and not nh0.any() and T0 == B.T0


@pytest.mark.parametrize("k", range(B.NCHAINS))
def test_occupation_of_a_part_of_the_trace(pkg, k):
    """After the first segment only: the cut lies between a wall's hit and its thaw, so the coordinate is frozen at the last event -- for no time."""
    ev = B.so_far(k, 0)
    zl, zh, nl, nh, T = pkg.trace.barrier_occupation(ev, B.T0, B.X0[k], B.TH0[k], B.BARRIERS)
    assert T == ev["t"][-1]
    if k == 0:  # up to (2.0, 0, 2.0, 0.0): coordinate 1 thawed at 1.5 from its frozen start, 2 thawed after 0.5, 3 frozen since 1.25
        assert same_bits(zl, [0.0, 0.0, 0.5, 0.75]) and same_bits(zh, [0.0, 1.5, 0.0, 0.0])
        assert np.array_equal(nl, [0, 0, 1, 1]) and np.array_equal(nh, [1, 0, 0, 0])
    else:       # up to (3.75, 0, 2.0, 0.0)
        assert same_bits(zl, [0.75, 0.0, 0.0, 0.0]) and same_bits(zh, [0.0, 1.0, 1.5, 0.0])
        assert np.array_equal(nl, [0, 0, 0, 0]) and np.array_equal(nh, [1, 1, 1, 0])


@pytest.mark.parametrize("k", range(B.NCHAINS))
def test_the_other_mirrors_follow_the_path_from_theta_eff(pkg, k):
    """mean and discretize of the trace started at (t0, x0, θ_eff) give the hand values; started at θ0 -- what a returned trace records -- the
    grid of a coordinate that starts frozen differs."""
    tr = pkg.FactTrace(None, B.T0, B.X0[k], B.TH_EFF[k], B.EVENTS[k])
    assert same_bits(pkg.trace.mean(tr), B.MEAN[k])
    g, X = pkg.trace.discretize(tr, B.DT)
    assert same_bits(g, B.GRID_T) and same_bits(X, B.GRID_X[k])
    if k == 0:  # (chain 0's frozen coordinate thaws at 1.5, behind the grid time 1; chain 1's at 0.75, before it)
        quirk = pkg.FactTrace(None, B.T0, B.X0[k], B.TH0[k], B.EVENTS[k])
        assert pkg.trace.discretize(quirk, B.DT)[1][1, 1] == 2.5 != B.GRID_X[k][1, 1]


def frozen_time_independent(r, t0, th_eff):
    """Per coordinate: the time with θ = 0 over [t0, T_last] of the path through the events (numpy's pairwise sum, not the sequential one), and
    the number of θ = 0 events"""
    d = len(th_eff)
    T = r["t"][-1]
    z, n = np.zeros(d), np.zeros(d, dtype=np.int64)
    for i in range(d):
        own = r["i"] == i
        t = np.concatenate([[t0], r["t"][own], [T]])
        th = np.concatenate([[th_eff[i]], r["theta"][own]])
        z[i] = np.sum(np.diff(t) * (th == 0))
        n[i] = int(np.sum(r["theta"][own] == 0))
    return z, n


def check_run(pkg, r, x0, th0, barriers):
    assert r["status"] == R.REF_OK
    ev = np.zeros(len(r["t"]), dtype=B.EVENT_DTYPE)
    ev["t"], ev["i"], ev["x"], ev["theta"] = r["t"], r["i"], r["x"], r["theta"]
    zl, zh, nl, nh, T = pkg.trace.barrier_occupation(ev, 0.0, x0, th0, barriers)
    th_eff, _ = pkg.trace.barrier_start(x0, th0, barriers)
    z, n = frozen_time_independent(r, 0.0, th_eff)
    assert T == r["t"][-1]
    nev = np.bincount(r["i"], minlength=len(x0)) + 1
    assert np.all(np.abs((zl + zh) - z) <= nev * 2.0 ** -52 * np.abs(z)), (zl + zh, z)
    assert np.array_equal((nl + nh).astype(np.int64), n)
    assert r["nhit"] == int(n.sum()) > 0  # (the restatement's own count of hits)
    # a hit lands on the barrier it is counted for
    lo, hi, *_ = R.barrier_table(barriers, len(x0))
    for i in range(len(x0)):
        own = np.nonzero(r["i"] == i)[0]
        hits = own[r["theta"][own] == 0]
        assert int(nl[i]) == int(np.sum(r["x"][hits] == lo[i]) if lo[i] != hi[i] else nl[i])
        assert int(nh[i]) == int(np.sum(r["x"][hits] == hi[i]) if lo[i] != hi[i] else nh[i])
    return zl, zh, nl, nh


@pytest.mark.parametrize("name", ["BOX_1D", "STICKY_1D"])
def test_occupation_of_a_1d_run(pkg, name):
    bar = getattr(K, name)
    r = K.run_1d(bar, 8.0, 3)
    zl, zh, nl, nh = check_run(pkg, r, np.array([1.0]), np.array([0.8]), bar)
    if name == "BOX_1D":
        assert zl[0] == 0 and zh[0] == 0 and nl[0] + nh[0] > 0  # walls: hits, no time
    else:
        assert zl[0] + zh[0] > 0
        moving = K.batch_means_1d(r, 1.0, 0.8, r["t"][-1], "moving", B=1)[0]  # the fraction of [0, T_last] away from the level
        assert abs((1.0 - (zl[0] + zh[0]) / r["t"][-1]) - moving) <= len(r["t"]) * 2.0 ** -52


def test_occupation_of_a_d8_run_with_mixed_rules_and_a_frozen_start(pkg):
    G = K.precision8()
    bar = K.mixed_barriers(8)
    x0, th0 = K.state8(1)
    x0 = K.fit_state(x0, bar)[0]
    th0 = th0[0]
    x0[4] = 0.5 if th0[4] > 0 else -1.0  # coordinate 4 starts frozen on the barrier of its direction ((−1, 0.5), sticky)
    r = R.stickyzz(0.0, x0, th0, 6.0, K.c8(G), bar, gamma=0.9 * G, target_gamma=G, seed=11)
    first = np.nonzero(r["i"] == 4)[0][0]
    assert r["kind"][first] == R.EV_THAW
    zl, zh, nl, nh = check_run(pkg, r, x0, th0, bar)
    assert (zh[4] if th0[4] > 0 else zl[4]) >= r["t"][first]  # the frozen start counts from t0, on the side of θ0
    assert zl[0] == zh[0] == 0 and nl[0] == nh[0] == 0  # coordinate 0 has no barrier
