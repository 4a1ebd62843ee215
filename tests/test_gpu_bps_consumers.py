"""The device consumers of the Bouncy Particle family's traces (csrc/pdmp_consume_bps.hip, pdmp_ensemble_bps_consume_*; -m gpu) against the
sequential C reference tests/ref/pdmp_trace_ref.c, BIT FOR BIT (NaNs -- cummean's and mean's 0/0 -- by position):

  1. the hand-made traces of tests/pdmp_consumer_cases.py through pdmp_debug_bps_trace_append: begin, then per segment append -> bps_consume() ->
     checks against the trace SO FAR -> trace_reset() (or none: a segment grown in place);
  2. what the hook and the entry points refuse, with their codes; the factorised calls still refuse a BPS ensemble;
  3. pdmp / sspdmp with consume=dict(dt, points) on BouncyParticle, Boomerang, the sticky BouncyParticle and the speed-recorded form, in at least
     three slices: the extra element equals the reference applied to the returned host trace, the other elements those of a run without the
     keyword, and trace=False returns the same extra element;
  4. one shape at d = 1024."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import pdmp_consumer_cases as PC
import pdmp_trace_ref_lib as R

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """bit for bit, NaNs by position"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(bits(a[ok]), bits(b[ok]))


def open_case(pkg, c, begin=True):
    """A BPS ensemble in the state of case c, bps_consume_begin done: nothing has run (a sticky one holds the event its set_state_bps wrote)"""
    L = pkg._lib
    G = sp.identity(c.d, format="csc")
    ens = pkg.Ensemble(c.nchains, c.d, sampler=L.SAMPLER_BPS, factor=2.0, trace_capacity=c.trace_capacity)
    if c.mu is not None:
        ens.set_flow_boomerang(pkg.GaussianTarget(G, c.mu), pkg.Boomerang(G, c.mu, 1.0))
    else:
        ens.set_flow_bps(pkg.BouncyParticle(G, np.zeros(c.d), 1.0))
    if c.sticky:
        ens.set_bps_sticky(np.full(c.d, 0.8))
    ens.set_state_bps(c.t0, c.x0, c.th0, 10.0, np.arange(c.nchains, dtype=np.uint64) + 1)
    if begin:
        ens.bps_consume_begin(c.dt, c.K)
    return ens


def all_rows(ens, chain, K):
    """The K rows of the grid buffer and npoints, through the C entry point (the wrapper raises where npoints > K)"""
    out = np.empty((K, ens.d))
    npts = C.c_int64()
    st = ens._L.pdmp_ensemble_bps_consume_discretized(ens._h, int(chain), 0, int(K), out.ctypes.data, C.byref(npts), None)
    assert st == 0
    return out, int(npts.value)


@pytest.mark.parametrize("name", PC.NAMES)
def test_consumers_on_a_hand_made_trace(gpu_pkg, name):
    pkg = gpu_pkg
    c = PC.case(name)
    with open_case(pkg, c) as ens:
        ens.bps_consume_cummean(True)
        assert np.all(ens.counters()["ntrace"] == (1 if c.sticky else 0))
        prev = [None] * c.nchains
        held = [0] * c.nchains  # events in the buffer in front of this segment (a segment grown without a reset)
        for s in range(c.nseg):
            for k in range(c.nchains):
                t, x, th, f = c.segment(k, s)
                if c.sticky and s == 0:  # the event set_state_bps wrote: (t0, x0, θ0, all free)
                    dt_, dx, dth = ens.bps_trace(k)
                    assert same_bits(dt_, t) and same_bits(dx, x) and same_bits(dth, th) and np.array_equal(ens.bps_trace_free(k), f)
                else:
                    ens.debug_bps_trace_append(k, t, x, th, f)
            ens.bps_consume()
            cnt = ens.counters()
            m, T = ens.bps_consume_mean()
            if c.sticky:
                p, Tp = ens.bps_consume_inclusion()
                assert same_bits(Tp, T)
            for k in range(c.nchains):
                a, b = c.cuts[k][s], c.cuts[k][s + 1]
                r = PC.reference(name, k, s)
                assert cnt["ntrace"][k] == held[k] + (b - a) and cnt["nevents"][k] == b
                dt_, dx, dth = ens.bps_trace(k, counters=cnt)  # the buffer holds what was appended
                lo = b - held[k] - (b - a)
                assert same_bits(dt_, c.t[k][lo:b]) and same_bits(dx, c.x[k][lo:b]) and same_bits(dth, c.th[k][lo:b])
                assert same_bits(T[k], r["T"]) and same_bits(m[k], r["mean"])
                if c.sticky:
                    assert same_bits(p[k], r["inclusion"])
                rows, npts = all_rows(ens, k, c.K)
                assert npts == r["npoints"]
                n = min(npts, c.K)
                assert same_bits(rows[:n], r["grid"][:n])
                assert not rows[n:].view(np.uint64).any()  # rows at and behind npoints still hold the zeros begin put there
                if prev[k] is not None:
                    assert same_bits(rows[:len(prev[k])], prev[k])  # rows read after an earlier segment come back unchanged
                prev[k] = rows[:n].copy()
                if npts > c.K:
                    assert name == "short_grid"
                    with pytest.raises(ValueError, match="bps_consume_begin was given %d points" % c.K):
                        ens.bps_consume_discretized(k)
                else:
                    gt, got = ens.bps_consume_discretized(k)
                    assert same_bits(gt, r["grid_t"]) and same_bits(got, r["grid"][:npts])
                if b > a:  # the rows beside the NEW slots
                    assert same_bits(ens.bps_consume_cummean_rows(k, b - a, first=held[k]), r["cummean"][a:b])
            if s in c.grow:
                held = [held[k] + c.cuts[k][s + 1] - c.cuts[k][s] for k in range(c.nchains)]
            else:
                ens.trace_reset()
                held = [0] * c.nchains
        if name == "short_grid":
            assert npts > c.K


def test_the_hook_and_the_entry_points_refuse_what_they_must(gpu_pkg):
    pkg = gpu_pkg
    L = pkg._lib
    lib = L.load()
    INV = L.PDMP_ERR_INVALID
    c = PC.case("neg")
    t, x, th = c.t[0], c.x[0], c.th[0]
    d = c.d

    def refused(call, *a, **kw):
        with pytest.raises(L.PdmpError) as ei:
            call(*a, **kw)
        assert ei.value.code == INV, ei.value

    with open_case(pkg, c, begin=False) as ens:  # everything but begin comes after begin
        refused(ens.debug_bps_trace_append, 0, t[:1], x[:1], th[:1])
        for call in (ens.bps_consume, ens.bps_consume_mean, ens.bps_consume_inclusion, ens.bps_consume_cummean):
            refused(call)
        refused(ens.bps_consume_cummean_rows, 0, 1)
        assert lib.pdmp_ensemble_bps_consume_discretized(ens._h, 0, 0, 0, None, None, None) == INV
        refused(ens.bps_consume_begin, 0.0, 4)   # grid_points > 0 with grid_dt not positive
        refused(ens.bps_consume_begin, -1.0, 4)
        refused(ens.bps_consume_begin, 0.25, -1)
        ens.run(c.t0 + 0.5)
        refused(ens.bps_consume_begin, 0.25, 4)  # after the first run
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, trace_capacity=0) as ens:  # begin needs a trace buffer
        ens.set_flow_bps(pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0))
        refused(ens.bps_consume_begin, 0.25, 4)  # before set_state_bps
        ens.set_state_bps(c.t0, c.x0, c.th0, 10.0, np.ones(1, dtype=np.uint64))
        refused(ens.bps_consume_begin, 0.25, 4)
    with open_case(pkg, c) as ens:
        refused(ens.bps_consume_inclusion)       # not a sticky ensemble
        refused(ens.debug_bps_trace_append, 1, t[:1], x[:1], th[:1])   # a bad chain
        refused(ens.debug_bps_trace_append, -1, t[:1], x[:1], th[:1])
        assert lib.pdmp_debug_bps_trace_append(ens._h, 0, t.ctypes.data, x.ctypes.data, th.ctypes.data, None, -1) == INV  # n < 0
        refused(ens.debug_bps_trace_append, 0, t[:1], x[:1], th[:1], np.ones((1, d), dtype=bool))  # f on an ensemble that is not sticky
        cap = c.trace_capacity
        refused(ens.debug_bps_trace_append, 0, t[:cap + 1], x[:cap + 1], th[:cap + 1])  # over capacity: nothing is written
        assert ens.counters()["ntrace"][0] == 0
        refused(ens.bps_consume_cummean_rows, 0, 1)  # before bps_consume_cummean(True)
        ens.bps_consume_cummean(True)
        refused(ens.bps_consume_cummean_rows, 0, cap + 1)
        refused(ens.bps_consume_mean, 0, 2)      # a chain range past the ensemble
        assert lib.pdmp_ensemble_bps_consume_discretized(ens._h, 0, 0, c.K + 1, None, None, None) == INV
        assert lib.pdmp_ensemble_bps_consume_discretized(ens._h, 1, 0, 1, None, None, None) == INV
        ens.debug_bps_trace_append(0, t[:cap], x[:cap], th[:cap])
        refused(ens.debug_bps_trace_append, 0, t[:1], x[:1], th[:1])  # ... nor behind a full segment
        ens.debug_bps_trace_append(0, t[:0], x[:0], th[:0])           # (an empty append fits)
        cn = ens.counters()
        assert cn["ntrace"][0] == cn["nevents"][0] == cap
        refused(ens.run, 5.0, L.RUN_STOP_BEFORE)  # the state no longer matches the trace ...
        ens.set_state_bps(c.t0, c.x0, c.th0, 10.0, np.ones(1, dtype=np.uint64))
        refused(ens.bps_consume)                  # ... until the next set_state_bps, which also ends the consumers
        ens.run(c.t0 + 0.5)
    with open_case(pkg, PC.case("sticky130")) as ens:  # a sticky ensemble's events carry masks
        cs = PC.case("sticky130")
        refused(ens.debug_bps_trace_append, 0, cs.t[0][1:2], cs.x[0][1:2], cs.th[0][1:2])
    with pkg.Ensemble(1, d) as ens:  # a factorised ensemble
        G = sp.identity(d, format="csc")
        ens.set_flow(pkg.ZigZag(G, np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_state(0.0, c.x0, c.th0, np.ones(d), np.ones(1, dtype=np.uint64))
        refused(ens.bps_consume_begin, 0.25, 4)
        for call in (ens.bps_consume, ens.bps_consume_mean, ens.bps_consume_inclusion, ens.bps_consume_cummean):
            refused(call)
        refused(ens.bps_consume_cummean_rows, 0, 1)
        refused(ens.debug_bps_trace_append, 0, t[:1], x[:1], th[:1])
        assert lib.pdmp_ensemble_bps_consume_discretized(ens._h, 0, 0, 0, None, None, None) == INV


def test_the_factorised_calls_still_refuse_a_bps_ensemble(gpu_pkg):
    pkg = gpu_pkg
    L = pkg._lib
    c = PC.case("neg")
    ev = np.zeros(1, dtype=L.EVENT_DTYPE)
    with open_case(pkg, c) as ens:
        for call, a in ((ens.consume_begin, (0.25, 4)), (ens.debug_trace_append, (0, ev))):
            with pytest.raises(L.PdmpError) as ei:
                call(*a)
            assert ei.value.code == L.PDMP_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- end to end
def tridiag(d):
    return sp.diags([np.full(d - 1, -0.3), np.full(d, 1.2), np.full(d - 1, -0.3)], [-1, 0, 1], format="csc")


def run_args(pkg, kind, d, rng):
    """(call, args, keywords, dt, points) of one sampler of the family"""
    I = sp.identity(d, format="csc")
    if kind == "bps":
        return pkg.pdmp, [None, 0.0, None, None, 120.0, 1e-3, pkg.BouncyParticle(I, np.zeros(d), 1.0)], dict(), 0.25, 600
    if kind == "boomerang":
        mf = rng.standard_normal(d)
        return pkg.pdmp, [pkg.GaussianTarget(1.2 * I, mf), 0.0, None, None, 200.0, 3.0, pkg.Boomerang(I, mf, 0.5)], dict(adapt=True), 0.5, 600
    if kind == "sticky":
        return pkg.sspdmp, [None, 0.0, None, None, 40.0, 0.5, pkg.BouncyParticle(I, np.zeros(d), 1.0), 1.5], dict(), 0.25, 400
    return (pkg.pdmp, [pkg.GaussianTarget(tridiag(d)), 0.0, None, None, 200, pkg.LocalBound(5.0), pkg.BouncyParticle(None, None, 1.0, 0.9)], dict(),
            0.5, 1200)


def check_extra(pkg, extra, traces, dt, sticky, mu):
    """The extra element of a consume=... run against the C reference applied to the returned host traces"""
    nch = len(traces)
    assert np.shape(extra["mean"]) == (nch, len(traces[0].x0)) and np.shape(extra["T"]) == (nch,)
    for k, tr in enumerate(traces):
        r = R.consume(tr.t0, tr.x0, tr.θ0, tr.t, tr.x, tr.θ, f=tr.f, mu=mu, dt=dt, K=len(extra["grid_t"][k]))
        assert same_bits(extra["T"][k], r["T"]) and same_bits(extra["mean"][k], r["mean"])
        assert r["npoints"] == len(extra["grid_t"][k]) and same_bits(extra["grid_t"][k], r["grid_t"]) and same_bits(extra["grid_x"][k], r["grid"])
        if sticky:
            assert same_bits(extra["inclusion"][k], r["inclusion"])
        else:
            assert "inclusion" not in extra


def same_results(u, v):
    """the four elements of two runs, bit for bit"""
    for q0, q1 in zip(u[0], v[0]):
        assert same_bits(q0.t, q1.t) and same_bits(q0.x, q1.x) and same_bits(q0.θ, q1.θ)
        assert (q0.f is None) == (q1.f is None) and (q0.f is None or np.array_equal(q0.f, q1.f))
    for a, b in zip(u[1:4], v[1:4]):
        for p, q in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert np.array_equal(p, q)


@pytest.mark.parametrize("kind", ["bps", "boomerang", "sticky", "modern"])
def test_sampler_keyword(gpu_pkg, kind):
    pkg = gpu_pkg
    rng = np.random.default_rng(31)
    d, nch, cap = 8, 4, 40
    call, a, kw, dt, points = run_args(pkg, kind, d, rng)
    a[2], a[3] = rng.standard_normal((nch, d)), rng.standard_normal((nch, d))
    mu = a[6].μ if kind == "boomerang" else None
    r0 = call(*a, seed=4, trace_capacity=cap, **kw)
    r1 = call(*a, seed=4, trace_capacity=cap, consume=dict(dt=dt, points=points), **kw)
    assert len(r0) == 4 and len(r1) == 5
    nev = [len(tr.t) for tr in r1[0]]
    assert min(nev) >= 3 * cap and max(nev) < 1000, nev  # at least three slices, a few hundred events
    same_results(r0, r1)
    check_extra(pkg, r1[4], r1[0], dt, kind == "sticky", mu)
    r2 = call(*a, seed=4, trace_capacity=cap, trace=False, consume=dict(dt=dt, points=points), **kw)  # nothing is copied to the host
    assert all(len(tr.t) == 0 for tr in r2[0])
    for key in r1[4]:
        for p, q in zip(r1[4][key], r2[4][key]):
            assert same_bits(p, q), key
    # one chain: squeezed
    a[2], a[3] = a[2][0], a[3][0]
    r3 = call(*a, seed=4, trace_capacity=cap, consume=dict(dt=dt, points=points), **kw)
    assert same_bits(r3[4]["mean"], r1[4]["mean"][0]) and same_bits(r3[4]["grid_x"], r1[4]["grid_x"][0]) and r3[4]["T"] == r1[4]["T"][0]
    with pytest.raises(ValueError, match="trace_capacity must be positive"):
        call(*a, seed=4, trace_capacity=0, consume=dict(dt=dt, points=points), **kw)
    with pytest.raises(ValueError, match="was given 3 points"):
        call(*a, seed=4, trace_capacity=cap, consume=dict(dt=dt, points=3), **kw)


def test_one_shape_at_d_1024(gpu_pkg):
    """C2's d = 1024 (16 strips per chain), 8 chains of about 50 events, two slices: against the C reference on the returned traces"""
    pkg = gpu_pkg
    rng = np.random.default_rng(32)
    d, nch = 1024, 8
    I = sp.identity(d, format="csc")
    x0, th0 = rng.standard_normal((nch, d)), rng.standard_normal((nch, d))
    r = pkg.pdmp(None, 0.0, x0, th0, 3.5, 1e-3, pkg.BouncyParticle(I, np.zeros(d), 1.0), seed=7, trace_capacity=32, consume=dict(dt=0.01, points=500))
    nev = [len(tr.t) for tr in r[0]]
    assert 25 <= min(nev) and max(nev) <= 120, nev
    check_extra(pkg, r[4], r[0], 0.01, False, None)
