"""The device trace consumers of the flows with a refresh clock -- a ZigZag with λref > 0, a FactBoomerang: Ensemble.refresh_consume_begin, the
unordered walk of csrc/pdmp_consume.hip (-m gpu).  Such a trace is sorted within a coordinate only (a refreshed coordinate is recorded at its own,
stale clock); the contract is tests/ref/refresh_trace_ref.c, the reference's consumers taken in trace order, and the device agrees with it bit
for bit: rows, npoints, mean, T and the cummean pairs (NaNs by position).  tests/test_refresh_consumer_cases_ref.py holds that contract to
trace.py, to the oracle's restatement of the reference's iterator and, for the FactBoomerang, to the iterator restated step by step.

  table        every hand-made trace of tests/refresh_consumer_cases.py through pdmp_debug_trace_append, consumed twice in ONE ensemble: chain 1
               in the slices the table gives (append, consume, reset), chain 0 whole in the last consume -- equal bytes, equal to the contract
  end to end   two chains each, a trace buffer small enough for several refills: the ZigZag with λref = 4 on the 16 x 16 lattice (local
               kernel), the same with adaptscale (general kernel) and a FactBoomerang on problems.maintest_precision(8) (general kernel)
  keyword      spdmp(..., consume=dict(dt=..., points=...)) equals the Ensemble calls; trace=False returns no events and the same dict
  refusals     every status code of include/pdmp_mi355.h's paragraph, and that a refusal leaves mean and rows as they were"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import refresh_consumer_cases as RC
import refresh_trace_ref_lib as R

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-12, atol=1e-15)  # the project's tolerance for mean / cummean against trace.py


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """bit for bit, NaNs by position (a 0/0 has one sign on the host and another on the device)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(bits(a[ok]), bits(b[ok]))


def flow_of(pkg, c):
    G = sp.identity(c.d, format="csc")
    return G, (pkg.FactBoomerang(G, c.mu, 0.5) if c.mu is not None else pkg.ZigZag(G, np.zeros(c.d), λref=1.0))


def open_case(pkg, c, nchains, begin=True):
    """An ensemble of `nchains` chains in the state of case c, refresh_consume_begin done: nothing has run, the traces are empty"""
    assert RC.EVENT_DTYPE == pkg._lib.EVENT_DTYPE
    G, F = flow_of(pkg, c)
    ens = pkg.Ensemble(nchains, c.d, trace_capacity=c.trace_capacity)
    ens.set_flow(F)
    ens.set_target(pkg.GaussianTarget(G))
    ens.set_state(c.t0, np.tile(c.x0, (nchains, 1)), np.tile(c.th0, (nchains, 1)), np.ones(c.d), np.arange(nchains, dtype=np.uint64) + 1)
    if begin:
        ens.refresh_consume_begin(c.dt, c.K)
    return ens


def all_rows(ens, chain, K):
    """The K rows of the grid buffer and npoints, through the C entry point (the wrapper raises where npoints > K)"""
    out = np.empty((K, ens.d))
    npts = C.c_int64()
    assert ens._L.pdmp_ensemble_consume_discretized(ens._h, int(chain), 0, int(K), out.ctypes.data, C.byref(npts), None) == 0
    return out, int(npts.value)


def check_chain(c, r, rows, npts, mean, T, cm_t, cm_y):
    n = min(r["npoints"], c.K)
    assert npts == r["npoints"] and T == r["T"]
    assert same(rows[:n], r["grid"][:n])
    assert not rows[n:].view(np.uint64).any()  # rows at and behind npoints were never written
    assert same(mean, r["mean"])
    assert same(cm_t, r["cummean_t"]) and same(cm_y, r["cummean_y"])


@pytest.mark.parametrize("name", RC.NAMES)
def test_table_bit_for_bit_whole_and_split(gpu_pkg, name):
    pkg = gpu_pkg
    c = RC.case(name)
    r = RC.reference(name)
    with open_case(pkg, c, 2) as ens:
        ens.consume_cummean(True)
        cm = [[], []]
        for s in range(c.nseg):
            seg = c.segment(s)
            ens.debug_trace_append(1, seg)
            if s == c.nseg - 1:
                ens.debug_trace_append(0, c.events)
            ens.consume()
            if len(seg):
                cm[1].append(ens.consume_cummean_pairs(1, len(seg)))
            if s == c.nseg - 1:
                cm[0].append(ens.consume_cummean_pairs(0, len(c.events)))
            else:  # the split chain so far against the contract on the events so far; chain 0 has consumed nothing
                rs = RC.reference(name, c.cuts[s + 1])
                rows, npts = all_rows(ens, 1, c.K)
                n = min(rs["npoints"], c.K)
                assert npts == rs["npoints"] and same(rows[:n], rs["grid"][:n]) and not rows[n:].view(np.uint64).any()
                rows0, npts0 = all_rows(ens, 0, c.K)
                assert npts0 == 1 and same(rows0[0], c.x0) and not rows0[1:].view(np.uint64).any()
            ens.trace_reset()
        mean, T = ens.consume_mean()
        got = []
        for k in range(2):
            rows, npts = all_rows(ens, k, c.K)
            cm_t = np.concatenate([p[0] for p in cm[k]])
            cm_y = np.concatenate([p[1] for p in cm[k]])
            check_chain(c, r, rows, npts, mean[k], T[k], cm_t, cm_y)
            got.append((rows, npts, cm_t, cm_y))
        assert got[0][1] == got[1][1] and all(got[0][q].tobytes() == got[1][q].tobytes() for q in (0, 2, 3))  # rows, cummean t and y
        assert mean[0].tobytes() == mean[1].tobytes() and T[0] == T[1]
        if name == "short_grid":  # the run went past the grid: reported, unclamped -- and the wrapper says so
            assert r["npoints"] > c.K
            with pytest.raises(ValueError, match="consume_begin was given %d points" % c.K):
                ens.consume_discretized(0)
        else:
            gt, gx = ens.consume_discretized(1)
            assert same(gt, r["grid_t"]) and same(gx, r["grid"][:r["npoints"]])
            tr = pkg.FactTrace(flow_of(pkg, c)[1] if c.mu is not None else None, c.t0, c.x0, c.th0, c.events)
            grid, X = pkg.trace.discretize(tr, c.dt)
            assert same(gt, grid) and (same(gx, X) if c.mu is None else np.allclose(gx, X, rtol=0, atol=1e-12))
            assert np.allclose(mean[1], pkg.trace.mean(tr), **TOL)


def test_twelve_events_cut_at_every_position(gpu_pkg):
    """cut13 in 13 chains of one ensemble: chain q gets events[:q], a consume, a reset, events[q:], a consume -- the same bytes in all 13"""
    pkg = gpu_pkg
    c = RC.case("cut13")
    r = RC.reference("cut13")
    n = len(c.events)
    assert n == 12
    with open_case(pkg, c, n + 1) as ens:
        ens.consume_cummean(True)
        cm = []
        for q in range(n + 1):
            ens.debug_trace_append(q, c.events[:q])
        ens.consume()
        first = [ens.consume_cummean_pairs(q, q) for q in range(n + 1)]
        ens.trace_reset()
        for q in range(n + 1):
            ens.debug_trace_append(q, c.events[q:])
        ens.consume()
        mean, T = ens.consume_mean()
        for q in range(n + 1):
            second = ens.consume_cummean_pairs(q, n - q)
            rows, npts = all_rows(ens, q, c.K)
            check_chain(c, r, rows, npts, mean[q], T[q], np.concatenate([first[q][0], second[0]]), np.concatenate([first[q][1], second[1]]))
            cm.append(rows.tobytes() + mean[q].tobytes())
        assert len(set(cm)) == 1


# ------------------------------------------------------------------------------------------------------------------ end to end
def e2e_problem(pkg, name):
    rng = np.random.default_rng(77)
    if name == "boom":
        G = pkg.problems.maintest_precision(8)
        d = G.shape[0]
        mu = np.linspace(-0.5, 0.5, d)
        return dict(G=G, F=pkg.FactBoomerang(G, mu, 5.0), target=pkg.GaussianTarget(G, mu), x0=mu + rng.standard_normal((2, d)),
                    th0=rng.standard_normal((2, d)), c=np.full(d, 10.0), T=200.0, cap=256, dt=0.5, adaptscale=False, kernel="zz_general")
    G = pkg.problems.gmrf_precision(16)
    d = G.shape[0]
    return dict(G=G, F=pkg.ZigZag(G, np.zeros(d), λref=4.0), target=pkg.GaussianTarget(G), x0=rng.standard_normal((2, d)),
                th0=rng.choice([-1.0, 1.0], (2, d)), c=pkg.problems.column_norms(G), T=15.0, cap=1024, dt=0.25, adaptscale=name == "zz_adaptscale",
                kernel="zz_general" if name == "zz_adaptscale" else "zz_local")


def run_ensemble(pkg, p, K, seed=11):
    """The Ensemble calls: refresh_consume_begin, then run / consume / drain until every chain is through.  Returns (events per chain, mean, T,
    grids, slices, kernel)."""
    L = pkg._lib
    d = p["x0"].shape[1]
    with pkg.Ensemble(2, d, trace_capacity=p["cap"]) as ens:
        ens.set_flow(p["F"])
        ens.set_target(p["target"])
        if p["adaptscale"]:
            ens.set_adaptscale(True)
        ens.set_state(0.0, p["x0"], p["th0"], p["c"], np.uint64(seed) + np.arange(2, dtype=np.uint64))
        ens.refresh_consume_begin(p["dt"], K)
        events, slices = [[], []], 0
        while True:
            ens.run(p["T"], L.RUN_REFERENCE_TAIL)
            cnt = ens.counters()
            assert not np.any(cnt["status"] == L.CHAIN_BOUND_VIOLATED)
            ens.consume()
            for k in range(2):
                if cnt["ntrace"][k]:
                    events[k].append(ens.trace(k, 0, int(cnt["ntrace"][k]), counters=cnt))
            ens.trace_reset()
            slices += 1
            if not L.needs_rerun(cnt["status"]):
                break
        mean, T = ens.consume_mean()
        grids = [ens.consume_discretized(k) for k in range(2)]
        return [np.concatenate(e) for e in events], mean, T, grids, slices, ens.kernel_name()


@pytest.mark.parametrize("name", ["zz_local", "zz_adaptscale", "boom"])
def test_end_to_end_against_the_contract_and_trace_py(gpu_pkg, name):
    """Sampled traces, consumed slice by slice while the buffer is refilled, against the contract on the concatenated host trace (bit for bit)
    and trace.py (discretize bit for bit on the ZigZag, the FactBoomerang within 1e-12; mean within rtol 1e-12).

    Stale events (time below the running maximum before them) per chain, counted on the CPU oracle (oracle_lib.spdmp_zigzag, seeds 11 and 12 on
    other initial states): ZigZag λref = 4, T = 15 on the 16 x 16 lattice: 60 and 57 of 2967 and 2957 events (with adaptscale 68 and 58);
    FactBoomerang λref = 5, c = 10, T = 100 on maintest_precision(8): 24 and 26 of 616 and 632 events, so T = 200 here.  About one event in
    fifty is stale, not nearly every refresh: a refreshed coordinate's clock lags only if it has not been touched since the queue moved on."""
    pkg = gpu_pkg
    p = e2e_problem(pkg, name)
    K = int(p["T"] / p["dt"]) + 64
    events, mean, T, grids, slices, kernel = run_ensemble(pkg, p, K)
    assert slices >= 3 and kernel.startswith(p["kernel"]), (slices, kernel)
    mu = p["F"].μ if name == "boom" else None
    for k in range(2):
        ev = events[k]
        assert RC.stale_events(ev) >= 20 and RC.own_order_kept(ev, p["x0"].shape[1]), RC.stale_events(ev)
        r = R.consume(0.0, p["x0"][k], p["th0"][k], ev, mu=mu, dt=p["dt"], K=K)
        gt, gx = grids[k]
        assert r["npoints"] <= K and T[k] == r["T"] == ev["t"][-1]
        assert same(gt, r["grid_t"]) and same(gx, r["grid"][:r["npoints"]]) and same(mean[k], r["mean"])
        tr = pkg.FactTrace(p["F"], 0.0, p["x0"][k], p["th0"][k], ev)
        grid, X = pkg.trace.discretize(tr, p["dt"])
        assert same(gt, grid) and (same(gx, X) if mu is None else np.allclose(gx, X, rtol=0, atol=1e-12))
        assert np.allclose(mean[k], pkg.trace.mean(tr), **TOL)


@pytest.mark.parametrize("name", ["zz_local", "boom"])
def test_spdmp_keyword_equals_the_ensemble_calls(gpu_pkg, name):
    pkg = gpu_pkg
    p = e2e_problem(pkg, name)
    K = int(p["T"] / p["dt"]) + 64
    events, mean, T, grids, _, _ = run_ensemble(pkg, p, K)
    out = []
    for trace in (True, False):
        tr, _, _, _, cons = pkg.spdmp(p["target"], 0.0, p["x0"], p["th0"], p["T"], p["c"], p["F"], seed=11, trace_capacity=p["cap"], trace=trace,
                                      consume=dict(dt=p["dt"], points=K))
        assert sorted(cons) == ["T", "grid_t", "grid_x", "mean"]
        assert same(cons["mean"], mean) and same(cons["T"], T)
        for k in range(2):
            assert same(cons["grid_t"][k], grids[k][0]) and same(cons["grid_x"][k], grids[k][1])
            assert len(tr[k].events) == (len(events[k]) if trace else 0)
            if trace:
                assert tr[k].events.tobytes() == events[k].tobytes()
        out.append(cons)
    for key in ("cov", "hist", "condition"):  # refused before any device call
        bad = dict(dt=p["dt"], points=K)
        bad[key] = "diag" if key == "cov" else dict(lo=-1.0, hi=1.0, bins=4) if key == "hist" else (np.zeros(1), np.ones(1))
        with pytest.raises(TypeError, match="refresh clock"):
            pkg.spdmp(p["target"], 0.0, p["x0"], p["th0"], p["T"], p["c"], p["F"], device=10 ** 6, consume=bad)


# ------------------------------------------------------------------------------------------------------------------ calls and refusals
def test_calls_and_refusals(gpu_pkg):
    pkg = gpu_pkg
    L = pkg._lib
    INV, UNS = L.PDMP_ERR_INVALID, L.PDMP_ERR_UNSUPPORTED

    def code(fn):
        with pytest.raises(L.PdmpError) as ei:
            fn()
        return ei.value.code, str(ei.value)

    d = 4
    G = sp.identity(d, format="csc")
    x0, th0, seeds = np.zeros((1, d)), np.ones((1, d)), np.array([1], dtype=np.uint64)

    def fact(flow, cap=16, sampler=L.SAMPLER_ZIGZAG_LOCAL, state=True, **kw):
        ens = pkg.Ensemble(1, d, sampler=sampler, trace_capacity=cap, **kw)
        ens.set_flow(flow)
        ens.set_target(pkg.GaussianTarget(G))
        if sampler == L.SAMPLER_STICKY_ZIGZAG:
            ens.set_sticky(np.ones(d))
        if state:
            ens.set_state(0.0, x0, th0, np.ones(d), seeds)
        return ens

    zz, zzr, fb = pkg.ZigZag(G, np.zeros(d)), pkg.ZigZag(G, np.zeros(d), λref=1.0), pkg.FactBoomerang(G, np.zeros(d), 0.5)
    with fact(zz) as e:  # a ZigZag without refresh clock: its own entry serves it, and the message says so
        cd, msg = code(lambda: e.refresh_consume_begin(0.5, 4))
        assert cd == INV and "pdmp_ensemble_consume_begin" in msg
        e.consume_begin(0.5, 4)
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, trace_capacity=16) as e:
        assert code(lambda: e.refresh_consume_begin())[0] == INV
    with fact(zz, sampler=L.SAMPLER_STICKY_ZIGZAG, factor=1.5) as e:
        assert code(lambda: e.refresh_consume_begin())[0] == INV
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BARRIER_ZIGZAG, factor=1.5, trace_capacity=16) as e:
        e.set_flow(zz)
        e.set_target(pkg.GaussianTarget(G))
        b = pkg.StickyBarriers((-1.0, 1.0), ("reflect", "reflect"), (np.inf, np.inf))
        e.set_barriers(np.full(d, b.x[0]), np.full(d, b.x[1]), np.full(d, L.BARRIER_RULES[b.rule[0]], dtype=np.int32),
                       np.full(d, L.BARRIER_RULES[b.rule[1]], dtype=np.int32), np.full(d, b.κ[0]), np.full(d, b.κ[1]), False)
        e.set_state(0.0, x0, th0, np.ones(d), seeds)
        assert code(lambda: e.refresh_consume_begin())[0] == INV
    for F in (zzr, fb):
        with fact(F, cap=0) as e:
            assert code(lambda: e.refresh_consume_begin())[0] == INV  # no trace buffer
        with fact(F, state=False) as e:
            assert code(lambda: e.refresh_consume_begin())[0] == INV  # before set_state
        with fact(F) as e:
            cd, msg = code(lambda: e.consume_begin(0.5, 4))  # consume_begin itself keeps refusing these flows, in its own words
            assert cd == UNS and "piecewise-linear" in msg
            assert code(lambda: e.consume())[0] == INV       # begin first
            assert code(lambda: e.refresh_consume_begin(0.5, -1))[0] == INV
            assert code(lambda: e.refresh_consume_begin(0.0, 4))[0] == INV
            assert code(lambda: e.refresh_consume_begin(-1.0, 4))[0] == INV
            e.refresh_consume_begin(0.5, 8)
            ev = np.zeros(3, dtype=L.EVENT_DTYPE)
            ev["t"], ev["i"], ev["x"], ev["theta"] = [0.75, 1.75, 0.25], [0, 1, 2], [1.0, 2.0, 3.0], [1.0, -1.0, 1.0]
            e.debug_trace_append(0, ev)
            e.consume()
            before = (e.consume_mean()[0].tobytes(), all_rows(e, 0, 8)[0].tobytes(), all_rows(e, 0, 8)[1])
            assert before[2] == 4
            refusals = [lambda: e.consume_async(), lambda: e.consume_condition(np.zeros(d), np.ones(d), 4), lambda: e.consume_pairs([0], [0]),
                        lambda: e.consume_hist([0], 0.0, 1.0, 4), lambda: e.consume_inclusion()]
            for fn in refusals:
                cd, msg = code(fn)
                # (consume_condition on a FactBoomerang keeps its older reason: src/condition.jl has no hitting time for the rotation)
                assert cd == UNS and ("sorted within a coordinate only" in msg or (F is fb and "no method for the Boomerang flows" in msg)), msg
                assert (e.consume_mean()[0].tobytes(), all_rows(e, 0, 8)[0].tobytes(), all_rows(e, 0, 8)[1]) == before
            assert len(e.subtrace(0, [0, 2])) == 2  # subtrace serves it unchanged
        with fact(F, cap=64) as e:
            e.run(1.0, L.RUN_STOP_BEFORE)
            assert code(lambda: e.refresh_consume_begin())[0] == INV  # after the first run
