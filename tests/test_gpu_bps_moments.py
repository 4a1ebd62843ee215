"""Path moments of BouncyParticle / Boomerang on the device (pdmp_ensemble_set_bps_moments / pdmp_ensemble_bps_moments, -m gpu):
the moments never change the chains, they equal trace.path_moments of the drained trace, and the ZigZag's batch-means / ESS / path-integral
entry points accept a BPS ensemble that keeps them."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

import bps_width_cases as BW

pytestmark = pytest.mark.gpu


WIDTHS = (129, 256, 257, 513)  # NS = 4 and 8 with empty trailing slots, FULL of NS = 4, NS = 16 with seven empty slots


def _case(pkg, name, d, rng):
    """(setup(ens), c, adapt, flow, info) of one dispatcher branch (adapt everywhere: a constant Boomerang bound or a target of its own
    can be violated; only the "adapt" case is meant to be)."""
    I = sp.identity(d, format="csc")
    z = np.zeros(d)
    if name == "iso":  # Γ = I, μ = 0: the IDENT kernels (FULL at d = 64 NS; launch_big beyond 1024)
        B = pkg.BouncyParticle(I, z, 1.0)
        return (lambda e: e.set_flow_bps(B)), 1e-3, False, B, {}
    if name == "diag":  # Γ = I, μ ≠ 0: diagonal, not IDENT
        B = pkg.BouncyParticle(I, rng.standard_normal(d), 1.0)
        return (lambda e: e.set_flow_bps(B)), 1e-3, False, B, {}
    if d in WIDTHS:  # no square: the Γ of the slot-count matrix (tests/bps_width_cases.py), which couples slots and lanes
        G = BW.coupling_gamma(d)
    else:
        G = pkg.problems.gmrf_precision(int(round(np.sqrt(d)))) if d >= 64 else pkg.problems.maintest_precision(d)
    if name == "csc":  # general Γ with the identity mass: the CSC gather without the extended instantiation
        B = pkg.BouncyParticle(G, z, 0.7, L=I)
        return (lambda e: e.set_flow_bps(B)), 1.0, False, B, {}
    if name == "mass":  # general Γ with its Cholesky factor: extended instantiation
        B = pkg.BouncyParticle(G, rng.standard_normal(d) * 0.3, 0.7, 0.2)
        return (lambda e: e.set_flow_bps(B)), 1.0, False, B, {}
    if name in ("own_target", "adapt"):  # a target of its own: GlobalBound keeps the flow's Γ = I -- with a tiny c the bound is violated
        B = pkg.BouncyParticle(I, z, 1.0)
        tgt = pkg.GaussianTarget(G)

        def setup(e):
            e.set_flow_bps(B)
            e.set_target(tgt)
        return setup, (1e-3 if name == "adapt" else 2.0), True, B, {}
    if name == "local":
        B = pkg.BouncyParticle(G, z, 0.7)
        return (lambda e: (e.set_flow_bps(B), e.set_bps_options(True, False))), 1.0, False, B, {}
    if name == "subsample":
        B = pkg.BouncyParticle(G, z, 0.7)
        return (lambda e: (e.set_flow_bps(B), e.set_bps_options(False, True))), 1.0, False, B, {"hides": True}
    if name in ("boom_diag", "boom_csc"):  # (a diagonal target other than the flow's I: grad_correct! leaves a gradient, reflections happen)
        mf = rng.standard_normal(d)
        B = pkg.Boomerang(I, mf, 0.5)
        tgt = pkg.GaussianTarget(sp.diags(rng.uniform(1.3, 2.0, d), format="csc") if name == "boom_diag" else G, mf)
        return (lambda e: e.set_flow_boomerang(tgt, B)), (3.0 if name == "boom_diag" else 8.0), True, B, {}
    if name == "boom_mass":
        mf = rng.standard_normal(d)
        B = pkg.Boomerang(G, mf, 0.5)
        return (lambda e: e.set_flow_boomerang(pkg.GaussianTarget(G, mf), B)), 8.0, True, B, {}
    raise ValueError(name)


def _drive(pkg, name, d, order, *, nch=3, cap=4, schedule=((2.0, "stop"), (3.5, "stop"), (4.0, "tail")), seed=5):
    """Run one case with moments of `order` through `schedule` (each step re-run on TRACE_FULL, the trace drained after every launch);
    moments read at every stop.  Returns traces, counters, final state, [(T, J1, J2)]."""
    L = pkg._lib
    rng = np.random.default_rng(d * 31 + len(name))
    setup, c, adapt, F, info = _case(pkg, name, d, rng)
    x0, th0 = rng.standard_normal((nch, d)), rng.standard_normal((nch, d))
    ev = [[] for _ in range(nch)]
    moms = []
    with pkg.Ensemble(nch, d, sampler=L.SAMPLER_BPS, adapt=adapt, factor=2.0, trace_capacity=cap) as ens:
        setup(ens)
        if order:
            ens.set_bps_moments(order)
        ens.set_state_bps(0.0, x0, th0, c, seed + np.arange(nch, dtype=np.uint64))
        nrun = 0
        for T, kind in schedule:
            while True:
                ens.run(T, L.RUN_STOP_BEFORE if kind == "stop" else L.RUN_REFERENCE_TAIL)
                nrun += 1
                cnt = ens.counters()
                for k in range(nch):
                    if cnt["ntrace"][k]:
                        ev[k].append(ens.bps_trace(k, counters=cnt))
                ens.trace_reset()
                if not L.needs_rerun(cnt["status"]):
                    break
            if order and kind == "stop":
                moms.append((T,) + ens.bps_moments(T))
        cnt = ens.counters()
        fs = ens.bps_final_state()
    traces = []
    for k in range(nch):
        t = np.concatenate([p[0] for p in ev[k]]) if ev[k] else np.empty(0)
        x = np.concatenate([p[1] for p in ev[k]]) if ev[k] else np.empty((0, d))
        th = np.concatenate([p[2] for p in ev[k]]) if ev[k] else np.empty((0, d))
        traces.append(pkg.PDMPTrace(F, 0.0, x0[k].copy(), th0[k].copy(), t, x, th))
    return traces, cnt, fs, moms, nrun, info


def _check_against_host(pkg, traces, moms, d):
    for T, J1, J2 in moms:
        for k, tr in enumerate(traces):
            keep = tr.t < T  # (the trace was drained after the stop at the last T: events past T came later)
            sub = pkg.PDMPTrace(tr.F, tr.t0, tr.x0, tr.θ0, tr.t[keep], tr.x[keep], tr.θ[keep])
            h1, h2 = pkg.trace.path_moments(sub, T)
            s2 = np.abs(h2).max()
            s1 = np.sqrt((T - tr.t0) * s2)  # >= ∫|x_i| dt for every i (Cauchy-Schwarz)
            assert np.max(np.abs(J1[k] - h1)) <= 1e-9 * s1, (k, T, np.max(np.abs(J1[k] - h1)), s1)
            assert J2 is not None and np.max(np.abs(J2[k] - h2)) <= 1e-9 * s2, (k, T, np.max(np.abs(J2[k] - h2)), s2)


CASES = [("iso", 1), ("iso", 63), ("iso", 64), ("iso", 100), ("iso", 1024), ("iso", 4096), ("diag", 100), ("diag", 1024),
         ("csc", 8), ("csc", 100), ("mass", 8), ("mass", 100), ("own_target", 100), ("adapt", 100), ("local", 100), ("subsample", 100),
         ("boom_diag", 8), ("boom_diag", 1024), ("boom_csc", 100), ("boom_mass", 100)]
CASES += [(name, d) for d in WIDTHS for name in ("iso", "csc", "mass", "boom_csc")]  # the moment-keeping forms at 4, 8 and 16 slots per lane


@pytest.mark.parametrize("name,d", CASES)
def test_moments_are_bit_transparent_and_equal_the_trace(gpu_pkg, name, d):
    """Order 2 against order 0 over several launches (a small trace buffer: TRACE_FULL resumes), STOP_BEFORE stops and a reference
    tail: identical traces, counters and final state; at every stop J(T) equals trace.path_moments of the drained trace."""
    pkg = gpu_pkg
    sched = ((0.6, "stop"), (1.1, "stop"), (1.3, "tail")) if d >= 1024 else ((2.0, "stop"), (3.5, "stop"), (4.0, "tail"))
    cap = 1 if name in ("subsample", "boom_diag") else 4  # (subsample records refreshments only; few events on the diagonal Boomerang)
    tr0, c0, f0, _, n0, _ = _drive(pkg, name, d, 0, schedule=sched, cap=cap)
    tr2, c2, f2, moms, n2, info = _drive(pkg, name, d, 2, schedule=sched, cap=cap)
    assert n0 == n2 and n0 > len(sched)  # several launches per step
    assert np.array_equal(c0, c2)
    for a, b in zip(tr0, tr2):
        assert np.array_equal(a.t, b.t) and np.array_equal(a.x, b.x) and np.array_equal(a.θ, b.θ)
    for key in ("t", "x", "theta", "c"):
        assert np.array_equal(f0[key], f2[key]), key
    assert sum(len(q.t) for q in tr0) > 6
    if name == "adapt":
        assert np.any(f0["c"] > 1e-3)  # the bound was violated and adapted
    if not info.get("hides"):  # (subsample hides accepted reflections from the trace: transparency only)
        _check_against_host(pkg, tr2, moms, d)


def test_moments_start_at_zero_after_set_state(gpu_pkg):
    """J(t0) = 0 right after set_state_bps -- also where set_state_bps's placement probes ran launches in between (4096 x 1024 x cap 64
    is exactly 2 GiB per event array) and after a second set_state on a used ensemble."""
    pkg = gpu_pkg
    L = pkg._lib
    for nch, d, cap in ((4, 64, 8), (4096, 1024, 64)):
        rng = np.random.default_rng(nch)
        x0, th0 = rng.standard_normal((nch, d)), rng.standard_normal((nch, d))
        with pkg.Ensemble(nch, d, sampler=L.SAMPLER_BPS, trace_capacity=cap) as ens:
            ens.set_flow_bps(pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0))
            ens.set_bps_moments(2)
            ens.set_state_bps(0.0, x0, th0, 1e-3, np.arange(nch, dtype=np.uint64))
            J1, J2 = ens.bps_moments(0.0)
            assert not J1.any() and not J2.any()
            ens.run(0.2, L.RUN_STOP_BEFORE)
            ens.trace_reset()
            assert np.abs(ens.bps_moments(0.2)[1]).max() > 0
            ens.set_state_bps(0.0, x0, th0, 1e-3, np.arange(nch, dtype=np.uint64))
            J1, J2 = ens.bps_moments(0.0)
            assert not J1.any() and not J2.any()


def test_existing_entry_points_accept_a_bps_ensemble_with_moments(gpu_pkg):
    """Order 1: batch_means, path_integrals, ess_begin / _batch / _end and parallel.Comm.reduce_moments equal the sums formed on the host
    from bps_moments differences."""
    pkg = gpu_pkg
    L = pkg._lib
    nch, d = 6, 100
    rng = np.random.default_rng(7)
    x0, th0 = rng.standard_normal((nch, d)), rng.standard_normal((nch, d))
    with pkg.parallel.Comm(0, 1, 0) as comm, pkg.Ensemble(nch, d, sampler=L.SAMPLER_BPS, trace_capacity=0) as ens:
        ens.set_flow_bps(pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0))
        ens.set_bps_moments(1)
        ens.set_state_bps(0.0, x0, th0, 1e-3, np.arange(nch, dtype=np.uint64))

        def J(T):
            ens.run(T, L.RUN_STOP_BEFORE)
            j1, j2 = ens.bps_moments(T)
            assert j2 is None
            return j1

        def close(a, b):
            assert np.allclose(a, b, rtol=1e-12, atol=1e-12 * np.abs(b).max()), np.abs(a - b).max()

        J1 = J(1.0)
        s1, s2 = ens.batch_means(0.0, 1.0)  # (the first batch starts at the ensemble's t0: jprev = 0)
        close(s1, (J1 / 1.0).sum(0))
        close(s2, ((J1 / 1.0) ** 2).sum(0))
        J2 = J(2.5)
        s1, s2 = ens.batch_means(1.0, 2.5)
        Y = (J2 - J1) / 1.5
        close(s1, Y.sum(0))
        close(s2, (Y * Y).sum(0))
        probes = np.array([0, 17, 99], dtype=np.int64)
        close(ens.path_integrals(2.5, probes), J2[:, probes])
        J3 = J(3.0)
        r1, r2 = comm.reduce_moments(ens, 2.5, 3.0)
        Y = (J3 - J2) / 0.5
        close(r1, Y.sum(0))
        close(r2, (Y * Y).sum(0))
        # ESS: begin at 3, four batches of 0.5
        ens.ess_begin(3.0)
        Js = [J3]
        for b in range(1, 5):
            Js.append(J(3.0 + 0.5 * b))
            ens.ess_batch(3.0 + 0.5 * b)
        ens.run(6.0, L.RUN_STOP_BEFORE)  # (ess_end reads what the batches left, not the state)
        sy, sy2, sm, sm2, nb, T0, T1 = ens.ess_end()
        Ys = [(Js[b] - Js[b - 1]) / 0.5 for b in range(1, 5)]
        M = (Js[4] - Js[0]) / 2.0
        close(sy, sum(Y.sum(0) for Y in Ys))
        close(sy2, sum((Y * Y).sum(0) for Y in Ys))
        close(sm, M.sum(0))
        close(sm2, (M * M).sum(0))
        assert nb == 4 and T0 == 3.0 and T1 == 5.0


def test_refusals_return_a_status(gpu_pkg):
    pkg = gpu_pkg
    L = pkg._lib
    d, nch = 8, 3
    I = sp.identity(d, format="csc")
    rng = np.random.default_rng(9)
    x0, th0 = rng.standard_normal((nch, d)), rng.standard_normal((nch, d))
    seeds = np.arange(nch, dtype=np.uint64)

    def refused(call):
        with pytest.raises(L.PdmpError) as ei:
            call()
        assert ei.value.code == L.PDMP_ERR_INVALID, str(ei.value)
        return str(ei.value)

    with pkg.Ensemble(nch, d, sampler=L.SAMPLER_BPS, trace_capacity=4) as ens:
        ens.set_flow_bps(pkg.BouncyParticle(I, np.zeros(d), 1.0))
        refused(lambda: ens.set_bps_moments(3))
        refused(lambda: ens.set_bps_moments(-1))
        ens.set_bps_moments(1)
        ens.set_state_bps(0.0, x0, th0, 1e-3, seeds)
        refused(lambda: ens.set_bps_moments(2))  # after set_state_bps
        j = np.empty((nch, d))
        assert L.load().pdmp_ensemble_bps_moments(ens._h, 0.0, 0, nch, j.ctypes.data, j.ctypes.data) == L.PDMP_ERR_INVALID  # J2 at order 1
        ens.run(5.0, L.RUN_STOP_BEFORE)  # (a full trace buffer: some chains pause before 5)
        cnt = ens.counters()
        fs = ens.bps_final_state()
        paused = np.flatnonzero(cnt["status"] == L.CHAIN_TRACE_FULL)
        assert len(paused)  # a TRACE_FULL pause whose next event lies before T
        msg = refused(lambda: ens.bps_moments(5.0))
        assert int(re.search(r"chain (\d+)", msg).group(1)) in paused.tolist(), msg
        refused(lambda: ens.batch_means(0.0, 5.0))
        ens.bps_moments(float(fs["t"][paused[0]]), int(paused[0]), 1)  # (that chain alone, at its own clock)
        ens.trace_reset()
        while True:
            ens.run(5.0, L.RUN_STOP_BEFORE)
            st = ens.counters()["status"]
            ens.trace_reset()
            if not L.needs_rerun(st):
                break
        ens.bps_moments(5.0)
        refused(lambda: ens.bps_moments(1e6))  # T past a chain's next event
        ens.run(5.0, L.RUN_REFERENCE_TAIL)  # every chain's clock passes 5
        ens.trace_reset()
        msg = refused(lambda: ens.bps_moments(5.0))  # T below a chain's clock
        assert "chain" in msg
        refused(lambda: ens.ess_begin(5.0))
    with pkg.Ensemble(nch, d, trace_capacity=4) as ens:  # a ZigZag ensemble
        ens.set_flow(pkg.ZigZag(I, np.zeros(d)))
        refused(lambda: ens.set_bps_moments(1))
    with pkg.Ensemble(nch, d, sampler=L.SAMPLER_BPS, trace_capacity=4) as ens:  # order 0 refuses as before
        ens.set_flow_bps(pkg.BouncyParticle(I, np.zeros(d), 1.0))
        ens.set_state_bps(0.0, x0, th0, 1e-3, seeds)
        ens.run(1.0, L.RUN_STOP_BEFORE)
        refused(lambda: ens.batch_means(0.0, 1.0))
        refused(lambda: ens.ess_begin(1.0))
        refused(lambda: ens.bps_moments(1.0))


def test_statistics_at_c2_width(gpu_pkg):
    """4096 x 1024, stationary start, λref = 1, T = 30, no trace, order 2: the pooled time averages estimate N(0, I)."""
    pkg = gpu_pkg
    L = pkg._lib
    nch, d, T = 4096, 1024, 30.0
    rng = np.random.default_rng(30)
    x0, th0 = rng.standard_normal((nch, d)), rng.standard_normal((nch, d))
    with pkg.Ensemble(nch, d, sampler=L.SAMPLER_BPS, trace_capacity=0) as ens:
        ens.set_flow_bps(pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0))
        ens.set_bps_moments(2)
        ens.set_state_bps(0.0, x0, th0, 1e-3, np.arange(nch, dtype=np.uint64))
        ens.run(T, L.RUN_STOP_BEFORE)
        assert np.all(ens.counters()["status"] == L.CHAIN_OK)
        J1, J2 = ens.bps_moments(T)
    m = J1 / T  # [nch x d]
    pooled = m.mean()
    se = m.mean(1).std(ddof=1) / np.sqrt(nch)  # spread between chains of the chain's coordinate average
    assert abs(pooled) < 5 * se, (pooled, se)
    assert abs((J2 / T).mean() - 1.0) < 0.01


@pytest.mark.parametrize("flow", ["bps", "boomerang"])
def test_sampler_keyword(gpu_pkg, flow):
    """pdmp(..., moments=True): the first four elements bit for bit those of moments=False; mean / var those of trace.path_moments."""
    pkg = gpu_pkg
    rng = np.random.default_rng(11)
    d = 40
    I = sp.identity(d, format="csc")
    if flow == "bps":
        args = (None, 0.0, None, None, 6.0, 1e-3, pkg.BouncyParticle(I, np.zeros(d), 1.0))
    else:
        mf = rng.standard_normal(d)
        args = (pkg.GaussianTarget(1.2 * I, mf), 0.0, None, None, 6.0, 3.0, pkg.Boomerang(I, mf, 0.5))
    for nch in (1, 3):
        x0 = rng.standard_normal((nch, d)) if nch > 1 else rng.standard_normal(d)
        th0 = rng.standard_normal(x0.shape)
        a = list(args)
        a[2], a[3] = x0, th0
        r0 = pkg.pdmp(*a, seed=4, trace_capacity=8, adapt=True)
        r1 = pkg.pdmp(*a, seed=4, trace_capacity=8, adapt=True, moments=True)
        assert len(r0) == 4 and len(r1) == 5
        trs0, trs1 = (r0[0], r1[0]) if nch > 1 else ([r0[0]], [r1[0]])
        for q0, q1 in zip(trs0, trs1):
            assert np.array_equal(q0.t, q1.t) and np.array_equal(q0.x, q1.x) and np.array_equal(q0.θ, q1.θ)
        for u, v in zip(r0[1:4], r1[1:4]):
            for p, q in zip(u if isinstance(u, tuple) else (u,), v if isinstance(v, tuple) else (v,)):
                assert np.array_equal(p, q)
        mom = r1[4]
        assert mom["T"] == 6.0
        means = np.atleast_2d(mom["mean"])
        vars_ = np.atleast_2d(mom["var"])
        assert means.shape == (nch, d)
        for k, tr in enumerate(trs1):
            h1, h2 = pkg.trace.path_moments(tr, 6.0)
            hm = h1 / 6.0
            assert np.allclose(means[k], hm, rtol=1e-9, atol=1e-9 * np.sqrt(np.abs(h2).max() / 6.0))
            assert np.allclose(vars_[k], h2 / 6.0 - hm * hm, rtol=1e-8, atol=1e-9 * np.abs(h2).max() / 6.0)
        r2 = pkg.pdmp(*a, seed=4, trace=False, adapt=True, moments=True)  # the trace-free run: same moments
        assert np.array_equal(np.atleast_2d(r2[4]["mean"]), means) and np.array_equal(np.atleast_2d(r2[4]["var"]), vars_)
