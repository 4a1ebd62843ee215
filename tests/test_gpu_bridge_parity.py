"""The diffusion bridge in the Faber-Schauder basis (research/diffusion_bridge/) on gfx950 -- zz_bridge_run_kernel, csrc/pdmp_bridge.inc --
against its CPU restatement (tests/ref/bridge_ref.c), bit for bit, through the C ABI and the public samplers (-m gpu)."""
import numpy as np
import pytest
import scipy.sparse as sp

import bridge_ref_lib as R

pytestmark = pytest.mark.gpu
SCRIPT = dict(alpha=1.5, beta=0.1, omega=2 * np.pi)  # diffbridge.jl:7-9


def flow(pkg, d):
    return pkg.ZigZag(sp.identity(d, format="csc"), np.zeros(d))


def device_run(pkg, L, T, x0, th0, c, seeds, TP, *, alpha, beta, omega, adapt=False, factor=1.8, cap=1 << 14, slices=()):
    """Every chain to T′ through the C ABI: PDMP_RUN_STOP_BEFORE to each of `slices`, then the reference tail; the trace is drained whenever a
    launch returns.  Returns (events per chain, counters, final state, launches)."""
    Lb = pkg._lib
    d = (2 << L) + 1
    nch = x0.shape[0]
    events = [[] for _ in range(nch)]
    launches = 0
    with pkg.Ensemble(nch, d, adapt=adapt, factor=factor, trace_capacity=cap) as ens:
        ens.set_flow(flow(pkg, d))
        ens.set_target(pkg.DiffusionBridgeTarget(L, T, alpha, beta, omega))
        ens.set_state(0.0, x0, th0, c, seeds)
        for Tk, flags in [(s, Lb.RUN_STOP_BEFORE) for s in slices] + [(TP, Lb.RUN_REFERENCE_TAIL)]:
            while True:
                ens.run(Tk, flags)
                launches += 1
                cnt = ens.counters()
                for k in range(nch):
                    if cnt["ntrace"][k]:
                        events[k].append(ens.trace(k, counters=cnt))
                ens.trace_reset()
                if not Lb.needs_rerun(cnt["status"]):
                    break
        assert ens.kernel_name() == "zz_bridge_run_kernel"
        cnt, fs = ens.counters(), ens.final_state()
    ev = [np.concatenate(e) if e else np.empty(0, dtype=Lb.EVENT_DTYPE) for e in events]
    return ev, cnt, fs, launches


def compare(ev, cnt, fs, refs, chains=None):
    """events, num, nacc, nevents, ndraw_main, ndraw_global, status, final (t, x, θ), per-coordinate acc and the adapted c: bitwise."""
    for k, r in zip(range(len(refs)) if chains is None else chains, refs):
        assert int(cnt["status"][k]) == r["status"], (k, int(cnt["status"][k]), r["status"])
        assert len(ev[k]) == r["nevents"] == len(r["t"]), (k, len(ev[k]), r["nevents"])
        for f in ("i", "t", "x", "theta"):
            assert np.array_equal(ev[k][f], r[f]), (k, f, int(np.argmax(ev[k][f] != r[f])))
        got = tuple(int(cnt[f][k]) for f in ("num", "nacc", "nevents", "ndraw_main", "ndraw_global"))
        assert got == (r["num"], r["nacc"], r["nevents"], r["ndraw_main"], r["ndraw_global"]), (k, got)
        assert np.array_equal(fs["t"][k], r["t_state"]) and np.array_equal(fs["x"][k], r["x_final"]) and np.array_equal(fs["theta"][k], r["theta_final"]), k
        assert np.array_equal(fs["c"][k], r["c_final"]) and np.array_equal(fs["acc"][k], r["acc"]), k
        assert cnt["t_last"][k] == r["t_last"]


def pair(pkg, L, TP, seed, *, T=2.0, u=1.5, v=-0.5, nch=3, c_scale=1.0, adapt=True, drift=SCRIPT, **kw):
    x0, th0, c = pkg.problems.diffusion_bridge_problem(L, T, u, v, nchains=nch, rng=np.random.default_rng(seed))
    c = c * c_scale
    seeds = np.uint64(seed) + np.arange(nch, dtype=np.uint64)
    out = device_run(pkg, L, T, x0, th0, c, seeds, TP, adapt=adapt, **drift, **kw)
    refs = [R.bridge(x0[k], th0[k], TP, c, L=L, T=T, adapt=adapt, seed=int(seeds[k]), **drift) for k in range(nch)]
    compare(out[0], out[1], out[2], refs)
    return out, refs


# L, T′: the smallest sizes at which the loop takes another shape -- one interior coordinate and one level; two levels; d = 65, the first
# size past one key per lane (two key blocks); d = 257, the script's; d = 2049, the largest shipped (33 key blocks, 11 levels), short T′
SHAPES = [(0, 400.0), (1, 200.0), (5, 30.0), (7, 8.0), (10, 1.5)]


@pytest.mark.parametrize("L,TP", SHAPES, ids=["L%d" % s[0] for s in SHAPES])
def test_shapes_adapting_from_c_1(gpu_pkg, L, TP):
    """adapt = True from c = 1, the script's configuration: the violation-and-grow path runs in every chain (asserted on the restatement)."""
    _, refs = pair(gpu_pkg, L, TP, 11 + L)
    assert all(r["status"] == R.REF_OK and r["nadapt"] > 0 and r["nevents"] > 50 for r in refs)
    assert all(r["i"].min() >= 1 and r["i"].max() <= (2 << L) - 1 for r in refs)  # (the end points never pop)


@pytest.mark.parametrize("uv", [(1.5, -0.5), (0.7, 0.7)], ids=["u_ne_v", "u_eq_v"])
@pytest.mark.parametrize("omega", [2 * np.pi, 1.0], ids=["omega_2pi", "omega_1"])
def test_fixed_bound_never_violated(gpu_pkg, uv, omega):
    """adapt = False with a bound the restatement shows is never violated (status OK to T′, every accept below its bound)."""
    _, refs = pair(gpu_pkg, 4, 6.0, 31, u=uv[0], v=uv[1], adapt=False, c_scale=400.0, drift=dict(alpha=1.5, beta=0.1, omega=omega))
    assert all(r["status"] == R.REF_OK and r["nadapt"] == 0 and r["nevents"] > 50 and r["num"] > 50000 for r in refs)


def test_bound_violated_at_the_same_event(gpu_pkg):
    """adapt = False with c too small: BOUND_VIOLATED in both, after the same events and draws; the public call raises the reference's error."""
    pkg = gpu_pkg
    (ev, cnt, _, _), refs = pair(pkg, 4, 50.0, 41, adapt=False, c_scale=2.0)
    assert all(r["status"] == R.REF_BOUND_VIOLATED for r in refs) and np.all(cnt["status"] == pkg._lib.CHAIN_BOUND_VIOLATED)
    x0, th0, c = pkg.problems.diffusion_bridge_problem(4, 2.0, 1.5, -0.5, rng=np.random.default_rng(41))
    with pytest.raises(RuntimeError, match="too small"):
        pkg.spdmp(pkg.DiffusionBridgeTarget(4, 2.0), 0.0, x0, th0, 50.0, 2.0 * c, flow(pkg, 33), pkg.SelfMoving(), seed=41)


def test_across_launches(gpu_pkg, monkeypatch):
    """Five PDMP_RUN_STOP_BEFORE slices, a trace buffer of 4 events, and PDMP_LAUNCH_COUNT_LIMIT pauses: the bytes of the restatement's
    one-shot run each time (compare() inside pair())."""
    pkg = gpu_pkg
    (_, _, _, n1), refs = pair(pkg, 5, 12.0, 51, slices=(1.0, 4.5, 4.75, 8.0, 11.0))
    assert n1 == 6 and all(r["nevents"] > 300 for r in refs)
    (_, _, _, n2), _ = pair(pkg, 3, 12.0, 52, cap=4)
    assert n2 > 20
    monkeypatch.setenv("PDMP_LAUNCH_COUNT_LIMIT", "300")
    (_, _, _, n3), refs = pair(pkg, 5, 12.0, 51)
    assert n3 > 5 and min(r["ndraw_main"] for r in refs) > 5 * 300


def test_stalled_chain(gpu_pkg):
    """|ωx| beyond pdmp_sincos' range: PDMP_CHAIN_STALLED at the first proposal, as the restatement."""
    _, refs = pair(gpu_pkg, 2, 5.0, 61, drift=dict(alpha=1.5, beta=0.1, omega=1e12))
    assert all(r["status"] == R.REF_STALLED and r["num"] == 0 for r in refs)


def test_256_chains_first_and_last(gpu_pkg):
    pkg = gpu_pkg
    L, T, TP, nch = 5, 2.0, 10.0, 256
    x0, th0, c = pkg.problems.diffusion_bridge_problem(L, T, 1.5, -0.5, nchains=nch, rng=np.random.default_rng(71))
    seeds = np.uint64(71) + np.arange(nch, dtype=np.uint64)
    ev, cnt, fs, _ = device_run(pkg, L, T, x0, th0, c, seeds, TP, adapt=True, **SCRIPT)
    refs = [R.bridge(x0[k], th0[k], TP, c, L=L, T=T, adapt=True, seed=int(seeds[k]), **SCRIPT) for k in (0, nch - 1)]
    compare(ev, cnt, fs, refs, chains=(0, nch - 1))
    assert np.all(cnt["status"] == pkg._lib.CHAIN_OK) and np.all(cnt["nevents"] > 100)


def test_public_call_and_consumers(gpu_pkg):
    """spdmp(target, 0.0, ξ0, θ0, T′, c, ZigZag(I, 0), SelfMoving(), adapt=True) returns the usual 4-tuple, bit for bit the restatement's;
    with and without the marker; consume=dict(dt, points) adds the device consumers' results: pdmp_ensemble_consume_discretized equals
    trace.discretize on the returned trace bit for bit and consume_mean equals trace.mean (tests/test_gpu_consumers.py's tolerances)."""
    pkg = gpu_pkg
    L, T, TP = 5, 2.0, 20.0
    d = (2 << L) + 1
    x0, th0, c = pkg.problems.diffusion_bridge_problem(L, T, 1.5, -0.5, nchains=2, rng=np.random.default_rng(81))
    tgt = pkg.DiffusionBridgeTarget(L, T, **{"α": 1.5, "β": 0.1, "ω": 2 * np.pi})
    args = (tgt, 0.0, x0, th0, TP, c, flow(pkg, d))
    tr, (t, x, th), (acc, num), cc = pkg.spdmp(*args, pkg.SelfMoving(), adapt=True, seed=81)
    for k in range(2):
        r = R.bridge(x0[k], th0[k], TP, c, L=L, T=T, adapt=True, seed=81 + k, **SCRIPT)
        for f in ("i", "t", "x", "theta"):
            assert np.array_equal(tr[k].events[f], r[f])
        assert np.array_equal(t[k], r["t_state"]) and np.array_equal(x[k], r["x_final"]) and np.array_equal(th[k], r["theta_final"])
        assert np.array_equal(acc[k], r["acc"]) and int(num[k]) == r["num"] and np.array_equal(cc[k], r["c_final"]) and r["nadapt"] > 0
    plain = pkg.spdmp(*args, adapt=True, seed=81)  # (the marker is carried by the target's type)
    assert all(plain[0][k].events.tobytes() == tr[k].events.tobytes() for k in range(2))
    dt, K = 0.37, 64
    out = pkg.spdmp(*args, pkg.ExtendedForm(), adapt=True, seed=81, trace_capacity=300, consume=dict(dt=dt, points=K))
    assert len(out) == 5 and all(out[0][k].events.tobytes() == tr[k].events.tobytes() for k in range(2)) and len(tr[0].events) > 500
    for k in range(2):
        grid, X = pkg.trace.discretize(tr[k], dt)
        assert len(grid) > 40 and np.array_equal(out[4]["grid_t"][k], grid) and np.array_equal(out[4]["grid_x"][k], X)
        assert np.allclose(out[4]["mean"][k], pkg.trace.mean(tr[k]), rtol=1e-12, atol=1e-15) and out[4]["T"][k] == tr[k].events["t"][-1]
        paths = pkg.trace.faber_schauder_path(X, np.linspace(0, T, 9)[:-1], L, T)
        assert paths.shape == (len(grid), 8) and np.allclose(paths[:, 0], 1.5, rtol=0, atol=1e-12)  # every sampled bridge starts at u
    one = pkg.spdmp(tgt, 0.0, x0[0], th0[0], TP, c, flow(pkg, d), pkg.SelfMoving(), adapt=True, seed=81, trace=False, consume=dict(dt=dt, points=K))
    assert len(one[0].events) == 0 and np.array_equal(one[4]["grid_x"], out[4]["grid_x"][0]) and np.array_equal(one[4]["mean"], out[4]["mean"][0])


def test_subtrace_and_cummean_serve_the_bridge_trace(gpu_pkg):
    """pdmp_ensemble_subtrace_copy and pdmp_ensemble_consume_cummean on a bridge ensemble, against trace.py on the same events."""
    pkg = gpu_pkg
    L, T = 3, 2.0
    d = (2 << L) + 1
    x0, th0, c = pkg.problems.diffusion_bridge_problem(L, T, 1.5, -0.5, nchains=1, rng=np.random.default_rng(91))
    with pkg.Ensemble(1, d, adapt=True, trace_capacity=4096) as ens:
        ens.set_flow(flow(pkg, d))
        ens.set_target(pkg.DiffusionBridgeTarget(L, T))
        ens.set_state(0.0, x0, th0, c, np.array([91], dtype=np.uint64))
        ens.consume_begin()
        ens.consume_cummean(True)
        ens.run(20.0, pkg._lib.RUN_STOP_BEFORE)
        ens.consume()
        ev = ens.trace(0)
        assert 200 < len(ev) < 4096
        tr = pkg.FactTrace(flow(pkg, d), 0.0, x0[0], th0[0], ev)
        J = np.array([1, 4, 8, 15])
        sub = ens.subtrace(0, J)
        want = pkg.trace.subtrace(tr, J)
        assert sub.tobytes() == np.ascontiguousarray(want.events).tobytes()
        tt, yy = ens.consume_cummean_pairs(0, len(ev))
        cm = pkg.trace.cummean(tr)  # per coordinate: (times, running means), the first entry being (t0, x0)
        nxt = np.ones(d, dtype=np.int64)
        for k, e in enumerate(ev):
            i = int(e["i"])
            assert tt[k] == cm[i][0][nxt[i]] and np.isclose(yy[k], cm[i][1][nxt[i]], rtol=1e-12, atol=1e-15), k
            nxt[i] += 1


def test_refusals(gpu_pkg):
    """Every refusal of pdmp_ensemble_set_target_diffusion_bridge and of set_state under it, by status and the word in the message; the
    path-integral family answers UNSUPPORTED naming the target."""
    pkg = gpu_pkg
    Lb = pkg._lib
    L, T = 3, 2.0
    d = (2 << L) + 1
    x0, th0, c = pkg.problems.diffusion_bridge_problem(L, T, 1.5, -0.5, nchains=2, rng=np.random.default_rng(5))
    seeds = np.array([3, 4], dtype=np.uint64)
    tgt = pkg.DiffusionBridgeTarget(L, T)

    def refused(fn, code, word):
        with pytest.raises(Lb.PdmpError) as ei:
            fn()
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    def fresh(F=None, sampler=Lb.SAMPLER_ZIGZAG_LOCAL, dd=d, **kw):
        e = pkg.Ensemble(2, dd, sampler=sampler, trace_capacity=64, **kw)
        e.set_flow(flow(pkg, dd) if F is None else F)
        return e

    inf, nan = float("inf"), float("nan")
    with fresh() as e:  # the arguments
        refused(lambda: e.set_target(pkg.DiffusionBridgeTarget(L + 1, T)), Lb.PDMP_ERR_INVALID, "(2 << L) + 1")
        refused(lambda: e.set_target(pkg.DiffusionBridgeTarget(-1, T)), Lb.PDMP_ERR_INVALID, "L = -1")
        refused(lambda: e.set_target(pkg.DiffusionBridgeTarget(L, 0.0)), Lb.PDMP_ERR_INVALID, "T = 0")
        refused(lambda: e.set_target(pkg.DiffusionBridgeTarget(L, -1.0)), Lb.PDMP_ERR_INVALID, "T = -1")
        refused(lambda: e.set_target(pkg.DiffusionBridgeTarget(L, inf)), Lb.PDMP_ERR_INVALID, "finite")
        for bad in (dict(α=nan), dict(β=inf), dict(ω=-inf)):
            refused(lambda: e.set_target(pkg.DiffusionBridgeTarget(L, T, **bad)), Lb.PDMP_ERR_INVALID, "finite")
        e.set_target(tgt)
        th_bad = th0.copy()
        th_bad[1, d - 1] = 1.0
        refused(lambda: e.set_state(0.0, x0, th_bad, c, seeds), Lb.PDMP_ERR_UNSUPPORTED, "end points")
        th_bad = th0.copy()
        th_bad[0, 0] = -1.0
        refused(lambda: e.set_state(0.0, x0, th_bad, c, seeds), Lb.PDMP_ERR_UNSUPPORTED, "end points")
        refused(lambda: e.set_state_synthetic(0.0, c, 1), Lb.PDMP_ERR_UNSUPPORTED, "explicit state")
        e.set_state(0.0, x0, th0, c, seeds)
        refused(lambda: e.set_target(tgt), Lb.PDMP_ERR_INVALID, "state exists")  # a state already exists
        e.run(1.0, Lb.RUN_STOP_BEFORE)
        assert e.kernel_name() == "zz_bridge_run_kernel"
        refused(lambda: e.path_integrals(1.0, np.arange(d)), Lb.PDMP_ERR_UNSUPPORTED, "diffusion-bridge")
        refused(lambda: e.batch_means(0.0, 1.0), Lb.PDMP_ERR_UNSUPPORTED, "diffusion-bridge")
        refused(lambda: e.ess_begin(1.0), Lb.PDMP_ERR_UNSUPPORTED, "diffusion-bridge")
    with fresh() as e:  # the later target call wins
        e.set_target(tgt)
        e.set_target(pkg.GaussianTarget(sp.identity(d, format="csc"), None))
        e.set_state(0.0, x0, th0, np.ones(d), seeds)
        e.run(1.0)
        assert e.kernel_name() != "zz_bridge_run_kernel"
    for sampler in (Lb.SAMPLER_ZIGZAG_ALL, Lb.SAMPLER_STICKY_ZIGZAG, Lb.SAMPLER_BARRIER_ZIGZAG):  # another sampler
        with fresh(sampler=sampler) as e:
            refused(lambda: e.set_target(tgt), Lb.PDMP_ERR_INVALID, "PDMP_SAMPLER_ZIGZAG_LOCAL")
    with pkg.Ensemble(2, d, sampler=Lb.SAMPLER_BPS, trace_capacity=64) as e:
        refused(lambda: e.set_target(tgt), Lb.PDMP_ERR_INVALID, "PDMP_SAMPLER_ZIGZAG_LOCAL")
    L11 = 11
    with pkg.Ensemble(1, (2 << L11) + 1, trace_capacity=64) as e:  # beyond the largest shipped level
        e.set_flow(flow(pkg, (2 << L11) + 1))
        refused(lambda: e.set_target(pkg.DiffusionBridgeTarget(L11, T)), Lb.PDMP_ERR_UNSUPPORTED, "L = 11")

    def state_refused(e, word):
        e.set_target(tgt)
        refused(lambda: e.set_state(0.0, x0, th0, c, seeds), Lb.PDMP_ERR_UNSUPPORTED, word)

    tri = sp.diags([np.full(d - 1, 0.1), np.ones(d), np.full(d - 1, 0.1)], [-1, 0, 1], format="csc")
    with fresh(F=pkg.ZigZag(tri, np.zeros(d))) as e:
        state_refused(e, "identity")
    with fresh(F=pkg.ZigZag(2.0 * sp.identity(d, format="csc"), np.zeros(d))) as e:
        state_refused(e, "identity")
    mu = np.zeros(d)
    mu[4] = 0.5
    with fresh(F=pkg.ZigZag(sp.identity(d, format="csc"), mu)) as e:
        state_refused(e, "μ")
    with fresh(F=pkg.ZigZag(sp.identity(d, format="csc"), np.zeros(d), λref=0.5)) as e:
        state_refused(e, "refresh")
    with fresh(F=pkg.FactBoomerang(sp.identity(d, format="csc"), np.zeros(d), 0.5)) as e:
        state_refused(e, "FactBoomerang")
    with fresh() as e:
        e.set_neighbourhood(tri)
        state_refused(e, "set_neighbourhood")
    with fresh() as e:
        e.set_gradient_tracking(True)
        state_refused(e, "gradient tracking")
    with fresh() as e:
        e.set_local_bound(True)
        state_refused(e, "LocalBound")
    with fresh(F=pkg.ZigZag(sp.identity(d, format="csc"), np.zeros(d), λref=0.5)) as e:  # (adaptscale needs a refresh clock to be switched on at all)
        e.set_adaptscale(True)
        state_refused(e, "adaptscale")
