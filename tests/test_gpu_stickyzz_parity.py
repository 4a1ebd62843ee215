"""The ZigZag with sticky and reflecting barriers (stickyzz, src/stickyzz.jl) on gfx950 -- zz_barrier_run_kernel, csrc/pdmp_barrier.hip -- against
its CPU restatement (tests/ref/stickyzz_ref.c), bit for bit, through the public samplers and the C ABI (-m gpu)."""
import numpy as np
import pytest
import scipy.sparse as sp

import oracle_lib as O
import stickyzz_cases as K
import stickyzz_ref_lib as R

pytestmark = pytest.mark.gpu
INF = float("inf")


def run_pair(pkg, G, Gt, x0, th0, c, barriers, T, seed, *, mu_t=None, mu_b=None, t0=0.0, strong=False, adapt=False, **kw):
    """The device run of every chain and the restatement's, compared bit for bit: events (t, i, x, θ), final (t, x, θ), (acc, num), returned c,
    t′, frozen flags, saved speeds.  mu_b: the flow's mean (default 0), t0: the start time.  Returns (device output, list of the restatement's runs)."""
    d = G.shape[0]
    bl = barriers if isinstance(barriers, list) else [barriers] * d
    out = pkg.stickyzz(pkg.GaussianTarget(Gt, mu_t), t0, x0, th0, T, c, pkg.ZigZag(G, np.zeros(d) if mu_b is None else mu_b), K.barriers_for(pkg, bl, d), seed=seed,
                       strong_upperbounds=strong, adapt=adapt, details=True, **kw)
    tr, tp, (t, x, th), (acc, num), det = out
    refs = []
    for k in range(x0.shape[0]):
        r = R.stickyzz(t0, x0[k], th0[k], T, c, bl, gamma=G, mu=mu_b, target_gamma=Gt, target_mu=mu_t, strong_upperbounds=strong, adapt=adapt, seed=seed + k)
        refs.append(r)
        assert r["status"] == R.REF_OK
        ev = tr[k].events
        assert len(ev) == r["nevents"] == len(r["t"]), (k, len(ev), r["nevents"])
        for f in ("i", "t", "x", "theta"):
            assert np.array_equal(ev[f], r[f]), (k, f, int(np.argmax(ev[f] != r[f])))
        assert (int(acc[k]), int(num[k])) == (r["nacc"], r["num"])
        assert tp[k] == r["t_final"]
        assert np.array_equal(t[k], r["t_state"]) and np.array_equal(x[k], r["x_final"]) and np.array_equal(th[k], r["theta_final"])
        assert np.array_equal(det["c"][k], r["c_final"])
        assert np.array_equal(det["frozen"][k], r["frozen"]) and np.array_equal(det["θ_saved"][k], r["theta_saved"])
    return out, refs


def problem8(nchains=3):
    G = K.precision8()
    x0, th0 = K.state8(nchains)
    return G, x0, th0, K.c8(G)


@pytest.mark.parametrize("barrier", [K.BOX_1D, K.STICKY_1D], ids=["reflecting_box", "sticky_at_0"])
def test_1d(gpu_pkg, barrier):
    """Both d = 1 cases of tests/test_stickyzz_ref.py at T = 200 (κ = Inf walls: the thaw key equals t′ and the same coordinate pops next)."""
    one, two = sp.csc_matrix(np.array([[1.0]])), sp.csc_matrix(np.array([[2.0]]))
    x0, th0 = np.array([[1.0], [0.3], [1.0]]), np.array([[0.8], [-1.0], [-0.8]])
    _, refs = run_pair(gpu_pkg, one, two, x0, th0, np.array([20.0]), barrier, 200.0, 1, mu_t=np.array([0.9]))
    assert all(r["nhit"] > 5 and r["nthaw"] > 5 for r in refs)


D8_SETS = {
    "sticky_at_0": ((0.0, 0.0), ("sticky", "sticky"), (0.5, 0.5)),
    "reflect_box": ((-1.0, 0.5), ("reflect", "reflect"), (100.0, 100.0)),  # test/sticky_test.jl:85
    "walls": ((-1.0, 0.5), ("reflect", "reflect"), (INF, INF)),
}


@pytest.mark.parametrize("name", ["sticky_at_0", "reflect_box", "walls", "mixed"])
def test_d8(gpu_pkg, name):
    """problems.maintest_precision(8), flow 0.9Γ, c = 0.7 column norms, T = 200: four barrier sets."""
    G, x0, th0, c = problem8()
    bar = K.mixed_barriers(8) if name == "mixed" else [D8_SETS[name]] * 8
    x0 = K.fit_state(x0, bar) if name != "sticky_at_0" else x0
    _, refs = run_pair(gpu_pkg, 0.9 * G, G, x0, th0, c, bar, 200.0, 7)
    assert all(r["nhit"] > 20 and r["nthaw"] > 20 and r["nrefl"] > 20 for r in refs)


def test_d8_flow_mean_and_start_time(gpu_pkg):
    """The mixed set through the public sampler with a flow mean that is not the target's (which has none) and t0 = 1.5: the `gx − gmu` of the
    setup and of the re-bound, and the t0 of the first hit, reflection and thaw keys.  adapt: the bound is centred elsewhere than the target."""
    G, x0, th0, c = problem8()
    bar = K.mixed_barriers(8)
    mu_b = 0.4 * np.random.default_rng(31).standard_normal(8)
    _, refs = run_pair(gpu_pkg, 0.9 * G, G, K.fit_state(x0, bar), th0, c, bar, 101.5, 7, mu_b=mu_b, t0=1.5, adapt=True)
    assert all(r["nhit"] > 20 and r["nthaw"] > 20 and r["nrefl"] > 20 and r["t"][0] > 1.5 for r in refs)
    zero = R.stickyzz(1.5, K.fit_state(x0, bar)[0], th0[0], 101.5, c, bar, gamma=0.9 * G, target_gamma=G, adapt=True, seed=7)
    assert not np.array_equal(zero["t"][:50], refs[0]["t"][:50])  # (the mean is not a no-op in this case)


def test_d8_strong_upperbounds(gpu_pkg):
    G, x0, th0, c = problem8()
    bar = K.mixed_barriers(8)
    _, refs = run_pair(gpu_pkg, 0.9 * G, G, K.fit_state(x0, bar), th0, c, bar, 200.0, 9, strong=True)
    assert all(r["nhit"] > 20 for r in refs)


def test_d8_adapt_and_bound_violation(gpu_pkg):
    """A c small enough that the restatement itself adapts at least once (asserted on its side, so the branch is known to run); the same c
    without adapt raises the bound error, and the chain status is BOUND_VIOLATED as in the restatement."""
    pkg = gpu_pkg
    G, x0, th0, c = problem8()
    bar = K.mixed_barriers(8)
    x0 = K.fit_state(x0, bar)
    c_small = 0.02 * c
    _, refs = run_pair(pkg, 0.9 * G, G, x0, th0, c_small, bar, 200.0, 13, adapt=True)
    assert all(r["nadapt"] >= 1 for r in refs) and all(np.any(r["c_final"] > c_small) for r in refs)
    tgt, Z, bl = pkg.GaussianTarget(G, None), pkg.ZigZag(0.9 * G, np.zeros(8)), K.barriers_for(pkg, bar, 8)
    with pytest.raises(RuntimeError, match="too small"):
        pkg.stickyzz(tgt, 0.0, x0, th0, 200.0, c_small, Z, bl, seed=13)
    tab = R.barrier_table(bar, 8)
    with pkg.Ensemble(x0.shape[0], 8, sampler=pkg._lib.SAMPLER_BARRIER_ZIGZAG, factor=1.5, trace_capacity=4096) as ens:
        ens.set_flow(Z)
        ens.set_target(tgt)
        ens.set_barriers(tab[0], tab[1], tab[2], tab[3], tab[4], tab[5])
        ens.set_state(0.0, x0, th0, c_small, np.uint64(13) + np.arange(x0.shape[0], dtype=np.uint64))
        ens.run(200.0)
        cnt = ens.counters()
    for k in range(x0.shape[0]):
        r = R.stickyzz(0.0, x0[k], th0[k], 200.0, c_small, bar, gamma=0.9 * G, target_gamma=G, seed=13 + k)
        assert r["status"] == R.REF_BOUND_VIOLATED and cnt["status"][k] == pkg._lib.CHAIN_BOUND_VIOLATED
        assert (int(cnt["nacc"][k]), int(cnt["num"][k]), int(cnt["nevents"][k]), int(cnt["ndraw_main"][k])) == (r["nacc"], r["num"], r["nevents"], r["ndraw_main"])


def test_d8_start_frozen(gpu_pkg):
    """x0[i] exactly on the barrier of its direction of travel for three coordinates, two of them neighbours: they start frozen, and the
    setup's bounds see θ = 0 at the earlier ones (src/stickyzz.jl:198-208)."""
    G, x0, th0, c = problem8()
    bar = [((-1.0, 0.5), ("sticky", "reflect"), (0.7, 2.0))] * 8
    x0 = K.fit_state(x0, bar)
    cols = sp.csc_matrix(G)
    i = next(i for i in range(8) if cols.indptr[i + 1] - cols.indptr[i] > 1)
    j = next(int(r) for r in cols.indices[cols.indptr[i]:cols.indptr[i + 1]] if r != i)
    k = next(q for q in range(8) if q not in (i, j))
    for q in (i, j, k):
        x0[:, q] = np.where(th0[:, q] > 0, 0.5, -1.0)
    (_, _, _, _, _), refs = run_pair(gpu_pkg, 0.9 * G, G, x0, th0, c, bar, 100.0, 17)
    for r in refs:  # the first event of each of the three is its thaw
        for q in (i, j, k):
            first = np.nonzero(r["i"] == q)[0][0]
            assert r["kind"][first] == R.EV_THAW


def test_d144_three_key_blocks(gpu_pkg):
    """problems.gmrf_precision(12): d = 144, three key blocks -- the level-1 queue crosses blocks.  Mixed barriers, κ drawn from (0.3, 1.3)."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(12)
    rng = np.random.default_rng(5)
    bar = K.mixed_barriers(144, rng)
    x0 = K.fit_state(0.5 * rng.standard_normal((2, 144)), bar)
    th0 = rng.choice([-1.0, 1.0], size=(2, 144))
    _, refs = run_pair(pkg, G, G, x0, th0, pkg.problems.column_norms(G), bar, 25.0, 21)
    assert all(r["nhit"] > 50 and r["nthaw"] > 50 and len(set(r["i"] // 64)) == 3 for r in refs)


def test_across_launches(gpu_pkg, monkeypatch):
    """The d = 8 mixed case with a trace capacity of about 1/7 of its event count, and with PDMP_LAUNCH_COUNT_LIMIT set low: the bytes of the
    single-launch run."""
    pkg = gpu_pkg
    G, x0, th0, c = problem8(2)
    bar = K.mixed_barriers(8)
    x0 = K.fit_state(x0, bar)
    args = (pkg.GaussianTarget(G, None), 0.0, x0, th0, 200.0, c, pkg.ZigZag(0.9 * G, np.zeros(8)), K.barriers_for(pkg, bar, 8))
    one = pkg.stickyzz(*args, seed=7, details=True, trace_capacity=1 << 16)
    nev = min(len(tr.events) for tr in one[0])
    assert nev > 700

    def same(a, b):
        for k in range(2):
            assert a[0][k].events.tobytes() == b[0][k].events.tobytes()
        assert np.array_equal(a[1], b[1])
        assert all(np.array_equal(p, q) for p, q in zip(a[2], b[2])) and all(np.array_equal(p, q) for p, q in zip(a[3], b[3]))
        assert all(np.array_equal(a[4][f], b[4][f]) for f in a[4])

    same(one, pkg.stickyzz(*args, seed=7, details=True, trace_capacity=nev // 7))
    monkeypatch.setenv("PDMP_LAUNCH_COUNT_LIMIT", "300")
    same(one, pkg.stickyzz(*args, seed=7, details=True, trace_capacity=1 << 16))


def test_refusals(gpu_pkg):
    """Every PDMP_ERR_INVALID / PDMP_ERR_UNSUPPORTED condition of include/pdmp_mi355.h returns its code; an sspdmp ensemble refuses set_barriers,
    a barrier ensemble refuses set_sticky and pdmp_ensemble_consume_begin."""
    pkg = gpu_pkg
    L = pkg._lib
    G, x0, th0, c = problem8(1)
    d = 8
    Z, tgt = pkg.ZigZag(0.9 * G, np.zeros(d)), pkg.GaussianTarget(G, None)
    good = R.barrier_table(((-1.0, 0.5), ("reflect", "sticky"), (2.0, INF)), d)
    seeds = np.array([3], dtype=np.uint64)

    def code(fn):
        with pytest.raises(L.PdmpError) as ei:
            fn()
        return ei.value.code

    def fresh(flow=Z, target=tgt, sampler=L.SAMPLER_BARRIER_ZIGZAG, **kw):
        e = pkg.Ensemble(1, d, sampler=sampler, factor=1.5, trace_capacity=256, **kw)
        e.set_flow(flow)
        if target is not None:
            e.set_target(target)
        return e

    def with_table(**change):
        tab = dict(zip(("lo", "hi", "rlo", "rhi", "klo", "khi"), (a.copy() for a in good)))
        for f, (idx, v) in change.items():
            tab[f][idx] = v
        return tab["lo"], tab["hi"], tab["rlo"], tab["rhi"], tab["klo"], tab["khi"]

    with fresh() as e:  # the table itself
        assert code(lambda: e.set_barriers(*with_table(lo=(2, 0.7)))) == L.PDMP_ERR_INVALID  # lo > hi
        assert code(lambda: e.set_barriers(*with_table(klo=(1, 0.0)))) == L.PDMP_ERR_INVALID
        assert code(lambda: e.set_barriers(*with_table(khi=(1, -1.0)))) == L.PDMP_ERR_INVALID
        assert code(lambda: e.set_barriers(*with_table(khi=(1, float("nan"))))) == L.PDMP_ERR_INVALID
        assert code(lambda: e.set_barriers(*with_table(rlo=(0, 3)))) == L.PDMP_ERR_INVALID
        assert code(lambda: e.set_barriers(*with_table(rhi=(0, -1)))) == L.PDMP_ERR_INVALID
        assert code(lambda: e.set_state(0.0, x0, th0, c, seeds)) == L.PDMP_ERR_INVALID  # no barriers set
        e.set_barriers(*good)
        xin = K.fit_state(x0, [((-1.0, 0.5),)] * d)
        th_bad = th0.copy()
        th_bad[0, 4] = 0.0
        assert code(lambda: e.set_state(0.0, xin, th_bad, c, seeds)) == L.PDMP_ERR_INVALID  # θ0[i] == 0
        x_bad = xin.copy()
        x_bad[0, 2] = 0.6
        assert code(lambda: e.set_state(0.0, x_bad, th0, c, seeds)) == L.PDMP_ERR_INVALID  # x0 outside [lo, hi]
        assert code(lambda: e.set_sticky(np.ones(d))) == L.PDMP_ERR_INVALID
        e.set_state(0.0, xin, th0, c, seeds)
        assert code(lambda: e.consume_begin()) == L.PDMP_ERR_UNSUPPORTED
        e.run(1.0)  # (the state that was accepted runs)
        assert e.kernel_name() == "zz_barrier_run_kernel"
    nodiag = sp.csc_matrix(0.9 * G).tolil()
    nodiag[3, 3] = 0.0
    nodiag = sp.csc_matrix(nodiag)
    nodiag.eliminate_zeros()
    Znd = pkg.ZigZag.__new__(pkg.ZigZag)
    Znd.Γ, Znd.μ, Znd.σ, Znd.λref, Znd.ρ = nodiag, np.zeros(d), np.ones(d), 0.0, 0.0
    e = pkg.Ensemble(1, d, sampler=L.SAMPLER_BARRIER_ZIGZAG, factor=1.5, trace_capacity=256)
    with e:
        assert code(lambda: e.set_flow(Znd)) == L.PDMP_ERR_INVALID  # a flow Γ without a diagonal entry
    xin = K.fit_state(x0, [((-1.0, 0.5),)] * d)

    def unsupported(e):
        e.set_barriers(*good)
        return code(lambda: e.set_state(0.0, xin, th0, c, seeds))

    with fresh(flow=pkg.ZigZag(0.9 * G, np.zeros(d), λref=0.5)) as e:  # a refresh clock
        assert unsupported(e) == L.PDMP_ERR_UNSUPPORTED
    with fresh() as e:  # G ≠ G1
        e.set_neighbourhood(sp.csc_matrix(np.ones((d, d))))
        e.set_target(tgt)
        assert unsupported(e) == L.PDMP_ERR_UNSUPPORTED
    with fresh() as e:
        e.set_gradient_tracking(True)
        assert unsupported(e) == L.PDMP_ERR_UNSUPPORTED
    with fresh() as e:
        e.set_local_bound(True)
        assert unsupported(e) == L.PDMP_ERR_UNSUPPORTED
    with fresh() as e:  # adaptscale is a keyword of spdmp: the setter itself refuses every other sampler, so set_state never sees it
        assert code(lambda: e.set_adaptscale(True)) == L.PDMP_ERR_UNSUPPORTED
    rng = np.random.default_rng(1)
    logistic = pkg.LogisticTarget(sp.csc_matrix(rng.standard_normal((20, d))), rng.integers(0, 2, 20), np.ones(20), np.zeros(d), 0.01, 2)
    with fresh(target=logistic) as e:  # the logistic target
        assert unsupported(e) == L.PDMP_ERR_UNSUPPORTED
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BARRIER_ZIGZAG, factor=1.5, trace_capacity=64) as e:  # a FactBoomerang flow
        assert code(lambda: e.set_flow(pkg.FactBoomerang(0.9 * G, np.zeros(d), 0.5))) == L.PDMP_ERR_UNSUPPORTED
    # a neighbourhood beyond 64 members: the general kernel's, which stickyzz does not run on
    dd = 70
    dense = sp.csc_matrix(np.eye(dd) * 3.0 + np.ones((dd, dd)) * 0.01)
    with pkg.Ensemble(1, dd, sampler=L.SAMPLER_BARRIER_ZIGZAG, factor=1.5, trace_capacity=64) as e:
        e.set_flow(pkg.ZigZag(dense, np.zeros(dd)))
        e.set_target(pkg.GaussianTarget(dense, None))
        e.set_barriers(*R.barrier_table(K.NO_BARRIER, dd))
        assert code(lambda: e.set_state(0.0, np.zeros((1, dd)), np.ones((1, dd)), np.ones(dd), seeds)) == L.PDMP_ERR_UNSUPPORTED
    with fresh(sampler=L.SAMPLER_STICKY_ZIGZAG) as e:  # an sspdmp ensemble still refuses set_barriers
        assert code(lambda: e.set_barriers(*good)) == L.PDMP_ERR_INVALID


def test_device_poisson_time3_L_equals_the_oracle(gpu_pkg_parity):
    """poisson_time3_L and the other scalars of the barrier kernel as compiled inside pdmp_barrier.hip (pdmp_debug_barrier_eval, parity build):
    bit for bit the oracle's orc_poisson_time3 on the branch grid, and the restatement's hitting time."""
    L = gpu_pkg_parity._lib
    a, b, u = K.poisson_time3_grid()
    dev = L.barrier_eval(L.BARRIER_FN_PT3_L, a, b, u)[0]
    assert np.array_equal(dev, np.array([O.poisson_time3(p, q, 0.01, s) for p, q, s in zip(a, b, u)]))
    assert np.array_equal(dev, R.poisson_time3(a, b, 0.01, u))
    x = np.array([0.5, 0.5, 0.25, 0.25, 2.0, 0.3, 0.3, -0.0, 0.0])
    v = np.array([1.0, -1.0, 0.5, -0.5, 1.0, 1.0, -1.0, 1.0, -0.5])
    bar = np.array([0.5, 0.5, 1.5, -1.0, 1.5, INF, -INF, 0.0, 0.0])
    assert np.array_equal(L.barrier_eval(L.BARRIER_FN_HIT, x, v, bar)[0], R.hitting_time(x, v, bar))
    g = np.array([-1.5, 0.0, -0.0, 2.5, 1.0])
    out = L.barrier_eval(L.BARRIER_FN_RATES, g, np.array([1.0, -3.0, 0.5, -0.25, 0.0]), np.array([0.5, 1.0, -0.5, 0.25, -0.0]))
    assert np.array_equal(out[0], np.maximum(g, 0.0)) and np.array_equal(out[1], np.array([1.5, 0.0, 0.0, 0.0, 0.0]))


def test_default_library_has_no_barrier_probe(gpu_pkg):
    L = gpu_pkg._lib
    with pytest.raises(L.PdmpError) as ei:
        L.barrier_eval(L.BARRIER_FN_PT3_L, np.array([1.0]), np.array([1.0]), np.array([0.5]))
    assert ei.value.code == L.PDMP_ERR_UNSUPPORTED


def test_host_consumers_on_the_returned_trace(gpu_pkg):
    """trace.discretize and trace.mean on a returned Ξ agree with the same functions on the restatement's events."""
    pkg = gpu_pkg
    G, x0, th0, c = problem8(2)
    bar = K.mixed_barriers(8)
    x0 = K.fit_state(x0, bar)
    (tr, _, _, _, _), refs = run_pair(pkg, 0.9 * G, G, x0, th0, c, bar, 100.0, 7)
    for k, r in enumerate(refs):
        ev = np.zeros(len(r["t"]), dtype=pkg._lib.EVENT_DTYPE)
        ev["t"], ev["i"], ev["x"], ev["theta"] = r["t"], r["i"], r["x"], r["theta"]
        mine = pkg.FactTrace(tr[k].F, 0.0, x0[k].copy(), th0[k].copy(), ev)
        ga, xa = pkg.trace.discretize(tr[k], 0.5)
        gb, xb = pkg.trace.discretize(mine, 0.5)
        assert np.array_equal(ga, gb) and np.array_equal(xa, xb) and len(ga) > 150
        assert np.array_equal(pkg.trace.mean(tr[k]), pkg.trace.mean(mine))
        # A :reflect barrier holds the path on its side.  A :sticky one lets the thawed coordinate through (hitting_time's ">=", src/stickyzz.jl:122)
        # and a :reversible one does whenever its coin keeps the sign, so neither bounds the path.
        lo = np.array([b[0][0] if b[1][0] == "reflect" else -INF for b in bar])
        hi = np.array([b[0][1] if b[1][1] == "reflect" else INF for b in bar])
        assert np.all(xa >= lo - 1e-12) and np.all(xa <= hi + 1e-12)
        assert np.any(xa < np.array([b[0][0] for b in bar])) or np.any(xa > np.array([b[0][1] for b in bar]))  # (and :sticky ones are passed)


def test_sspdmp2_and_one_barrier_for_all_coordinates(gpu_pkg):
    """sspdmp2(target, t0, x0, θ0, T, c, None, Z, κ) (src/stickyzz.jl:323-339) is stickyzz with barriers (0, 0), :sticky, (κ[i], κ[i]); one
    StickyBarriers passed to stickyzz stands for all coordinates."""
    pkg = gpu_pkg
    G, x0, th0, c = problem8(2)
    tgt, Z = pkg.GaussianTarget(G, None), pkg.ZigZag(0.9 * G, np.zeros(8))
    kap = np.linspace(0.4, 1.8, 8)
    tr2, (acc2, num2) = pkg.sspdmp2(tgt, 0.0, x0, th0, 100.0, c, None, Z, kap, seed=7)
    bl = [pkg.StickyBarriers((0.0, 0.0), ("sticky", "sticky"), (k, k)) for k in kap]
    tr, _, _, (acc, num) = pkg.stickyzz(tgt, 0.0, x0, th0, 100.0, c, Z, bl, seed=7)
    for k in range(2):
        assert tr2[k].events.tobytes() == tr[k].events.tobytes() and len(tr[k].events) > 300 and np.any(tr[k].events["theta"] == 0)
    assert np.array_equal(acc2, acc) and np.array_equal(num2, num)
    with pytest.raises(TypeError):
        pkg.sspdmp2(tgt, 0.0, x0, th0, 100.0, c, G, Z, kap)
    one = pkg.StickyBarriers((-1.0, 0.5), ("sticky", "reflect"), (0.7, INF))
    xin = K.fit_state(x0, [((-1.0, 0.5),)] * 8)
    a = pkg.stickyzz(tgt, 0.0, xin[0], th0[0], 100.0, c, Z, one, seed=3, details=True)
    b = pkg.stickyzz(tgt, 0.0, xin[0], th0[0], 100.0, c, Z, [one] * 8, seed=3, details=True)
    r = R.stickyzz(0.0, xin[0], th0[0], 100.0, c, (one.x, one.rule, one.κ), gamma=0.9 * G, target_gamma=G, seed=3)
    assert a[0].events.tobytes() == b[0].events.tobytes() and a[1] == b[1] == r["t_final"] and a[3] == b[3] == (r["nacc"], r["num"])
    assert np.array_equal(a[0].events["t"], r["t"]) and np.array_equal(a[0].events["x"], r["x"]) and np.array_equal(a[4]["frozen"], r["frozen"])


def test_path_integrals_count_the_time_spent_frozen_at_a_level(gpu_pkg):
    """pdmp_ensemble_path_integrals of a barrier ensemble against the exact integral of the returned trace (tests/exact_path.py, the derived
    bound 3 (m + 1) u X L of tests/test_gpu_path_integrals.py with m = num + nevents + 1): mixed barriers with sticky levels away from 0 and
    finite κ, slice by slice with a refilled trace buffer; then a coordinate that starts frozen on its barrier.  A frozen coordinate's clock
    stands still; its stretch at the barrier LEVEL enters the integral when it thaws (and through the read while it is still frozen).
    The path of a frozen start begins with slope 0, not θ0: the exact path is given that (a trace records (t0, x0, θ0) as the reference's does)."""
    from fractions import Fraction as Fr

    import exact_path as E
    import test_gpu_path_integrals as P

    pkg = gpu_pkg
    L = pkg._lib
    G, x0, th0, c = problem8(3)
    bar = K.mixed_barriers(8)
    x0 = K.fit_state(x0, bar)
    tab = R.barrier_table(bar, 8)

    def setup(ens):  # (run_case offers one hook, before the flow is set: the barriers go in with its set_path_integrals call, after flow and target)
        plain = ens.set_path_integrals

        def with_barriers(enable=True):
            ens.set_barriers(*tab)
            plain(enable)
        ens.set_path_integrals = with_barriers

    _, cnt, paths = P.run_case(pkg, "stickyzz-mixed-d8", G=0.9 * G, Gt=G, nch=3, slices=(20.0, 40.0, 60.0), cap=100, expect="zz_barrier_run_kernel",
                               c=c, sampler=L.SAMPLER_BARRIER_ZIGZAG, factor=1.5, x0=x0, th0=th0, seed=5, min_events=500, setup=setup)
    assert all(p.own[4] > 10 for p in paths)  # (coordinate 4 sticks at −1 and at 0.5)

    x0[:, 4] = np.where(th0[:, 4] > 0, 0.5, -1.0)  # starts frozen at a level that is not 0 (κ = 3.0 / 0.4)
    T = 30.0
    with pkg.Ensemble(3, 8, sampler=L.SAMPLER_BARRIER_ZIGZAG, factor=1.5, trace_capacity=4096) as ens:
        ens.set_flow(pkg.ZigZag(0.9 * G, np.zeros(8)))
        ens.set_target(pkg.GaussianTarget(G, None))
        ens.set_barriers(*tab)
        ens.set_state(0.0, x0, th0, c, np.uint64(50) + np.arange(3, dtype=np.uint64))
        ens.run(T, L.RUN_STOP_BEFORE)
        cnt = ens.counters()
        assert np.all(cnt["status"] == L.CHAIN_OK)
        J = ens.path_integrals(T, np.arange(8))
        for k in range(3):
            ev = ens.trace(k, counters=cnt)
            first = ev[ev["i"] == 4][0]
            assert first["x"] == x0[k, 4] and first["theta"] != 0 and first["t"] > 0  # its first event is its thaw, after a while at the level
            th_eff = th0[k].copy()
            th_eff[4] = 0.0
            p = E.ExactPath(0.0, x0[k], th_eff)
            p.feed(ev)
            want, X, Ln = p.J(T), p.absmax(T), p.length(T)
            m = int(cnt["num"][k]) + int(cnt["nevents"][k]) + 1
            for i in range(8):
                assert abs(Fr(float(J[k, i])) - want[i]) <= E.bound_J(m, X[i], Ln[i]), (k, i, float(J[k, i]), float(want[i]))
