"""Sticky Bouncy Particle / Boomerang on gfx950 (csrc/pdmp_bps_sticky.inc) vs the sequential restatement of src/ss_not_fact.jl
(tests/ref/sticky_notfact_ref.c), through the Python sspdmp and the C ABI (-m gpu): events (t, x, θ, f), counters, final state bit for bit."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import sticky_ref_lib as R
import sticky_stats as S
from test_sticky_notfact_ref import envelope_ok, reference_sticky_boomerang, structural_checks

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))  # (−0 and +0 differ: x[i] = -0*θ[i])


def problem(pkg, flow, d, seed, gamma="I", own_target=False, rho=0.0, lam=0.8):
    """flow "bps": BouncyParticle(Γ, μ, λ; ρ) on its own Γ(x − μ), or with a target of its own; "boom": Boomerang(I, μ_flow, λ; ρ) on a
    Gaussian target, μ_flow with zero and non-zero entries."""
    rng = np.random.default_rng(seed)
    if gamma == "I":
        G = sp.identity(d, format="csc")
    elif d == 8:
        G = pkg.problems.maintest_precision(8)
    else:
        G = sp.csc_matrix(sp.identity(d) * 1.5 + sp.diags([0.3 * np.ones(d - 1), 0.3 * np.ones(d - 1)], [-1, 1]))
    mu = np.where(np.arange(d) % 3 == 0, 0.0, 0.3 * rng.standard_normal(d))
    P = dict(flow=flow, d=d, G=G, lam=lam, rho=rho, target=None)
    if flow == "bps":
        P["mu"] = np.zeros(d) if gamma == "I" else mu
        P["F"] = pkg.BouncyParticle(G, P["mu"], lam, rho)
        if own_target:
            Gt = sp.csc_matrix(sp.identity(d) * 1.2 + sp.diags([0.2 * np.ones(d - 1), 0.2 * np.ones(d - 1)], [-1, 1])) if d > 1 else sp.identity(1, format="csc") * 1.2
            P["target"] = (sp.csc_matrix(Gt), 0.1 * rng.standard_normal(d))
    else:
        P["mu"] = 0.2 * rng.standard_normal(d)  # the target's mean
        P["mu_flow"] = mu
        P["F"] = pkg.Boomerang(sp.identity(d, format="csc"), mu, lam, rho)
    return P


def ref_run(P, x0, th0, T, c, kappa, seed, strong=False, adapt=False, factor=2.0, t0=0.0):
    """kappa: a scalar or one value per coordinate."""
    kw = dict(flow_kind=0 if P["flow"] == "bps" else 1, gamma=P["G"], mu=P["mu"], lambda_ref=P["lam"], rho=P["rho"], strong_upperbounds=strong,
              adapt=adapt, factor=factor, seed=seed, ev_cap=400000)
    if P["flow"] == "bps":
        kw["target"] = P["target"]
    else:
        kw["mu_flow"] = P["mu_flow"]
    return R.sspdmp_notfact(t0, x0, th0, T, c, kappa, **kw)


def dev_target(pkg, P):
    if P["flow"] == "boom":
        return pkg.GaussianTarget(P["G"], P["mu"])
    return None if P["target"] is None else pkg.GaussianTarget(P["target"][0], P["target"][1])


def check(pkg, P, T, c, kappa, nch=2, seed=5, strong=False, adapt=False, trace_capacity=None, t0=0.0, state=None, refs=None):
    """The Python sspdmp against the restatement: events (t, x, θ, f), (acc, num), final (t, x, θ, c).  Then the same chains on an ensemble
    of their own (check_counters_and_final): nrefresh, ndraw_main, nevents, final f and θf, which sspdmp does not return.
    kappa: a scalar or [d]; state: (x0, θ0), each [nch x d], instead of the seeded draw; refs: the restatement's runs where the caller has them."""
    d = P["d"]
    rng = np.random.default_rng(seed)
    x0, th0 = (rng.standard_normal((nch, d)), rng.standard_normal((nch, d))) if state is None else state
    nch = x0.shape[0]
    tr, (t, x, th), (acc, num), cout = pkg.sspdmp(dev_target(pkg, P), t0, x0, th0, T, c, P["F"], kappa, strong_upperbounds=strong, adapt=adapt,
                                                  seed=seed, trace_capacity=trace_capacity)
    nfz = 0
    given, refs = refs, []
    for k in range(nch):
        r = ref_run(P, x0[k], th0[k], T, c, kappa, seed + k, strong=strong, adapt=adapt, t0=t0) if given is None else given[k]
        refs.append(r)
        assert r["status"] == R.REF_OK and r["nevents"] == len(r["t"])
        assert len(tr[k].t) == r["nevents"], (k, len(tr[k].t), r["nevents"])
        assert same(tr[k].t, r["t"]) and same(tr[k].x, r["x"]) and same(tr[k].θ, r["theta"]) and np.array_equal(tr[k].f, r["f"])
        assert tr[k].f0.all()
        assert (int(acc[k]), int(num[k])) == (r["nacc"], r["num"])
        assert t[k] == r["t_final"] and same(x[k], r["x_final"]) and same(th[k], r["theta_final"]) and cout[k] == r["c_final"]
        nfz += int((~r["f"]).any(1).sum())
    check_counters_and_final(pkg, P, T, c, kappa, x0, th0, seed, strong, adapt, refs, t0=t0)
    return tr, nfz


def check_counters_and_final(pkg, P, T, c, kappa, x0, th0, seed, strong, adapt, refs, t0=0.0):
    """The chains of check() once more on an Ensemble (seeds seed + k as sspdmp gives them): every counter the restatement keeps, the final
    state, the final free mask and the saved speeds θf, bit for bit; a frozen coordinate carries θf ≠ 0 and a free one θf = 0."""
    L = pkg._lib
    nch, d = x0.shape
    with raw_ensemble(pkg, P, nch, 4096, adapt=adapt) as ens:
        ens.set_bps_sticky(kappa, strong)
        ens.set_state_bps(t0, x0, th0, c, np.uint64(seed) + np.arange(nch, dtype=np.uint64))
        for _ in range(100000):
            ens.run(T, L.RUN_REFERENCE_TAIL)
            cnt = ens.counters()
            assert not np.any(cnt["status"] == L.CHAIN_BOUND_VIOLATED)
            ens.trace_reset()
            if not L.needs_rerun(cnt["status"]):
                break
        cnt = ens.counters()
        fs = ens.bps_final_state()
        fin = ens.bps_final_sticky()
    for k, r in enumerate(refs):
        assert cnt["status"][k] == L.CHAIN_OK
        for name, key in (("num", "num"), ("nacc", "nacc"), ("nrefresh", "nrefresh"), ("ndraw_main", "ndraw_main"), ("nevents", "nevents")):
            assert int(cnt[name][k]) == r[key], (k, name, int(cnt[name][k]), r[key])
        assert fs["t"][k] == r["t_final"] and fs["c"][k] == r["c_final"] and same(fs["x"][k], r["x_final"]) and same(fs["theta"][k], r["theta_final"])
        assert np.array_equal(fin["f"][k], r["f_final"]) and same(fin["theta_f"][k], r["theta_f"])
        assert np.all(fin["theta_f"][k][~fin["f"][k]] != 0) and np.all(fin["theta_f"][k][fin["f"][k]] == 0)


@pytest.mark.parametrize("d", [1, 7, 64, 100, 129, 257, 1024])
@pytest.mark.parametrize("flow", ["bps", "boom"])
def test_identity_precision_every_width(gpu_pkg, flow, d):
    """Γ = I at 1, 2 and 16 slots per lane (partial last slot), and at 4 and 8 with wholly empty trailing slots (d = 129, 257); κ = 1.5 so that
    coordinates freeze and thaw all the time.  Every slot count with a Γ that couples slots: tests/test_gpu_bps_widths.py."""
    P = problem(gpu_pkg, flow, d, 100 + d, rho=0.0 if d % 2 else 0.95)
    T = 20.0 if d <= 100 else 3.0
    # (Γ = I makes the BouncyParticle's bound exact: no adaptation needed; the Boomerang's c adapts to |μ_flow − μ_target|)
    tr, nfz = check(gpu_pkg, P, T, 0.5 if flow == "bps" else 2.0, 1.5, seed=40 + d, adapt=flow == "boom")
    assert nfz > 5
    for q in tr:
        structural_checks(0.0, q.x0, q.θ0, q.t, q.x, q.θ, q.f)


@pytest.mark.parametrize("strong", [False, True])
@pytest.mark.parametrize("kappa", [1.5, 1000.0])
def test_sparse_precision_own_target_kappa_and_strong_upperbounds(gpu_pkg, kappa, strong):
    pkg = gpu_pkg
    check(pkg, problem(pkg, "bps", 8, 1, gamma="sparse", rho=0.95), 25.0, 6.0, kappa, seed=11, strong=strong, adapt=True)
    check(pkg, problem(pkg, "bps", 100, 2, gamma="sparse", own_target=True), 8.0, 20.0, kappa, seed=12, strong=strong, adapt=True)
    check(pkg, problem(pkg, "boom", 8, 3, gamma="sparse", rho=0.95), 25.0, 10.0, kappa, seed=13, strong=strong, adapt=True)
    check(pkg, problem(pkg, "boom", 100, 4, gamma="sparse"), 8.0, 30.0, kappa, seed=14, strong=strong, adapt=True)


def raw_ensemble(pkg, P, nch, cap, adapt=False, factor=2.0):
    ens = pkg.Ensemble(nch, P["d"], sampler=pkg._lib.SAMPLER_BPS, adapt=adapt, factor=factor, trace_capacity=cap)
    if P["flow"] == "boom":
        ens.set_flow_boomerang(dev_target(pkg, P), P["F"])
    else:
        ens.set_flow_bps(P["F"])
        if P["target"] is not None:
            ens.set_target(dev_target(pkg, P))
    return ens


def drain(pkg, ens, k, acc):
    cnt = ens.counters()
    n = int(cnt["ntrace"][k])
    d = ens.d
    t, x, th = np.empty(n), np.empty((n, d)), np.empty((n, d))
    f = np.empty((n, d), dtype=np.uint8)
    L = pkg._lib
    L.check(ens._L.pdmp_ensemble_bps_trace_copy(ens._h, k, 0, n, t.ctypes.data, x.ctypes.data, th.ctypes.data))
    L.check(ens._L.pdmp_ensemble_bps_trace_free_copy(ens._h, k, 0, n, f.ctypes.data))
    acc.append((t, x, th, f.astype(bool)))


def raw_final(pkg, ens):
    n, d = ens.nchains, ens.d
    f = np.empty((n, d), dtype=np.uint8)
    thf = np.empty((n, d))
    pkg._lib.check(ens._L.pdmp_ensemble_bps_final_sticky(ens._h, 0, n, f.ctypes.data, thf.ctypes.data))
    return f.astype(bool), thf


@pytest.mark.parametrize("flow", ["bps", "boom"])
def test_adapt_and_bound_violation_match_the_restatement(gpu_pkg, flow):
    """A c small enough to be violated: with adapt the chain multiplies it and goes on like the restatement (same c at the end); without, it
    ends as PDMP_CHAIN_BOUND_VIOLATED at the restatement's proposal (same num, nacc, draws, clock).  Through the raw C ABI, with the final f / θf."""
    pkg = gpu_pkg
    d = 8
    P = problem(pkg, flow, d, 7, gamma="sparse")
    if flow == "bps":  # a target three times as stiff as the flow's Γ: the bound c + θ'Γ(x − μ) + θ'Γθ·s is too small until c has grown
        P["target"] = (sp.csc_matrix(3.0 * P["G"]), P["mu"])
    c0 = 0.05 if flow == "bps" else 0.3
    rng = np.random.default_rng(3)
    x0, th0 = rng.standard_normal((2, d)), rng.standard_normal((2, d))
    seeds = np.array([91, 92], dtype=np.uint64)
    for adapt in (True, False):
        with raw_ensemble(pkg, P, 2, 200000, adapt=adapt) as ens:
            kap = np.full(d, 1.5)
            pkg._lib.check(ens._L.pdmp_ensemble_set_bps_sticky(ens._h, kap.ctypes.data, 0))
            ens.set_state_bps(0.0, x0, th0, c0, seeds)
            ens.run(30.0, pkg._lib.RUN_REFERENCE_TAIL)
            cnt = ens.counters()
            fs = ens.bps_final_state()
            f_fin, thf_fin = raw_final(pkg, ens)
            for k in range(2):
                r = ref_run(P, x0[k], th0[k], 30.0, c0, 1.5, int(seeds[k]), adapt=adapt)
                if adapt:
                    assert r["status"] == R.REF_OK and r["c_final"] > c0 and cnt["status"][k] == pkg._lib.CHAIN_OK
                else:
                    assert r["status"] == R.REF_BOUND_VIOLATED and cnt["status"][k] == pkg._lib.CHAIN_BOUND_VIOLATED
                ev = []
                drain(pkg, ens, k, ev)
                assert same(ev[0][0], r["t"]) and same(ev[0][1], r["x"]) and same(ev[0][2], r["theta"]) and np.array_equal(ev[0][3], r["f"])
                assert (int(cnt["num"][k]), int(cnt["nacc"][k]), int(cnt["nrefresh"][k]), int(cnt["ndraw_main"][k]), int(cnt["nevents"][k])) == \
                    (r["num"], r["nacc"], r["nrefresh"], r["ndraw_main"], r["nevents"])
                assert fs["t"][k] == r["t_final"] and fs["c"][k] == r["c_final"] and same(fs["x"][k], r["x_final"]) and same(fs["theta"][k], r["theta_final"])
                assert np.array_equal(f_fin[k], r["f_final"]) and same(thf_fin[k], r["theta_f"])


@pytest.mark.parametrize("flow", ["bps", "boom"])
def test_resumption_small_buffer_and_stop_before_slices(gpu_pkg, flow):
    """A trace buffer of 8 events drained again and again equals one large buffer; PDMP_RUN_STOP_BEFORE slices followed by the reference's
    tail equal one reference-tail run -- events, counters, draws, final state, f and θf."""
    pkg = gpu_pkg
    L = pkg._lib
    d = 100
    P = problem(pkg, flow, d, 17, gamma="sparse", rho=0.5)
    c0, T = (20.0, 6.0) if flow == "bps" else (30.0, 6.0)
    rng = np.random.default_rng(8)
    x0, th0 = rng.standard_normal((2, d)), rng.standard_normal((2, d))
    seeds = np.array([5, 6], dtype=np.uint64)
    kap = np.full(d, 1.5)

    def run(cap, slices):
        out = [[] for _ in range(2)]
        with raw_ensemble(pkg, P, 2, cap, adapt=True) as ens:
            L.check(ens._L.pdmp_ensemble_set_bps_sticky(ens._h, kap.ctypes.data, 0))
            ens.set_state_bps(0.0, x0, th0, c0, seeds)
            plan = [(s, L.RUN_STOP_BEFORE) for s in slices] + [(T, L.RUN_REFERENCE_TAIL)]
            for Ts, flags in plan:
                for _ in range(100000):
                    ens.run(Ts, flags)
                    cnt = ens.counters()
                    assert not np.any(cnt["status"] == L.CHAIN_BOUND_VIOLATED)
                    for k in range(2):
                        if cnt["ntrace"][k]:
                            drain(pkg, ens, k, out[k])
                    ens.trace_reset()
                    if not L.needs_rerun(cnt["status"]):
                        break
            cnt = ens.counters()
            fs = ens.bps_final_state()
            fin = raw_final(pkg, ens)
        ev = [tuple(np.concatenate([p[j] for p in out[k]]) for j in range(4)) for k in range(2)]
        return ev, cnt, fs, fin

    base = run(100000, [])
    for k in range(2):
        r = ref_run(P, x0[k], th0[k], T, c0, 1.5, int(seeds[k]), adapt=True)
        assert same(base[0][k][0], r["t"]) and same(base[0][k][1], r["x"]) and np.array_equal(base[0][k][3], r["f"])
        assert int(base[1]["ndraw_main"][k]) == r["ndraw_main"] and len(r["t"]) > 40
    for other in (run(8, []), run(100000, [1.0, 2.5, 2.5, 4.0])):
        for k in range(2):
            for j in range(3):
                assert same(other[0][k][j], base[0][k][j]), (k, j)
            assert np.array_equal(other[0][k][3], base[0][k][3])
        for name in ("num", "nacc", "nrefresh", "ndraw_main", "nevents", "status"):
            assert np.array_equal(other[1][name], base[1][name]), name
        for name in ("t", "c", "x", "theta"):
            assert same(other[2][name], base[2][name]), name
        assert np.array_equal(other[3][0], base[3][0]) and same(other[3][1], base[3][1])


def test_refusals(gpu_pkg):
    """Every refusal of include/pdmp_mi355.h's sticky section, by status and by the option the message names."""
    pkg = gpu_pkg
    L = pkg._lib
    d = 8
    G = pkg.problems.maintest_precision(d)
    I = sp.identity(d, format="csc")
    x0 = np.ones((1, d))
    seeds = np.array([1], dtype=np.uint64)
    kap = np.full(d, 1.5)
    B = pkg.BouncyParticle(I, np.zeros(d), 0.5)

    def refused(ens, code, word):
        with pytest.raises(L.PdmpError) as ei:
            ens.set_state_bps(0.0, x0, x0 * 0.5, 1.0, seeds)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, trace_capacity=64) as ens:
        with pytest.raises(L.PdmpError) as ei:  # before a flow
            ens.set_bps_sticky(kap)
        assert ei.value.code == L.PDMP_ERR_INVALID
        ens.set_flow_bps(B)
        for bad in (0.0, -1.0, np.inf, np.nan):
            k2 = kap.copy()
            k2[3] = bad
            with pytest.raises(L.PdmpError) as ei:
                ens.set_bps_sticky(k2)
            assert ei.value.code == L.PDMP_ERR_INVALID
        assert ens._L.pdmp_ensemble_set_bps_sticky(ens._h, None, 0) == L.PDMP_ERR_INVALID
        ens.set_bps_sticky(kap)
        ens.set_bps_options(local_bound=True)
        refused(ens, L.PDMP_ERR_UNSUPPORTED, "local_bound")
        ens.set_bps_options(subsample=True)
        refused(ens, L.PDMP_ERR_UNSUPPORTED, "subsample")
        ens.set_bps_options()
        ens.set_bps_moments(1)
        refused(ens, L.PDMP_ERR_UNSUPPORTED, "set_bps_moments")
        ens.set_bps_moments(0)
        ens.set_state_bps(0.0, x0, x0 * 0.5, 1.0, seeds)  # accepted
        with pytest.raises(L.PdmpError) as ei:  # a state exists
            ens.set_bps_sticky(kap)
        assert ei.value.code == L.PDMP_ERR_INVALID
        # set_flow_* clears the setting: a plain ensemble again (no sticky trace to read)
        ens.set_flow_bps(B)
        ens.set_state_bps(0.0, x0, x0 * 0.5, 1.0, seeds)
        f = np.empty((1, d), dtype=np.uint8)
        assert ens._L.pdmp_ensemble_bps_final_sticky(ens._h, 0, 1, f.ctypes.data, None) == L.PDMP_ERR_INVALID
        assert ens._L.pdmp_ensemble_bps_trace_free_copy(ens._h, 0, 0, 1, f.ctypes.data) == L.PDMP_ERR_INVALID
    # a sticky BouncyParticle with Γ ≠ I needs no mass factor (the loop never reads F.L) ...
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, trace_capacity=64) as ens:
        B2 = pkg.BouncyParticle(G, np.zeros(d), 0.5)
        B2.L = None
        ens.set_flow_bps(B2)
        ens.set_bps_sticky(kap)
        ens.set_state_bps(0.0, x0, x0 * 0.5, 5.0, seeds)
    # ... a sticky Boomerang takes the identity factor, handed over explicitly, and refuses a general one
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, trace_capacity=64) as ens:
        Bo = pkg.Boomerang(G, np.zeros(d), 0.5)  # L = cholesky(Γ).L
        ens.set_flow_boomerang(pkg.GaussianTarget(G, np.zeros(d)), Bo)
        ens.set_bps_sticky(kap)
        refused(ens, L.PDMP_ERR_UNSUPPORTED, "mass factor")
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_ZIGZAG_LOCAL, trace_capacity=64) as ens:  # wrong sampler
        assert ens._L.pdmp_ensemble_set_bps_sticky(ens._h, kap.ctypes.data, 0) == L.PDMP_ERR_INVALID
    with pkg.Ensemble(1, 1100, sampler=L.SAMPLER_BPS, trace_capacity=4) as ens:  # d > 1024: refused, never a fallback
        ens.set_flow_bps(pkg.BouncyParticle(sp.identity(1100, format="csc"), np.zeros(1100), 0.5))
        ens.set_bps_sticky(1.5)
        with pytest.raises(L.PdmpError) as ei:
            ens.set_state_bps(0.0, np.ones((1, 1100)), np.ones((1, 1100)), 1.0, seeds)
        assert ei.value.code == L.PDMP_ERR_UNSUPPORTED and "1024" in str(ei.value)
    with pytest.raises(TypeError):
        pkg.sspdmp(None, 0.0, x0[0], x0[0], 1.0, 1.0, B, kap, reversible=True)
    with pytest.raises(TypeError):
        pkg.sspdmp(None, 0.0, x0[0], x0[0], 1.0, 1.0, B, kap, G=I)


def test_plain_ensemble_after_a_sticky_one_is_unchanged(gpu_pkg):
    import oracle_lib as O
    pkg = gpu_pkg
    d = 64
    I = sp.identity(d, format="csc")
    rng = np.random.default_rng(2)
    x0, th0 = rng.standard_normal((2, d)), rng.standard_normal((2, d))
    B = pkg.BouncyParticle(I, np.zeros(d), 1.0)
    pkg.sspdmp(None, 0.0, x0, th0, 5.0, 0.5, B, 1.5, seed=3)
    tr, (t, x, th), (acc, num), cout = pkg.pdmp(None, 0.0, x0, th0, 10.0, 1e-3, B, seed=3)
    for k in range(2):
        r = O.pdmp_bps(I, None, x0[k], th0[k], 1e-3, 10.0, lambda_ref=1.0, seed=3 + k, ev_cap=200000)
        assert np.array_equal(tr[k].t, r["t_ev"]) and np.array_equal(tr[k].x, r["x_ev"]) and np.array_equal(tr[k].θ, r["theta_ev"])
        assert (int(acc[k]), int(num[k])) == (r["nacc"], r["num"]) and np.array_equal(x[k], r["x"])


def test_device_scalars_equal_the_host_values(gpu_pkg):
    """pdmp_debug_sticky_eval: pdmp_atan and both freezing times as compiled inside pdmp_bps.hip, bit for bit the host's."""
    from test_detmath_atan import atan_table
    pkg = gpu_pkg
    x = atan_table()
    x = np.concatenate([x, -x, [np.inf, -np.inf, np.nan]])

    def dev(fn, a, b, c):
        a, b, c = (np.ascontiguousarray(v, dtype=np.float64) for v in (a, b, c))
        out = np.empty(len(a))
        pkg._lib.check(pkg._lib.load().pdmp_debug_sticky_eval(0, fn, len(a), a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data))
        return out

    z = np.zeros(len(x))
    assert np.array_equal(bits(dev(0, x, z, z)), bits(R.ref_atan(x)))
    rng = np.random.default_rng(4)
    n = 4000
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    m = np.where(rng.random(n) < 0.3, 0.0, 0.5 * rng.standard_normal(n))
    a[::7] = 0.0
    a[3::11] = -0.0
    b[5::13] = 0.0
    # x = 0 with θ = 0 is atan(0/0): a NaN on both sides, whose sign and payload are outside the contract (include/pdmp_debug.h: x86-64 and
    # gfx950 produce different default NaNs).  Those points are taken out of the table and checked on their own below; everything else,
    # ±Inf included, is compared on its bits.
    both0 = (a == 0) & (b == 0)
    assert both0.sum() > 10
    a0, b0, m0 = a[both0], b[both0], m[both0]
    a, b, m = a[~both0], b[~both0], m[~both0]
    assert ((a == 0) & (b != 0)).sum() > 100 and ((b == 0) & (a != 0)).sum() > 100 and (m == 0).sum() > 500
    for fn, want in ((1, R.freezing_time_linear(a, b)), (2, R.freezing_time_boomerang(a, b, m))):
        got = dev(fn, a, b, m)
        assert not np.isnan(want).any()
        bad = np.nonzero(bits(got) != bits(want))[0]
        assert bad.size == 0, (fn, [(a[k], b[k], m[k], got[k], want[k]) for k in bad[:8]])
    # 0/0: the Boomerang's freezing time is a NaN on the host and on the device wherever it is one on either (μ = 0: atan(0/0))
    got0, want0 = dev(2, a0, b0, m0), R.freezing_time_boomerang(a0, b0, m0)
    assert np.array_equal(np.isnan(got0), np.isnan(want0)) and np.isnan(want0).any()
    assert np.array_equal(bits(got0[~np.isnan(got0)]), bits(want0[~np.isnan(want0)]))
    assert np.array_equal(bits(dev(1, a0, b0, m0)), bits(R.freezing_time_linear(a0, b0)))  # (θx >= 0: +Inf, no division)


def test_reference_envelope_on_the_device(gpu_pkg):
    """@testset "Sticky Boomerang" (test/sticky.jl:67-92) as ONE sspdmp call of three chains (seeds 1, 2, 3 on the problem of seed 1, each with
    its own x0, θ0): the reference's thresholds, majority of three."""
    pkg = gpu_pkg
    P = reference_sticky_boomerang(pkg, 1)
    rng = np.random.default_rng(1)
    x0 = rng.random((3, P["d"]))
    th0 = rng.choice([-1.0, -0.5, 0.5, 1.0], (3, P["d"]))
    B = pkg.Boomerang(sp.identity(P["d"], format="csc"), P["mu"], P["lambda_ref"], P["rho"])
    tr, _, _, _ = pkg.sspdmp(pkg.GaussianTarget(P["G"], P["mu"]), 0.0, x0, th0, P["T"], P["c"], B, P["kappa"], seed=1)
    assert sum(envelope_ok(pkg, P, q) for q in tr) >= 2


@pytest.mark.parametrize("flow", ["bps", "boomerang"])
def test_closed_form_at_ensemble_width(gpu_pkg, flow):
    """P(x_i ≠ 0) = κ√(2π)/(1 + κ√(2π)) with 256 chains, d = 64, as ONE sspdmp call: T = 400, the free fraction over [200, T_last] (the Bouncy
    Particle's slow relaxation at d = 64 is burnt in, tests/test_sticky_notfact_ref.py), |mean − exact| < 4 SE between chains.  The
    restatement gives z = +1.96 (BouncyParticle) and z = +1.90 (Boomerang) on these seeds, and the device equals it bit for bit."""
    pkg = gpu_pkg
    nch, d, T, burn = 256, 64, 400.0, 200.0
    kind, c = S.CLOSED_FORM[flow]
    x0, th0 = S.closed_form_state(nch, d)
    I = sp.identity(d, format="csc")
    F = pkg.Boomerang(I, np.zeros(d), S.LAMBDA_REF) if kind else pkg.BouncyParticle(I, np.zeros(d), S.LAMBDA_REF)
    tr, _, _, _ = pkg.sspdmp(pkg.GaussianTarget(I, np.zeros(d)) if kind else None, 0.0, x0, th0, T, c, F, S.KAPPA, seed=S.SEED)
    fr = np.array([S.free_fraction(q.t, q.f, burn).mean() for q in tr])
    z, m, se = S.z_score(fr)
    print("closed form on the device, %s: mean %.5f exact %.5f SE %.5f z %+.2f" % (flow, m, S.p_free_exact(S.KAPPA), se, z))
    assert abs(z) < 4
    p = np.array([pkg.trace.inclusion_prob(q) for q in tr[:4]])
    assert np.all(p > 0.5) and np.all(p < 1)
