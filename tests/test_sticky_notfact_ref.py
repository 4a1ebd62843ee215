"""The sequential restatement of the reference's sticky Bouncy Particle / Boomerang (tests/ref/sticky_notfact_ref.c, src/ss_not_fact.jl) held to
the reference's own pins -- before the device loop is held to the restatement bit for bit (tests/test_gpu_sticky_bps_parity.py)."""
import numpy as np
import scipy.sparse as sp

import sticky_ref_lib as R
import sticky_stats as S


def reference_sticky_boomerang(pkg, seed):
    """@testset "Sticky Boomerang" (test/sticky.jl:67-92): Γ of the suite, μ = rand(d), x0 = rand(d), θ0 = rand([-1, -.5, .5, 1], d), κ = 1000,
    B = Boomerang(I, μ, 0.5, 0.95), c = 10, T = 1000."""
    d = 8
    G = pkg.problems.maintest_precision(d)
    rng = np.random.default_rng(seed)
    mu = rng.random(d)
    x0 = rng.random(d)
    th0 = rng.choice([-1.0, -0.5, 0.5, 1.0], d)
    return dict(d=d, G=G, mu=mu, x0=x0, th0=th0, kappa=1000.0, c=10.0, T=1000.0, dt=0.5, lambda_ref=0.5, rho=0.95)


def envelope_ok(pkg, P, tr):
    """mean(abs.(mean(xs) - μ)) < 2/sqrt(T) and mean(abs.(cov(xs) - inv(Matrix(Γ)))) < 2.5/sqrt(T), test/sticky.jl:87-91"""
    ts, xs = pkg.trace.discretize(tr, P["dt"])
    e1 = np.mean(np.abs(xs.mean(0) - P["mu"]))
    e2 = np.mean(np.abs(np.cov(xs.T) - np.linalg.inv(P["G"].toarray())))
    print("sticky Boomerang envelope: %.4f < %.4f, %.4f < %.4f" % (e1, 2 / np.sqrt(P["T"]), e2, 2.5 / np.sqrt(P["T"])))
    return bool(e1 < 2 / np.sqrt(P["T"]) and e2 < 2.5 / np.sqrt(P["T"]))


def ref_trace(pkg, P, seed):
    r = R.sspdmp_notfact(0.0, P["x0"], P["th0"], P["T"], P["c"], P["kappa"], flow_kind=1, gamma=P["G"], mu=P["mu"], lambda_ref=P["lambda_ref"],
                         rho=P["rho"], mu_flow=P["mu"], seed=seed, ev_cap=2000000)
    assert r["status"] == R.REF_OK and r["nevents"] == len(r["t"])
    B = pkg.Boomerang(sp.identity(P["d"], format="csc"), P["mu"], P["lambda_ref"], P["rho"])
    return pkg.PDMPTrace(B, 0.0, P["x0"].copy(), P["th0"].copy(), r["t"], r["x"], r["theta"], f0=np.ones(P["d"], dtype=bool), f=r["f"]), r


def test_reference_sticky_boomerang_envelope(pkg):
    """test/sticky.jl:67-92 as written, thresholds 2/√T and 2.5/√T, majority of three seeds (as tests/test_gpu_bps_parity.py does for the
    Bouncy Particle's envelope)."""
    ok = 0
    for seed in (1, 2, 3):
        P = reference_sticky_boomerang(pkg, seed)
        tr, _ = ref_trace(pkg, P, seed)
        ok += envelope_ok(pkg, P, tr)
    assert ok >= 2


def test_closed_form_free_probability():
    """Γ = I, μ = 0, κ_i = 1.5: P(x_i ≠ 0) = κ√(2π)/(1 + κ√(2π)) = 0.78991 for the BouncyParticle (λref = 1) and the Boomerang.
    64 chains, d = 4, T = 200, x0, θ0 ~ N(0, I); the estimate is the time each coordinate is free over [t0, T_last], averaged over the
    coordinates, and |mean over chains − exact| < 4 SE with the between-chain standard error.  Seeds are fixed: observed z = +0.66
    (BouncyParticle: mean 0.79166, SE 0.00262) and z = +1.33 (Boomerang: mean 0.79250, SE 0.00194).  (At d = 64 the Bouncy Particle needs
    a burn-in: over [0, 100] the same estimate sits 8 SE high, over [200, 400] with 256 chains z = +1.96 -- the device test's choice.)"""
    for flow in ("bps", "boomerang"):
        z, m, se = S.z_score(S.closed_form_ref(flow, 64, 4, 200.0, 0.0))
        print("closed form %s: mean %.5f exact %.5f SE %.5f z %+.2f" % (flow, m, S.p_free_exact(S.KAPPA), se, z))
        assert abs(z) < 4


def structural_checks(t0, x0, th0, ev_t, ev_x, ev_th, ev_f):
    """event times do not decrease; a frozen coordinate has x = ±0, θ = 0; f flips one coordinate at a time, only at a freeze / thaw of that
    coordinate (a freeze zeroes θ_i at x_i = 0, a thaw restores a non-zero θ_i there); the first event is (t0, x0, θ0, ones).
    The event (t, x, θ, f) does not carry θf (sevent, :100-102).  What it shows of θf is asserted at every event: a thaw sets θ_i = θf_i, so
    θ_i ≠ 0 after every thaw says that the speed saved over that frozen stretch was not 0; the stretches still frozen at the end are
    covered by the final θf (theta_f ≠ 0 where f_final is False), which the callers compare."""
    assert ev_t[0] == t0 and np.array_equal(ev_x[0], x0) and np.array_equal(ev_th[0], th0) and ev_f[0].all()
    assert np.all(np.diff(ev_t) >= 0)
    assert np.all(ev_x[~ev_f] == 0) and np.all(ev_th[~ev_f] == 0)
    flips = ev_f[1:] != ev_f[:-1]
    assert flips.sum(1).max() <= 1
    k, i = np.nonzero(flips)
    froze = ~ev_f[k + 1, i]
    assert np.all(ev_x[k + 1, i] == 0)                                      # both happen at 0
    assert np.all(ev_th[k + 1, i][froze] == 0) and np.all(ev_th[k, i][froze] != 0)
    assert np.all(ev_th[k + 1, i][~froze] != 0)
    return int(froze.sum()), int((~froze).sum())


def test_structure_of_the_trace():
    rng = np.random.default_rng(5)
    d = 7
    G = sp.identity(d, format="csc")
    for kind, c in ((0, 0.5), (1, 2.0)):
        for strong in (False, True):
            x0, th0 = rng.standard_normal(d), rng.standard_normal(d)
            mu_flow = np.array([0.0, 0.3, 0.0, -0.2, 0.0, 0.0, 0.1]) if kind == 1 else None
            r = R.sspdmp_notfact(0.0, x0, th0, 60.0, c, 1.5, flow_kind=kind, gamma=G, mu=np.zeros(d), lambda_ref=0.7, rho=0.3, mu_flow=mu_flow,
                                 strong_upperbounds=strong, seed=21)
            assert r["status"] == R.REF_OK
            nf, nt = structural_checks(0.0, x0, th0, r["t"], r["x"], r["theta"], r["f"])
            assert nf > 10 and nt > 10
            # the final state continues the last event: frozen coordinates carry a saved speed, free ones none
            assert np.all(r["theta_f"][~r["f_final"]] != 0) and np.all(r["theta_f"][r["f_final"]] == 0)
            assert np.array_equal(r["f_final"], r["f"][-1]) and r["t_final"] == r["t"][-1] and r["t_final"] >= 60.0
