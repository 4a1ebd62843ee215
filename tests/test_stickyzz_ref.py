"""The CPU restatement of stickyzz (tests/ref/stickyzz_ref.c, src/stickyzz.jl): its three-parameter poisson_time against the oracle's and the
integral identity, and the process itself -- no barrier, a reflecting box, sticking at 0, the thaw rules.  No GPU: the device kernel is held
to this restatement bit for bit by tests/test_gpu_stickyzz_parity.py."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.stats

import oracle_lib as O
import stickyzz_cases as K
import stickyzz_ref_lib as R

INF = float("inf")


def test_poisson_time3_equals_the_oracle_and_inverts_the_integrated_rate():
    """poisson_time((a, b, c), u), src/poissontime.jl:39-65, c = 0.01: bit for bit orc_poisson_time3 on a grid that takes every branch, and
    every value τ satisfies ∫₀^τ (c + (a + b s)⁺) ds = −log u to 1e-10 relative."""
    a, b, u = K.poisson_time3_grid()
    c = 0.01
    mine = R.poisson_time3(a, b, c, u)
    theirs = np.array([O.poisson_time3(p, q, c, s) for p, q, s in zip(a, b, u)])
    assert np.array_equal(mine, theirs)
    assert set(K.poisson_time3_branch(p, q, c, s) for p, q, s in zip(a, b, u)) == set(K.POISSON_TIME3_BRANCHES)
    for p, q, s, tau in zip(a, b, u, mine):
        assert tau > 0 and math.isfinite(tau)
        want = -math.log(s)
        got = K.integrated_rate(p, q, c, tau)
        assert abs(got - want) <= 1e-10 * want, (p, q, s, tau, got, want)


def test_hitting_time_keeps_the_reference_sic():
    """hitting_time, :119-127: Inf when v (x − barrier) >= 0 -- also ON the barrier --, else −(x − barrier)/v; infinite barriers are never hit."""
    assert R.hitting_time(0.5, 1.0, 0.5)[0] == INF and R.hitting_time(0.5, -1.0, 0.5)[0] == INF
    assert R.hitting_time(0.25, 0.5, 1.5)[0] == 2.5 and R.hitting_time(0.25, -0.5, -1.0)[0] == 2.5
    assert R.hitting_time(2.0, 1.0, 1.5)[0] == INF  # past it, moving away
    assert R.hitting_time(0.3, 1.0, INF)[0] == INF and R.hitting_time(0.3, -1.0, -INF)[0] == INF


def test_without_barriers_every_event_is_an_accepted_reflection():
    """StickyBarriers() everywhere: no hit and no thaw, one event per accepted proposal."""
    G = K.precision8()
    x0, th0 = K.state8(1)
    r = R.stickyzz(0.0, x0[0], th0[0], 100.0, K.c8(G), K.NO_BARRIER, gamma=0.9 * G, target_gamma=G, seed=5)
    assert r["status"] == R.REF_OK and r["nhit"] == 0 and r["nthaw"] == 0
    assert r["nevents"] == r["nrefl"] == r["nacc"] > 100 and np.all(r["kind"] == R.EV_REFLECTION)
    assert not r["frozen"].any() and np.all(r["theta_final"] != 0)
    assert np.all(np.abs(r["theta"]) == np.abs(th0[0][r["i"]]))  # a reflection negates, nothing else touches a speed


def test_reflecting_box_1d_stays_inside_and_has_the_truncated_normal_mean():
    """d = 1, target N(0.9, 0.5), flow Γ = [1], c = 20, barriers (−0.2, 1.5), :reflect, κ = Inf, T = 2000.  Every x of the trace lies in [lo, hi];
    the time average of x against scipy's truncnorm mean within 4 standard errors of the run's own 32 batch means (false-alarm rate 6e-5; the
    seed is fixed).  Observed: mean 0.75044 against 0.74813, standard error 0.00555 (0.42 standard errors)."""
    T = 2000.0
    r = K.run_1d(K.BOX_1D, T, seed=1)
    assert r["status"] == R.REF_OK
    assert r["x"].min() >= -0.2 and r["x"].max() <= 1.5 and r["nhit"] > 100 and abs(r["nhit"] - r["nthaw"]) <= 1
    hit = r["kind"] == R.EV_HIT
    assert np.all(np.isin(r["x"][hit], [-0.2, 1.5])) and np.all(r["theta"][hit] == 0)
    assert np.array_equal(r["t"][1:][hit[:-1]], r["t"][:-1][hit[:-1]])  # κ = Inf: the thaw follows its hit at the same time
    bm = K.batch_means_1d(r, 1.0, 0.8, T, "x")
    mean, se = bm.mean(), bm.std(ddof=1) / math.sqrt(len(bm))
    s = math.sqrt(0.5)
    want = scipy.stats.truncnorm.mean((-0.2 - 0.9) / s, (1.5 - 0.9) / s, loc=0.9, scale=s)
    print("reflecting box: mean %.5f truncnorm %.5f se %.5f (%.2f se)" % (mean, want, se, (mean - want) / se))
    assert abs(mean - want) < 4 * se


def test_sticky_at_zero_1d_spends_the_closed_form_fraction_of_time_away_from_zero():
    """test/sticky.jl:7-36's parameters (σ² = 0.5, μ = 0.9, x0 = 1, θ0 = 0.8, flow Γ = [1], c = 20, T = 2000) with barriers (0, 0), :sticky,
    κ = 1.5: the fraction of time away from 0 against w = √(2π)σ / (√(2π)σ + exp(−μ²/2σ²)/κ) (:30), 4 standard errors of 32 batch means.
    Observed: 0.88424 against w = 0.85666, standard error 0.00730 (3.78 standard errors).  That formula is the weight at unit speed: a
    coordinate of speed |θ| meets 0 at the rate |θ| π(0), so the weight of this run (|θ| = 0.8) is √(2π)σ / (√(2π)σ + |θ| exp(−μ²/2σ²)/κ) =
    0.88194, from which the run is 0.32 standard errors away -- also asserted, at the same 4 standard errors."""
    T = 2000.0
    r = K.run_1d(K.STICKY_1D, T, seed=1)
    assert r["status"] == R.REF_OK and r["nhit"] > 100
    hit = r["kind"] == R.EV_HIT
    assert np.all(r["x"][hit] == 0) and np.all(r["theta"][hit] == 0)
    thaw = r["kind"] == R.EV_THAW
    assert np.all(np.abs(r["theta"][thaw]) == 0.8) and np.all(r["x"][thaw] == 0)
    bm = K.batch_means_1d(r, 1.0, 0.8, T, "moving")
    frac, se = bm.mean(), bm.std(ddof=1) / math.sqrt(len(bm))
    s, mu, kappa = math.sqrt(0.5), 0.9, 1.5
    w = math.sqrt(2 * math.pi) * s / (math.sqrt(2 * math.pi) * s + math.exp(-0.5 * mu ** 2 / s ** 2) / kappa)
    w_speed = math.sqrt(2 * math.pi) * s / (math.sqrt(2 * math.pi) * s + 0.8 * math.exp(-0.5 * mu ** 2 / s ** 2) / kappa)
    print("sticky at 0: fraction %.5f w %.5f (%.2f se) w at speed 0.8 %.5f (%.2f se) se %.5f" % (frac, w, (frac - w) / se, w_speed, (frac - w_speed) / se, se))
    assert abs(frac - w) < 4 * se
    assert abs(frac - w_speed) < 4 * se


@pytest.mark.parametrize("rule", ["reversible", "reflect", "sticky"])
def test_thaw_rules(rule):
    """After a :reversible thaw both signs occur over a run; after a :reflect thaw the speed is always the opposite of the saved one; a :sticky
    thaw keeps it."""
    G = K.precision8()
    x0, th0 = K.state8(1)
    bar = ((-0.6, 0.7), (rule, rule), (2.0, 2.0))
    r = R.stickyzz(0.0, np.clip(x0[0], -0.5, 0.5), th0[0], 300.0, K.c8(G), bar, gamma=0.9 * G, target_gamma=G, seed=11)
    assert r["status"] == R.REF_OK
    saved = {}
    ratios = []
    for k in range(len(r["t"])):
        i = int(r["i"][k])
        if r["kind"][k] == R.EV_HIT:
            saved[i] = K.speed_before(r, k, th0[0])
        elif r["kind"][k] == R.EV_THAW:
            ratios.append(r["theta"][k] / saved.pop(i))
    ratios = np.array(ratios)
    assert len(ratios) > 100 and np.all(np.abs(ratios) == 1.0)
    if rule == "reversible":
        assert 0.3 < np.mean(ratios < 0) < 0.7
    elif rule == "reflect":
        assert np.all(ratios == -1.0)
    else:
        assert np.all(ratios == 1.0)
