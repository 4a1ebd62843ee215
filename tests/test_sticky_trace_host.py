"""trace.discretize / trace.inclusion_prob on the traces of the sticky Bouncy Particle / Boomerang (PDMPTrace with f0, f), against a direct
per-segment evaluation; traces without f behave as before."""
import numpy as np
import pytest
import scipy.sparse as sp

import sticky_ref_lib as R


def make(pkg, kind):
    d = 5
    rng = np.random.default_rng(9 + kind)
    x0, th0 = rng.standard_normal(d), rng.standard_normal(d)
    mu = np.array([0.4, 0.0, -0.3, 0.0, 0.2])
    r = R.sspdmp_notfact(0.0, x0, th0, 40.0, 2.0 if kind else 0.5, 1.5, flow_kind=kind, gamma=sp.identity(d, format="csc"), mu=mu if kind else np.zeros(d),
                         lambda_ref=0.8, mu_flow=mu if kind else None, seed=4)
    I = sp.identity(d, format="csc")
    F = pkg.Boomerang(I, mu, 0.8) if kind else pkg.BouncyParticle(I, np.zeros(d), 0.8)
    tr = pkg.PDMPTrace(F, 0.0, x0.copy(), th0.copy(), r["t"], r["x"], r["theta"], f0=np.ones(d, dtype=bool), f=r["f"])
    return tr, mu


@pytest.mark.parametrize("kind", [0, 1])
def test_discretize_holds_frozen_coordinates_still(pkg, kind):
    """src/trace.jl:129-150 with smove_forward!(…, f, …): every grid point flows from the latest event, free coordinates only."""
    tr, mu = make(pkg, kind)
    dt = 0.37
    ts, xs = pkg.trace.discretize(tr, dt)
    assert (~tr.f).any()
    te = np.concatenate([[tr.t0], tr.t])
    X = np.vstack([tr.x0[None], tr.x])
    TH = np.vstack([tr.θ0[None], tr.θ])
    Fm = np.vstack([tr.f0[None], tr.f])
    assert len(ts) == len(xs) and ts[0] == tr.t0 and np.all(ts < tr.t[-1]) and ts[-1] + dt >= tr.t[-1] - 1e-9
    frozen_seen = 0
    for g, row in zip(ts, xs):
        k = np.searchsorted(te, g, side="right") - 1
        tau = g - te[k]
        for i in range(len(tr.x0)):
            if not Fm[k, i]:
                want = X[k, i]
                frozen_seen += 1
                assert want == 0
            elif kind:
                want = (X[k, i] - mu[i]) * np.cos(tau) + TH[k, i] * np.sin(tau) + mu[i]
            else:
                want = X[k, i] + TH[k, i] * tau
            assert row[i] == pytest.approx(want, rel=0, abs=1e-12)
    assert frozen_seen > 10


@pytest.mark.parametrize("kind", [0, 1])
def test_inclusion_prob_is_the_free_fraction(pkg, kind):
    tr, _ = make(pkg, kind)
    p = pkg.trace.inclusion_prob(tr)
    te = np.concatenate([[tr.t0], tr.t])
    Fm = np.vstack([tr.f0[None], tr.f])
    want = np.zeros(len(tr.x0))
    for k in range(len(te) - 1):
        want += Fm[k] * (te[k + 1] - te[k])
    want /= te[-1] - tr.t0
    assert np.allclose(p, want, rtol=0, atol=1e-12) and np.all(p > 0.3) and np.all(p < 1)


def test_traces_without_f_are_untouched(pkg):
    tr, _ = make(pkg, 1)
    plain = pkg.PDMPTrace(tr.F, tr.t0, tr.x0, tr.θ0, tr.t, tr.x, tr.θ)
    assert plain.f is None and plain.f0 is None
    ts, xs = pkg.trace.discretize(plain, 0.37)
    ts2, xs2 = pkg.trace.discretize(tr, 0.37)
    assert np.array_equal(ts, ts2) and not np.array_equal(xs, xs2)  # (μ ≠ 0: an unmasked rotation moves the frozen coordinates)
    with pytest.raises(TypeError):
        pkg.trace.inclusion_prob(plain)
