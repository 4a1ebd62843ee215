"""Path moments of BouncyParticle / Boomerang on the host: trace.path_moments against quadrature, and the C ABI of the device moments
(pdmp_ensemble_set_bps_moments / pdmp_ensemble_bps_moments) declared and bound.  No GPU needed."""
import os
import re

import numpy as np
import scipy.sparse as sp

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flow(tr, x, th, s):
    """(x, θ) a time s after (x, θ) along the trace's free flow."""
    if type(tr.F).__name__ == "Boomerang":
        m = tr.F.μ
        return (x - m) * np.cos(s) + th * np.sin(s) + m, -(x - m) * np.sin(s) + th * np.cos(s)
    return x + th * s, th


def _simpson(tr, T, n=400):
    """(∫x, ∫x²) over [t0, T] by composite Simpson on every segment (the path is smooth between events)."""
    d = len(tr.x0)
    te = np.concatenate([[tr.t0], tr.t])
    X = np.vstack([tr.x0[None], np.asarray(tr.x).reshape(-1, d)])
    TH = np.vstack([tr.θ0[None], np.asarray(tr.θ).reshape(-1, d)])
    w = np.ones(n + 1)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    s1, s2 = np.zeros(d), np.zeros(d)
    for k in range(len(te)):
        a = te[k]
        b = min(te[k + 1], T) if k + 1 < len(te) else T
        if not b > a:
            continue
        s = np.linspace(0.0, b - a, n + 1)[:, None]
        xs, _ = _flow(tr, X[k][None], TH[k][None], s)
        h = (b - a) / n
        s1 += h / 3 * (w[:, None] * xs).sum(0)
        s2 += h / 3 * (w[:, None] * xs * xs).sum(0)
    return s1, s2


def _random_trace(pkg, boom, d, nev, rng, mu_f=None, t0=0.0):
    """A synthetic trace: free flow between events, a new θ at every event (what a reflection or a refreshment leaves)."""
    I = sp.identity(d, format="csc")
    F = pkg.Boomerang(I, np.zeros(d) if mu_f is None else mu_f, 1.0) if boom else pkg.BouncyParticle(I, np.zeros(d), 1.0)
    x0, th0 = rng.standard_normal(d), rng.standard_normal(d)
    t = t0 + np.cumsum(rng.exponential(0.7, nev))
    xs, ths = np.empty((nev, d)), np.empty((nev, d))
    x, th, tl = x0.copy(), th0.copy(), t0
    for k in range(nev):
        probe = pkg.PDMPTrace(F, 0.0, x, th)
        x, _ = _flow(probe, x, th, t[k] - tl)
        th = rng.standard_normal(d)
        xs[k], ths[k], tl = x, th, t[k]
    return pkg.PDMPTrace(F, t0, x0, th0, t, xs, ths)


def _close(got, ref, rtol=1e-9):
    for g, r in zip(got, ref):
        assert np.allclose(g, r, rtol=rtol, atol=rtol * np.abs(r).sum() / len(r)), np.max(np.abs(g - r))


def test_path_moments_bouncy_particle_against_quadrature(pkg):
    rng = np.random.default_rng(1)
    tr = _random_trace(pkg, False, 5, 30, rng, t0=0.5)
    for T in (tr.t[-1], tr.t[-1] + 0.37, tr.t[12] + 0.1):  # at the last event, inside the open last segment, events after T cut off
        _close(pkg.trace.path_moments(tr, T), _simpson(tr, T))


def test_path_moments_boomerang_against_quadrature(pkg):
    rng = np.random.default_rng(2)
    for mu_f in (None, rng.standard_normal(4) * 3):  # rotation about 0 and about μ_f ≠ 0
        tr = _random_trace(pkg, True, 4, 25, rng, mu_f=mu_f)
        for T in (tr.t[-1] + 0.8, tr.t[7] + 0.05):
            _close(pkg.trace.path_moments(tr, T), _simpson(tr, T))


def test_path_moments_of_an_empty_trace(pkg):
    rng = np.random.default_rng(3)
    d = 3
    x0, th0 = rng.standard_normal(d), rng.standard_normal(d)
    tr = pkg.PDMPTrace(pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0), 1.0, x0, th0)
    j1, j2 = pkg.trace.path_moments(tr, 3.0)
    assert np.allclose(j1, 2.0 * x0 + 2.0 * th0, rtol=1e-14)  # ∫_0^2 (x0 + θ0 s) ds
    assert np.allclose(j2, 2.0 * x0 ** 2 + 4.0 * x0 * th0 + 8.0 / 3.0 * th0 ** 2, rtol=1e-14)
    mu = rng.standard_normal(d)
    trb = pkg.PDMPTrace(pkg.Boomerang(sp.identity(d, format="csc"), mu, 1.0), 0.0, x0, th0)
    _close(pkg.trace.path_moments(trb, 2.5), _simpson(trb, 2.5))
    z1, z2 = pkg.trace.path_moments(tr, 1.0)
    assert not z1.any() and not z2.any()


def test_path_moments_of_an_oracle_trace(pkg):
    """A trace of the oracle's pdmp_bps (BouncyParticle on a general Γ, and Boomerang): positions are continuous along the free flow
    (so path_moments' model of the path is the process'), and the closed forms agree with quadrature."""
    G = pkg.problems.maintest_precision(8)
    d = G.shape[0]
    rng = np.random.default_rng(4)
    x0, th0 = rng.standard_normal(d), rng.standard_normal(d)
    r = O.pdmp_bps(G, None, x0, th0, 1.1, 60.0, lambda_ref=0.5, seed=8, ev_cap=20000)
    B = pkg.BouncyParticle(G, np.zeros(d), 0.5)
    muf = rng.standard_normal(d)
    rb = O.pdmp_bps(sp.identity(d, format="csc"), muf, x0, th0, 3.0, 60.0, lambda_ref=0.5, seed=9, ev_cap=20000, boomerang_mu=muf)
    Bb = pkg.Boomerang(sp.identity(d, format="csc"), muf, 0.5)
    for F, res in ((B, r), (Bb, rb)):
        assert res["status"] == 0 and len(res["t_ev"]) > 10
        tr = pkg.PDMPTrace(F, 0.0, x0, th0, res["t_ev"], res["x_ev"], res["theta_ev"])
        te = np.concatenate([[0.0], tr.t])
        X = np.vstack([x0[None], tr.x])
        TH = np.vstack([th0[None], tr.θ])
        xe, _ = _flow(tr, X[:-1], TH[:-1], np.diff(te)[:, None])
        assert np.allclose(xe, X[1:], rtol=1e-9, atol=1e-9)
        T = 0.5 * (tr.t[-2] + tr.t[-1])
        _close(pkg.trace.path_moments(tr, T), _simpson(tr, T))


def test_moment_calls_declared_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdmp_mi355.h")).read(), flags=re.S)
    for name in ("pdmp_ensemble_set_bps_moments", "pdmp_ensemble_bps_moments"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in pkg._lib.EXPORTED_SYMBOLS
    import inspect
    body = inspect.getsource(pkg._lib)
    assert "L.pdmp_ensemble_set_bps_moments.argtypes = [vp, C.c_int]" in body
    assert "L.pdmp_ensemble_bps_moments.argtypes = [vp, f64, i64, i64, vp, vp]" in body
    assert callable(pkg.Ensemble.set_bps_moments) and callable(pkg.Ensemble.bps_moments)
