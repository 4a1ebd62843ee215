"""trace.conditional_trace (the host mirror of the device's conditional-trace consumers) on oracle-made chains (CPU only).

1. It equals the sequential statement of the contract (tests/ref/condition_ref.c: ref_condition_fact / ref_condition_pdmp) bit for bit.
2. The contract against src/condition.jl written line by line (the *_literal pair): the reference recomputes τ from the point it just put on the
   plane and so may emit one crossing again inside the same event segment; with those repeats dropped (a literal hit found before the same
   event as its predecessor) the two lists have the same length, NO hit is excluded, and times and rows agree within
       δt = 4 (K + d) 2⁻⁵² ‖n‖₁ (max|x| + max|p|) / |h|        δx = δt max|θ| + K 2⁻⁵² max|x|
   (K events: the reference accumulates one rounding per move of every coordinate; h = ⟨θ, n⟩ of the hit's piece).  The seeds below are the
   first ones tried: none had to be replaced for a hit within δt of a corner.
3. Every row lies on the plane: |⟨row − p, n⟩| stays within the same bound, read both ways: the number δt itself, and δt carried into the
   residual's units, |h| δt = 4 (K + d) 2⁻⁵² ‖n‖₁ (max|x| + max|p|).  The smaller of the two is asserted.
Every case asserts at least 10 hits."""
import numpy as np
import pytest
import scipy.sparse as sp

import condition_ref_lib as CR
import oracle_lib as O
import sticky_ref_lib as R

U = 2.0 ** -52


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def tridiag(d):
    return sp.csc_matrix(sp.identity(d) * 1.5 + sp.diags([0.3 * np.ones(d - 1), 0.3 * np.ones(d - 1)], [-1, 1]))


_chains = {}


def chain(pkg, name):
    """One oracle-made trace per name, made once"""
    if name in _chains:
        return _chains[name]
    P = pkg.problems
    rng = np.random.default_rng(11)
    if name == "gmrf":  # spdmp on the 8 x 8 grid-Laplace GMRF, started in stationarity
        G = P.gmrf_precision(8)
        x0, th0 = P.gmrf_stationary_sample(8, 1, rng)[0], rng.choice([-1.0, 1.0], 64)
        r = O.spdmp_zigzag(G, None, G, x0, th0, 2.0 * P.column_norms(G), 50.0, seed=31)
        assert r["status"] == 0
        tr = pkg.FactTrace(pkg.ZigZag(G, np.zeros(64)), 0.0, x0, th0, r["events"])
    elif name == "zz70":
        G = tridiag(70)
        x0, th0 = 0.5 * rng.standard_normal(70), rng.choice([-1.0, 1.0], 70)
        r = O.spdmp_zigzag(G, None, G, x0, th0, 2.0 * P.column_norms(G), 40.0, seed=32)
        assert r["status"] == 0
        tr = pkg.FactTrace(pkg.ZigZag(G, np.zeros(70)), 0.0, x0, th0, r["events"])
    elif name == "stickyzz":
        G = P.maintest_precision(8)
        x0, th0 = rng.random(8), rng.choice([-1.0, 1.0], 8)
        r = O.sspdmp_zigzag(G, None, G, x0, th0, 2.0 * P.column_norms(G), np.full(8, 0.8), 200.0, seed=33)
        assert r["status"] == 0
        tr = pkg.FactTrace(pkg.ZigZag(G, np.zeros(8)), 0.0, x0, th0, r["events"])
    elif name in ("bps16", "bps70"):
        d = int(name[3:])
        G = sp.identity(d, format="csc")
        x0, th0 = rng.standard_normal(d), rng.standard_normal(d)
        r = O.pdmp_bps(G, None, x0, th0, 1e-3, 150.0, lambda_ref=1.0, seed=34, ev_cap=100000)
        tr = pkg.PDMPTrace(pkg.BouncyParticle(G, np.zeros(d), 1.0), 0.0, x0, th0, r["t_ev"], r["x_ev"], r["theta_ev"])
    elif name == "sbps8":
        G = P.maintest_precision(8)
        x0, th0 = rng.standard_normal(8), rng.standard_normal(8)
        r = R.sspdmp_notfact(0.0, x0, th0, 150.0, 10.0, 1.0, flow_kind=0, gamma=G, mu=None, lambda_ref=1.0, seed=35)
        assert r["status"] == 0
        tr = pkg.PDMPTrace(pkg.BouncyParticle(G, np.zeros(8), 1.0), 0.0, x0, th0, r["t"], r["x"], r["theta"])
        tr.f0, tr.f = np.ones(8, dtype=bool), r["f"]
        assert not tr.f.all()  # coordinates do freeze
    _chains[name] = tr
    return tr


def plane(d, kind):
    """(p, n) of the four kinds of normal the issue names; p near the targets' mean, so that stationary paths cross often"""
    rng = np.random.default_rng(5)
    n = np.zeros(d)
    if kind == "e_i":
        n[3 % d] = 1.0
    elif kind == "e_i-e_j":
        n[3 % d], n[12 % d] = 1.0, -1.0
    elif kind == "block65":
        n[3:68] = rng.standard_normal(65)
    else:
        n[:] = rng.standard_normal(d)
    return 0.05 * rng.standard_normal(d), n


CASES = [(c, k) for c in ("gmrf", "stickyzz", "bps16", "sbps8") for k in ("e_i", "e_i-e_j", "dense")] + [("zz70", "block65"), ("bps70", "block65")]


@pytest.mark.parametrize("name,kind", CASES)
def test_conditional_trace_equals_the_contract_bit_for_bit(pkg, name, kind):
    tr = chain(pkg, name)
    p, n = plane(len(tr.x0), kind)
    ref = CR.of_trace(tr, p, n)
    t, X = pkg.trace.conditional_trace(tr, p, n)
    assert ref["nhits"] == len(ref["t"]) >= 10
    assert same_bits(t, ref["t"]) and same_bits(X, ref["x"])
    assert np.all(np.diff(t) > 0)


def bounds(tr, p, n, h):
    d = len(tr.x0)
    if hasattr(tr, "events"):
        K, xs, ths = len(tr.events), np.concatenate([tr.x0, tr.events["x"]]), np.concatenate([tr.θ0, tr.events["theta"]])
    else:
        K, xs, ths = len(tr.t), np.concatenate([tr.x0, np.ravel(tr.x)]), np.concatenate([tr.θ0, np.ravel(tr.θ)])
    mx, mth = np.abs(xs).max(), np.abs(ths).max()
    dt = 4 * (K + d) * U * np.abs(n).sum() * (mx + np.abs(p).max()) / np.abs(h)
    return dt, dt * mth + K * U * mx


@pytest.mark.parametrize("name,kind", CASES)
def test_the_contract_against_the_reference_line_by_line(pkg, name, kind):
    tr = chain(pkg, name)
    p, n = plane(len(tr.x0), kind)
    ref = CR.of_trace(tr, p, n)
    lit = CR.of_trace(tr, p, n, literal=True)
    assert lit["nhits"] == len(lit["t"])
    keep = np.concatenate([[True], np.diff(lit["k"]) != 0]) if len(lit["k"]) else np.zeros(0, dtype=bool)
    assert keep.sum() == ref["nhits"] >= 10  # equal lengths: no hit of either list is left out of the comparison
    dt, dx = bounds(tr, p, n, ref["h"])
    et, ex = np.abs(lit["t"][keep] - ref["t"]), np.abs(lit["x"][keep] - ref["x"]).max(axis=1)
    print("%s/%s: %d hits (%d literal), max time error %.3g (bound %.3g), max row error %.3g (bound %.3g)"
          % (name, kind, ref["nhits"], lit["nhits"], et.max(), dt.min(), ex.max(), dx.min()))
    assert np.all(et <= dt) and np.all(ex <= dx)


@pytest.mark.parametrize("name,kind", CASES)
def test_every_row_lies_on_the_plane(pkg, name, kind):
    tr = chain(pkg, name)
    p, n = plane(len(tr.x0), kind)
    ref = CR.of_trace(tr, p, n)
    dt, _ = bounds(tr, p, n, ref["h"])
    res = np.abs((ref["x"] - p[None]) @ n)
    bound = np.minimum(dt, np.abs(ref["h"]) * dt)
    print("%s/%s: max residual %.3g, smallest bound %.3g" % (name, kind, res.max(), bound.min()))
    assert len(res) >= 10 and np.all(res <= bound)


def test_boomerang_traces_and_bad_planes_are_refused(pkg):
    tr = chain(pkg, "bps16")
    d = len(tr.x0)
    boom = pkg.PDMPTrace(pkg.Boomerang(sp.identity(d, format="csc"), np.zeros(d), 1.0), tr.t0, tr.x0, tr.θ0, tr.t, tr.x, tr.θ)
    with pytest.raises(TypeError, match="Boomerang"):
        pkg.trace.conditional_trace(boom, np.zeros(d), np.ones(d))
    fz = chain(pkg, "stickyzz")
    fboom = pkg.FactTrace(pkg.FactBoomerang(sp.identity(8, format="csc"), np.zeros(8), 0.1), fz.t0, fz.x0, fz.θ0, fz.events)
    with pytest.raises(TypeError, match="Boomerang"):
        pkg.trace.conditional_trace(fboom, np.zeros(8), np.ones(8))
    for p, n in ((np.zeros(d), np.zeros(d)), (np.full(d, np.nan), np.ones(d)), (np.zeros(d), np.full(d, np.inf)), (np.zeros(d - 1), np.ones(d - 1))):
        with pytest.raises(ValueError):
            pkg.trace.conditional_trace(tr, p, n)


def test_bridge_point_condition_is_the_bridge_value(pkg):
    """⟨ξ − p, n⟩ = X_s(ξ) − a for every coefficient vector: n is the row of the Faber-Schauder synthesis at s, ⟨p, n⟩ = a"""
    L, T, s, a = 3, 2.0, 0.7, 0.4
    p, n = pkg.problems.bridge_point_condition(L, T, s, a)
    rng = np.random.default_rng(1)
    xi = rng.standard_normal((5, (2 << L) + 1))
    Xs = pkg.trace.faber_schauder_path(xi, s, L, T)
    assert np.allclose((xi - p[None]) @ n, Xs - a, rtol=0, atol=1e-14)
    assert np.count_nonzero(n) == L + 3
