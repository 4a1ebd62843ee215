"""tests/exact_path.py itself (host only): hand-computed rationals, and the derived bound held against honest float64 host arithmetic on
oracle traces before any kernel is asked to keep it."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import exact_path as E
import oracle_lib as O


def _events(rows):
    ev = np.zeros(len(rows), dtype=O.EVENT_DTYPE)
    for k, (t, i, x, th) in enumerate(rows):
        ev[k]["t"], ev[k]["i"], ev[k]["x"], ev[k]["theta"] = t, i, x, th
    return ev


def test_hand_computed_trace_with_freeze_thaw_refresh_and_t0():
    """d = 2, t0 = 3: coordinate 0 has its first event BEFORE t0 (signed first segment), a refresh that changes |θ| and a reflection;
    coordinate 1 freezes at 1.0 (θ = 0), thaws at 4.0."""
    t0, x0, th0 = 3.0, [1.0, -2.0], [1.0, -1.0]
    ev = _events([(0.5, 0, -1.5, -1.0),   # Δ = -2.5: -2.5 (1 + 1 (-1.25))      =  5/8
                  (1.0, 1, 0.0, 0.0),     # Δ = -2:   -2 (-2 + (-1)(-1))        =  2        (freeze)
                  (2.0, 0, -3.0, 0.5),    # Δ = 1.5:  1.5 (-1.5 + (-1)(0.75))   = -27/8     (refresh, |θ| 1 -> 1/2)
                  (4.0, 1, 0.0, 2.0),     # Δ = 3:    frozen                    =  0        (thaw)
                  (5.0, 0, -1.5, -0.5)])  # Δ = 3:    3 (-3 + 0.5 (1.5))        = -27/4
    # T = 6: tails 1 (-1.5 + (-0.5)(0.5)) = -7/4 and 2 (0 + 2 (1)) = 4
    assert E.exact_J(t0, x0, th0, ev, 6.0) == [Fr(5, 8) - Fr(27, 8) - Fr(27, 4) - Fr(7, 4), Fr(2) + 0 + 4]
    assert E.exact_J(t0, x0, th0, ev, 6.0) == [Fr(-45, 4), Fr(6)]
    # T = 4.5: the event at 5 is ignored; tails 2.5 (-3 + 0.5 (1.25)) = -95/16 and 0.5 (0 + 2 (0.25)) = 1/4
    assert E.exact_J(t0, x0, th0, ev, 4.5) == [Fr(5, 8) - Fr(27, 8) - Fr(95, 16), Fr(2) + Fr(1, 4)]
    # a read while coordinate 1 is frozen: the same J at both ends of [1.5, 3.5]
    assert E.exact_J(t0, x0, th0, ev, 1.5)[1] == E.exact_J(t0, x0, th0, ev, 3.5)[1] == Fr(2)
    assert E.exact_absmax(t0, x0, th0, ev, 6.0) == [3.0, 4.0]
    p = E.ExactPath(t0, x0, th0)
    p.feed(ev)
    assert p.length(6.0) == [Fr(5, 2) + Fr(3, 2) + 3 + 1, 2 + 3 + 2] and p.own == [3, 2]
    # non-dyadic floats are the rationals they are
    assert E.exact_J(0.0, [0.1], [0.3], _events([]), 0.7) == [Fr(0.7) * (Fr(0.1) + Fr(0.3) * Fr(0.7) / 2)]
    # per-coordinate order: a refresh trace may be globally unordered, a coordinate's own times may not decrease
    E.exact_J(0.0, [0.0, 0.0], [1.0, 1.0], _events([(2.0, 0, 2.0, -1.0), (1.0, 1, 1.0, -1.0)]), 3.0)
    with pytest.raises(AssertionError):
        E.exact_J(0.0, [0.0, 0.0], [1.0, 1.0], _events([(2.0, 0, 2.0, -1.0), (1.0, 0, 1.0, -1.0)]), 3.0)


def _oracle_cases(pkg):
    """(name, t0, x0, θ0, T, oracle result): the configurations of test_gpu_path_integrals.py that the oracle states on the host."""
    rng = np.random.default_rng(5)
    out = []

    def start(d, sigma=None):
        s = np.ones(d) if sigma is None else sigma
        return rng.standard_normal(d), s * rng.choice([-1.0, 1.0], d)

    G = pkg.problems.gmrf_precision(16)
    d = G.shape[0]
    c = pkg.problems.column_norms(G)
    x0, th0 = start(d)
    out.append(("lattice16", 0.0, x0, th0, 6.0, O.spdmp_zigzag(G, None, G, x0, th0, c, 6.0, seed=3)))
    out.append(("lattice16-tracked", 0.0, x0, th0, 6.0, O.spdmp_zigzag(G, None, G, x0, th0, c, 6.0, seed=3, tracked=True)))
    out.append(("lattice16-refresh", 0.0, x0, th0, 6.0, O.spdmp_zigzag(G, None, G, x0, th0, c, 6.0, seed=4, lambda_ref=0.3)))
    sg = rng.uniform(0.5, 2.0, d)
    mu = 5.0 + rng.standard_normal(d)
    xs, ths = start(d, sg)
    out.append(("lattice16-mean-speeds", 0.0, xs + mu, ths, 4.0,
                O.spdmp_zigzag(G, mu, G, xs + mu, ths, 2.0 * c, 4.0, seed=6, target_mu=mu, sigma=sg)))
    out.append(("lattice16-adapt", 0.0, x0, th0, 4.0, O.spdmp_zigzag(G, None, G, x0, th0, 0.01 * c, 4.0, seed=7, adapt=True)))
    out.append(("lattice16-all", 0.0, x0, th0, 3.0, O.spdmp_zigzag(G, None, G, x0, th0, c, 3.0, seed=8, move_all=True)))
    G24 = pkg.problems.gmrf_precision(24)
    x24, th24 = start(G24.shape[0])
    out.append(("lattice24-t0=3", 3.0, x24, th24, 5.0,
                O.spdmp_zigzag(G24, None, G24, x24, th24, pkg.problems.column_norms(G24), 5.0, t0=3.0, seed=9)))
    Gs = pkg.problems.gmrf_precision(16, 0.5)
    r = O.sspdmp_zigzag(Gs, None, Gs, x0, th0, 1.5 * pkg.problems.column_norms(Gs), np.full(d, 0.8), 14.0, seed=10)
    assert np.sum(r["events"]["theta"] == 0.0) > 20  # freezes
    out.append(("sticky16", 0.0, x0, th0, 14.0, r))
    return out


def test_float64_host_arithmetic_keeps_the_bound(pkg):
    """trace.moments(tr, T)[0]·(T − t0) and trace.mean(tr)·T_last of oracle traces against exact_J, inside 3 (m + 1) u X L with
    m = own events + 1; and the bound a device comparison will use (m from the chain's counters) stays below 1e-6·X·L."""
    worst = {}
    for name, t0, x0, th0, T, r in _oracle_cases(pkg):
        ev = r["events"]
        assert len(ev) > 500, name
        tr = pkg.FactTrace(None, t0, x0, th0, ev)
        p = E.ExactPath(t0, x0, th0)
        p.feed([e for e in ev if e["t"] <= T])
        J, X, L = p.J(T), p.absmax(T), p.length(T)
        got = pkg.trace.moments(tr, T)[0] * (T - t0)
        use = 0.0
        for i in range(len(x0)):
            b = E.bound_J(p.own[i] + 1, X[i], L[i])
            err = abs(Fr(float(got[i])) - J[i])
            assert err <= b, (name, i, float(err), float(b))
            if b:
                use = max(use, float(err / b))
            # the bound of the device comparison (moving evaluation: m <= num + nevents + 1) cannot become vacuous
            assert E.bound_J(r["num"] + len(ev) + 1, X[i], L[i]) < Fr(1, 10 ** 6) * Fr(X[i]) * L[i], (name, i)
        # mean(Ξ): the integral up to each coordinate's last own event over the last event time, trapezoids to the RECORDED positions.
        # The recorded end point x_k is not the exact path's (x_{k-1} + θ Δ): under the moving evaluation it has been through every move
        # of the coordinate since its previous own event, 2u·X each, and the trapezoid carries half of it over Δ_k.  With a handful of
        # moves between own events that stays inside own events + 1 (at most 0.37 of it on the cases below).  Two cases move a
        # coordinate far more often or further than its own events tell: G = All() (every proposal of the chain moves it: 1.14 of the
        # own-events bound) and t0 = 3 (carried back to t ≈ 0 and forward again at |x| up to X + 3|θ|: 2.15).  Those moves are not in
        # the trace; as for a device read they are bounded by the chain's counters, num + nevents + 1.
        q = E.ExactPath(t0, x0, th0)
        q.feed(ev)
        m = pkg.trace.mean(tr) * ev["t"][-1]
        for i in range(len(x0)):
            if q.own[i]:
                moves = r["num"] + len(ev) + 1 if name in ("lattice16-all", "lattice24-t0=3") else q.own[i] + 1
                assert abs(Fr(float(m[i])) - q.I[i]) <= E.bound_J(moves, q.X[i], q.L[i]), (name, i)
        worst[name] = use
    print("largest |moments - exact| / bound per case:", worst)
    assert max(worst.values()) < 1.0
