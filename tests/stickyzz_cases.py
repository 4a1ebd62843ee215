"""Cases and helpers shared by tests/test_stickyzz_ref.py and tests/test_gpu_stickyzz_parity.py (stickyzz, src/stickyzz.jl): the branch grid of
the three-parameter poisson_time, the d = 1 and d = 8 problems with their barrier sets, batch means of a 1-d trace.  A barrier is the plain
triple ((lo, hi), (rule_lo, rule_hi), (κ_lo, κ_hi)) -- what tests/stickyzz_ref_lib.py takes; barriers_for(pkg, ...) makes the package's
StickyBarriers of it."""
import math

import numpy as np
import scipy.sparse as sp

import stickyzz_ref_lib as R

INF = float("inf")
NO_BARRIER = ((-INF, INF), ("reflect", "reflect"), (INF, INF))  # StickyBarriers(), src/stickyzz.jl:25
BOX_1D = ((-0.2, 1.5), ("reflect", "reflect"), (INF, INF))
STICKY_1D = ((0.0, 0.0), ("sticky", "sticky"), (1.5, 1.5))

POISSON_TIME3_BRANCHES = (43, 45, 48, 52, 54, 58, 60, 62)  # the return lines of src/poissontime.jl:39-65


def poisson_time3_branch(a, b, c, u):
    lu = math.log(u)
    if b > 0:
        if a < 0:
            return 43 if -c * a / b + lu < 0.0 else 45
        return 48
    if b == 0:
        return 52 if a > 0 else 54
    if a <= 0.0:
        return 58
    return 60 if -c * a / b - a * a / (2 * b) + lu > 0.0 else 62


def poisson_time3_grid():
    """(a, b, u) over signs and sizes of a and b and small, middling and large u: with c = 0.01 every branch of src/poissontime.jl:39-65.
    u stops at 0.97: the square-root branches (:43, :48, :60) form a small τ as the difference of two quotients of size (a + c)/b, so the
    digits of τ fall with τ/((a + c)/b) -- the reference's own formula in double precision (at u = 0.9999, a = 20, b = −0.4, τ = 5e-6 the
    integral identity holds to 2.2e-10 only)."""
    A = [-5.0, -0.7, -0.0, 0.0, 0.3, 2.0, 20.0]
    B = [-3.0, -0.4, 0.0, 0.5, 4.0]
    U = [0.03, 0.4, 0.97]
    g = np.array([(a, b, u) for a in A for b in B for u in U])
    return g[:, 0].copy(), g[:, 1].copy(), g[:, 2].copy()


def integrated_rate(a, b, c, tau):
    """∫₀^τ (c + (a + b s)⁺) ds, in closed form."""
    def pos_area(s0, s1):  # ∫ (a + b s) ds over [s0, s1] where the integrand is >= 0
        return a * (s1 - s0) + 0.5 * b * (s1 * s1 - s0 * s0)

    if b == 0:
        area = max(a, 0.0) * tau
    else:
        root = -a / b  # a + b s changes sign here
        if b > 0:
            area = pos_area(max(root, 0.0), tau) if tau > root else 0.0
        else:
            area = pos_area(0.0, min(root, tau)) if root > 0 else 0.0
    return c * tau + area


def run_1d(barrier, T, seed):
    """test/sticky.jl:7-36's problem: target N(0.9, 0.5), flow Γ = [1] with μ = 0, c = 20, x0 = 1, θ0 = 0.8."""
    one, two = sp.csc_matrix(np.array([[1.0]])), sp.csc_matrix(np.array([[2.0]]))
    return R.stickyzz(0.0, [1.0], [0.8], T, [20.0], barrier, gamma=one, target_gamma=two, target_mu=[0.9], seed=seed)


def batch_means_1d(r, x0, th0, T, what, B=32):
    """The B batch means over [0, T] of x (what = "x") or of the indicator of moving (what = "moving": θ ≠ 0, the time away from a sticky
    level) of a 1-d run: exact integrals of the piecewise-linear path through the events (t0 = 0)."""
    t = np.concatenate([[0.0], r["t"]])
    x = np.concatenate([[x0], r["x"]])
    th = np.concatenate([[th0], r["theta"]])

    def piece(k, dt):
        return dt * (x[k] + 0.5 * th[k] * dt) if what == "x" else dt * (th[k] != 0)

    cum = np.concatenate([[0.0], np.cumsum(piece(np.arange(len(t) - 1), np.diff(t)))])
    edges = np.linspace(0.0, T, B + 1)
    k = np.searchsorted(t, edges, side="right") - 1
    F = cum[k] + piece(k, edges - t[k])
    return np.diff(F) / np.diff(edges)


def speed_before(r, k, th0):
    """θ of coordinate i = r["i"][k] just before event k: that of i's previous event, or θ0[i]."""
    i = r["i"][k]
    prev = np.nonzero(r["i"][:k] == i)[0]
    return r["theta"][prev[-1]] if len(prev) else th0[i]


def _pkg():
    from __graft_entry__ import load_package
    return load_package()


def precision8():
    return _pkg().problems.maintest_precision(8)


def c8(G, scale=0.7):
    return scale * _pkg().problems.column_norms(G)


def state8(nchains, d=8, seed=3):
    """x0 ~ N(0, 1) clipped into (−0.9, 0.4) -- inside every box used here --, θ0 from {±1, ±0.5} (test/sticky.jl:51)."""
    rng = np.random.default_rng(seed)
    x0 = np.clip(rng.standard_normal((nchains, d)), -0.9, 0.4)
    th0 = rng.choice([-1.0, -0.5, 0.5, 1.0], size=(nchains, d))
    return x0, th0


def mixed_barriers(d, rng=None):
    """Each coordinate different (cycled over d): no barrier, one-sided (2.5, Inf) as in examples/positivityconstraint.jl:46, sticky below with
    reflecting above, reversible, different κ on the two sides, a wall above only.  With rng: κ drawn from (0.3, 1.3).  fit_state moves a
    start into its barriers."""
    base = [NO_BARRIER,
            ((2.5, INF), ("reflect", "reflect"), (INF, INF)),
            ((-1.0, 0.6), ("sticky", "reflect"), (0.8, 40.0)),
            ((-0.95, 0.45), ("reversible", "reversible"), (1.2, 1.2)),
            ((-1.0, 0.5), ("sticky", "sticky"), (0.4, 3.0)),
            ((-INF, 0.5), ("reflect", "reflect"), (INF, INF)),
            ((-0.9, 0.4), ("reflect", "sticky"), (INF, 0.7)),
            ((-1.2, 0.8), ("reversible", "sticky"), (2.0, 0.5))]
    out = []
    for i in range(d):
        x, rule, kap = base[i % len(base)]
        if rng is not None:
            kap = tuple(float(rng.uniform(0.3, 1.3)) for _ in range(2))
        out.append((x, rule, kap))
    return out


def fit_state(x0, barriers):
    """x0 [nchains x d] with every coordinate strictly inside its barriers (at least 0.05 from a finite one)."""
    lo = np.array([b[0][0] for b in barriers]) + 0.05
    hi = np.array([b[0][1] for b in barriers]) - 0.05
    with np.errstate(invalid="ignore"):  # (−inf + inf where a coordinate has no barrier: not selected)
        return np.where(lo > hi, 0.5 * (lo + hi), np.clip(x0, lo, hi))


def barriers_for(pkg, barriers, d):
    if isinstance(barriers, tuple):
        barriers = [barriers] * d
    return [pkg.StickyBarriers(*b) for b in barriers]
