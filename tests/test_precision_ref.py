"""tests/ref/precision_ref.c, the sequential restatement of the precision case study (casestudies/precision/precision.jl: the sticky ZigZag on
the Cholesky factor of a precision matrix), held on the CPU to what does not depend on it: the potential's finite difference, a brute-force
index map, its own one-shot run, and the closed-form sticky posterior at n = 2.  The device kernel (csrc/pdmp_precision.inc) is held to this
file bit for bit by tests/test_gpu_precision_parity.py."""
import math

import numpy as np
import pytest

import precision_ref_lib as R
from precision_cases import DIAGONAL_FREEZE, N2, lower_index, n2_flow, stalled_input


def phi(YY, N, g0, u, n):
    """ϕ(u) = ½ Σ_c L[:,c]ᵀ YY L[:,c] − N Σ_c log L[c,c] + (γ0/2)(Σ_{r>c} L[r,c]² + Σ_c (L[c,c] − 1)²)"""
    r, c = lower_index(n)
    L = np.zeros((n, n))
    L[r, c] = u
    dg = np.diag(L)
    off = L - np.diag(dg)
    return 0.5 * np.trace(L.T @ YY @ L) - N * np.log(dg).sum() + 0.5 * g0 * ((off**2).sum() + ((dg - 1.0)**2).sum())


@pytest.mark.parametrize("g0", [0.0, 0.3])
def test_gradient_is_the_potentials(g0):
    """ref_precision_grad against the central difference of ϕ at ε = 1e-4, every coordinate of n = 5, N = 10, diagonals in [0.5, 2].  The
    difference's error is ε²/6 · |ϕ‴| = ε²/6 · 2N/u³ <= 1e-8/6 · 20/0.125 < 3e-7 (the quadratic part has none), rounding of ϕ ~ 1e2 · 2^-52 / ε
    < 1e-9: the bound 1e-6 (1 + |g|) holds with room, and a missing −N/u term (>= 5) or a wrong column offset does not pass it."""
    n, N, eps = 5, 10.0, 1e-4
    rng = np.random.default_rng(7)
    B = rng.standard_normal((n, 12))
    YY = B @ B.T
    YY = 0.5 * (YY + YY.T)
    r, c = lower_index(n)
    u = rng.standard_normal(n * (n + 1) // 2)
    u[r == c] = rng.uniform(0.5, 2.0, n)
    for i in range(u.size):
        up, um = u.copy(), u.copy()
        up[i] += eps
        um[i] -= eps
        fd = (phi(YY, N, g0, up, n) - phi(YY, N, g0, um, n)) / (2 * eps)
        g = R.grad(YY, N, g0, u, i)
        assert abs(g - fd) <= 1e-6 * (1 + abs(g)), (i, g, fd)


def test_index_map_against_enumeration():
    """k0(c) = c n − c (c − 1)/2 and the column of i, against the enumeration of the lower triangle column by column, n = 1 .. 64."""
    for n in range(1, 65):
        i = 0
        for c in range(n):
            assert R.k0(n, c) == i
            for r in range(c, n):
                assert R.col(n, i) == c and R.k0(n, c) + (r - c) == i
                i += 1
        assert i == n * (n + 1) // 2
        r, c = lower_index(n)
        assert np.array_equal(np.array([R.col(n, k) for k in range(i)]), c) and np.all(r >= c)


def _chain5(seed, **kw):
    n, N = 5, 40.0
    rng = np.random.default_rng(100 + seed)
    B = rng.standard_normal((n, 40))
    YY = B @ B.T
    YY = 0.5 * (YY + YY.T)
    r, c = lower_index(n)
    d = r.size
    x0 = 0.2 * rng.standard_normal(d)
    x0[r == c] = rng.uniform(0.7, 1.3, n)
    th0 = rng.choice([-1.0, 1.0], d)
    gam = YY[r, r] + np.where(r == c, N, 0.0)
    mu = np.where(r == c, 1.0, 0.0)
    return R.Chain(YY, N, x0, th0, 1.0, gam, mu, 0.5, adapt=True, seed=seed, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(reversible=True, strong_upperbounds=True, gamma0=0.3)], ids=["plain", "rev_strong_g0"])
def test_slices_equal_one_shot(kw):
    """Slices with STOP_BEFORE, then the reference tail, leave the bytes of a one-shot run: events, counters, draws and state."""
    one = _chain5(3, **kw)
    one.run(30.0)
    a = one.result()
    cut = _chain5(3, **kw)
    for Tk in (0.5, 7.25, 7.3, 19.0):
        cut.run(Tk, R.RUN_STOP_BEFORE)
        assert cut.S.status == R.REF_OK and np.all(cut.Q >= Tk)
    cut.run(30.0)
    b = cut.result()
    assert a["nevents"] > 300 and a["nadapt"] > 0 and (a["theta"] == 0).sum() > 5
    for k in a:
        assert (a[k].tobytes() == b[k].tobytes()) if isinstance(a[k], np.ndarray) else (a[k] == b[k]), k


def _time_averages(r, x0, th0):
    """(∫x_i dt / T [d], time with x_i = 0 = θ_i / T [d]) of one chain's events, T = the last event's time"""
    d = x0.size
    T = r["t"][-1]
    mean, zero = np.empty(d), np.empty(d)
    for i in range(d):
        m = r["i"] == i
        t = np.concatenate([[0.0], r["t"][m], [T]])
        x = np.concatenate([[x0[i]], r["x"][m]])
        th = np.concatenate([[th0[i]], r["theta"][m]])
        dt = np.diff(t)
        mean[i] = (dt * (x + 0.5 * th * dt)).sum() / T
        zero[i] = dt[(x == 0) & (th == 0)].sum() / T
    return mean, zero


def test_exact_posterior_n2():
    """n = 2, YY = [[12, 1.5], [1.5, 9]], N = 10, γ0 = 0, κ = 1: the sticky invariant law is closed form.  With A = YY,
    s = A11 − A12²/A22, the column (L11, L21) has density ∝ L11^N exp(−½ vᵀAv) off the axis L21 = 0 and κ⁻¹ L11^N exp(−½ A11 L11²) on it:
    Z0/Z1 = (s/A11)^((N+1)/2) / √(2π/A22) = 1.06597, p0 = P(L21 = 0) = (Z0/Z1)/κ / (1 + (Z0/Z1)/κ) = 0.51597; E_a = Γ((N+2)/2)/Γ((N+1)/2) √(2/a)
    is the mean of the density ∝ v^N exp(−a v²/2): E L11 = p0 E_A11 + (1 − p0) E_s, E L21 = (1 − p0)(−A12/A22) E_s, E L22 = E_A22.
    64 chains of the restatement (seeds 0 .. 63, adapt, T = 4000): each of the four within 4 between-chain standard errors; no chain STALLED."""
    YY, N, kappa = N2["YY"], N2["N"], 1.0
    A11, A12, A22 = YY[0, 0], YY[0, 1], YY[1, 1]
    s = A11 - A12 * A12 / A22
    z = (s / A11) ** ((N + 1) / 2) / math.sqrt(2 * math.pi / A22)
    assert abs(z - 1.06597) < 1e-5
    p0 = (z / kappa) / (1 + z / kappa)
    assert abs(p0 - 0.51597) < 1e-5

    def E(a):
        return math.exp(math.lgamma((N + 2) / 2) - math.lgamma((N + 1) / 2)) * math.sqrt(2 / a)

    exact = np.array([p0, p0 * E(A11) + (1 - p0) * E(s), (1 - p0) * (-A12 / A22) * E(s), E(A22)])
    gam, mu = n2_flow()
    x0, th0 = mu.copy(), np.array([1.0, -1.0, 1.0])
    got = np.empty((64, 4))
    for seed in range(64):
        r = R.precision(YY, N, x0, th0, 4000.0, 1.0, gam, mu, kappa, adapt=True, seed=seed, ev_cap=1 << 19)
        assert r["status"] == R.REF_OK and r["nevents"] > 10000
        mean, zero = _time_averages(r, x0, th0)
        assert zero[0] == 0 and zero[2] == 0  # (no diagonal ever froze)
        got[seed] = [zero[1], mean[0], mean[1], mean[2]]
    est, se = got.mean(axis=0), got.std(axis=0, ddof=1) / 8
    print("exact", exact, "estimate", est, "se", se, "z", (est - exact) / se)
    assert np.all(se < 0.01)
    assert np.all(np.abs(est - exact) <= 4 * se), (est, exact, se)


def test_diagonal_freeze_stalls():
    """A diagonal of L that reaches 0 would make the next gradient N/0: the freeze popped for it ends the chain as STALLED before any state
    changes.  The input (precision_cases.stalled_input: L11 started at 0.1 going down, N = 1e-3, c = 50, seed chosen by running this
    restatement) is pinned by status, event count, proposals and draws; the GPU parity test runs the same input."""
    a = stalled_input()
    ch = R.Chain(a["YY"], a["N"], a["x0"], a["th0"], a["c"], a["gam"], a["mu"], a["kappa"], adapt=False, seed=a["seed"])
    ch.run(5.0)
    r = ch.result()
    assert r["status"] == R.REF_STALLED
    assert (r["nevents"], r["num"], r["ndraw_main"]) == (DIAGONAL_FREEZE["nevents"], DIAGONAL_FREEZE["num"], DIAGONAL_FREEZE["ndraw_main"])
    assert ch.f[0] == 1 and ch.Q[0] == ch.Q.min() and ch.th[0] < 0 and ch.x[0] > 0  # the diagonal's freeze is what was popped; nothing of it changed
    assert (r["theta"] == 0).sum() == 7 and 0 in r["i"]  # (off-diagonal freezes and a reflection of L11 itself came first)
    assert r["t_last"] < ch.Q[0]
    again = ch.run(50.0)  # an ended chain stays ended
    assert len(again["t"]) == 0 and ch.S.status == R.REF_STALLED
