"""tests/ref/bridge_ref.c -- the sequential restatement of the reference's diffusion-bridge sampler (research/diffusion_bridge/) -- held to what
it restates, without a GPU: the gradient to a finite difference of the potential, the sampled bridge to the Brownian and Ornstein-Uhlenbeck
bridges' closed forms, the index helpers to brute force, and a sliced run to a one-shot one."""
import numpy as np
import pytest

import bridge_ref_lib as R

SCRIPT = dict(alpha=1.5, beta=0.1, omega=2 * np.pi)  # diffbridge.jl:7-9


def hat(i, s, L, T):
    """Basis function i (0-based, interior) at the times s, written out: a tent on [δk, δ(k+1)) with peak √T / (2 √(2^(L−l)))."""
    l = (i & -i).bit_length() - 1
    k = i >> (l + 1)
    m = L - l
    delta = T / 2 ** m
    mid = delta * (k + 0.5)
    inside = (s >= delta * k) & (s < delta * (k + 1))
    return np.where(inside, np.sqrt(T) / (2 * np.sqrt(2.0 ** m)) - np.abs(s - mid) * np.sqrt(2.0 ** m) / np.sqrt(T), 0.0)


def path(xi, s, L, T):
    d = (2 << L) + 1
    X = s / np.sqrt(T) * xi[-1] + np.sqrt(T) * (1 - s / T) * xi[0]
    for i in range(1, d - 1):
        X = X + xi[i] * hat(i, s, L, T)
    return X


def test_formula_pin():
    """Mean of ref_bridge_grad over the stratified grid u = (q + ½)/4096 against the central difference of
    ϕ(ξ) = ½ Σ ξ_i² + ½ ∫₀ᵀ (b² + b′)(X_s) ds (composite Simpson, 2¹⁴ intervals), L = 3, the script's drift.  A wrong b′ fails it.

    Tolerance, per coordinate i of level l (m = L − l, δ = T/2^m, N = 4096, ε = 1e-4, h_S = T/2¹⁴), from bounds on the drift's derivatives
    |b| <= β X + α =: B0, |b^(n)| <= α ωⁿ (+ β for n = 1) =: Bn with X >= sup |X_s|, and the path's slope
    |X′_s| <= |ξ_last − ξ_first|/√T + Σ_lev max_j |ξ_j| √(2^(L−lev))/√T =: S (X_s is linear on every interval of the finest dyadic grid):
      midpoint   the mean is the midpoint rule for ∫ f, f(s) = ½ Λ_i(s) H(X_s), H = 2 b b′ + b″, over the support; the kinks of X and Λ_i lie on
                 cell boundaries (multiples of T/2^(L+1); 4096 cells per support), so the error is <= δ (δ/N)²/24 · sup |f″| with
                 |f″| <= ½ (2 |Λ′| |H′| S + |Λ| |H″| S²), |Λ′| = √(2^m)/√T, |Λ| <= √T/(2 √(2^m)),
                 |H′| <= 2 B1² + 2 B0 B2 + B3, |H″| <= 6 B1 B2 + 2 B0 B3 + B4;
      difference ε²/6 · sup |∂³ϕ/∂ξ_i³| with ∂³ϕ/∂ξ_i³ = ½ ∫ H″(X_s) Λ_i(s)³ ds, <= ½ |H″| |Λ|³ δ;
      Simpson    each of the two ϕ values carries <= T h_S⁴/180 · sup |F⁗|, F = ½ (b² + b′)(X_s): F⁗ = G⁗(X) S⁴ on every panel (the kinks lie
                 on even grid points), |G⁗| <= ½ (2 B0 B4 + 8 B1 B3 + 6 B2² + B5); the quotient divides their sum by 2 ε;
      rounding   ϕ is a sum of 2¹⁴ terms of size <= |F| max: 2 · 2¹⁴ · 2⁻⁵³ · (|ϕ| + 1) / (2 ε) -- below 1e-7.
    The sum is about 2e-3 at the top level and 1e-5 at the finest; the stray factor 2 of the script's b′ moves the gradient by 0.05 .. 1."""
    L, T = 3, 2.0
    d = (2 << L) + 1
    al, be, om = SCRIPT["alpha"], SCRIPT["beta"], SCRIPT["omega"]
    rng = np.random.default_rng(7)
    xi = 0.5 * rng.uniform(-1, 1, d)
    xi[0], xi[-1] = 1.5 / np.sqrt(T), -0.5 / np.sqrt(T)
    N, eps, NS = 4096, 1e-4, 1 << 14
    sgrid = np.linspace(0.0, T, NS + 1)
    w = np.ones(NS + 1)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    w *= T / NS / 3

    def phi(x, bp_factor=1.0):
        sg = np.minimum(sgrid, np.nextafter(T, 0))  # (the tents are defined on [0, T))
        X = path(x, sg, L, T)
        b = -be * X + al * np.sin(om * X)
        bp = -be + bp_factor * al * om * np.cos(om * X)
        return 0.5 * np.sum(x ** 2) + 0.5 * np.sum(w * (b * b + bp))

    Xmax = np.max(np.abs(path(xi, np.minimum(sgrid, np.nextafter(T, 0)), L, T))) + 0.05
    B0 = be * Xmax + al
    B = [B0, be + al * om] + [al * om ** n for n in range(2, 6)]
    H1 = 2 * B[1] ** 2 + 2 * B[0] * B[2] + B[3]
    H2 = 6 * B[1] * B[2] + 2 * B[0] * B[3] + B[4]
    G4 = 0.5 * (2 * B[0] * B[4] + 8 * B[1] * B[3] + 6 * B[2] ** 2 + B[5])
    lev_of = np.array([R.lvl(i, L) for i in range(d)])
    S = abs(xi[-1] - xi[0]) / np.sqrt(T) + sum(np.max(np.abs(xi[1:-1][lev_of[1:-1] == lev])) * np.sqrt(2.0 ** (L - lev)) / np.sqrt(T) for lev in range(L + 1))
    simpson = T * (T / NS) ** 4 / 180 * G4 * S ** 4
    worst_wrong = 0.0
    for i in range(1, d - 1):
        m = L - lev_of[i]
        delta = T / 2 ** m
        lam, dlam = np.sqrt(T) / (2 * np.sqrt(2.0 ** m)), np.sqrt(2.0 ** m) / np.sqrt(T)
        tol = (delta * (delta / N) ** 2 / 24 * 0.5 * (2 * dlam * H1 * S + lam * H2 * S ** 2) + eps ** 2 / 6 * 0.5 * H2 * lam ** 3 * delta
               + 2 * simpson / (2 * eps) + 1e-7)
        gs = []
        for q in range(N):
            st, g = R.bridge_grad(xi.copy(), np.zeros(d), np.zeros(d), i, 0.0, (q + 0.5) / N, L=L, T=T, alpha=al, beta=be, omega=om)
            assert st == R.REF_OK
            gs.append(g)
        e = np.zeros(d)
        e[i] = eps
        fd = (phi(xi + e) - phi(xi - e)) / (2 * eps)
        assert abs(np.mean(gs) - fd) <= tol, (i, np.mean(gs), fd, tol)
        fd_wrong = (phi(xi + e, 2.0) - phi(xi - e, 2.0)) / (2 * eps)
        worst_wrong = max(worst_wrong, abs(np.mean(gs) - fd_wrong) / tol)
    assert worst_wrong > 20  # (the check has the power it is there for: the script's b′ = −β + 2 α ω cos(ωx) is far outside the tolerance)


def _event_array(pkg, r):
    ev = np.zeros(len(r["t"]), dtype=pkg._lib.EVENT_DTYPE)
    ev["t"], ev["i"], ev["x"], ev["theta"] = r["t"], r["i"], r["x"], r["theta"]
    return ev


# the restatement's spread over seeds 0..7 (standard deviation, T′ = 1000, the first tenth discarded, grid 0.05), measured with this file's recipe
SPREAD = {(0.0, 0.0): (0.0299, 0.0427), (0.0, 1.0): (0.0152, 0.0146)}


@pytest.mark.parametrize("beta", [0.0, 1.0], ids=["brownian_bridge", "ou_bridge"])
def test_bridge_statistics(pkg, beta):
    """Time average and variance of X(T/2) along the restatement's chain, T = 2, L = 5, u = 1.5, v = −0.5, T′ = 1000 (the first tenth discarded,
    ξ read every 0.05), against the closed forms: mean (u sinh β(T−s) + v sinh βs)/sinh βT and variance sinh βs sinh β(T−s)/(β sinh βT),
    the β -> 0 limits (u (T−s) + v s)/T and s (T−s)/T for the Brownian bridge (α = 0 in both cases).
    Envelope: 3 x the spread of the restatement over seeds 0..7, measured once with this recipe:
      α = β = 0      mean 0.4869 +- 0.0299 (closed form 0.5),    variance 0.5212 +- 0.0427 (0.5)
      α = 0, β = 1   mean 0.3227 +- 0.0152 (closed form 0.3240), variance 0.3794 +- 0.0146 (0.3808)
    The test runs seeds 8 and 9, which were not among them."""
    L, T, u, v, TP = 5, 2.0, 1.5, -0.5, 1000.0
    d = (2 << L) + 1
    s = T / 2
    if beta == 0:
        mean, var = (u * (T - s) + v * s) / T, s * (T - s) / T
    else:
        mean = (u * np.sinh(beta * (T - s)) + v * np.sinh(beta * s)) / np.sinh(beta * T)
        var = np.sinh(beta * s) * np.sinh(beta * (T - s)) / (beta * np.sinh(beta * T))
    sd_mean, sd_var = SPREAD[(0.0, beta)]
    for seed in (8, 9):
        x0, th0, c = pkg.problems.diffusion_bridge_problem(L, T, u, v, rng=np.random.default_rng(100 + seed))
        r = R.bridge(x0, th0, TP, c, L=L, T=T, alpha=0.0, beta=beta, omega=1.0, adapt=True, seed=seed)
        assert r["status"] == R.REF_OK and r["nevents"] > 20000
        tr = pkg.FactTrace(pkg.ZigZag(np.eye(d), np.zeros(d)), 0.0, x0.copy(), th0.copy(), _event_array(pkg, r))
        tg, xs = pkg.trace.discretize(tr, 0.05)
        X = pkg.trace.faber_schauder_path(xs[tg >= 0.1 * TP], s, L, T)
        assert abs(X.mean() - mean) <= 3 * sd_mean, (seed, X.mean(), mean)
        assert abs(X.var() - var) <= 3 * sd_var, (seed, X.var(), var)


def test_index_helpers_against_brute_force(pkg):
    """lvl, the index j of (s, lev) and Λ against their definitions written out, L <= 6; the support of basis function i is [δk, δ(k+1));
    ref_dotpsi and trace.faber_schauder_path equal the sum over all basis functions."""
    T = 2.0
    rng = np.random.default_rng(3)
    for L in range(7):
        d = (2 << L) + 1
        want_lvl = [L] + [next(l for l in range(L + 1) if (i >> l) & 1) for i in range(1, d - 1)] + [L]
        assert [R.lvl(i, L) for i in range(d)] == want_lvl
        s = np.sort(np.concatenate([rng.uniform(0, T, 200), T * np.arange(2 << L) / (2 << L)]))  # (dyadic points included: the half-open ends)
        for i in range(1, d - 1):
            l = want_lvl[i]
            k, delta = i >> (l + 1), T / 2 ** (L - l)
            idx = np.array([R.index(x, l, L, T) for x in s])
            inside = (s >= delta * k) & (s < delta * (k + 1))
            assert np.array_equal(idx == i, inside), (L, i)  # level l's covering function at s is i exactly on i's support
            lam = np.array([R.Lambda(x, L - l, T) for x in s])
            assert np.allclose(np.where(inside, lam, 0.0), hat(i, s, L, T), rtol=0, atol=1e-14)
        xi = rng.standard_normal(d)
        brute = path(xi, s, L, T)
        assert np.allclose([R.dotpsi(xi, x, L, T) for x in s], brute, rtol=0, atol=1e-12 * (L + 2))
        assert np.allclose(pkg.trace.faber_schauder_path(xi, s, L, T), brute, rtol=0, atol=1e-12 * (L + 2))
        assert np.allclose(pkg.trace.faber_schauder_path(np.stack([xi, 2 * xi]), s, L, T), np.stack([brute, 2 * brute]), rtol=0, atol=1e-11 * (L + 2))
    assert np.isnan(R.dotpsi(np.zeros(5), T, 1, T))  # "out of bounds", faberschauder.jl:17
    with pytest.raises(ValueError):
        pkg.trace.faber_schauder_path(np.zeros(5), T, 1, T)


@pytest.mark.parametrize("adapt", [True, False])
def test_sliced_run_equals_one_shot(pkg, adapt):
    """The restatement resumed over five PDMP_RUN_STOP_BEFORE slices and a reference tail is the one-shot run, byte for byte."""
    L, T, TP = 4, 2.0, 40.0
    x0, th0, c = pkg.problems.diffusion_bridge_problem(L, T, 1.5, -0.5, rng=np.random.default_rng(5))
    c = c * (1.0 if adapt else 400.0)
    kw = dict(L=L, T=T, adapt=adapt, seed=21, **SCRIPT)
    one = R.bridge(x0, th0, TP, c, **kw)
    assert one["status"] == R.REF_OK and one["nevents"] > 500 and (one["nadapt"] > 0) == adapt
    ch = R.Chain(x0, th0, c, **kw)
    for Tk in (3.0, 11.0, 11.5, 25.0, 39.0):
        ch.run(Tk, R.RUN_STOP_BEFORE)
        assert ch.S.t_last < Tk
    ch.run(TP, R.RUN_REFERENCE_TAIL)
    two = ch.result()
    for f, a in one.items():
        assert np.array_equal(a, two[f]), f


def test_stall_and_bound_violation_statuses(pkg):
    """|ωx| beyond pdmp_sincos' range stalls the chain at its first proposal; a c that is too small without adapt ends it as BOUND_VIOLATED."""
    L, T = 2, 2.0
    x0, th0, c = pkg.problems.diffusion_bridge_problem(L, T, 1.5, -0.5, rng=np.random.default_rng(5))
    r = R.bridge(x0, th0, 5.0, c, L=L, T=T, alpha=1.5, beta=0.1, omega=1e12, seed=1)
    assert r["status"] == R.REF_STALLED and r["num"] == 0 and r["ndraw_global"] == 1
    r = R.bridge(x0, th0, 50.0, 0.01 * c, L=L, T=T, seed=1, **SCRIPT)
    assert r["status"] == R.REF_BOUND_VIOLATED and r["nacc"] == r["nevents"] + 1
