"""The sequential restatement of the speed-recorded Bouncy Particle on a logistic-regression target (tests/ref/bps_logistic_ref.c) held to
independent truth on the CPU -- its dϕ and ∇ϕ! to a NumPy evaluation, its samples to the posterior by quadrature, its loop to the draw table of
modern_bps_ref.c -- before the device loop is held to the restatement bit for bit (tests/test_gpu_bps_logistic_parity.py)."""
import math
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import bps_logistic_ref_lib as B

EPS = np.finfo(np.float64).eps


def truth(A, y, m, g0, x, th):
    """dϕ, ∇ϕ and the sums of the absolute values of their terms, by math.fsum and np.exp."""
    A = np.asarray(sp.csc_matrix(A).toarray())
    eta, zeta = [math.fsum(r * x) for r in A], [math.fsum(r * th) for r in A]
    eta, zeta = np.array(eta), np.array(zeta)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-eta))
    r = m * p - y
    w = m * p * (1.0 - p)
    t1 = list(r * zeta) + list(g0 * th * x)
    t2 = list(w * zeta * zeta) + list(g0 * th * th)
    s1, s2 = math.fsum(np.abs(t1)), math.fsum(np.abs(t2))
    grad, sg = np.empty(A.shape[1]), np.empty(A.shape[1])
    for e in range(A.shape[1]):
        terms = list(A[:, e] * r) + [g0 * x[e]]
        grad[e], sg[e] = math.fsum(terms), math.fsum(np.abs(terms))
    return np.array([math.fsum(t1), math.fsum(t2)]), np.array([s1, s2]), grad, sg, p


@pytest.mark.parametrize("g0", [0.0, 0.7])
@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_pointwise_against_numpy(kind, g0):
    """|ref − truth| <= 64 eps Σ|terms| per output, the terms being those of the output's own sum (r_i ζ_i and γ0 θ_k x_k; w_i ζ_i² and
    γ0 θ_k²; a_ie r_i and γ0 x_e).  Each term is a product of at most four factors; p and w come through pdmp_exp (< 1 ulp,
    tests/test_detmath_accuracy.py) and ζ, η through idots of at most 17 products, so a term is good to about (4 + 2·17) eps of its size where
    nothing cancels inside it, and the 64-lane sum of n = 200 terms adds (n/64 + 6) eps: inside 64 eps of Σ|terms|.  The figures are printed."""
    rng = np.random.default_rng(11 + int(g0 * 10) + (kind == "sparse"))
    n, d = 200, 17
    A = rng.standard_normal((n, d))
    if kind == "sparse":
        A = sp.csc_matrix(A * (rng.random((n, d)) < 0.15))
    m = rng.integers(1, 6, n).astype(np.float64)
    y = np.floor(rng.random(n) * (m + 1))
    for _ in range(5):
        x, th = 0.8 * rng.standard_normal(d), rng.standard_normal(d)
        dphi, grad = B.evaluate(A, y, m, g0, x, th)
        td, sd, tg, sg, _ = truth(A, y, m, g0, x, th)
        print(kind, g0, np.abs(dphi - td) / (EPS * sd), np.max(np.abs(grad - tg) / (EPS * sg)))
        assert np.all(np.abs(dphi - td) <= 64 * EPS * sd)
        assert np.all(np.abs(grad - tg) <= 64 * EPS * sg)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_extreme_linear_predictor(sign):
    """|η| ≈ 750 on one row: p is exactly 1 or 0 there, its variance 0, nothing is NaN, and the outputs still meet the pointwise bound."""
    rng = np.random.default_rng(5)
    n, d = 40, 3
    A = rng.standard_normal((n, d))
    A[7] = sign * np.array([750.0, 0.0, 0.0])
    x, th = np.array([1.0, 0.3, -0.2]), np.array([0.5, -1.0, 0.25])
    m = np.full(n, 2.0)
    y = np.ones(n)
    dphi, grad = B.evaluate(A, y, m, 0.7, x, th)
    td, sd, tg, sg, p = truth(A, y, m, 0.7, x, th)
    assert p[7] == (1.0 if sign > 0 else 0.0)
    assert np.all(np.isfinite(dphi)) and np.all(np.isfinite(grad))
    assert np.all(np.abs(dphi - td) <= 64 * EPS * sd) and np.all(np.abs(grad - tg) <= 64 * EPS * sg)
    # that row alone, γ0 = 0: r = m p − y exactly, the variance term vanishes
    one = A[7:8]
    dphi1, grad1 = B.evaluate(one, [1.0], [2.0], 0.0, x, th)
    r = 2.0 * (1.0 if sign > 0 else 0.0) - 1.0
    assert dphi1[1] == 0.0 and dphi1[0] == r * (sign * 750.0 * 0.5) and np.array_equal(grad1, [sign * 750.0 * r, 0.0, 0.0])


@pytest.fixture(scope="module")
def envelope():
    E = B.envelope_case()
    mean, cov = B.posterior_quadrature(E, 8.0, 801)
    return E, mean, cov


def run_envelope(E, seed, **kw):
    args = dict(A=E["A"], y=E["y"], m=E["m"], gamma0=E["gamma0"], lambda_ref=E["lambda_ref"], rho=E["rho"], adapt=True, seed=seed)
    T = kw.pop("T", E["nrec"])
    c = kw.pop("c", E["c"])
    args.update(kw)
    return B.pdmp(0.0, E["x0"], E["th0"], T, c, **args)


def test_quadrature_is_converged(envelope):
    """The product grid [−8, 8]², 801 nodes per axis: twice the width, and twice the density, change the mean and covariance by < 1e-9."""
    E, mean, cov = envelope
    for hw, pts in ((16.0, 1601), (8.0, 1601)):
        m2, c2 = B.posterior_quadrature(E, hw, pts)
        assert np.max(np.abs(m2 - mean)) < 1e-9 and np.max(np.abs(c2 - cov)) < 1e-9


def test_posterior_envelope(envelope):
    """d = 2, n = 30, γ0 = 1, λref = 1, ρ = 0.9, adapt: the envelope form of test/maintest.jl on coordinates standardised by the quadrature
    truth, mean|mean(z)| < 3/√n and mean|cov(z) − I| < 3/√n.
    Seeds 0..19 of the restatement alone.  With 800 records the mean passes on 20 of 20 and the covariance on 18 of 20 (largest figures
    0.070 / 0.117 against 0.106): fewer than 19, so the run was lengthened, the bound kept.  With 1600 records (this test): 20 of 20 and
    20 of 20, largest figures 0.047 / 0.073 against the bound 0.075.  (3200 records: 20 and 19 of 20, 0.027 / 0.054 against 0.053 -- the
    samples are correlated, so the figures shrink with the bound, not faster.)  Asserted on seeds 0, 1, 2."""
    E, mean, cov = envelope
    for seed in B.ENVELOPE_SEEDS:
        r = run_envelope(E, seed)
        assert r["status"] == B.REF_OK and r["nevents"] == E["nrec"] == len(r["t"])
        m, cv, bound = B.envelope_stats(r["x"], mean, cov)
        print("seed %d: mean %.4f cov %.4f bound %.4f" % (seed, m, cv, bound))
        assert m < bound and cv < bound


@pytest.mark.parametrize("kw", [{}, dict(oscn=True), dict(oscn=True, rho=1.0), dict(u_diag=[0.5, 2.0]), dict(L=[[1.2, 0.0], [0.3, 0.8]])])
def test_draw_count_follows_the_draw_table(envelope, kw):
    E = envelope[0]
    r = run_envelope(E, 9, T=250, **kw)
    assert r["status"] == B.REF_OK and r["nrefresh"] > 0 and r["num"] > 0 and r["nacc"] > 0
    assert r["ndraw_main"] == B.predicted_draws(r, E["d"])
    # a width with two Box-Muller rows: d = 100 -> 64 blocks per randn(d)
    rng = np.random.default_rng(1)
    d, n = 100, 130
    A = sp.csc_matrix(rng.standard_normal((n, d)) * (rng.random((n, d)) < 0.1))
    y = (rng.random(n) < 0.5).astype(np.float64)
    r = B.pdmp(0.0, 0.1 * rng.standard_normal(d), rng.standard_normal(d), 40, 40.0, A=A, y=y, gamma0=1.0, lambda_ref=1.0, rho=0.5, seed=2,
               adapt=True, oscn=kw.get("oscn", False))
    assert r["status"] == B.REF_OK and B.draw_blocks(d) == 64 and r["ndraw_main"] == B.predicted_draws(r, d)


def test_gradient_sign_for_a_one_column_design():
    """At x = 0 every p is 1/2: ∇ϕ = Σ a_i (m_i/2 − y_i), the opposite sign of Σ a_i (y_i − m_i/2)."""
    a = np.array([[1.0], [1.0], [1.0], [1.0]])
    m = np.array([2.0, 4.0, 1.0, 3.0])
    for y, s in (([2.0, 4.0, 1.0, 3.0], 1.0), ([0.0, 0.0, 0.0, 0.0], -1.0), ([1.0, 2.0, 0.5, 1.5], 0.0)):
        y = np.array(y)
        dphi, grad = B.evaluate(a, y, m, 0.0, [0.0], [1.0])
        assert np.sign(grad[0]) == -np.sign(np.sum(y - m / 2)) == -s
        assert grad[0] == np.sum(m / 2 - y) and dphi[0] == grad[0] and dphi[1] == np.sum(m) / 4


def test_adapt_multiplies_c_by_factor_at_each_violation(envelope):
    E = envelope[0]
    r = run_envelope(E, 6, T=300, c=1e-20, factor=2.0)
    assert r["status"] == B.REF_OK and r["nviol"] >= 3 and r["nevents"] == 300
    c2 = 1e-20
    for _ in range(r["nviol"]):
        c2 *= 2.0
    assert r["c_final"] == c2
    r3 = run_envelope(E, 6, T=300, c=1e-20, factor=3.0)
    c3 = 1e-20
    for _ in range(r3["nviol"]):
        c3 *= 3.0
    assert r3["c_final"] == c3 and 2 <= r3["nviol"] < r["nviol"]
    bad = run_envelope(E, 6, T=300, c=1e-20, adapt=False)
    assert bad["status"] == B.REF_BOUND_VIOLATED and bad["nviol"] == 1 and bad["nevents"] < 300 and bad["c_final"] == 1e-20


def test_restatement_under_sanitizers():
    """A stand-alone program (the file's own main: d = 8, n = 100, the four flow forms, the pointwise evaluator) under ASan and UBSan."""
    exe = B.build_sanitized_driver()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("status 0 records 200") == 4 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
