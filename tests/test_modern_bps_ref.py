"""The sequential restatement of the reference's speed-recorded Bouncy Particle driver (tests/ref/modern_bps_ref.c,
src/not_fact_samplers.jl:151-384) held to the reference's own envelopes and to the structure of its loop -- before the device loop is held
to the restatement bit for bit (tests/test_gpu_modern_bps_parity.py)."""
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import modern_bps_ref_lib as M

ENVELOPE_SEEDS = (0, 1, 2)  # also what the device's envelope test runs


@pytest.fixture(scope="module")
def case(pkg):
    return M.envelope_case(pkg.problems.maintest_precision(8))


def run_form(E, form, seed, T=None, **kw):
    extra = dict(L=E["L"]) if form == "L" else (dict(u_diag=E["u"]) if form == "U" else {})
    extra.update(kw)
    rho = extra.pop("rho", E["rho"])
    c = extra.pop("c", E["c"])
    return M.pdmp(0.0, E["x0"], E["th0"], E["n"] if T is None else T, c, gamma=E["gamma"], lambda_ref=E["lambda_ref"], rho=rho, seed=seed, **extra)


@pytest.mark.parametrize("form", ["L", "U"])
def test_reference_envelopes(case, form):
    """test/maintest.jl:209-242 (L = LowerTriangular(I + 0.4 randn)) and the diagonal-U form with u = 0.5 + k/4: d = 8, the suite's Γ,
    c = 20, λref = 1, ρ = 0.9, n = 800 samples; mean|mean(xs)| < 3/√n and mean|cov(xs) − Γ⁻¹| < 3/√n.
    Seeds 0..19 of the restatement: the L form passes the mean envelope on 20 of 20 and the covariance envelope on 20 of 20; the U form
    20 of 20 and 20 of 20 (largest figures 0.033 / 0.044 and 0.050 / 0.087 against the bound 0.106).  Asserted on seeds 0, 1, 2."""
    for seed in ENVELOPE_SEEDS:
        r = run_form(case, form, seed)
        assert r["status"] == M.REF_OK and r["nevents"] == case["n"] == len(r["t"])
        m, cv, bound = M.envelope_stats(r["x"], case["gamma"])
        print("form %s seed %d: mean %.4f cov %.4f bound %.4f" % (form, seed, m, cv, bound))
        assert m < bound and cv < bound


def test_records_lie_on_the_speed_time_grid(case):
    """V ≡ 1 (L form): the k-th record lies at t0 + k/λref up to accumulated rounding."""
    for lam in (1.0, 3.0):
        r = M.pdmp(0.25, case["x0"], case["th0"], 400, case["c"], gamma=case["gamma"], lambda_ref=lam, rho=0.9, L=case["L"], seed=5)
        assert r["status"] == M.REF_OK
        k = np.arange(1, 401)
        assert np.all(np.abs(r["t"] - (0.25 + k / lam)) <= 1e-9 * (1 + r["t"]))
    # the U form records in proportion to speed: not on that grid
    r = run_form(case, "U", 5)
    assert not np.all(np.abs(r["t"] - np.arange(1, case["n"] + 1)) <= 1e-9 * (1 + r["t"]))


def test_int_T_counts_records_and_float_T_ends_past_T(case):
    for form in ("I", "L", "U"):
        r = run_form(case, form, 3, T=137)
        assert r["status"] == M.REF_OK and r["nevents"] == 137 and len(r["t"]) == 137
        r = run_form(case, form, 3, T=50.5)
        assert r["status"] == M.REF_OK and r["nevents"] == len(r["t"])
        assert r["t"][-1] >= 50.5 and np.all(r["t"][:-1] < 50.5) and r["t_final"] == r["t"][-1]
        assert np.all(np.diff(r["t"]) > 0)
        # both limits: whichever comes first
        a = run_form(case, form, 3, T=(50.5, 10))
        assert a["nevents"] == 10 and np.array_equal(a["t"], r["t"][:10])
        b = run_form(case, form, 3, T=(r["t"][4], 1000))
        assert b["nevents"] == 5 and np.array_equal(b["x"], r["x"][:5])


def test_oscn_with_rho_one_is_the_pure_reflection(case):
    """ρ = 1 and oscn: v − 2vₚ, which is reflect! with L = I up to the rounding of its two forms, and no normals are drawn -- the draw
    count is that of a run without oscn draws, and |θ| is preserved by every bounce (refreshments with ρ = 1 leave θ as it is)."""
    r = run_form(case, "I", 4, T=200, oscn=True, rho=1.0)
    assert r["status"] == M.REF_OK and r["nacc"] > 50 and r["noscn_draws"] == 0
    assert r["ndraw_main"] == M.predicted_draws(r, case["d"])
    n0 = np.linalg.norm(case["th0"])
    assert np.allclose(np.linalg.norm(r["theta"], axis=1), n0, rtol=1e-9)
    # the first bounce of the plain reflection lies where oscn's does, and gives the same θ to rounding
    p = run_form(case, "I", 4, T=200, rho=1.0)
    k = int(np.argmax(np.any(r["theta"] != case["th0"], axis=1)))
    assert np.allclose(r["theta"][k], p["theta"][k], rtol=1e-12, atol=1e-14) and r["t"][k] == p["t"][k]
    # ρ < 1 draws a randn(d) per accepted bounce
    q = run_form(case, "I", 4, T=200, oscn=True, rho=0.9)
    assert q["noscn_draws"] == q["nacc"] > 0 and q["ndraw_main"] == M.predicted_draws(q, case["d"])


def test_adapt_multiplies_c_by_factor_at_each_violation(case):
    """On a Gaussian target the bound a + bτ is the rate plus c exactly, so only a c below the rounding of the rate is ever violated:
    c = 1e-20 is, until the factor has lifted it there."""
    r = run_form(case, "L", 6, T=300, c=1e-20, adapt=True, factor=2.0)
    assert r["status"] == M.REF_OK and r["nviol"] >= 3 and r["nevents"] == 300
    assert r["c_final"] == 1e-20 * 2.0 ** r["nviol"]
    r3 = run_form(case, "L", 6, T=300, c=1e-20, adapt=True, factor=3.0)
    c3 = 1e-20
    for _ in range(r3["nviol"]):
        c3 *= 3.0
    assert r3["c_final"] == c3 and 2 <= r3["nviol"] < r["nviol"]
    # the same start without adapt: the reference's error
    bad = run_form(case, "L", 6, T=300, c=1e-20)
    assert bad["status"] == M.REF_BOUND_VIOLATED and bad["nviol"] == 1 and bad["nevents"] < 300 and bad["c_final"] == 1e-20


@pytest.mark.parametrize("form,kw", [("I", {}), ("L", {}), ("U", {}), ("I", dict(oscn=True)), ("I", dict(oscn=True, rho=0.0))])
def test_draw_count_follows_the_draw_table(case, form, kw):
    for d in (8,):
        r = run_form(case, form, 9, T=250, **kw)
        assert r["status"] == M.REF_OK
        assert r["nrefresh"] > 0 and r["num"] > 0 and r["nexpire"] > 0
        assert r["ndraw_main"] == M.predicted_draws(r, d)
    # a width with two Box-Muller rows: d = 100 -> 64 blocks per randn(d)
    d = 100
    G = sp.diags([np.full(d - 1, -0.4), np.full(d, 2.0), np.full(d - 1, -0.4)], [-1, 0, 1], format="csc")
    rng = np.random.default_rng(1)
    r = M.pdmp(0.0, rng.standard_normal(d), rng.standard_normal(d), 60, 40.0, gamma=G, lambda_ref=1.0, rho=0.5, seed=2,
               u_diag=(0.5 + rng.random(d)) if form == "U" else None, oscn=kw.get("oscn", False))
    assert r["status"] == M.REF_OK and M.draw_blocks(d) == 64 and r["ndraw_main"] == M.predicted_draws(r, d)


def test_restatement_under_sanitizers():
    """A stand-alone program (the file's own main: d = 8, both forms, a dense L, oscn) under AddressSanitizer and UBSan."""
    exe = M.build_sanitized_driver()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("status 0 records 200") == 4 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
