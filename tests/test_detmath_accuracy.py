"""Accuracy of the shared numerical contract (include/pdmp_detmath.h) and of the oracle's scalar helpers against exact references
(mpmath at high precision), at the edges tabulated in detmath_tables.py.  test_gpu_detmath.py then holds every device copy to these host
functions bit for bit, so what is pinned here holds on the device too."""
import hashlib
import math

import mpmath as mp
import numpy as np
import pytest
from scipy import stats

import detmath_tables as T
import oracle_lib as O

mp.mp.prec = 256
EPS = 2.0 ** -52


def L():
    return O.lib()


def ulp(y):
    """spacing of the doubles at the exact value y (mpf): 2^(e-52), and 2^-1074 in the subnormal range"""
    y = abs(mp.mpf(y))
    if y == 0 or y < mp.mpf(2) ** -1022:
        return mp.mpf(2) ** -1074
    return mp.mpf(2) ** (mp.floor(mp.log(y, 2)) - 52)


def ulp_err(got, exact):
    return float(abs(mp.mpf(got) - exact) / ulp(exact))


# ------------------------------------------------------------------------------------------------------------------ u01, log, exp

def test_u01_extremes():
    bits = T.u01_bits()
    u = np.array([L().orc_bits_to_u01(int(b)) for b in bits])
    assert u.min() >= T.U_MIN and u.max() <= T.U_MAX
    assert L().orc_bits_to_u01(0) == T.U_MIN and L().orc_bits_to_u01((1 << 64) - 1) == T.U_MAX
    assert L().orc_bits_to_u01(0xFFF) == T.U_MIN and L().orc_bits_to_u01(0x1000) == 3 * T.U_MIN  # only the top 52 bits count
    m = (bits >> np.uint64(12)).astype(np.float64)
    assert np.array_equal(u, (m + 0.5) * 2.0 ** -52)  # exact: (m + 1/2) 2^-52


def test_log_within_one_ulp():
    worst = 0.0
    for x in T.log_inputs():
        e = ulp_err(L().orc_log(float(x)), mp.log(mp.mpf(float(x))))
        worst = max(worst, e)
        assert e <= 1.0, (x, e)
    assert worst > 0.5  # (the table reaches the hard cases)


def test_log_domain_is_normal_numbers():
    """pdmp_log is documented for positive normal doubles; below that it does not follow log.  Pinned, not fixed: no caller gets there."""
    assert L().orc_log(T.MIN_NORMAL) == pytest.approx(-708.3964185322641, abs=1e-12)
    for x in (1e-310, T.TINY, 0.0):
        assert -709.1 < L().orc_log(x) < -709.0  # the true log(1e-310) is -713.8


def test_exp_within_one_ulp_and_subnormal_spacing():
    worst = 0.0
    for x in T.exp_inputs():
        x = float(x)
        if not math.isfinite(x) or x > T.EXP_HI or x < T.EXP_LO:
            continue
        e = ulp_err(L().orc_exp(x), mp.exp(mp.mpf(x)))  # (subnormal results: in units of 2^-1074)
        worst = max(worst, e)
        assert e <= 1.0, (x.hex(), L().orc_exp(x), e)
    assert worst > 0.5


def test_exp_saturates_exactly_at_the_fdlibm_thresholds():
    assert T.EXP_HI == float.fromhex("0x1.62e42fefa39efp+9") and T.EXP_LO == float.fromhex("-0x1.74910d52d3051p+9")
    hi_up, lo_down = math.nextafter(T.EXP_HI, math.inf), math.nextafter(T.EXP_LO, -math.inf)
    assert math.isfinite(L().orc_exp(T.EXP_HI)) and L().orc_exp(T.EXP_HI) == pytest.approx(1.7976931348622732e308, rel=1e-15)
    assert L().orc_exp(hi_up) == math.inf and float(mp.exp(mp.mpf(hi_up))) == math.inf
    assert L().orc_exp(T.EXP_LO) == T.TINY and L().orc_exp(lo_down) == 0.0
    assert float(mp.exp(mp.mpf(lo_down))) == 0.0  # (the correctly rounded value is 0 there too)
    assert L().orc_exp(math.inf) == math.inf and L().orc_exp(-math.inf) == 0.0 and math.isnan(L().orc_exp(math.nan))
    assert L().orc_exp(0.0) == 1.0 and L().orc_exp(-0.0) == 1.0


# ------------------------------------------------------------------------------------------------------------------ sincos

SINCOS_ABS = 2.5e-16  # measured 1.9e-16 (both outputs, whole domain, tables below); stated in pdmp_detmath.h


def test_sincos_absolute_error_over_the_whole_domain():
    worst = 0.0
    for x in T.sincos_inputs():
        x = float(x)
        if not abs(x) <= T.SINCOS_MAX:
            continue
        s, c = O.sincos(x)
        es = abs(mp.mpf(s) - mp.sin(mp.mpf(x)))
        ec = abs(mp.mpf(c) - mp.cos(mp.mpf(x)))
        worst = max(worst, float(es), float(ec))
        assert es <= SINCOS_ABS and ec <= SINCOS_ABS, (x, s, c, float(es), float(ec))
        if abs(x) < 1e-8:  # small arguments: sin x = x and cos x = 1 to the last bit (sin(-0) is +0: the reduction subtracts 0 * pi/2)
            assert s == x and c == 1.0, (x, s, c)
    assert worst > 1e-16


def test_sincos_nan_past_the_domain_and_for_nonfinite():
    assert all(math.isfinite(v) for v in O.sincos(T.SINCOS_MAX) + O.sincos(-T.SINCOS_MAX))
    for x in (math.nextafter(T.SINCOS_MAX, math.inf), -math.nextafter(T.SINCOS_MAX, math.inf), 2e9, 1e10, 1e300, T.MAX, math.inf,
              -math.inf, math.nan):
        s, c = O.sincos(x)
        assert math.isnan(s) and math.isnan(c), (x, s, c)


def test_sincos_bits_unchanged_below_two_pow_20_pi_half():
    """Below 2^20 pi/2 the reduction is the one every golden and parity result was made with: its bits are pinned (a digest of 60000
    evaluations), so that a change of that path shows up here and not as a moved fixture."""
    r = np.random.default_rng(2024)
    xs = np.concatenate([r.uniform(-T.SINCOS_SPLIT, T.SINCOS_SPLIT, 20000), r.uniform(-50, 50, 20000),
                         r.uniform(-1, 1, 19998) * 2.0 ** r.integers(-40, 0, 19998), [T.SINCOS_SPLIT, -T.SINCOS_SPLIT]])
    h = hashlib.sha256()
    for x in xs:
        s, c = O.sincos(float(x))
        h.update(np.array([s, c]).tobytes())
    assert h.hexdigest()[:16] == "0d5f99bb76071a56"


def test_sincos2pi_octant_points_and_accuracy():
    r2 = math.sqrt(0.5)
    for k in range(8):
        s, c = O.sincos2pi(k / 8)
        ts, tc = mp.sinpi(mp.mpf(k) / 4), mp.cospi(mp.mpf(k) / 4)
        if k % 2 == 0:  # exactly 0 and +-1
            assert (s, c) == (float(ts), float(tc)), (k, s, c)
        else:  # +-sqrt(1/2) within an ulp, the right signs
            assert ulp_err(abs(s), mp.sqrt(0.5)) <= 1 and ulp_err(abs(c), mp.sqrt(0.5)) <= 1, (k, s, c)
            assert np.sign(s) == np.sign(float(ts)) and np.sign(c) == np.sign(float(tc)), (k, s, c)
    worst = 0.0
    for v in T.sincos2pi_inputs():
        s, c = O.sincos2pi(float(v))
        es = float(abs(mp.mpf(s) - mp.sinpi(2 * mp.mpf(float(v)))))
        ec = float(abs(mp.mpf(c) - mp.cospi(2 * mp.mpf(float(v)))))
        worst = max(worst, es, ec)
        assert es <= 2.5e-16 and ec <= 2.5e-16, (v, es, ec)
    assert worst > 5e-17


# ------------------------------------------------------------------------------------------------------------------ Box-Muller

def _bm_exact(u1, u2):
    rad = mp.sqrt(-2 * mp.log(mp.mpf(u1)))
    return rad, rad * mp.cospi(2 * mp.mpf(u2)), rad * mp.sinpi(2 * mp.mpf(u2))


def test_box_muller_both_branches_within_a_few_ulp():
    """z = rad * cos / sin(2 pi u2): a few ulp of rad (the trigonometric factor is accurate in absolute terms, not near its zeros)"""
    a, b = T.randn_inputs()
    for u1, u2 in zip(a.tolist(), b.tolist()):
        rad, z0, z1 = _bm_exact(u1, u2)
        g0, g1 = O.randn2_from_u(u1, u2)
        assert L().orc_randn_from_u(u1, u2) == g0  # pdmp_randn is the cosine branch of pdmp_randn2
        tol = 4 * ulp(rad)
        assert abs(mp.mpf(g0) - z0) <= tol and abs(mp.mpf(g1) - z1) <= tol, (u1, u2, g0, g1)
    z0max, _ = O.randn2_from_u(T.U_MIN, T.U_MIN)
    assert z0max == pytest.approx(math.sqrt(106 * math.log(2)), rel=1e-15)  # the largest |z| the stream can produce: sqrt(-2 log 2^-53)


def test_box_muller_distribution_per_branch():
    n = 20000
    z = np.array([O.randn2(0xB0C5, 0, k) for k in range(n)])
    for col in (0, 1):
        assert stats.kstest(z[:, col], "norm").pvalue > 1e-3, col
    assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 4 / math.sqrt(n)
    assert abs(np.corrcoef(z[:, 0] ** 2, z[:, 1] ** 2)[0, 1]) < 4 / math.sqrt(n)
    assert all(O.randn2(0xB0C5, 0, k)[0] == L().orc_randn(0xB0C5, 0, k) for k in range(200))


# ------------------------------------------------------------------------------------------------------------------ randint

def _bits64(seed, stream, n):
    r = O.philox([n & 0xFFFFFFFF, n >> 32, stream, 0], [seed & 0xFFFFFFFF, seed >> 32])
    return (int(r[0]) << 32) | int(r[1])


def test_randint_is_multiply_shift():
    seeds, draws, ns = T.randint_inputs()
    for s, d, n in zip(seeds.tolist(), draws.tolist(), ns.tolist()):
        got = L().orc_randint(int(s), 1, int(d), int(n))
        assert got == ((_bits64(int(s), 1, int(d)) >> 32) * int(n)) >> 32, (s, d, n)
        assert 0 <= got < n
    assert all(L().orc_randint(7, 1, k, 1) == 0 for k in range(100))


@pytest.mark.parametrize("n", T.RANDINT_N[1:])
def test_randint_counts(n):
    draws = np.array([L().orc_randint(0x5EED, 1, k, n) for k in range(30000)], dtype=np.int64)
    assert draws.min() >= 0 and draws.max() < n
    bins = min(n, 16)
    counts = np.bincount(draws * bins // n, minlength=bins)
    assert stats.chisquare(counts).pvalue > 1e-3, counts


# ------------------------------------------------------------------------------------------------------------------ sigmoid, pos

def test_sigmoid_and_pos():
    for x in T.sigmoid_inputs():
        x = float(x)
        got = L().orc_sigmoid(x)
        if math.isnan(x):
            assert math.isnan(got)
            continue
        exact = 1 / (1 + mp.exp(-mp.mpf(x))) if math.isfinite(x) else mp.mpf(x > 0)
        if x < -T.EXP_HI:  # exp(-x) overflows to +Inf and 1 / Inf is 0, where the true value is a subnormal number or 0
            assert got == 0.0 and exact < T.MIN_NORMAL, (x, got)
            continue
        assert abs(mp.mpf(got) - exact) <= 2 * ulp(exact), (x, got)
    assert L().orc_sigmoid(0.0) == 0.5 and L().orc_sigmoid(-0.0) == 0.5
    assert L().orc_sigmoid(710.0) == 1.0 and L().orc_sigmoid(math.inf) == 1.0
    assert L().orc_sigmoid(-710.0) == 0.0 and L().orc_sigmoid(-math.inf) == 0.0  # exp(710) = Inf: 1 / Inf
    assert 0.0 < L().orc_sigmoid(-709.0) < 1.3e-308 and L().orc_sigmoid(-T.EXP_HI) > 0.0
    assert L().orc_sigmoid(math.nextafter(-T.EXP_HI, -math.inf)) == 0.0
    for x in T.pos_inputs():
        got = L().orc_pos(float(x))
        if math.isnan(x):
            assert math.isnan(got)
        else:
            assert got == max(0.0, x) and math.copysign(1, got) == 1.0, (x, got)  # pos(-0.0) is +0.0


# ------------------------------------------------------------------------------------------------------------------ poisson_time

def _pt_exact(a, b, u):
    """exact root s of the integral of (a + b t)^+ over [0, s] = -log u; math.inf where there is none or it exceeds the largest double"""
    E = -mp.log(mp.mpf(u))
    a, b = mp.mpf(a), mp.mpf(b)
    if b == 0:
        return E / a if a > 0 else mp.inf
    if b > 0 and a < 0:
        return -a / b + mp.sqrt(2 * E / b)
    if b < 0 and (a <= 0 or E > a * a / (-2 * b)):
        return mp.inf
    return 2 * E / (a + mp.sqrt(a * a + 2 * b * E))  # the smaller root of b s^2 / 2 + a s = E, free of cancellation


def _pt_bound(a, b, u):
    """rounding error bound of the reference's formula sqrt(r^2 - q) - r (r = a/b, q = 2 log(u)/b) from its conditioning: a few ulp of
    every term, and the relative error of r^2 - q amplified by (r^2 + |q|) / S where it cancels (S = sqrt(|r^2 - q|))"""
    E = -mp.log(mp.mpf(u))
    if b == 0:
        return 4 * EPS * abs(E / a) + 4 * T.TINY
    r = mp.mpf(a) / b
    q = -2 * E / b
    D = (-q) if (b > 0 and a < 0) else r * r - q
    S = mp.sqrt(abs(D))
    if S == 0:
        return mp.inf
    # (intermediates in the subnormal range carry an absolute error of up to 2^-1075 each)
    return 8 * EPS * (abs(r) + S + (r * r + abs(q)) / S) + 4 * T.TINY * (1 + 1 / S)


def _classify(v):
    return "nan" if math.isnan(v) else "inf" if math.isinf(v) else "finite"


def overflows(a, b, u):
    """the reference's formula, and so every copy, returns an infinite time for a finite one where (a/b)^2 overflows (|b| < a 1e-154: the
    true time is about -log(u)/a) or 2 log(u) / b does (tiny b: the true time can still be finite).  It is +Inf, -Inf in the b < 0
    branch (-sqrt(Inf) - a/b: a time in the past), NaN where a/b itself overflows (Inf - Inf); and +Inf where a*a overflows in the
    admissibility test of the b < 0 branch."""
    if b == 0 or not (math.isfinite(a) and math.isfinite(b)):
        return False
    r, q = a / b, L().orc_log(u) * 2.0 / b
    return (math.isinf(r * r) and not (b > 0 and a < 0)) or math.isinf(q) or (b < 0 < a and math.isinf(a * a))  # (b > 0 > a: sqrt(-q) - r)


DOCUMENTED = {(1.0, 1e-160, 0.5): math.inf, (1.0, 1e-155, 0.5): math.inf, (-1e-10, 1e-310, 0.5): math.inf, (-0.0, 1e-310, 0.5): math.inf,
              (0.5, -1e-160, 0.5): -math.inf, (0.5, 1e-310, 0.5): math.nan}


def test_poisson_time_against_the_exact_root():
    a, b, u = T.poisson_inputs(L().orc_log)
    nfinite = ncancel = ndev = 0
    for ai, bi, ui in zip(a.tolist(), b.tolist(), u.tolist()):
        got = O.poisson_time(ai, bi, ui)
        if not (math.isfinite(ai) and math.isfinite(bi)):
            continue  # non-finite rates: the next test
        exact = _pt_exact(ai, bi, ui)
        want = "inf" if (exact == mp.inf or abs(exact) > T.MAX) else "finite"
        key = (ai, bi, ui)
        if bi < 0 < ai and abs(-mp.log(mp.mpf(ui)) - mp.mpf(ai) ** 2 / (-2 * mp.mpf(bi))) <= 16 * EPS * -mp.log(mp.mpf(ui)):
            continue  # on the admissibility bound to rounding: decided by the computed test (test_poisson_time_admissibility_boundary)
        if want == "finite" and overflows(ai, bi, ui):
            assert not math.isfinite(got), (key, got)
            ndev += 1
            continue
        if want == "finite" and _classify(got) == "nan":
            # the b < 0 admissibility boundary: the test lets -L equal its bound, where r^2 - q rounds to a tiny negative number
            assert bi < 0 < ai and float(mp.mpf(ai) / bi) ** 2 - 2 * L().orc_log(ui) / bi < 0, (key, got)
            continue
        assert _classify(got) == want, (key, got, exact)
        if want == "finite":
            err = abs(mp.mpf(got) - exact)
            assert err <= _pt_bound(ai, bi, ui) + 2 * ulp(exact), (key, got, float(exact), float(err))
            nfinite += 1
            ncancel += err > 64 * ulp(exact)
    assert nfinite > 2000 and ncancel > 0 and ndev >= len(DOCUMENTED)  # (the table has rows where the formula cancels and overflows)


def test_poisson_time_reference_formula_deviations_are_as_documented():
    # b -> 0+ with a > 0 cancels in sqrt((a/b)^2 + 2E/b) - a/b: a = 1, b = 1e-12 loses 1e-5 .. 1e-2 relative
    rel = []
    for k in range(200):
        u = L().orc_u01(0xCA7, 0, k)
        got, exact = O.poisson_time(1.0, 1e-12, u), _pt_exact(1.0, 1e-12, u)
        rel.append(float(abs(mp.mpf(got) - exact) / exact))
    assert 1e-5 < max(rel) < 1e-2 and np.median(rel) > 1e-6, (max(rel), np.median(rel))
    for key, value in DOCUMENTED.items():  # +-Inf where the time is finite
        got = O.poisson_time(*key)
        assert overflows(*key) and (got == value or math.isnan(got) and math.isnan(value)) and mp.isfinite(_pt_exact(*key)), key


def test_poisson_time_admissibility_boundary():
    """b < 0 < a: the time is finite iff -L <= -(a*a)/b + (a*a)/(2*b) as computed.  At the bound it is the finite root (or the NaN of
    the sqrt of a rounded tiny negative), one ulp past it +Inf."""
    bd = T.poisson_boundary(L().orc_log)
    assert len(bd["at"]) >= 5 and len(bd["above"]) >= 5 and len(bd["below"]) >= 5
    for row in bd["at"] + bd["above"]:
        assert not math.isinf(O.poisson_time(*row)), row
    for row in bd["below"]:
        assert O.poisson_time(*row) == math.inf, row
    assert any(math.isfinite(O.poisson_time(*row)) for row in bd["at"])


def test_poisson_time_nonfinite_rates():
    """what the reference's formula gives for NaN and +-Inf rates (no caller produces them; pinned so that every copy agrees)"""
    pt = O.poisson_time
    assert math.isnan(pt(math.nan, 1.0, 0.5)) and pt(math.nan, 0.0, 0.5) == math.inf and pt(math.nan, -1.0, 0.5) == math.inf
    assert pt(1.0, math.nan, 0.5) == math.inf and pt(-1.0, math.nan, 0.5) == math.inf
    assert math.isnan(pt(math.inf, 1.0, 0.5)) and pt(-math.inf, 1.0, 0.5) == math.inf
    assert pt(math.inf, 0.0, 0.5) == 0.0 and pt(-math.inf, 0.0, 0.5) == math.inf
    assert pt(1.0, math.inf, 0.5) == 0.0 and pt(1.0, -math.inf, 0.5) == math.inf
    assert pt(0.0, 0.0, 0.5) == math.inf and pt(-0.0, -0.0, 0.5) == math.inf and pt(0.0, -1.0, 0.5) == math.inf
