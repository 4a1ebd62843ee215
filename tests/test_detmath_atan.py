"""pdmp_atan (include/pdmp_detmath.h) and the freezing times built on it, host side: the values the device must reproduce bit for bit
(tests/test_gpu_sticky_bps_parity.py) held to mpmath here."""
import math

import mpmath as mp
import numpy as np

import sticky_ref_lib as R

mp.mp.prec = 200
EPS = 2.0 ** -53


def atan_table():
    """±0, subnormals, both sides of every reduction breakpoint (2^-27, 7/16, 11/16, 19/16, 39/16, 2^66), 2^±k sweeps, values above 2^66."""
    pts = [0.0, 5e-324, 1e-320, 2.2250738585072014e-308 / 2, 2.2250738585072014e-308]
    for b in (2.0 ** -27, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 66):
        pts += [np.nextafter(b, 0.0), b, np.nextafter(b, np.inf)]
    pts += list(2.0 ** np.arange(-80.0, 81.0))
    pts += list(1.37 * 2.0 ** np.arange(-60.0, 61.0))
    pts += [2.0 ** 67, 1e30, 1e300, 1.7976931348623157e308]
    pts += list(np.random.default_rng(7).uniform(0.0, 4.0, 2000))
    pts = np.unique(np.array(pts, dtype=np.float64))
    return pts  # ascending, non-negative


def ulp(v):
    return float(np.spacing(abs(v))) if v != 0 else 5e-324


def test_atan_is_within_one_ulp_of_mpmath_odd_and_monotone():
    x = atan_table()
    y = R.ref_atan(x)
    yn = R.ref_atan(-x)
    worst = 0.0
    for a, b in zip(x, y):
        err = abs(mp.mpf(float(b)) - mp.atan(mp.mpf(float(a)))) / ulp(float(b))
        worst = max(worst, float(err))
        assert err <= 1, (a, b, float(err))
    print("pdmp_atan: worst error %.3f ulp over %d points" % (worst, len(x)))
    assert np.array_equal(yn.view(np.uint64), (-y).view(np.uint64))  # odd, including -0 -> -0
    assert np.all(np.diff(y) >= 0)                                    # monotone on the ascending table
    assert np.all(np.diff(yn) <= 0)


def test_atan_special_values():
    y = R.ref_atan([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** 66, -2.0 ** 70])
    assert y[0] == 0 and not np.signbit(y[0]) and y[1] == 0 and np.signbit(y[1])
    assert y[2] == np.pi / 2 and y[3] == -np.pi / 2 and np.isnan(y[4]) and y[5] == np.pi / 2 and y[6] == -np.pi / 2


def first_zero(x, th, mu):
    """First τ > 0 with (x − μ) cos τ + θ sin τ + μ = 0 (the rotated coordinate, src/ss_not_fact.jl:88-97), by mpmath: the candidates
    φ ± acos(−μ/R) (mod 2π) refined with findroot; Inf when |μ| > R.  τ = 0 itself (x = 0) does not count."""
    x, th, mu = mp.mpf(x), mp.mpf(th), mp.mpf(mu)
    A = x - mu
    Rr = mp.sqrt(A * A + th * th)
    if abs(mu) > Rr:
        return mp.inf
    phi = mp.atan2(th, A)
    g = lambda s: A * mp.cos(s) + th * mp.sin(s) + mu
    cands = []
    for sgn in (1, -1):
        s = (phi + sgn * mp.acos(-mu / Rr)) % (2 * mp.pi)
        if abs(mu) < Rr:  # a simple zero: polish it
            s = mp.findroot(g, s) % (2 * mp.pi)
        if s < mp.mpf(10) ** -40 or 2 * mp.pi - s < mp.mpf(10) ** -40:
            s = 2 * mp.pi
        cands.append(s)
    return min(cands)


def test_boomerang_freezing_time_against_root_finding():
    """Tolerance, derived from the formula's operations (ε = 2^-53, every + − × ÷ sqrt correctly rounded, pdmp_atan within 1 ulp):
      μ = 0:  q = x/θ (ε relative); atan moves it by at most |q|/(1+q²) ε <= ε/2, plus its own ulp (ε·π/2 at most); π − · rounds once more
              (ε·π) and Float64(π) is off by 1.3e-16 < 2ε:  |error| <= ε(1/2 + π/2 + π + 2) < 7ε.
      μ ≠ 0:  u = x² − 2μx + θ² carries at most 4ε·S absolute, S = x² + |2μx| + θ²; sqrt(u) then sqrt(u)(ε + 2εS/u); the numerator
              n = sqrt(u) ∓ θ rounds once more, the denominator 2μ − x once, the quotient once: relative error of q at most
              ε(3 + K), K = sqrt(u)(1 + 2S/u)/|n| -- the one place where cancellation enters, computed per point.  atan halves it at
              worst, × 2 restores it; atan's own ulp (2 × ε·π/2), the addition of 2π (ε·2π) and Float64(2π)'s error (2.5e-16 < 3ε):
              |error| <= ε(3 + K + π + 2π + 3) < ε(16 + K).
    With K of order one that is a few ulp of a result of order one."""
    rng = np.random.default_rng(11)
    cases = []
    for _ in range(300):
        x, th = rng.normal(), rng.normal()
        cases.append((x, th, 0.0))                            # μ = 0
        cases.append((x, th, rng.normal() * 0.5))             # μ ≠ 0 (both u >= 0 and u < 0 occur)
        cases.append((0.0, th, rng.normal() * 0.5))           # x = 0: the zero at τ = 0 is not the answer
    cases.append((0.0, 0.7, 0.0))                             # μ = 0, x = 0: half a rotation
    n_inf = n_x0 = n_mu0 = n_gen = n_skip = 0
    for x, th, mu in cases:
        got = float(R.freezing_time_boomerang([x], [th], [mu])[0])
        want = first_zero(x, th, mu)
        if want == mp.inf:
            assert got == np.inf, (x, th, mu, got)
            n_inf += 1
            continue
        if mu == 0.0:
            tol = 7 * EPS
            n_mu0 += 1
        else:
            u = x * x - 2 * mu * x + th * th
            S = x * x + abs(2 * mu * x) + th * th
            su = np.sqrt(u)
            # K of the branch whose value is the answer (for x = 0 the other numerator is exactly 0 and yields t = 0, which max() drops)
            den = 2 * mu - x
            br = []
            for n, sg in ((su - th, 2.0), (su + th, -2.0)):
                v = sg * math.atan(n / den) if den != 0 else np.nan
                br.append((abs((v if v >= 0 else v + 2 * math.pi) - got), abs(n)))
            n_abs = min(br)[1]
            K = su * (1 + 2 * S / u) / n_abs if u > 0 and n_abs > 0 else np.inf
            if not np.isfinite(K) or K > 1e6:
                n_skip += 1  # (a point on the cancellation itself says nothing about the formula)
                continue
            tol = (16 + K) * EPS
            n_x0 += x == 0.0
            n_gen += x != 0.0
        assert abs(mp.mpf(got) - want) <= tol, (x, th, mu, got, float(want), float(abs(mp.mpf(got) - want)), tol)
    assert n_inf > 5 and n_x0 > 50 and n_mu0 > 100 and n_gen > 100  # every branch was exercised
    # K > 1e6 needs |sqrt(u) ∓ θ| below ~3e-6 sqrt(u): a set of probability ~1e-5 under these normal draws, i.e. 0.006 points expected of 600
    assert n_skip <= 1, n_skip


def test_linear_freezing_time():
    """freezing_time(x, θ, ::BouncyParticle) (src/ss_fact.jl:10-16): Inf when θx >= 0 (sic), else −x/θ."""
    x = np.array([1.0, -1.0, 1.0, 0.0, -0.0, 2.0])
    th = np.array([-0.5, 0.5, 0.5, 1.0, -1.0, -4.0])
    assert np.array_equal(R.freezing_time_linear(x, th), np.array([2.0, 2.0, np.inf, np.inf, np.inf, 0.5]))
