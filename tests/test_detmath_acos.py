"""pdmp_acos and pdmp_atan2 of include/pdmp_detmath.h (the two scalars of the arc histogram consumer), as the C statement's library
tests/ref/arc_hist_ref.c compiles them, against mpmath at 60 digits and within the errors the header states and derives (u = 2^-53):

    pdmp_acos(z), −1 < z < 1     |error| < 5u·acos(z);  z >= 1 -> 0, z <= −1 -> π (the double), NaN -> NaN
    pdmp_atan2(y, x), x > 0      |error| < 3.5u·|atan2(y, x)|, or <= 2^-1074 where y / x is subnormal or underflows
                      x < 0      |error| < 10u
                      x == 0     ±π/2 (the doubles: < u), (0, 0) -> +0.0 whatever the signs
    odd in y bit for bit for every y != 0.

No device: the bit-for-bit trace cases of tests/test_gpu_arc_hist.py cover the two functions as compiled into the kernel."""
import itertools
import math

import mpmath as mp
import numpy as np
import pytest

import arc_hist_ref_lib as AH

mp.mp.dps = 60
U = mp.mpf(2) ** -53
TINY = mp.mpf(2) ** -1074


def nudge(v, k):
    for _ in range(abs(k)):
        v = float(np.nextafter(v, math.inf if k > 0 else -math.inf))
    return v


def acos_table():
    zs = [0.0, -0.0, 0.5, -0.5, 5e-324, -5e-324, 2.0 ** -1022, 1e-300, -1e-300, 2.0 ** -30, -2.0 ** -30]
    for k in list(range(1, 54)):
        zs += [1.0 - 2.0 ** -k, -(1.0 - 2.0 ** -k)]
    for b in (0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** -27):  # the reduction breakpoints of pdmp_atan, mapped through sqrt((1 − z)/(1 + z)) = b
        z = float((1 - mp.mpf(b) ** 2) / (1 + mp.mpf(b) ** 2))
        zs += [nudge(z, k) for k in range(-3, 4)] + [nudge(-z, k) for k in range(-3, 4)]
    rng = np.random.default_rng(41)
    zs += list(rng.uniform(-1.0, 1.0, 400)) + list(1.0 - 10.0 ** rng.uniform(-15, 0, 100)) + list(-1.0 + 10.0 ** rng.uniform(-15, 0, 100))
    return [z for z in zs if -1.0 < z < 1.0]


def test_acos_inside_the_stated_error():
    worst = mp.mpf(0)
    for z in acos_table():
        exact = mp.acos(mp.mpf(z))
        err = abs(mp.mpf(AH.acos(z)) - exact)
        assert err < 5 * U * exact, (z, float(err / (U * exact)))
        worst = max(worst, err / (U * exact))
    print("pdmp_acos: worst error %.3f u·acos(z) of the stated 5" % float(worst))


def test_acos_ends_and_nan():
    pi = 3.141592653589793
    for z, want in ((1.0, 0.0), (nudge(1.0, 1), 0.0), (2.0, 0.0), (math.inf, 0.0), (-1.0, pi), (nudge(-1.0, -1), pi), (-7.5, pi), (-math.inf, pi)):
        got = AH.acos(z)
        assert got == want and math.copysign(1.0, got) == 1.0, (z, got)
    assert math.isnan(AH.acos(math.nan))
    assert AH.acos(0.0) == AH.acos(-0.0) == 2.0 * 0.7853981633974483  # 2·atan(1): π/2 rounded


def atan2_table():
    mags = [5e-324, 2.0 ** -1022, 1e-300, 2.0 ** -27, 1e-3, 0.4375, 0.5, 0.6875, 1.0, 1.1875, 1.5, 2.4375, 3.0, 1e3, 2.0 ** 66, 1e300, 1.7e308]
    pts = [(sy * y, sx * x) for y, x in itertools.product(mags, mags) for sy in (1, -1) for sx in (1, -1)]  # all four quadrants
    pts += [(s * y, z) for y in mags for s in (1, -1) for z in (0.0, -0.0)] + [(z, s * x) for x in mags for s in (1, -1) for z in (0.0, -0.0)]  # both axes
    rng = np.random.default_rng(42)
    pts += [tuple(v) for v in rng.standard_normal((600, 2))]
    return pts


def atan2_bound(y, x):
    exact = mp.atan2(mp.mpf(y), mp.mpf(x))
    if x > 0:
        return exact, mp.mpf("3.5") * U * abs(exact) + TINY
    return exact, (10 * U if x < 0 else U)


def test_atan2_inside_the_stated_error():
    worst = {1: mp.mpf(0), -1: mp.mpf(0)}
    for y, x in atan2_table():
        got = AH.atan2(y, x)
        if x == 0.0 and y == 0.0:
            continue
        exact, bound = atan2_bound(y, x)
        if x < 0 and y == 0.0:
            exact = mp.pi  # (a zero's sign is not looked at where x < 0: +π)
        err = abs(mp.mpf(got) - exact)
        assert err <= bound if x > 0 else err < bound, (y, x, got, float(err / U))
        if x != 0:
            worst[int(np.sign(x))] = max(worst[int(np.sign(x))], err / bound)
    print("pdmp_atan2: worst used fraction of the stated error %.3f (x > 0), %.3f (x < 0)" % (float(worst[1]), float(worst[-1])))


def test_atan2_zero_axes_and_nan():
    for y, x in itertools.product((0.0, -0.0), (0.0, -0.0)):
        got = AH.atan2(y, x)
        assert got == 0.0 and math.copysign(1.0, got) == 1.0  # (0, 0) gives 0 whatever the signs
    pio2 = 1.5707963267948966
    for z in (0.0, -0.0):
        assert AH.atan2(3.0, z) == pio2 and AH.atan2(-3.0, z) == -pio2 and AH.atan2(5e-324, z) == pio2
        assert AH.atan2(z, -2.0) == 3.141592653589793
    assert AH.atan2(0.0, 2.0) == 0.0 and math.copysign(1.0, AH.atan2(-0.0, 2.0)) == -1.0
    for y, x in ((math.nan, 1.0), (1.0, math.nan), (math.nan, math.nan), (math.nan, 0.0), (0.0, math.nan), (math.inf, math.inf)):
        assert math.isnan(AH.atan2(y, x))
    assert AH.atan2(math.inf, 1.0) == pio2 and abs(AH.atan2(-math.inf, -1.0) + pio2) < 10 * 2.0 ** -53 and AH.atan2(1.0, math.inf) == 0.0


def test_atan2_is_odd_in_y_bit_for_bit():
    for y, x in atan2_table():
        if y != 0.0 and not (x == 0.0 and y == 0.0):
            a, b = AH.atan2(y, x), AH.atan2(-y, x)
            assert np.float64(a).view(np.uint64) == np.float64(-b).view(np.uint64), (y, x)


def test_known_values():
    assert abs(mp.mpf(AH.acos(0.5)) - mp.pi / 3) < 5 * U * mp.pi / 3
    assert abs(mp.mpf(AH.atan2(1.0, -1.0)) - 3 * mp.pi / 4) < 10 * U
    assert AH.atan2(1.0, 1.0) == 0.7853981633974483
