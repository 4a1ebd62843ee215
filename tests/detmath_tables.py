"""Input tables for the scalar functions of the numerical contract (include/pdmp_detmath.h) and of the device's private copies of
poisson_time, sigmoid and pos: the edges where such code goes wrong -- thresholds and one ulp either side, signed zeros, subnormals,
overflow, NaN and +-Inf -- plus a seeded random body.  Shared by tests/test_detmath_accuracy.py (host against mpmath) and
tests/test_gpu_detmath.py (device against host, bit for bit)."""
import math

import numpy as np

INF, NAN = math.inf, math.nan
TINY = 5e-324                   # smallest subnormal
MIN_NORMAL = 2.2250738585072014e-308
MAX = 1.7976931348623157e308
U_MIN, U_MAX = 2.0 ** -53, 1 - 2.0 ** -53  # the extremes pdmp_u01 can return
EXP_HI = 709.782712893384       # pdmp_exp: +Inf above (fdlibm o_threshold)
EXP_LO = -745.1332191019411     # pdmp_exp: 0 below (fdlibm u_threshold)
SINCOS_MAX = 2.0 ** 30          # pdmp_sincos: NaN beyond
SINCOS_SPLIT = float.fromhex("0x1.921fb54442d18p+20")  # pdmp_sincos: the 33-bit reduction up to here, the 23-bit one above


def around(x, k=1):
    """x and its k neighbours on either side"""
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo, hi = math.nextafter(lo, -INF), math.nextafter(hi, INF)
        out += [lo, hi]
    return out


def _rng(tag):
    return np.random.default_rng(0xDE7 + tag)


def u01_bits():
    """64-bit inputs of pdmp_bits_to_u01 (as uint64)"""
    fixed = [0, 1, 0xFFF, 0x1000, 0x1FFF, 1 << 63, (1 << 64) - 1, (1 << 64) - 0x1000, 0xFFFFFFFFFFFFE000]
    return np.concatenate([np.array(fixed, dtype=np.uint64), _rng(1).integers(0, 1 << 64, 2000, dtype=np.uint64, endpoint=False)])


def log_inputs():
    xs = [U_MIN, U_MAX, 0.5, 1.0, 2.0, MIN_NORMAL, MAX, 1e-300, 1e300]
    for e in range(-60, 61, 3):  # the sqrt(2) split of the reduction, at many exponents
        m = math.sqrt(2.0) * 2.0 ** e
        xs += around(m, 2) + around(m / math.sqrt(2.0), 1)
    # 0x3ff6a09c... is where (hx + 0x95f64) carries into bit 20: both sides
    for hx in (0x3FF6A09B, 0x3FF6A09C, 0x3FF6A09D):
        for lx in (0, 0xFFFFFFFF):
            xs.append(float(np.array([(hx << 32) | lx], dtype=np.uint64).view(np.float64)[0]))
    # the adaptscale ratios (1 + acc) / (1 + 0.3 t), 1 + t and log(2) (oracle/pdmp_oracle.c, adaptscale)
    r = _rng(2)
    acc = r.integers(0, 10000, 400)
    t = r.uniform(0, 1e4, 400)
    xs += list((1.0 + acc) / (1.0 + 0.3 * t)) + list(1.0 + t)
    xs += list(r.random(1000) * (U_MAX - U_MIN) + U_MIN) + list(np.exp(r.uniform(-700, 700, 1000)))
    return np.array(xs)


def exp_inputs():
    xs = [0.0, -0.0, 1.0, -1.0, INF, -INF, NAN, TINY, -TINY, 1e-300, -1e-300]
    xs += around(EXP_HI, 2) + around(EXP_LO, 2)
    ln2 = math.log(2.0)
    # k = round(x / ln2) changes at (k + 1/2) ln2: the general scaling, the two-step scaling for subnormal results (k < -1021) and k > 1023
    for k in list(range(-1080, -1015)) + [-600, -1, 0, 1, 2, 600] + list(range(1018, 1025)):
        xs += around((k + 0.5) * ln2, 2) + [k * ln2]
    r = _rng(3)
    xs += list(r.uniform(EXP_LO, EXP_HI, 4000))
    xs += list(r.uniform(EXP_LO, -708.3, 1500))  # subnormal results
    xs += list(r.uniform(-1, 1, 500) * 2.0 ** r.integers(-60, 0, 500))
    return np.array(xs)


def sincos_inputs():
    xs = [0.0, -0.0, TINY, -TINY, 1e-310, -1e-310, MIN_NORMAL, 1e-200, INF, -INF, NAN, MAX, -MAX]
    xs += around(SINCOS_MAX, 2) + around(-SINCOS_MAX, 2) + around(SINCOS_SPLIT, 2) + around(-SINCOS_SPLIT, 2)
    xs += [1e8, -1e8, 2e9, 1e10, 1e300]
    # n pi/2 and pi/4 + n pi/2 (the quadrant boundaries and the reduced interval's ends), both reductions
    for n in list(range(-40, 41)) + [2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 12345678, 2 ** 29, 683565275]:
        xs += around(n * math.pi / 2, 1) + around(n * math.pi / 2 + math.pi / 4, 1)
    r = _rng(4)
    xs += list(r.uniform(-7, 7, 1000)) + list(r.uniform(-SINCOS_SPLIT, SINCOS_SPLIT, 1000))
    big = np.exp(r.uniform(math.log(SINCOS_SPLIT), math.log(SINCOS_MAX), 1000))
    xs += list(big * r.choice([-1.0, 1.0], 1000))
    return np.array(xs)


def sincos2pi_inputs():
    xs = [0.0, U_MIN, U_MAX, 0.5]
    for k in range(8):
        xs += [k / 8, k / 8 + 2.0 ** -53, k / 8 + 2.0 ** -52]
        if k:
            xs.append(k / 8 - 2.0 ** -53)
    xs += list(_rng(5).random(2000))
    return np.array([x for x in xs if 0.0 <= x < 1.0])


def randn_inputs():
    """(u1, u2) pairs of the Box-Muller draws"""
    u1s = [U_MIN, 2 * U_MIN, 1e-10, 0.5, 1 - 2.0 ** -20, U_MAX]
    u2s = [U_MIN, U_MAX, 0.25, 0.5, 0.75] + [k / 8 + d for k in range(8) for d in (-2.0 ** -53, 2.0 ** -53) if 0 < k / 8 + d < 1]
    a = [x for x in u1s for _ in u2s]
    b = [y for _ in u1s for y in u2s]
    r = _rng(6)
    a += list(r.random(2000) * (U_MAX - U_MIN) + U_MIN)
    b += list(r.random(2000) * (U_MAX - U_MIN) + U_MIN)
    return np.array(a), np.array(b)


RANDINT_N = [1, 2, 3, 2 ** 31 + 1, 2 ** 32 - 1]


def randint_inputs():
    """(seed, draw, n) rows of pdmp_randint on PDMP_STREAM_GLOBAL"""
    r = _rng(7)
    seeds = [0, 1, (1 << 64) - 1, 0x5EED0000] + list(r.integers(0, 1 << 63, 4))
    rows = [(s, d, n) for s in seeds for d in (0, 1, 2 ** 32, 2 ** 53 - 1, 12345) for n in RANDINT_N]
    return (np.array([s for s, _, _ in rows], dtype=np.uint64), np.array([d for _, d, _ in rows], dtype=np.float64),
            np.array([n for _, _, n in rows], dtype=np.float64))


def divsqrt_inputs():
    """(a, b) over the whole exponent range: subnormal operands and results, near overflow, zeros, Inf, NaN"""
    r = _rng(8)
    specials = [0.0, -0.0, TINY, -TINY, MIN_NORMAL, math.nextafter(MIN_NORMAL, 0), MAX, -MAX, 1.0, -1.0, 0.5, 3.0, INF, -INF, NAN]
    a = [x for x in specials for _ in specials]
    b = [y for _ in specials for y in specials]
    m1 = r.uniform(1, 2, 3000) * r.choice([-1.0, 1.0], 3000)
    m2 = r.uniform(1, 2, 3000)
    e1 = r.integers(-1074, 1024, 3000)
    e2 = r.integers(-1074, 1024, 3000)
    a += list(np.ldexp(m1, e1))
    b += list(np.ldexp(m2, e2))
    # results near the subnormal boundary and near overflow
    a += list(np.ldexp(r.uniform(1, 2, 500), -1000)) + list(np.ldexp(r.uniform(1, 2, 500), 1000))
    b += list(np.ldexp(r.uniform(1, 2, 500), 40)) + list(np.ldexp(r.uniform(0.5, 1, 500), -24))
    return np.array(a), np.array(b)


def sigmoid_inputs():
    xs = [0.0, -0.0, INF, -INF, NAN, TINY, -TINY]
    for v in (709.0, 709.782712893384, 710.0, 745.0, 745.1332191019411, 746.0, 36.0, 37.0, 1e300):
        xs += around(v) + around(-v)
    xs += list(_rng(9).uniform(-800, 800, 1000))
    return np.array(xs)


def pos_inputs():
    return np.array([0.0, -0.0, TINY, -TINY, 1.0, -1.0, MAX, -MAX, INF, -INF, NAN, -NAN, 1e-310, -1e-310] + list(_rng(10).normal(size=100)))


def poisson_boundary(log_fn):
    """(a, b, u) rows with b < 0 < a where -L = -log_fn(u) is exactly the computed admissibility bound -(a*a)/b + (a*a)/(2*b) of the
    b < 0 branch ("at"), or one ulp above or below it: found by walking b ulp by ulp from a^2 / (2L).  Plain Python floats are IEEE
    binary64 with round-to-nearest, the arithmetic of both the oracle and the device.  log_fn: pdmp_log (the oracle's)."""
    rows = {"at": set(), "below": set(), "above": set()}
    for u in (0.5, 0.1, 0.9, 0.36787944117144233, 1e-3, 0.75, 0.2, 0.6):
        E = -log_fn(u)
        for a in (1.0, 0.7, 3.0):
            for direction in (INF, -INF):
                b = (a * a) / (-2.0 * E)
                for _ in range(300):
                    T = -(a * a) / b + (a * a) / (2 * b)
                    if T == E:
                        rows["at"].add((a, b, u))
                    elif T == math.nextafter(E, INF):
                        rows["above"].add((a, b, u))
                    elif T == math.nextafter(E, -INF):
                        rows["below"].add((a, b, u))
                    b = math.nextafter(b, direction)
    return {k: sorted(v) for k, v in rows.items()}


def poisson_inputs(log_fn):
    """(a, b, u) rows of poisson_time: every branch and its boundary, signed zeros, tiny and huge rates, overflow of (a/b)^2 and of
    2 log(u) / b, NaN and +-Inf rates; plus the b < 0 admissibility boundary (poisson_boundary) and a random body."""
    av = [-2.0, -0.0, 0.0, 5e-324, -5e-324, 1e-300, 0.5, 3.0, -1e300, 1e300, NAN, INF, -INF]
    bv = [-3.0, -0.0, 0.0, 2.0, 1e-12, -1e-12, 1e-160, -1e-160, 1e-310, -1e-310, 5e-324, 1e300, -1e300, NAN, INF, -INF]
    uv = [U_MIN, 0.5, U_MAX, 0.36787944117144233]
    rows = [(a, b, u) for a in av for b in bv for u in uv]
    # the documented deviations of the reference's formula (test_detmath_accuracy.py): b -> 0+ with a > 0, (a/b)^2 and q overflow
    rows += [(1.0, 1e-12, 0.36787944117144233), (1.0, 1e-160, 0.5), (1.0, 1e-155, 0.5), (-1e-10, 1e-310, 0.5), (-0.0, 1e-310, 0.5),
             (0.5, -1e-160, 0.5), (0.5, 1e-310, 0.5)]
    bd = poisson_boundary(log_fn)
    rows += bd["at"] + bd["below"] + bd["above"]
    r = _rng(11)
    n = 3000
    a = r.uniform(-8, 8, n) * 10.0 ** r.integers(-6, 7, n)
    b = r.uniform(-4, 4, n) * 10.0 ** r.integers(-6, 7, n)
    b[::9] = 0.0
    u = r.random(n) * (U_MAX - U_MIN) + U_MIN
    rows += list(zip(a, b, u))
    arr = np.array(rows, dtype=np.float64)
    return arr[:, 0].copy(), arr[:, 1].copy(), arr[:, 2].copy()
