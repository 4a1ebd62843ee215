"""gfx950 evaluates the shared numerical contract bit-for-bit like the host (-m gpu)."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu


def test_device_math_matches_host_bitwise(gpu_pkg):
    n = 1 << 20
    for seed in (1, 0x5EED0000):
        dev = gpu_pkg._lib.math_probe(seed, n)
        host = O.math_probe(seed, n)
        for r, name in enumerate(["u01", "log", "div", "sqrt", "poisson_time", "randn", "exp", "sincos"]):
            same = (dev[r] == host[r]) | (np.isnan(dev[r]) & np.isnan(host[r]))
            assert same.all(), (name, int((~same).sum()), dev[r][~same][:3], host[r][~same][:3])
        assert np.isinf(host[4]).any() and np.isfinite(host[4]).any()  # both poisson_time outcomes exercised


# ------------------------------------------------------------------------------------------------ every scalar function, one by one
import detmath_tables as T  # noqa: E402

IDS = None


def math_ids():
    """PDMP_MATH_* of include/pdmp_debug.h -> (id, file, function) (file and function for the device copies)"""
    global IDS
    if IDS is None:
        import os
        import re
        src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pdmp_debug.h")).read()
        IDS = {m[0]: (int(m[1]), m[2] or None, m[3] or None)
               for m in re.findall(r"#define (PDMP_MATH_\w+) (\d+)\s*/\*\s*(?:(pdmp_\w+\.hip) (\w+))?", src)}
    return IDS


def _host(name, a, b, c):
    """the oracle's value of probe `name` at (a, b, c): a [2 x n] array like the device's"""
    L = O.lib()
    one = lambda f, *cols: np.vstack([O.vec(f, *cols), np.zeros(len(a))])  # noqa: E731
    bits = a.view(np.uint64)
    if name == "PDMP_MATH_U01":
        return one(lambda x: L.orc_bits_to_u01(x), bits)
    if name == "PDMP_MATH_LOG":
        return one(L.orc_log, a)
    if name == "PDMP_MATH_EXP":
        return one(L.orc_exp, a)
    if name == "PDMP_MATH_SINCOS":
        return O.vec(O.sincos, a)
    if name == "PDMP_MATH_SINCOS2PI":
        return O.vec(O.sincos2pi, a)
    if name == "PDMP_MATH_RANDN":
        return one(L.orc_randn_from_u, a, b)
    if name == "PDMP_MATH_RANDN2":
        return O.vec(O.randn2_from_u, a, b)
    if name == "PDMP_MATH_RANDINT":
        return one(lambda s, d, n: float(L.orc_randint(s, 1, int(d), int(n))), bits, b, c)
    if name == "PDMP_MATH_DIV":
        return np.vstack([a / b, np.zeros(len(a))])
    if name == "PDMP_MATH_SQRT":
        return np.vstack([np.sqrt(a), np.zeros(len(a))])
    if name.startswith("PDMP_MATH_PT_"):
        return one(O.poisson_time, a, b, c)
    if name.startswith("PDMP_MATH_SIGMOID_"):
        return one(L.orc_sigmoid, a)
    assert name.startswith("PDMP_MATH_POS_"), name
    return one(L.orc_pos, a)


def _inputs(name):
    n0 = None
    if name == "PDMP_MATH_U01":
        a = T.u01_bits().view(np.float64)
    elif name == "PDMP_MATH_LOG":
        a = T.log_inputs()
    elif name == "PDMP_MATH_EXP":
        a = T.exp_inputs()
    elif name == "PDMP_MATH_SINCOS":
        a = T.sincos_inputs()
    elif name == "PDMP_MATH_SINCOS2PI":
        a = T.sincos2pi_inputs()
    elif name in ("PDMP_MATH_RANDN", "PDMP_MATH_RANDN2"):
        a, n0 = T.randn_inputs()
        return a, n0, np.zeros(len(a))
    elif name == "PDMP_MATH_RANDINT":
        s, d, n = T.randint_inputs()
        return s.view(np.float64), d, n
    elif name in ("PDMP_MATH_DIV", "PDMP_MATH_SQRT"):
        a, b = T.divsqrt_inputs()
        if name == "PDMP_MATH_SQRT":
            a = np.concatenate([a, np.abs(a), b])
            return a, np.zeros(len(a)), np.zeros(len(a))
        return a, b, np.zeros(len(a))
    elif name.startswith("PDMP_MATH_PT_"):
        return T.poisson_inputs(O.lib().orc_log)
    elif name.startswith("PDMP_MATH_SIGMOID_"):
        a = T.sigmoid_inputs()
    else:
        a = T.pos_inputs()
    return a, np.zeros(len(a)), np.zeros(len(a))


def _same_bits(x, y):
    """equal bit for bit (so +0 != -0), or both NaN (any payload)"""
    return (x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))


@pytest.mark.parametrize("name", sorted(math_ids(), key=lambda k: math_ids()[k][0]))
def test_device_scalar_function_matches_host_bitwise(gpu_pkg_parity, name):
    """every function of the shared contract and every device copy of poisson_time / sigmoid / pos, called as it is by a probe kernel of
    the unit that owns it, equals the oracle bit for bit on the edge tables (detmath_tables.py).  A probe checks the copy's arithmetic
    under the library's build flags, not its inlined form in each kernel: the chain parity tests cover that."""
    a, b, c = _inputs(name)
    a, b, c = (np.ascontiguousarray(v, dtype=np.float64) for v in (a, b, c))
    dev = gpu_pkg_parity._lib.math_eval(math_ids()[name][0], a, b, c)
    with np.errstate(all="ignore"):
        host = _host(name, a, b, c)
    for row in (0, 1):
        same = _same_bits(dev[row], host[row])
        assert same.all(), (name, row, int((~same).sum()), list(zip(a[~same][:4], b[~same][:4], c[~same][:4])), dev[row][~same][:4],
                            host[row][~same][:4])

