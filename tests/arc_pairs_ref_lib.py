"""ctypes binding of tests/ref/arc_pairs_ref.c: the pair integrals S_ij = ∫ (x_i − z_i)(x_j − z_j) dt, J_i = ∫ (x_i − z_i) dt of a Boomerang's
PDMPTrace as the arc pair consumer's contract states them (ref_arc_pairs).  TEST INFRASTRUCTURE ONLY -- the product package never imports it.
Compiled with exactly the flags of oracle/Makefile into tests/ref/_build/ (git-ignored), or into a temporary directory where the tree is
read-only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "arc_pairs_ref.c")
_HDR = os.path.join(os.path.dirname(_HERE), "include", "pdmp_detmath.h")
CFLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]  # oracle/Makefile's

_lib = None


def build(force=False):
    out_dir = os.path.join(_HERE, "ref", "_build")
    try:
        os.makedirs(out_dir, exist_ok=True)
        if not os.access(out_dir, os.W_OK):
            raise OSError
    except OSError:
        out_dir = tempfile.mkdtemp(prefix="arc_pairs_ref_")
    lib = os.path.join(out_dir, "libarc_pairs_ref.so")
    if force or not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        tmp = lib + ".tmp.%d" % os.getpid()
        subprocess.check_call(["gcc"] + CFLAGS + ["-Wall", "-Wextra", "-shared", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, lib)
    return lib


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        vp, i64, f64 = C.c_void_p, C.c_int64, C.c_double
        L.ref_arc_pairs.restype = i64
        L.ref_arc_pairs.argtypes = [i64, i64, f64] + [vp] * 8 + [i64] + [vp] * 3 + [C.c_int] + [vp] * 3
        _lib = L
    return _lib


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.shape == shape, (a.shape, shape)
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data


def arcs(t0, x0, th0, t, x, th, mu, pi, pj, center=None, f0=None, f=None, exchanged=False):
    """One chain's PDMPTrace of a Boomerang with centre mu [d]: t [n], x and th [n x d], f [n x d] bool (a sticky trace; f0 [d], None = all
    free) or None.  Returns (S [npairs], J [d], T_last).  exchanged=True: the WRONG statement with ∫cos² and ∫sin² exchanged, which the
    tests hold the error bound against."""
    L = load()
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    d = x0.size
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    m = t.size
    th0, mu = _f64(th0, (d,)), _f64(mu, (d,))
    x = _f64(np.asarray(x, dtype=np.float64).reshape(m, d), (m, d))
    th = _f64(np.asarray(th, dtype=np.float64).reshape(m, d), (m, d))
    fb = None if f is None else np.ascontiguousarray(np.asarray(f).reshape(m, d) != 0, dtype=np.uint8)
    f0b = None if (f0 is None or f is None) else np.ascontiguousarray(np.asarray(f0).reshape(d) != 0, dtype=np.uint8)
    pi = np.ascontiguousarray(pi, dtype=np.int64).reshape(-1)
    pj = np.ascontiguousarray(pj, dtype=np.int64).reshape(-1)
    assert pi.size == pj.size and pi.size >= 1 and pi.min() >= 0 and pj.min() >= 0 and pi.max() < d and pj.max() < d
    c = None if center is None else _f64(center, (d,))
    S, J, T = np.empty(pi.size), np.empty(d), C.c_double()
    rc = L.ref_arc_pairs(d, m, float(t0), _ptr(x0), _ptr(th0), _ptr(f0b), _ptr(t), _ptr(x), _ptr(th), _ptr(fb), _ptr(mu), pi.size, _ptr(pi), _ptr(pj),
                         _ptr(c), int(bool(exchanged)), _ptr(S), _ptr(J), C.addressof(T))
    if rc < 0:
        raise MemoryError("ref_arc_pairs")
    return S, J, float(T.value)


def of_trace(tr, pi, pj, center=None, exchanged=False):
    """arcs() of a PDMPTrace object of the package whose flow is a Boomerang"""
    f = getattr(tr, "f", None)
    return arcs(tr.t0, tr.x0, tr.θ0, tr.t, tr.x, tr.θ, tr.F.μ, pi, pj, center, f0=getattr(tr, "f0", None) if f is not None else None, f=f,
                exchanged=exchanged)
