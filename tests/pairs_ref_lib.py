"""ctypes binding of tests/ref/pairs_ref.c: the pair integrals S_ij = ∫ (x_i − c_i)(x_j − c_j) dt, J_i = ∫ (x_i − c_i) dt as the device
consumers' contract states them (ref_pairs_fact / ref_pairs_pdmp).  TEST INFRASTRUCTURE ONLY -- the product package never imports it.
Compiled with exactly the flags of oracle/Makefile into tests/ref/_build/ (git-ignored), or into a temporary directory where the tree is
read-only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "pairs_ref.c")
CFLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]  # oracle/Makefile's
EVENT_DTYPE = np.dtype([("t", "<f8"), ("i", "<i8"), ("x", "<f8"), ("theta", "<f8")])

_lib = None


def build(force=False):
    out_dir = os.path.join(_HERE, "ref", "_build")
    try:
        os.makedirs(out_dir, exist_ok=True)
        if not os.access(out_dir, os.W_OK):
            raise OSError
    except OSError:
        out_dir = tempfile.mkdtemp(prefix="pairs_ref_")
    lib = os.path.join(out_dir, "libpairs_ref.so")
    if force or not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(_SRC):
        tmp = lib + ".tmp.%d" % os.getpid()
        subprocess.check_call(["gcc"] + CFLAGS + ["-Wall", "-Wextra", "-shared", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, lib)
    return lib


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        vp, i64, f64 = C.c_void_p, C.c_int64, C.c_double
        L.ref_pairs_fact.restype = L.ref_pairs_pdmp.restype = i64
        L.ref_pairs_fact.argtypes = [i64, i64, f64, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]
        L.ref_pairs_pdmp.argtypes = [i64, i64, f64] + [vp] * 7 + [i64] + [vp] * 6
        _lib = L
    return _lib


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.shape == shape, (a.shape, shape)
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data


def _pairs(d, pi, pj, center):
    pi = np.ascontiguousarray(pi, dtype=np.int64).reshape(-1)
    pj = np.ascontiguousarray(pj, dtype=np.int64).reshape(-1)
    assert pi.size == pj.size and pi.size >= 1 and pi.min() >= 0 and pj.min() >= 0 and pi.max() < d and pj.max() < d
    c = None if center is None else _f64(center, (d,))
    return pi, pj, c


def fact(t0, x0, th0, events, pi, pj, center=None):
    """One chain's FactTrace.  Returns (S [npairs], J [d], T_last)."""
    L = load()
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    d = x0.size
    th0 = _f64(th0, (d,))
    ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE)
    pi, pj, c = _pairs(d, pi, pj, center)
    S, J, T = np.empty(pi.size), np.empty(d), C.c_double()
    rc = L.ref_pairs_fact(d, len(ev), float(t0), _ptr(x0), _ptr(th0), _ptr(ev) if len(ev) else None, pi.size, _ptr(pi), _ptr(pj), _ptr(c), _ptr(S),
                          _ptr(J), C.addressof(T))
    if rc < 0:
        raise MemoryError("ref_pairs_fact")
    return S, J, float(T.value)


def pdmp(t0, x0, th0, t, x, th, pi, pj, center=None, f0=None, f=None):
    """One chain's PDMPTrace: t [n], x and th [n x d], f [n x d] bool (a sticky trace; f0 [d], None = all free) or None.  Returns as fact()."""
    L = load()
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    d = x0.size
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    m = t.size
    th0 = _f64(th0, (d,))
    x = _f64(np.asarray(x, dtype=np.float64).reshape(m, d), (m, d))
    th = _f64(np.asarray(th, dtype=np.float64).reshape(m, d), (m, d))
    fb = None if f is None else np.ascontiguousarray(np.asarray(f).reshape(m, d) != 0, dtype=np.uint8)
    f0b = None if (f0 is None or f is None) else np.ascontiguousarray(np.asarray(f0).reshape(d) != 0, dtype=np.uint8)
    pi, pj, c = _pairs(d, pi, pj, center)
    S, J, T = np.empty(pi.size), np.empty(d), C.c_double()
    L.ref_pairs_pdmp(d, m, float(t0), _ptr(x0), _ptr(th0), _ptr(f0b), _ptr(t), _ptr(x), _ptr(th), _ptr(fb), pi.size, _ptr(pi), _ptr(pj), _ptr(c),
                     _ptr(S), _ptr(J), C.addressof(T))
    return S, J, float(T.value)


def of_trace(tr, pi, pj, center=None):
    """fact() or pdmp() of a FactTrace / PDMPTrace object of the package"""
    if hasattr(tr, "events"):
        return fact(tr.t0, tr.x0, tr.θ0, tr.events, pi, pj, center)
    f = getattr(tr, "f", None)
    return pdmp(tr.t0, tr.x0, tr.θ0, tr.t, tr.x, tr.θ, pi, pj, center, f0=getattr(tr, "f0", None) if f is not None else None, f=f)
