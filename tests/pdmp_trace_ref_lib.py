"""ctypes binding of tests/ref/pdmp_trace_ref.c: the sequential restatement of the reference's PDMPTrace consumers (src/trace.jl:129-150, 229-266)
in the arithmetic of csrc/pdmp_consume_bps.hip.  TEST INFRASTRUCTURE ONLY -- the product package never imports it.  Compiled with exactly the
flags of oracle/Makefile into tests/ref/_build/ (git-ignored), or into a temporary directory where the tree is read-only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "pdmp_trace_ref.c")
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
        out_dir = tempfile.mkdtemp(prefix="pdmp_trace_ref_")
    lib = os.path.join(out_dir, "libpdmp_trace_ref.so")
    if force or not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        tmp = lib + ".tmp.%d" % os.getpid()
        subprocess.check_call(["gcc"] + CFLAGS + ["-Wall", "-Wextra", "-shared", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, lib)
    return lib


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.ref_pdmp_trace.restype = C.c_int64
        L.ref_pdmp_trace.argtypes = [C.c_int64, C.c_int64, C.c_double] + [C.c_void_p] * 7 + [C.c_double, C.c_int64] + [C.c_void_p] * 5
        _lib = L
    return _lib


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.shape == shape, (a.shape, shape)
    return a


def consume(t0, x0, th0, t, x, th, f=None, mu=None, dt=0.0, K=0, cummean=True):
    """One chain's whole trace: t [n], x and th [n x d], f [n x d] bool (a sticky trace) or None, mu [d] (the Boomerang's centre) or None.
    Returns dict(mean [d], T, cummean [n x d], inclusion [d] (sticky), grid [K x d] -- rows at and behind npoints are 0 --, npoints, grid_t)."""
    L = load()
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    d = x0.size
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    n = t.size
    th0 = _f64(th0, (d,))
    x = _f64(np.asarray(x, dtype=np.float64).reshape(n, d), (n, d))
    th = _f64(np.asarray(th, dtype=np.float64).reshape(n, d), (n, d))
    fb = None if f is None else np.ascontiguousarray(np.asarray(f).reshape(n, d) != 0, dtype=np.uint8)
    mub = None if mu is None else _f64(mu, (d,))
    K = int(K)
    grid = np.full((K, d), np.nan) if K > 0 else None
    mean = np.empty(d)
    cm = np.empty((n, d)) if cummean else None
    incl = np.empty(d) if f is not None else None
    T = C.c_double()
    ptr = lambda a: None if a is None else a.ctypes.data
    npts = L.ref_pdmp_trace(d, n, float(t0), ptr(x0), ptr(th0), ptr(t), ptr(x), ptr(th), ptr(fb), ptr(mub), float(dt), K, ptr(grid), ptr(mean), ptr(cm),
                            ptr(incl), C.addressof(T))
    if npts < 0:
        raise MemoryError("ref_pdmp_trace")
    out = dict(mean=mean, T=float(T.value), cummean=cm, npoints=int(npts), grid=grid)
    if incl is not None:
        out["inclusion"] = incl
    if K > 0:
        out["grid_t"] = float(t0) + float(dt) * np.arange(min(int(npts), K), dtype=np.float64)
    return out
