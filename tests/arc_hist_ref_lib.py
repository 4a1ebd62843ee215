"""ctypes binding of tests/ref/arc_hist_ref.c: the marginal histograms (occupation times per bin) of a Boomerang's PDMPTrace as the arc histogram
consumer's contract states them (ref_arc_hist, one piece alone, and pdmp_acos / pdmp_atan2 of include/pdmp_detmath.h as that library compiles
them).  TEST INFRASTRUCTURE ONLY -- the product package never imports it.  Compiled with exactly the flags of oracle/Makefile into
tests/ref/_build/ (git-ignored), or into a temporary directory where the tree is read-only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "arc_hist_ref.c")
_DEPS = [_SRC, os.path.join(_HERE, "ref", "hist_ref.c"), os.path.join(os.path.dirname(_HERE), "include", "pdmp_detmath.h")]
CFLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]  # oracle/Makefile's

_lib = None


def build(force=False):
    out_dir = os.path.join(_HERE, "ref", "_build")
    try:
        os.makedirs(out_dir, exist_ok=True)
        if not os.access(out_dir, os.W_OK):
            raise OSError
    except OSError:
        out_dir = tempfile.mkdtemp(prefix="arc_hist_ref_")
    lib = os.path.join(out_dir, "libarc_hist_ref.so")
    if force or not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in _DEPS):
        tmp = lib + ".tmp.%d" % os.getpid()
        subprocess.check_call(["gcc"] + CFLAGS + ["-Wall", "-Wextra", "-shared", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, lib)
    return lib


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        vp, i64, f64 = C.c_void_p, C.c_int64, C.c_double
        L.ref_arc_acos.restype = L.ref_arc_atan2.restype = f64
        L.ref_arc_acos.argtypes = [f64]
        L.ref_arc_atan2.argtypes = [f64, f64]
        L.ref_arc_hist_piece.restype = None
        L.ref_arc_hist_piece.argtypes = [f64, f64, i64, f64, f64, C.c_int, f64, f64, C.c_int, vp, vp]
        L.ref_arc_hist.restype = i64
        L.ref_arc_hist.argtypes = [i64, i64, f64] + [vp] * 8 + [i64] + [vp] * 3 + [i64, C.c_int] + [vp] * 3
        _lib = L
    return _lib


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.shape == shape, (a.shape, shape)
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data


def acos(z):
    return float(load().ref_arc_acos(float(z)))


def atan2(y, x):
    return float(load().ref_arc_atan2(float(y), float(x)))


def _bins(d, coords, lo, hi, bins):
    coords = np.arange(d, dtype=np.int64) if coords is None else np.ascontiguousarray(coords, dtype=np.int64).reshape(-1)
    assert coords.size >= 1 and coords.min() >= 0 and coords.max() < d and len(np.unique(coords)) == coords.size and 1 <= bins <= 4096
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), coords.shape))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64), coords.shape))
    assert np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)
    return coords, lo, hi


def piece(lo, hi, bins, xc, thc, free, mu, tau, H=None, Z=0.0, wrong=False):
    """One piece added to a row H [bins + 2] (zeros when None) and to Z.  Returns (H, Z)."""
    H = np.zeros(bins + 2) if H is None else _f64(H, (bins + 2,)).copy()
    z = C.c_double(Z)
    load().ref_arc_hist_piece(float(lo), float(hi), int(bins), float(xc), float(thc), int(bool(free)), float(mu), float(tau), int(bool(wrong)),
                              _ptr(H), C.addressof(z))
    return H, float(z.value)


def arcs(t0, x0, th0, t, x, th, mu, coords, lo, hi, bins, f0=None, f=None, wrong=False, pieces=False):
    """One chain's PDMPTrace of a Boomerang with centre mu [d]: t [n], x and th [n x d], f [n x d] bool (a sticky trace; f0 [d], None = all
    free) or None.  Returns (H [m x (bins + 2)], Z [m], T_last), with pieces=True also the number of pieces with tau > 0.  wrong=True: the
    WRONG statement with ψ0 of the opposite sign, which the tests hold the error bound against."""
    L = load()
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    d = x0.size
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    n = t.size
    th0, mu = _f64(th0, (d,)), _f64(mu, (d,))
    x = _f64(np.asarray(x, dtype=np.float64).reshape(n, d), (n, d))
    th = _f64(np.asarray(th, dtype=np.float64).reshape(n, d), (n, d))
    fb = None if f is None else np.ascontiguousarray(np.asarray(f).reshape(n, d) != 0, dtype=np.uint8)
    f0b = None if (f0 is None or f is None) else np.ascontiguousarray(np.asarray(f0).reshape(d) != 0, dtype=np.uint8)
    coords, lo, hi = _bins(d, coords, lo, hi, bins)
    H, Z, T = np.empty((coords.size, bins + 2)), np.empty(coords.size), C.c_double()
    rc = L.ref_arc_hist(d, n, float(t0), _ptr(x0), _ptr(th0), _ptr(f0b), _ptr(t), _ptr(x), _ptr(th), _ptr(fb), _ptr(mu), coords.size, _ptr(coords),
                        _ptr(lo), _ptr(hi), int(bins), int(bool(wrong)), _ptr(H), _ptr(Z), C.addressof(T))
    return (H, Z, float(T.value), int(rc)) if pieces else (H, Z, float(T.value))


def of_trace(tr, coords, lo, hi, bins, wrong=False):
    """arcs() of a PDMPTrace object of the package whose flow is a Boomerang"""
    f = getattr(tr, "f", None)
    return arcs(tr.t0, tr.x0, tr.θ0, tr.t, tr.x, tr.θ, tr.F.μ, coords, lo, hi, bins, f0=getattr(tr, "f0", None) if f is not None else None, f=f,
                wrong=wrong)
