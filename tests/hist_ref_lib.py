"""ctypes binding of tests/ref/hist_ref.c: the marginal histograms (occupation times per bin) as the device consumers' contract states them
(ref_hist_fact / ref_hist_pdmp, the bins and the piece alone).  TEST INFRASTRUCTURE ONLY -- the product package never imports it.
Compiled with exactly the flags of oracle/Makefile into tests/ref/_build/ (git-ignored), or into a temporary directory where the tree is
read-only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "hist_ref.c")
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
        out_dir = tempfile.mkdtemp(prefix="hist_ref_")
    lib = os.path.join(out_dir, "libhist_ref.so")
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
        L.ref_hist_fact.restype = L.ref_hist_pdmp.restype = L.ref_hist_bin_of.restype = i64
        L.ref_hist_edge.restype = f64
        L.ref_hist_piece.restype = L.ref_hist_pool.restype = None
        L.ref_hist_bin_of.argtypes = [f64, f64, i64, f64]
        L.ref_hist_edge.argtypes = [f64, f64, i64, i64]
        L.ref_hist_piece.argtypes = [f64, f64, i64, f64, f64, f64, vp, vp]
        L.ref_hist_fact.argtypes = [i64, i64, f64, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp]
        L.ref_hist_pdmp.argtypes = [i64, i64, f64] + [vp] * 7 + [i64] + [vp] * 3 + [i64] + [vp] * 3
        L.ref_hist_pool.argtypes = [i64, i64, vp, vp]
        _lib = L
    return _lib


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.shape == shape, (a.shape, shape)
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data


def _bins(d, coords, lo, hi, bins):
    coords = np.arange(d, dtype=np.int64) if coords is None else np.ascontiguousarray(coords, dtype=np.int64).reshape(-1)
    assert coords.size >= 1 and coords.min() >= 0 and coords.max() < d and len(np.unique(coords)) == coords.size and 1 <= bins <= 4096
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), coords.shape))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64), coords.shape))
    assert np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)
    return coords, lo, hi


def bin_of(lo, hi, bins, x):
    return int(load().ref_hist_bin_of(float(lo), float(hi), int(bins), float(x)))


def edge(lo, hi, bins, k):
    return float(load().ref_hist_edge(float(lo), float(hi), int(bins), int(k)))


def piece(lo, hi, bins, a, v, tau, H=None, Z=0.0):
    """One piece added to a row H [bins + 2] (zeros when None) and to Z.  Returns (H, Z)."""
    H = np.zeros(bins + 2) if H is None else _f64(H, (bins + 2,)).copy()
    z = C.c_double(Z)
    load().ref_hist_piece(float(lo), float(hi), int(bins), float(a), float(v), float(tau), _ptr(H), C.addressof(z))
    return H, float(z.value)


def fact(t0, x0, th0, events, coords, lo, hi, bins, pieces=False):
    """One chain's FactTrace.  Returns (H [m x (bins + 2)], Z [m], T_last), with pieces=True also the number of pieces with tau > 0."""
    L = load()
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    d = x0.size
    th0 = _f64(th0, (d,))
    ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE)
    coords, lo, hi = _bins(d, coords, lo, hi, bins)
    H, Z, T = np.empty((coords.size, bins + 2)), np.empty(coords.size), C.c_double()
    rc = L.ref_hist_fact(d, len(ev), float(t0), _ptr(x0), _ptr(th0), _ptr(ev) if len(ev) else None, coords.size, _ptr(coords), _ptr(lo), _ptr(hi),
                         int(bins), _ptr(H), _ptr(Z), C.addressof(T))
    if rc < 0:
        raise MemoryError("ref_hist_fact")
    return (H, Z, float(T.value), int(rc)) if pieces else (H, Z, float(T.value))


def pdmp(t0, x0, th0, t, x, th, coords, lo, hi, bins, f0=None, f=None, pieces=False):
    """One chain's PDMPTrace: t [n], x and th [n x d], f [n x d] bool (a sticky trace; f0 [d], None = all free) or None.  Returns as fact()."""
    L = load()
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    d = x0.size
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    n = t.size
    th0 = _f64(th0, (d,))
    x = _f64(np.asarray(x, dtype=np.float64).reshape(n, d), (n, d))
    th = _f64(np.asarray(th, dtype=np.float64).reshape(n, d), (n, d))
    fb = None if f is None else np.ascontiguousarray(np.asarray(f).reshape(n, d) != 0, dtype=np.uint8)
    f0b = None if (f0 is None or f is None) else np.ascontiguousarray(np.asarray(f0).reshape(d) != 0, dtype=np.uint8)
    coords, lo, hi = _bins(d, coords, lo, hi, bins)
    H, Z, T = np.empty((coords.size, bins + 2)), np.empty(coords.size), C.c_double()
    rc = L.ref_hist_pdmp(d, n, float(t0), _ptr(x0), _ptr(th0), _ptr(f0b), _ptr(t), _ptr(x), _ptr(th), _ptr(fb), coords.size, _ptr(coords), _ptr(lo),
                         _ptr(hi), int(bins), _ptr(H), _ptr(Z), C.addressof(T))
    return (H, Z, float(T.value), int(rc)) if pieces else (H, Z, float(T.value))


def pool(rows):
    """rows [n x ...] summed over the chains in order, sequentially per entry, from 0.0"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    n = rows.shape[0]
    out = np.empty(rows.shape[1:])
    load().ref_hist_pool(n, out.size, _ptr(rows), _ptr(out))
    return out


def of_trace(tr, coords, lo, hi, bins, pieces=False):
    """fact() or pdmp() of a FactTrace / PDMPTrace object of the package"""
    if hasattr(tr, "events"):
        return fact(tr.t0, tr.x0, tr.θ0, tr.events, coords, lo, hi, bins, pieces=pieces)
    f = getattr(tr, "f", None)
    return pdmp(tr.t0, tr.x0, tr.θ0, tr.t, tr.x, tr.θ, coords, lo, hi, bins, f0=getattr(tr, "f0", None) if f is not None else None, f=f, pieces=pieces)
