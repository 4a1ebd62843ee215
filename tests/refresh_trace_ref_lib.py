"""ctypes binding of tests/ref/refresh_trace_ref.c: the sequential statement of the FactTrace consumers on a trace that is sorted within a
coordinate only (a ZigZag with a refresh clock, a FactBoomerang) in the arithmetic of the unordered walk of csrc/pdmp_consume.hip, and the
reference's own iterator restated step by step.  TEST INFRASTRUCTURE ONLY -- the product package never imports it.  Compiled with exactly the
flags of oracle/Makefile into tests/ref/_build/ (git-ignored), or into a temporary directory where the tree is read-only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "refresh_trace_ref.c")
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
        out_dir = tempfile.mkdtemp(prefix="refresh_trace_ref_")
    lib = os.path.join(out_dir, "librefresh_trace_ref.so")
    if force or not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        tmp = lib + ".tmp.%d" % os.getpid()
        subprocess.check_call(["gcc"] + CFLAGS + ["-Wall", "-Wextra", "-shared", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, lib)
    return lib


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.ref_refresh_trace.restype = C.c_int64
        L.ref_refresh_trace.argtypes = [C.c_int64, C.c_int64, C.c_double] + [C.c_void_p] * 7 + [C.c_double, C.c_int64] + [C.c_void_p] * 6
        L.ref_refresh_steps.restype = C.c_int64
        L.ref_refresh_steps.argtypes = [C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_double, C.c_int64] + [C.c_void_p] * 3
        _lib = L
    return _lib


def _args(x0, th0, events, mu):
    x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1)
    d = x0.size
    th0 = np.ascontiguousarray(th0, dtype=np.float64).reshape(-1)
    assert th0.size == d
    et = np.ascontiguousarray(events["t"], dtype=np.float64)
    ei = np.ascontiguousarray(events["i"], dtype=np.int64)
    ex = np.ascontiguousarray(events["x"], dtype=np.float64)
    eth = np.ascontiguousarray(events["theta"], dtype=np.float64)
    assert len(ei) == 0 or (ei.min() >= 0 and ei.max() < d)
    mub = None if mu is None else np.ascontiguousarray(mu, dtype=np.float64).reshape(-1)
    assert mub is None or mub.size == d
    return d, x0, th0, et, ei, ex, eth, mub


def _ptr(a):
    return None if a is None else a.ctypes.data


def consume(t0, x0, th0, events, mu=None, dt=0.0, K=0):
    """One chain's whole trace (EVENT_DTYPE events in trace order; mu [d]: the FactBoomerang's centre, None: the linear flow).  Returns
    dict(mean [d], T (the last event's time), t_max, cummean_t [n], cummean_y [n], grid [K x d] -- rows at and behind npoints are 0 --,
    npoints (not clamped to K), grid_t)."""
    L = load()
    d, x0, th0, et, ei, ex, eth, mub = _args(x0, th0, events, mu)
    n, K = len(et), int(K)
    grid = np.full((K, d), np.nan) if K > 0 else None
    mean, cm_t, cm_y = np.empty(d), np.empty(n), np.empty(n)
    T, tm = C.c_double(), C.c_double()
    npts = L.ref_refresh_trace(d, n, float(t0), _ptr(x0), _ptr(th0), _ptr(et), _ptr(ei), _ptr(ex), _ptr(eth), _ptr(mub), float(dt), K, _ptr(grid),
                               _ptr(mean), _ptr(cm_t), _ptr(cm_y), C.addressof(T), C.addressof(tm))
    if npts < 0:
        raise MemoryError("ref_refresh_trace")
    out = dict(mean=mean, T=float(T.value), t_max=float(tm.value), cummean_t=cm_t, cummean_y=cm_y, npoints=int(npts), grid=grid)
    if K > 0:
        out["grid_t"] = float(t0) + float(dt) * np.arange(min(int(npts), K), dtype=np.float64)
    return out


def steps(t0, x0, th0, events, dt, mu=None, cap=1 << 16):
    """collect(discretize(Ξ, dt)) by the reference's own iterator, step by step: (ts [m], xs [m x d], steps [m x d]) -- steps = the number of
    move_forward! calls an entry has been through since its coordinate's last event."""
    L = load()
    d, x0, th0, et, ei, ex, eth, mub = _args(x0, th0, events, mu)
    ts, xs, st = np.empty(cap), np.empty((cap, d)), np.empty((cap, d), dtype=np.int64)
    m = L.ref_refresh_steps(d, float(t0), _ptr(x0), _ptr(th0), len(et), _ptr(et), _ptr(ei), _ptr(ex), _ptr(eth), _ptr(mub), float(dt), cap, _ptr(ts),
                            _ptr(xs), _ptr(st))
    if m < 0:
        raise MemoryError("ref_refresh_steps")
    assert m <= cap, (m, cap)
    return ts[:m].copy(), xs[:m].copy(), st[:m].copy()
