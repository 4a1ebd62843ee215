"""ctypes binding of tests/ref/condition_ref.c: the conditional trace (src/condition.jl) as the device consumers' contract states it
(ref_condition_fact / ref_condition_pdmp) and line by line as the reference writes it (the *_literal pair).  TEST INFRASTRUCTURE ONLY -- the
product package never imports it.  Compiled with exactly the flags of oracle/Makefile into tests/ref/_build/ (git-ignored), or into a temporary
directory where the tree is read-only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "condition_ref.c")
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
        out_dir = tempfile.mkdtemp(prefix="condition_ref_")
    lib = os.path.join(out_dir, "libcondition_ref.so")
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
        for name in ("ref_condition_fact", "ref_condition_pdmp", "ref_condition_fact_literal", "ref_condition_pdmp_literal"):
            getattr(L, name).restype = i64
        L.ref_condition_fact.argtypes = [i64, i64, f64] + [vp] * 5 + [i64] + [vp] * 3
        L.ref_condition_pdmp.argtypes = [i64, i64, f64] + [vp] * 9 + [i64] + [vp] * 3
        L.ref_condition_fact_literal.argtypes = [i64, i64, f64] + [vp] * 5 + [i64, i64] + [vp] * 3
        L.ref_condition_pdmp_literal.argtypes = [i64, i64, f64] + [vp] * 9 + [i64, i64] + [vp] * 3
        _lib = L
    return _lib


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.shape == shape, (a.shape, shape)
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data


def _outs(n, d, extra):
    return np.empty(n), np.empty((n, d)), np.empty(n, dtype=extra)


def fact(t0, x0, th0, events, p, n, max_hits=None, literal=False, max_rehits=64):
    """One chain's FactTrace.  Returns dict(t [m], x [m x d], nhits, h [m]) -- m = min(nhits, max_hits) -- or with literal=True dict(t, x, nhits,
    k [m]: the event index each hit was found before)."""
    L = load()
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    d = x0.size
    th0, p, n = _f64(th0, (d,)), _f64(p, (d,)), _f64(n, (d,))
    ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE)
    assert ev.size == 0 or (ev["i"].min() >= 0 and ev["i"].max() < d)
    cap = int(max_hits) if max_hits is not None else (max_rehits + 2) * (len(ev) + 1)
    ot, ox, oe = _outs(cap, d, np.int64 if literal else np.float64)
    if literal:
        nh = L.ref_condition_fact_literal(d, len(ev), float(t0), _ptr(x0), _ptr(th0), _ptr(ev), _ptr(p), _ptr(n), int(max_rehits), cap, _ptr(ot),
                                          _ptr(ox), _ptr(oe))
    else:
        nh = L.ref_condition_fact(d, len(ev), float(t0), _ptr(x0), _ptr(th0), _ptr(ev), _ptr(p), _ptr(n), cap, _ptr(ot), _ptr(ox), _ptr(oe))
    if nh < 0:
        raise MemoryError("ref_condition_fact")
    m = min(int(nh), cap)
    return {"t": ot[:m].copy(), "x": ox[:m].copy(), "nhits": int(nh), ("k" if literal else "h"): oe[:m].copy()}


def pdmp(t0, x0, th0, t, x, th, p, n, f0=None, f=None, max_hits=None, literal=False, max_rehits=64):
    """One chain's PDMPTrace: t [n], x and th [n x d], f [n x d] bool (a sticky trace; f0 [d], None = all free) or None.  Returns as fact()."""
    L = load()
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    d = x0.size
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    m_ev = t.size
    th0, p, n = _f64(th0, (d,)), _f64(p, (d,)), _f64(n, (d,))
    x = _f64(np.asarray(x, dtype=np.float64).reshape(m_ev, d), (m_ev, d))
    th = _f64(np.asarray(th, dtype=np.float64).reshape(m_ev, d), (m_ev, d))
    fb = None if f is None else np.ascontiguousarray(np.asarray(f).reshape(m_ev, d) != 0, dtype=np.uint8)
    f0b = None if f0 is None else np.ascontiguousarray(np.asarray(f0).reshape(d) != 0, dtype=np.uint8)
    cap = int(max_hits) if max_hits is not None else (max_rehits + 2) * (m_ev + 1)
    ot, ox, oe = _outs(cap, d, np.int64 if literal else np.float64)
    args = [d, m_ev, float(t0), _ptr(x0), _ptr(th0), _ptr(f0b), _ptr(t), _ptr(x), _ptr(th), _ptr(fb), _ptr(p), _ptr(n)]
    if literal:
        nh = L.ref_condition_pdmp_literal(*args, int(max_rehits), cap, _ptr(ot), _ptr(ox), _ptr(oe))
    else:
        nh = L.ref_condition_pdmp(*args, cap, _ptr(ot), _ptr(ox), _ptr(oe))
    if nh < 0:
        raise MemoryError("ref_condition_pdmp")
    m = min(int(nh), cap)
    return {"t": ot[:m].copy(), "x": ox[:m].copy(), "nhits": int(nh), ("k" if literal else "h"): oe[:m].copy()}


def of_trace(tr, p, n, **kw):
    """fact() or pdmp() of a FactTrace / PDMPTrace object of the package"""
    if hasattr(tr, "events"):
        return fact(tr.t0, tr.x0, tr.θ0, tr.events, p, n, **kw)
    f = getattr(tr, "f", None)
    return pdmp(tr.t0, tr.x0, tr.θ0, tr.t, tr.x, tr.θ, p, n, f0=getattr(tr, "f0", None) if f is not None else None, f=f, **kw)
