"""ctypes binding of tests/ref/stickyzz_ref.c: the sequential restatement of the reference's ZigZag with sticky and reflecting barriers
(src/stickyzz.jl).  TEST INFRASTRUCTURE ONLY -- the product package never imports it.  Compiled with exactly the flags of
oracle/Makefile into tests/ref/_build/ (git-ignored), or into a temporary directory where the tree is read-only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import scipy.sparse as sp

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "stickyzz_ref.c")
_HDR = os.path.join(os.path.dirname(_HERE), "include", "pdmp_detmath.h")
CFLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]  # oracle/Makefile's

REF_OK, REF_BOUND_VIOLATED = 0, 1
ACT_HIT, ACT_REFLECT, ACT_UNFREEZE = 0, 1, 2
EV_HIT, EV_THAW, EV_REFLECTION = 0, 1, 2
RULES = {"sticky": 0, "reflect": 1, "reversible": 2}

_lib = None


def build(force=False):
    out_dir = os.path.join(_HERE, "ref", "_build")
    try:
        os.makedirs(out_dir, exist_ok=True)
        if not os.access(out_dir, os.W_OK):
            raise OSError
    except OSError:
        out_dir = tempfile.mkdtemp(prefix="stickyzz_ref_")
    lib = os.path.join(out_dir, "libstickyzz_ref.so")
    if force or not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        tmp = lib + ".tmp.%d" % os.getpid()
        subprocess.check_call(["gcc"] + CFLAGS + ["-Wall", "-Wextra", "-shared", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, lib)
    return lib


class _Params(C.Structure):
    _fields_ = [("d", C.c_int64), ("adapt", C.c_int32), ("strong", C.c_int32),
                ("colptr", C.c_void_p), ("rowval", C.c_void_p), ("nzval", C.c_void_p), ("mu", C.c_void_p),
                ("t_colptr", C.c_void_p), ("t_rowval", C.c_void_p), ("t_nzval", C.c_void_p), ("t_mu", C.c_void_p),
                ("lo", C.c_void_p), ("hi", C.c_void_p), ("klo", C.c_void_p), ("khi", C.c_void_p), ("rlo", C.c_void_p), ("rhi", C.c_void_p),
                ("factor", C.c_double), ("seed", C.c_uint64)]


class _Result(C.Structure):
    _fields_ = [("num", C.c_int64), ("nacc", C.c_int64), ("nevents", C.c_int64), ("nhit", C.c_int64), ("nthaw", C.c_int64), ("nrefl", C.c_int64),
                ("nadapt", C.c_int64), ("ndraw_main", C.c_uint64), ("status", C.c_int32), ("pad_", C.c_int32), ("t", C.c_double)]


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.ref_poisson_time3.restype = C.c_double
        L.ref_poisson_time3.argtypes = [C.c_double] * 4
        L.ref_hitting_time.restype = C.c_double
        L.ref_hitting_time.argtypes = [C.c_double] * 3
        L.ref_stickyzz.restype = C.c_int
        L.ref_stickyzz.argtypes = [C.POINTER(_Params), C.c_double, C.c_double] + [C.c_void_p] * 11 + [C.c_int64, C.POINTER(_Result)]
        _lib = L
    return _lib


def poisson_time3(a, b, c, u):
    L = load()
    a, b, c, u = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float), np.asarray(c, float), np.asarray(u, float))
    return np.array([L.ref_poisson_time3(float(p), float(q), float(r), float(s)) for p, q, r, s in zip(a.ravel(), b.ravel(), c.ravel(), u.ravel())])


def hitting_time(x, v, bar):
    L = load()
    x, v, bar = np.broadcast_arrays(np.asarray(x, float), np.asarray(v, float), np.asarray(bar, float))
    return np.array([L.ref_hitting_time(float(p), float(q), float(r)) for p, q, r in zip(x.ravel(), v.ravel(), bar.ravel())])


def _csc(G):
    G = sp.csc_matrix(G)
    G.sort_indices()
    return (np.ascontiguousarray(G.indptr, dtype=np.int64), np.ascontiguousarray(G.indices, dtype=np.int64),
            np.ascontiguousarray(G.data, dtype=np.float64))


def barrier_table(barriers, d):
    """(lo, hi, rule_lo, rule_hi, κ_lo, κ_hi) arrays of a list of d (x, rule, κ) triples -- or objects with these attributes --, or of one for all."""
    def one(b):  # a StickyBarriers-like object, or a plain ((lo, hi), (rule_lo, rule_hi), (κ_lo, κ_hi))
        return hasattr(b, "x") or (isinstance(b, tuple) and len(b) == 3 and isinstance(b[1], tuple) and isinstance(b[1][0], str))

    if one(barriers):
        barriers = [barriers] * d
    trip = [(b.x, b.rule, b.κ) if hasattr(b, "x") else b for b in barriers]
    assert len(trip) == d
    lo = np.array([float(b[0][0]) for b in trip])
    hi = np.array([float(b[0][1]) for b in trip])
    rlo = np.array([RULES[str(b[1][0])] for b in trip], dtype=np.int32)
    rhi = np.array([RULES[str(b[1][1])] for b in trip], dtype=np.int32)
    klo = np.array([float(b[2][0]) for b in trip])
    khi = np.array([float(b[2][1]) for b in trip])
    return lo, hi, rlo, rhi, klo, khi


def stickyzz(t0, x0, th0, T, c, barriers, *, gamma, mu=None, target_gamma=None, target_mu=None, strong_upperbounds=False, adapt=False, factor=1.5,
             seed=0, ev_cap=None):
    """One chain.  gamma, mu: the flow ZigZag(Γ, μ) whose pattern is G = G1; target_gamma, target_mu: the Gaussian target (default: the flow's Γ,
    no mean).  Returns a dict: the events t, i, x, theta, kind (EV_*) of the stored events, the counters, status, the final t′ and
    t, x, theta, c, v_old (saved speeds), action, frozen."""
    L = load()
    x = np.array(x0, dtype=np.float64).copy()
    v = np.array(th0, dtype=np.float64).copy()
    d = x.size
    cc = np.ascontiguousarray(np.broadcast_to(np.asarray(c, dtype=np.float64), (d,))).copy()
    cp, rv, nz = _csc(gamma)
    mu = np.ascontiguousarray(np.zeros(d) if mu is None else mu, dtype=np.float64)
    tcp, trv, tnz = _csc(gamma if target_gamma is None else target_gamma)
    lo, hi, rlo, rhi, klo, khi = barrier_table(barriers, d)
    p = _Params()
    p.d, p.adapt, p.strong = d, int(bool(adapt)), int(bool(strong_upperbounds))
    p.colptr, p.rowval, p.nzval, p.mu = cp.ctypes.data, rv.ctypes.data, nz.ctypes.data, mu.ctypes.data
    p.t_colptr, p.t_rowval, p.t_nzval = tcp.ctypes.data, trv.ctypes.data, tnz.ctypes.data
    keep = [cp, rv, nz, mu, tcp, trv, tnz, lo, hi, rlo, rhi, klo, khi]
    if target_mu is not None:
        tmu = np.ascontiguousarray(target_mu, dtype=np.float64)
        p.t_mu = tmu.ctypes.data
        keep.append(tmu)
    p.lo, p.hi, p.klo, p.khi, p.rlo, p.rhi = lo.ctypes.data, hi.ctypes.data, klo.ctypes.data, khi.ctypes.data, rlo.ctypes.data, rhi.ctypes.data
    p.factor, p.seed = float(factor), int(seed)
    if ev_cap is None:
        ev_cap = int(max(4096, 64 * d * max(T - t0, 1.0)))
    ev_cap = int(ev_cap)
    t = np.empty(d)
    vold = np.empty(d)
    action = np.empty(d, dtype=np.int64)
    te, ie, xe, the = np.empty(ev_cap), np.empty(ev_cap, dtype=np.int64), np.empty(ev_cap), np.empty(ev_cap)
    ke = np.empty(ev_cap, dtype=np.int8)
    res = _Result()
    rc = L.ref_stickyzz(C.byref(p), float(t0), float(T), x.ctypes.data, v.ctypes.data, t.ctypes.data, cc.ctypes.data, vold.ctypes.data,
                        action.ctypes.data, te.ctypes.data, ie.ctypes.data, xe.ctypes.data, the.ctypes.data, ke.ctypes.data, ev_cap, C.byref(res))
    del keep
    if rc != 0:
        raise MemoryError("ref_stickyzz")
    n = int(min(res.nevents, ev_cap))
    return dict(t=te[:n].copy(), i=ie[:n].copy(), x=xe[:n].copy(), theta=the[:n].copy(), kind=ke[:n].copy(), num=int(res.num), nacc=int(res.nacc),
                nevents=int(res.nevents), nhit=int(res.nhit), nthaw=int(res.nthaw), nrefl=int(res.nrefl), nadapt=int(res.nadapt),
                ndraw_main=int(res.ndraw_main), status=int(res.status), t_final=float(res.t), t_state=t, x_final=x, theta_final=v, c_final=cc,
                theta_saved=vold, action=action, frozen=(v == 0) & (vold != 0))
