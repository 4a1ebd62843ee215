"""ctypes binding of tests/ref/sticky_notfact_ref.c: the sequential restatement of the reference's sticky Bouncy Particle / Boomerang
(src/ss_not_fact.jl).  TEST INFRASTRUCTURE ONLY -- the product package never imports it.  Compiled with exactly the flags of
oracle/Makefile into tests/ref/_build/ (git-ignored), or into a temporary directory where the tree is read-only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import scipy.sparse as sp

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "sticky_notfact_ref.c")
_HDR = os.path.join(os.path.dirname(_HERE), "include", "pdmp_detmath.h")
CFLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]  # oracle/Makefile's

REF_OK, REF_BOUND_VIOLATED, REF_FROZE_AWAY, REF_STALLED = 0, 1, 2, 3

_lib = None


def build(force=False):
    out_dir = os.path.join(_HERE, "ref", "_build")
    try:
        os.makedirs(out_dir, exist_ok=True)
        if not os.access(out_dir, os.W_OK):
            raise OSError
    except OSError:
        out_dir = tempfile.mkdtemp(prefix="sticky_ref_")
    lib = os.path.join(out_dir, "libsticky_notfact_ref.so")
    if force or not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        tmp = lib + ".tmp.%d" % os.getpid()
        subprocess.check_call(["gcc"] + CFLAGS + ["-Wall", "-Wextra", "-shared", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, lib)
    return lib


class _Params(C.Structure):
    _fields_ = [("d", C.c_int64), ("flow_kind", C.c_int32), ("adapt", C.c_int32), ("strong_upperbounds", C.c_int32), ("pad_", C.c_int32),
                ("colptr", C.c_void_p), ("rowval", C.c_void_p), ("nzval", C.c_void_p), ("mu", C.c_void_p),
                ("t_colptr", C.c_void_p), ("t_rowval", C.c_void_p), ("t_nzval", C.c_void_p), ("t_mu", C.c_void_p),
                ("mu_flow", C.c_void_p), ("kappa", C.c_void_p),
                ("lambda_ref", C.c_double), ("rho", C.c_double), ("c", C.c_double), ("factor", C.c_double), ("seed", C.c_uint64)]


class _Result(C.Structure):
    _fields_ = [("num", C.c_int64), ("nacc", C.c_int64), ("nrefresh", C.c_int64), ("nevents", C.c_int64), ("ndraw_main", C.c_uint64),
                ("status", C.c_int32), ("pad_", C.c_int32), ("t", C.c_double), ("c", C.c_double)]


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.ref_atan.restype = C.c_double
        L.ref_atan.argtypes = [C.c_double]
        L.ref_freezing_time_linear.restype = C.c_double
        L.ref_freezing_time_linear.argtypes = [C.c_double, C.c_double]
        L.ref_freezing_time_boomerang.restype = C.c_double
        L.ref_freezing_time_boomerang.argtypes = [C.c_double, C.c_double, C.c_double]
        L.ref_sspdmp_notfact.restype = C.c_int
        L.ref_sspdmp_notfact.argtypes = [C.POINTER(_Params), C.c_double, C.c_double] + [C.c_void_p] * 8 + [C.c_int64, C.c_void_p, C.POINTER(_Result)]
        _lib = L
    return _lib


def ref_atan(x):
    L = load()
    return np.array([L.ref_atan(float(v)) for v in np.atleast_1d(x)])


def freezing_time_linear(x, th):
    L = load()
    return np.array([L.ref_freezing_time_linear(float(a), float(b)) for a, b in zip(np.atleast_1d(x), np.atleast_1d(th))])


def freezing_time_boomerang(x, th, mu):
    L = load()
    return np.array([L.ref_freezing_time_boomerang(float(a), float(b), float(c))
                     for a, b, c in zip(np.atleast_1d(x), np.atleast_1d(th), np.atleast_1d(mu))])


def _csc(G):
    G = sp.csc_matrix(G)
    G.sort_indices()
    return (np.ascontiguousarray(G.indptr, dtype=np.int64), np.ascontiguousarray(G.indices, dtype=np.int64),
            np.ascontiguousarray(G.data, dtype=np.float64))


def sspdmp_notfact(t0, x0, th0, T, c, kappa, *, flow_kind, gamma, mu, lambda_ref, rho=0.0, mu_flow=None, target=None, strong_upperbounds=False,
                   adapt=False, factor=2.0, seed=0, ev_cap=None, want_free_time=False):
    """One chain.  flow_kind 0: BouncyParticle(gamma, mu, lambda_ref; rho), target = None or (Γt, μt); flow_kind 1: Boomerang(I, mu_flow,
    lambda_ref; rho) on the target Γ = gamma, μ = mu.  Returns a dict: events t [n], x, theta [n x d], f [n x d] bool (n = stored events),
    the counters, status, final t, x, theta, c, f, theta_f and (optionally) free_time [d]."""
    L = load()
    x = np.array(x0, dtype=np.float64).copy()
    th = np.array(th0, dtype=np.float64).copy()
    d = x.size
    cp, rv, nz = _csc(gamma)
    mu = np.ascontiguousarray(np.zeros(d) if mu is None else mu, dtype=np.float64)
    kap = np.ascontiguousarray(np.broadcast_to(np.asarray(kappa, dtype=np.float64), (d,)))
    p = _Params()
    p.d, p.flow_kind, p.adapt, p.strong_upperbounds = d, int(flow_kind), int(bool(adapt)), int(bool(strong_upperbounds))
    p.colptr, p.rowval, p.nzval, p.mu = cp.ctypes.data, rv.ctypes.data, nz.ctypes.data, mu.ctypes.data
    keep = [cp, rv, nz, mu, kap]
    if target is not None:
        tcp, trv, tnz = _csc(target[0])
        tmu = np.ascontiguousarray(np.zeros(d) if target[1] is None else target[1], dtype=np.float64)
        p.t_colptr, p.t_rowval, p.t_nzval, p.t_mu = tcp.ctypes.data, trv.ctypes.data, tnz.ctypes.data, tmu.ctypes.data
        keep += [tcp, trv, tnz, tmu]
    mf = np.ascontiguousarray(np.zeros(d) if mu_flow is None else mu_flow, dtype=np.float64)
    keep.append(mf)
    p.mu_flow, p.kappa = mf.ctypes.data, kap.ctypes.data
    p.lambda_ref, p.rho, p.c, p.factor, p.seed = float(lambda_ref), float(rho), float(c), float(factor), int(seed)
    if ev_cap is None:
        ev_cap = int(max(4096, 64 * d * max(T - t0, 1.0)))
    ev_cap = int(ev_cap)
    te = np.empty(ev_cap)
    xe = np.empty((ev_cap, d))
    the = np.empty((ev_cap, d))
    fe = np.empty((ev_cap, d), dtype=np.uint8)
    thf = np.empty(d)
    f = np.empty(d, dtype=np.uint8)
    ft = np.zeros(d) if want_free_time else None
    res = _Result()
    rc = L.ref_sspdmp_notfact(C.byref(p), float(t0), float(T), x.ctypes.data, th.ctypes.data, thf.ctypes.data, f.ctypes.data, te.ctypes.data,
                              xe.ctypes.data, the.ctypes.data, fe.ctypes.data, ev_cap, ft.ctypes.data if ft is not None else None, C.byref(res))
    if rc != 0:
        raise MemoryError("ref_sspdmp_notfact")
    n = int(min(res.nevents, ev_cap))
    return dict(t=te[:n].copy(), x=xe[:n].copy(), theta=the[:n].copy(), f=fe[:n].astype(bool), num=int(res.num), nacc=int(res.nacc),
                nrefresh=int(res.nrefresh), nevents=int(res.nevents), ndraw_main=int(res.ndraw_main), status=int(res.status),
                t_final=float(res.t), c_final=float(res.c), x_final=x, theta_final=th, f_final=f.astype(bool), theta_f=thf, free_time=ft)
