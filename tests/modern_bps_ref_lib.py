"""ctypes binding of tests/ref/modern_bps_ref.c: the sequential restatement of the reference's speed-recorded Bouncy Particle driver
(src/not_fact_samplers.jl:151-384).  TEST INFRASTRUCTURE ONLY -- the product package never imports it.  Compiled with exactly the flags of
oracle/Makefile into tests/ref/_build/ (git-ignored), or into a temporary directory where the tree is read-only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import scipy.sparse as sp

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "modern_bps_ref.c")
_HDR = os.path.join(os.path.dirname(_HERE), "include", "pdmp_detmath.h")
CFLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]  # oracle/Makefile's

REF_OK, REF_BOUND_VIOLATED, REF_STALLED = 0, 1, 2

_lib = None


def _out_dir():
    out_dir = os.path.join(_HERE, "ref", "_build")
    try:
        os.makedirs(out_dir, exist_ok=True)
        if not os.access(out_dir, os.W_OK):
            raise OSError
    except OSError:
        out_dir = tempfile.mkdtemp(prefix="modern_ref_")
    return out_dir


def _stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR))


def build(force=False):
    lib = os.path.join(_out_dir(), "libmodern_bps_ref.so")
    if force or _stale(lib):
        tmp = lib + ".tmp.%d" % os.getpid()
        subprocess.check_call(["gcc"] + CFLAGS + ["-Wall", "-Wextra", "-shared", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, lib)
    return lib


def build_sanitized_driver():
    """The stand-alone program (the file's own main) under AddressSanitizer and UBSan; returns its path."""
    exe = os.path.join(_out_dir(), "modern_bps_ref_asan")
    if _stale(exe):
        tmp = exe + ".tmp.%d" % os.getpid()
        subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-DMREF_MAIN", "-Wall", "-Wextra", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, exe)
    return exe


class _Params(C.Structure):
    _fields_ = [("d", C.c_int64), ("adapt", C.c_int32), ("oscn", C.c_int32),
                ("t_colptr", C.c_void_p), ("t_rowval", C.c_void_p), ("t_nzval", C.c_void_p), ("t_mu", C.c_void_p),
                ("Lcp", C.c_void_p), ("Lrv", C.c_void_p), ("Lnz", C.c_void_p), ("u_diag", C.c_void_p),
                ("lambda_ref", C.c_double), ("rho", C.c_double), ("c", C.c_double), ("factor", C.c_double), ("seed", C.c_uint64)]


class _Result(C.Structure):
    _fields_ = [("num", C.c_int64), ("nacc", C.c_int64), ("nrefresh", C.c_int64), ("nexpire", C.c_int64), ("nevents", C.c_int64),
                ("nviol", C.c_int64), ("noscn_draws", C.c_int64), ("ndraw_main", C.c_uint64), ("status", C.c_int32), ("pad_", C.c_int32),
                ("t", C.c_double), ("c", C.c_double), ("V", C.c_double)]


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.mref_pdmp.restype = C.c_int
        L.mref_pdmp.argtypes = [C.POINTER(_Params), C.c_double, C.c_double, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.POINTER(_Result)]
        _lib = L
    return _lib


def csc(G):
    G = sp.csc_matrix(G)
    G.sort_indices()
    return (np.ascontiguousarray(G.indptr, dtype=np.int64), np.ascontiguousarray(G.indices, dtype=np.int64),
            np.ascontiguousarray(G.data, dtype=np.float64))


def lower_csc(Lm):
    """A lower-triangular factor as CSC with every structural entry of the lower triangle kept (the diagonal first in each column)."""
    Lm = sp.csc_matrix(sp.tril(sp.csc_matrix(Lm)))
    Lm.sort_indices()
    return (np.ascontiguousarray(Lm.indptr, dtype=np.int64), np.ascontiguousarray(Lm.indices, dtype=np.int64),
            np.ascontiguousarray(Lm.data, dtype=np.float64))


def draw_blocks(d):
    return ((d + 127) >> 7) << 6


def predicted_draws(r, d):
    """The header's draw table, from the event counts of a run that ended with status OK."""
    R = draw_blocks(d)
    return 2 * (1 + r["nevents"] + r["nrefresh"] + r["nexpire"] + r["num"]) + r["num"] + R * (r["nrefresh"] + r["noscn_draws"])


def pdmp(t0, x0, th0, T, c, *, gamma, mu=None, lambda_ref=1.0, rho=0.0, L=None, u_diag=None, oscn=False, adapt=False, factor=2.0, seed=0,
         ev_cap=None):
    """One chain.  T: a float end time, or an int number of records (the reference's `T isa Int`); a pair (T, n) gives both limits.
    Returns a dict: records t [n], x, theta [n x d], the counters, status, final t, x, theta, c, V."""
    Lb = load()
    x = np.array(x0, dtype=np.float64).copy()
    th = np.array(th0, dtype=np.float64).copy()
    d = x.size
    if isinstance(T, tuple):
        T_end, nlim = float(T[0]), int(T[1])
    elif isinstance(T, (int, np.integer)) and not isinstance(T, bool):
        T_end, nlim = float("inf"), int(T)
    else:
        T_end, nlim = float(T), 0
    cp, rv, nz = csc(gamma)
    p = _Params()
    p.d, p.adapt, p.oscn = d, int(bool(adapt)), int(bool(oscn))
    p.t_colptr, p.t_rowval, p.t_nzval = cp.ctypes.data, rv.ctypes.data, nz.ctypes.data
    keep = [cp, rv, nz]
    if mu is not None:
        m = np.ascontiguousarray(mu, dtype=np.float64)
        p.t_mu = m.ctypes.data
        keep.append(m)
    if L is not None:
        lcp, lrv, lnz = lower_csc(L)
        p.Lcp, p.Lrv, p.Lnz = lcp.ctypes.data, lrv.ctypes.data, lnz.ctypes.data
        keep += [lcp, lrv, lnz]
    if u_diag is not None:
        u = np.ascontiguousarray(u_diag, dtype=np.float64)
        p.u_diag = u.ctypes.data
        keep.append(u)
    p.lambda_ref, p.rho, p.c, p.factor, p.seed = float(lambda_ref), float(rho), float(c), float(factor), int(seed)
    if ev_cap is None:
        ev_cap = nlim if nlim > 0 else int(max(64, 4 * lambda_ref * max(T_end - t0, 1.0) * 4))
    ev_cap = int(ev_cap)
    te = np.empty(ev_cap)
    xe = np.empty((ev_cap, d))
    the = np.empty((ev_cap, d))
    res = _Result()
    rc = Lb.mref_pdmp(C.byref(p), float(t0), T_end, nlim, x.ctypes.data, th.ctypes.data, te.ctypes.data, xe.ctypes.data, the.ctypes.data,
                      ev_cap, C.byref(res))
    if rc != 0:
        raise MemoryError("mref_pdmp")
    n = int(min(res.nevents, ev_cap))
    return dict(t=te[:n].copy(), x=xe[:n].copy(), theta=the[:n].copy(), num=int(res.num), nacc=int(res.nacc), nrefresh=int(res.nrefresh),
                nexpire=int(res.nexpire), nevents=int(res.nevents), nviol=int(res.nviol), noscn_draws=int(res.noscn_draws),
                ndraw_main=int(res.ndraw_main), status=int(res.status), t_final=float(res.t), c_final=float(res.c), V_final=float(res.V),
                x_final=x, theta_final=th)


# ---------------------------------------------------------------------------------------------- the reference's envelope case

def envelope_case(gamma, seed=2):
    """test/maintest.jl:209-242 in shape on the suite's Γ (problems.maintest_precision: Γ = SS', S = 1.3I + 0.5 sprandn(8, 8, 0.1)):
    L = LowerTriangular(I + 0.4 randn(d, d)), a non-constant diagonal u for the U form, x0 and θ0 standard normal, c = 20, λref = 1,
    ρ = 0.9, n = 800 samples.  (numpy's generator, not Julia's: the draws differ from the reference's, the construction is the same.)"""
    G = sp.csc_matrix(gamma)
    G.sort_indices()
    d = G.shape[0]
    rng = np.random.default_rng(seed)
    Lm = np.tril(np.eye(d) + 0.4 * rng.standard_normal((d, d)))
    u = 0.5 + np.arange(d) / 4.0
    x0 = rng.standard_normal(d)
    th0 = rng.standard_normal(d)
    return dict(d=d, gamma=G, L=Lm, u=u, x0=x0, th0=th0, c=20.0, lambda_ref=1.0, rho=0.9, n=800)


def envelope_stats(xs, gamma):
    n = xs.shape[0]
    m = np.mean(np.abs(xs.mean(axis=0)))
    cv = np.mean(np.abs(np.cov(xs.T) - np.linalg.inv(sp.csc_matrix(gamma).toarray())))
    return m, cv, 3.0 / np.sqrt(n)
