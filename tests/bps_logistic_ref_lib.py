"""ctypes binding of tests/ref/bps_logistic_ref.c: the sequential restatement of the speed-recorded Bouncy Particle on a Bayesian
logistic-regression target.  TEST INFRASTRUCTURE ONLY -- the product package never imports it.  Built the way modern_bps_ref_lib builds
modern_bps_ref.c (which the C file includes): the flags of oracle/Makefile, into tests/ref/_build/ (git-ignored) or a temporary directory."""
import ctypes as C
import os
import subprocess

import numpy as np
import scipy.sparse as sp

import modern_bps_ref_lib as M
from modern_bps_ref_lib import REF_BOUND_VIOLATED, REF_OK, REF_STALLED, draw_blocks, predicted_draws  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "bps_logistic_ref.c")
_DEPS = [_SRC, M._SRC, M._HDR]

_lib = None


def _stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(f) for f in _DEPS)


def build(force=False):
    lib = os.path.join(M._out_dir(), "libbps_logistic_ref.so")
    if force or _stale(lib):
        tmp = lib + ".tmp.%d" % os.getpid()
        subprocess.check_call(["gcc"] + M.CFLAGS + ["-Wall", "-Wextra", "-shared", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, lib)
    return lib


def build_sanitized_driver():
    """The stand-alone program (the file's own main) under AddressSanitizer and UBSan; returns its path."""
    exe = os.path.join(M._out_dir(), "bps_logistic_ref_asan")
    if _stale(exe):
        tmp = exe + ".tmp.%d" % os.getpid()
        subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-DBLREF_MAIN", "-Wall", "-Wextra", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, exe)
    return exe


class _Params(C.Structure):
    _fields_ = [("base", M._Params), ("n", C.c_int64), ("A_colptr", C.c_void_p), ("A_rowval", C.c_void_p), ("A_nzval", C.c_void_p),
                ("At_colptr", C.c_void_p), ("At_rowval", C.c_void_p), ("At_nzval", C.c_void_p), ("y", C.c_void_p), ("m", C.c_void_p),
                ("gamma0", C.c_double)]


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.blref_pdmp.restype = C.c_int
        L.blref_pdmp.argtypes = [C.POINTER(_Params), C.c_double, C.c_double, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.POINTER(M._Result)]
        L.blref_eval.restype = C.c_int
        L.blref_eval.argtypes = [C.POINTER(_Params)] + [C.c_void_p] * 4
        _lib = L
    return _lib


def design(A):
    """A and its transpose as CSC index / value arrays, explicit zeros kept, rows ascending."""
    A = sp.csc_matrix(A, dtype=np.float64)
    A.sort_indices()
    At = sp.csc_matrix(sp.csr_matrix((A.data, A.indices, A.indptr), shape=(A.shape[1], A.shape[0])))
    At.sort_indices()
    f = lambda a, t: np.ascontiguousarray(a, dtype=t)
    return A, At, [f(A.indptr, np.int64), f(A.indices, np.int64), f(A.data, np.float64),
                   f(At.indptr, np.int64), f(At.indices, np.int64), f(At.data, np.float64)]


def _params(A, y, m, gamma0):
    A, At, arrs = design(A)
    n, d = A.shape
    yv = np.ascontiguousarray(y, dtype=np.float64)
    mv = np.ones(n) if m is None else np.ascontiguousarray(m, dtype=np.float64)
    assert yv.shape == (n,) and mv.shape == (n,)
    p = _Params()
    p.base.d, p.n = d, n
    (p.A_colptr, p.A_rowval, p.A_nzval, p.At_colptr, p.At_rowval, p.At_nzval) = [a.ctypes.data for a in arrs]
    p.y, p.m, p.gamma0 = yv.ctypes.data, mv.ctypes.data, float(gamma0)
    return p, arrs + [yv, mv]


def evaluate(A, y, m, gamma0, x, th):
    """(dϕ [2], ∇ϕ [d]) of the restatement at (x, θ)."""
    Lb = load()
    p, keep = _params(A, y, m, gamma0)
    x = np.ascontiguousarray(x, dtype=np.float64)
    th = np.ascontiguousarray(th, dtype=np.float64)
    dphi = np.empty(2)
    grad = np.empty(p.base.d)
    if Lb.blref_eval(C.byref(p), x.ctypes.data, th.ctypes.data, dphi.ctypes.data, grad.ctypes.data) != 0:
        raise MemoryError("blref_eval")
    return dphi, grad


def pdmp(t0, x0, th0, T, c, *, A, y, m=None, gamma0=0.0, lambda_ref=1.0, rho=0.0, L=None, u_diag=None, oscn=False, adapt=False, factor=2.0,
         seed=0, ev_cap=None):
    """One chain; the arguments and the returned dict of modern_bps_ref_lib.pdmp with the target given as (A, y, m, gamma0)."""
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
    p, keep = _params(A, y, m, gamma0)
    assert p.base.d == d
    b = p.base
    b.adapt, b.oscn = int(bool(adapt)), int(bool(oscn))
    if L is not None:
        lcp, lrv, lnz = M.lower_csc(L)
        b.Lcp, b.Lrv, b.Lnz = lcp.ctypes.data, lrv.ctypes.data, lnz.ctypes.data
        keep += [lcp, lrv, lnz]
    if u_diag is not None:
        u = np.ascontiguousarray(u_diag, dtype=np.float64)
        b.u_diag = u.ctypes.data
        keep.append(u)
    b.lambda_ref, b.rho, b.c, b.factor, b.seed = float(lambda_ref), float(rho), float(c), float(factor), int(seed)
    if ev_cap is None:
        ev_cap = nlim if nlim > 0 else int(max(64, 4 * lambda_ref * max(T_end - t0, 1.0) * 4))
    ev_cap = int(ev_cap)
    te = np.empty(ev_cap)
    xe = np.empty((ev_cap, d))
    the = np.empty((ev_cap, d))
    res = M._Result()
    rc = Lb.blref_pdmp(C.byref(p), float(t0), T_end, nlim, x.ctypes.data, th.ctypes.data, te.ctypes.data, xe.ctypes.data, the.ctypes.data,
                       ev_cap, C.byref(res))
    if rc != 0:
        raise MemoryError("blref_pdmp")
    k = int(min(res.nevents, ev_cap))
    return dict(t=te[:k].copy(), x=xe[:k].copy(), theta=the[:k].copy(), num=int(res.num), nacc=int(res.nacc), nrefresh=int(res.nrefresh),
                nexpire=int(res.nexpire), nevents=int(res.nevents), nviol=int(res.nviol), noscn_draws=int(res.noscn_draws),
                ndraw_main=int(res.ndraw_main), status=int(res.status), t_final=float(res.t), c_final=float(res.c), V_final=float(res.V),
                x_final=x, theta_final=th)


# ---------------------------------------------------------------------------------------------- the posterior envelope case

ENVELOPE_SEEDS = (0, 1, 2)


def envelope_case():
    """d = 2, n = 30, γ0 = 1: a fixed seeded data set (numpy's generator), c = 20, λref = 1, ρ = 0.9, adapt; 1600 records (800 did not meet the
    19-of-20 condition of tests/test_bps_logistic_ref.py::test_posterior_envelope, whose docstring has the figures)."""
    rng = np.random.default_rng(20240)
    n, d = 30, 2
    A = rng.standard_normal((n, d))
    beta = np.array([1.0, -0.7])
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-A @ beta))).astype(np.float64)
    return dict(d=d, n=n, A=A, y=y, m=np.ones(n), gamma0=1.0, x0=np.zeros(d), th0=np.array([1.0, -1.0]) / np.sqrt(2.0), c=20.0, lambda_ref=1.0,
                rho=0.9, nrec=1600)


def posterior_quadrature(E, half_width, points):
    """Mean and covariance of exp(−ϕ) on the product grid [−half_width, half_width]² around 0 with `points` nodes per axis (trapezoid rule)."""
    g = np.linspace(-half_width, half_width, points)
    X1, X2 = np.meshgrid(g, g, indexing="ij")
    X = np.stack([X1.ravel(), X2.ravel()], axis=1)
    eta = X @ E["A"].T
    phi = (E["m"] * np.logaddexp(0.0, eta) - E["y"] * eta).sum(axis=1) + 0.5 * E["gamma0"] * (X * X).sum(axis=1)
    w = np.exp(-(phi - phi.min()))
    w /= w.sum()
    mean = w @ X
    Xc = X - mean
    cov = (Xc * w[:, None]).T @ Xc
    return mean, cov


def envelope_stats(xs, mean, cov):
    """test/maintest.jl's envelope form on coordinates standardised by the quadrature truth: z = L⁻¹(x − mean) with cov = L L'; returns
    mean|mean(z)|, mean|cov(z) − I| and the bound 3/√n."""
    Lc = np.linalg.cholesky(cov)
    z = np.linalg.solve(Lc, (xs - mean).T).T
    k = z.shape[0]
    return np.mean(np.abs(z.mean(axis=0))), np.mean(np.abs(np.cov(z.T) - np.eye(z.shape[1]))), 3.0 / np.sqrt(k)
