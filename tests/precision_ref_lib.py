"""ctypes binding of tests/ref/precision_ref.c: the sequential restatement of the reference's precision case study (the sticky ZigZag on the
Cholesky factor of a precision matrix, casestudies/precision/precision.jl).  TEST INFRASTRUCTURE ONLY -- the product package never imports it.
Compiled with exactly the flags of oracle/Makefile into tests/ref/_build/ (git-ignored), or into a temporary directory where the tree is
read-only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "precision_ref.c")
_HDR = os.path.join(os.path.dirname(_HERE), "include", "pdmp_detmath.h")
CFLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]  # oracle/Makefile's

REF_OK, REF_BOUND_VIOLATED, REF_STALLED = 0, 1, 2
RUN_REFERENCE_TAIL, RUN_STOP_BEFORE = 0, 1

_lib = None


def build(force=False):
    out_dir = os.path.join(_HERE, "ref", "_build")
    try:
        os.makedirs(out_dir, exist_ok=True)
        if not os.access(out_dir, os.W_OK):
            raise OSError
    except OSError:
        out_dir = tempfile.mkdtemp(prefix="precision_ref_")
    lib = os.path.join(out_dir, "libprecision_ref.so")
    if force or not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        tmp = lib + ".tmp.%d" % os.getpid()
        subprocess.check_call(["gcc"] + CFLAGS + ["-Wall", "-Wextra", "-shared", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, lib)
    return lib


class _Params(C.Structure):
    _fields_ = [("n", C.c_int32), ("adapt", C.c_int32), ("reversible", C.c_int32), ("strong_upperbounds", C.c_int32), ("N", C.c_double),
                ("gamma0", C.c_double), ("factor", C.c_double), ("seed", C.c_uint64), ("YY", C.c_void_p), ("gam", C.c_void_p), ("mu", C.c_void_p),
                ("kappa", C.c_void_p)]


class _State(C.Structure):
    _fields_ = [("num", C.c_int64), ("nacc", C.c_int64), ("nevents", C.c_int64), ("nadapt", C.c_int64), ("ndraw_main", C.c_uint64),
                ("status", C.c_int32), ("pad_", C.c_int32), ("t_event", C.c_double), ("t_last", C.c_double)]


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.ref_precision_k0.restype = C.c_int64
        L.ref_precision_k0.argtypes = [C.c_int32, C.c_int32]
        L.ref_precision_col.restype = C.c_int32
        L.ref_precision_col.argtypes = [C.c_int32, C.c_int64]
        L.ref_precision_grad.restype = C.c_double
        L.ref_precision_grad.argtypes = [C.c_int32, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_int64]
        L.ref_precision_run.restype = C.c_int
        L.ref_precision_run.argtypes = ([C.POINTER(_Params), C.c_int32, C.c_double, C.c_double, C.c_int32] + [C.c_void_p] * 14
                                        + [C.c_int64, C.POINTER(_State)])
        _lib = L
    return _lib


def k0(n, c):
    return int(load().ref_precision_k0(int(n), int(c)))


def col(n, i):
    return int(load().ref_precision_col(int(n), int(i)))


def grad(YY, N, gamma0, u, i):
    """ref_precision_grad: ∂ϕ/∂u_i in the device's summation order."""
    YY = np.ascontiguousarray(YY, dtype=np.float64)
    u = np.ascontiguousarray(u, dtype=np.float64)
    n = YY.shape[0]
    assert YY.shape == (n, n) and u.size == n * (n + 1) // 2
    return float(load().ref_precision_grad(n, YY.ctypes.data, float(N), float(gamma0), u.ctypes.data, int(i)))


class Chain:
    """One chain of the restatement, resumable: run(T, flags) continues where the last call stopped, as the device's launches do."""
    _STATE = ("x", "th", "c", "t", "t_old", "ba", "bb", "Q", "thf", "f")

    def __init__(self, YY, N, x0, th0, c, gam, mu, kappa, *, gamma0=0.0, t0=0.0, adapt=False, reversible=False, strong_upperbounds=False,
                 factor=1.5, seed=0, ev_cap=None):
        self.YY = np.ascontiguousarray(YY, dtype=np.float64)
        n = self.YY.shape[0]
        d = n * (n + 1) // 2
        self.n, self.d, self.t0 = n, d, float(t0)

        def vec(a):
            return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (d,))).copy()

        self.gam, self.mu, self.kappa = vec(gam), vec(mu), vec(kappa)
        p = _Params()
        p.n, p.adapt, p.reversible, p.strong_upperbounds = n, int(bool(adapt)), int(bool(reversible)), int(bool(strong_upperbounds))
        p.N, p.gamma0, p.factor, p.seed = float(N), float(gamma0), float(factor), int(seed)
        p.YY, p.gam, p.mu, p.kappa = self.YY.ctypes.data, self.gam.ctypes.data, self.mu.ctypes.data, self.kappa.ctypes.data
        self.p = p
        self.x = np.array(x0, dtype=np.float64).reshape(d).copy()
        self.th = np.array(th0, dtype=np.float64).reshape(d).copy()
        self.c = vec(c)
        self.t, self.t_old, self.ba, self.bb, self.Q, self.thf = (np.empty(d) for _ in range(6))
        self.f = np.zeros(d, dtype=np.uint8)
        self.S = _State()
        self.ev_cap = ev_cap
        self._parts = []
        self._fresh = True

    def run(self, Tend, flags=RUN_REFERENCE_TAIL, ev_cap=None):
        cap = int(ev_cap or self.ev_cap or max(4096, 4 * self.d * max(float(Tend) - self.t0, 1.0)))
        before = int(self.S.nevents) if not self._fresh else 0
        arrays = [getattr(self, a) for a in self._STATE]
        while True:
            te, ie, xe, the = np.empty(cap), np.empty(cap, dtype=np.int64), np.empty(cap), np.empty(cap)
            snap = [a.copy() for a in arrays]
            S2 = _State.from_buffer_copy(bytes(self.S))
            S2.nevents = 0  # (events are stored from slot 0 of this call's buffers)
            rc = load().ref_precision_run(C.byref(self.p), int(self._fresh), self.t0, float(Tend), int(flags), self.x.ctypes.data, self.th.ctypes.data,
                                          self.t.ctypes.data, self.c.ctypes.data, self.t_old.ctypes.data, self.ba.ctypes.data, self.bb.ctypes.data,
                                          self.Q.ctypes.data, self.thf.ctypes.data, self.f.ctypes.data, te.ctypes.data, ie.ctypes.data,
                                          xe.ctypes.data, the.ctypes.data, cap, C.byref(S2))
            assert rc == 0
            if S2.nevents <= cap:
                break
            for a, b in zip(arrays, snap):  # too small: again, larger
                a[:] = b
            cap = int(S2.nevents) + 16
        n = int(S2.nevents)
        S2.nevents = before + n
        self.S = S2
        self._fresh = False
        ev = dict(t=te[:n].copy(), i=ie[:n].copy(), x=xe[:n].copy(), theta=the[:n].copy())
        self._parts.append(ev)
        return ev

    def events(self):
        return {f: np.concatenate([p[f] for p in self._parts]) if self._parts else np.empty(0) for f in ("t", "i", "x", "theta")}

    def result(self):
        S = self.S
        ev = self.events()
        return dict(ev, num=int(S.num), nacc=int(S.nacc), nevents=int(S.nevents), nadapt=int(S.nadapt), ndraw_main=int(S.ndraw_main), ndraw_global=0,
                    status=int(S.status), t_event=float(S.t_event), t_last=float(S.t_last), t_state=self.t.copy(), x_final=self.x.copy(),
                    theta_final=self.th.copy(), thf_final=self.thf.copy(), c_final=self.c.copy(), f_final=self.f.copy())


def precision(YY, N, x0, th0, Tend, c, gam, mu, kappa, *, flags=RUN_REFERENCE_TAIL, ev_cap=None, **kw):
    """One chain in one call.  Returns the dict of Chain.result()."""
    ch = Chain(YY, N, x0, th0, c, gam, mu, kappa, ev_cap=ev_cap, **kw)
    ch.run(Tend, flags)
    return ch.result()
