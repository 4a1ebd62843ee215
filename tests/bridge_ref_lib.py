"""ctypes binding of tests/ref/bridge_ref.c: the sequential restatement of the reference's diffusion-bridge sampler (the local ZigZag with
the self-moving Faber-Schauder gradient, research/diffusion_bridge/).  TEST INFRASTRUCTURE ONLY -- the product package never imports it.
Compiled with exactly the flags of oracle/Makefile into tests/ref/_build/ (git-ignored), or into a temporary directory where the tree is
read-only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "bridge_ref.c")
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
        out_dir = tempfile.mkdtemp(prefix="bridge_ref_")
    lib = os.path.join(out_dir, "libbridge_ref.so")
    if force or not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        tmp = lib + ".tmp.%d" % os.getpid()
        subprocess.check_call(["gcc"] + CFLAGS + ["-Wall", "-Wextra", "-shared", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, lib)
    return lib


class _Params(C.Structure):
    _fields_ = [("L", C.c_int32), ("adapt", C.c_int32), ("T", C.c_double), ("alpha", C.c_double), ("beta", C.c_double), ("omega", C.c_double),
                ("factor", C.c_double), ("seed", C.c_uint64)]


class _State(C.Structure):
    _fields_ = [("num", C.c_int64), ("nacc", C.c_int64), ("nevents", C.c_int64), ("nadapt", C.c_int64), ("ndraw_main", C.c_uint64),
                ("ndraw_global", C.c_uint64), ("status", C.c_int32), ("pad_", C.c_int32), ("t_event", C.c_double), ("t_last", C.c_double)]


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.ref_Lambda.restype = C.c_double
        L.ref_Lambda.argtypes = [C.c_double, C.c_int32, C.c_double]
        L.ref_lvl.restype = C.c_int32
        L.ref_lvl.argtypes = [C.c_int64, C.c_int32]
        L.ref_index.restype = C.c_int64
        L.ref_index.argtypes = [C.c_double, C.c_int32, C.c_int32, C.c_double]
        L.ref_dotpsi.restype = C.c_double
        L.ref_dotpsi.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.c_double]
        L.ref_bridge_grad.restype = C.c_int
        L.ref_bridge_grad.argtypes = [C.POINTER(_Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.POINTER(C.c_double)]
        L.ref_bridge_run.restype = C.c_int
        L.ref_bridge_run.argtypes = ([C.POINTER(_Params), C.c_int32, C.c_double, C.c_double, C.c_int32] + [C.c_void_p] * 13
                                     + [C.c_int64, C.POINTER(_State)])
        _lib = L
    return _lib


def Lambda(t, lm, T):
    return load().ref_Lambda(float(t), int(lm), float(T))


def lvl(i, L):
    return int(load().ref_lvl(int(i), int(L)))


def index(s, lev, L, T):
    return int(load().ref_index(float(s), int(lev), int(L), float(T)))


def dotpsi(xi, s, L, T):
    xi = np.ascontiguousarray(xi, dtype=np.float64)
    assert xi.size == (2 << L) + 1
    return load().ref_dotpsi(xi.ctypes.data, float(s), int(L), float(T))


def _params(L, T, alpha, beta, omega, adapt=False, factor=1.8, seed=0):
    p = _Params()
    p.L, p.adapt, p.T, p.alpha, p.beta, p.omega, p.factor, p.seed = int(L), int(bool(adapt)), float(T), float(alpha), float(beta), float(omega), float(factor), int(seed)
    return p


def bridge_grad(xi, t, th, i, tp, u01, *, L, T, alpha, beta, omega):
    """ref_bridge_grad(ξ, t, θ, i, t′, u01): (status, gradient); ξ and t are moved IN PLACE (float64 arrays)."""
    assert xi.dtype == np.float64 and t.dtype == np.float64 and xi.flags.c_contiguous and t.flags.c_contiguous
    th = np.ascontiguousarray(th, dtype=np.float64)
    g = C.c_double(float("nan"))
    st = load().ref_bridge_grad(C.byref(_params(L, T, alpha, beta, omega)), xi.ctypes.data, t.ctypes.data, th.ctypes.data, int(i), float(tp),
                                float(u01), C.byref(g))
    return int(st), float(g.value)


class Chain:
    """One chain of the restatement, resumable: run(T′, flags) continues where the last call stopped, as the device's launches do."""

    def __init__(self, x0, th0, c, *, L, T, alpha, beta, omega, t0=0.0, adapt=False, factor=1.8, seed=0, ev_cap=None):
        self.p = _params(L, T, alpha, beta, omega, adapt, factor, seed)
        d = (2 << int(L)) + 1
        self.d, self.t0 = d, float(t0)
        self.x = np.array(x0, dtype=np.float64).reshape(d).copy()
        self.th = np.array(th0, dtype=np.float64).reshape(d).copy()
        self.c = np.ascontiguousarray(np.broadcast_to(np.asarray(c, dtype=np.float64), (d,))).copy()
        self.t, self.t_old, self.ba, self.bb, self.Q = (np.empty(d) for _ in range(5))
        self.acc = np.zeros(d, dtype=np.int64)
        self.S = _State()
        self.ev_cap = ev_cap
        self._parts = []
        self._fresh = True

    def run(self, Tend, flags=RUN_REFERENCE_TAIL, ev_cap=None):
        cap = int(ev_cap or self.ev_cap or max(4096, 4 * self.d * max(float(Tend) - self.t0, 1.0)))
        before = int(self.S.nevents) if not self._fresh else 0
        while True:
            te, ie, xe, the = np.empty(cap), np.empty(cap, dtype=np.int64), np.empty(cap), np.empty(cap)
            snap = [a.copy() for a in (self.x, self.th, self.c, self.t, self.t_old, self.ba, self.bb, self.Q, self.acc)], bytes(self.S)
            S2 = _State.from_buffer_copy(bytes(self.S))
            S2.nevents = 0  # (events are stored from slot 0 of this call's buffers)
            rc = load().ref_bridge_run(C.byref(self.p), int(self._fresh), self.t0, float(Tend), int(flags), self.x.ctypes.data, self.th.ctypes.data,
                                       self.t.ctypes.data, self.c.ctypes.data, self.t_old.ctypes.data, self.ba.ctypes.data, self.bb.ctypes.data,
                                       self.Q.ctypes.data, self.acc.ctypes.data, te.ctypes.data, ie.ctypes.data, xe.ctypes.data, the.ctypes.data,
                                       cap, C.byref(S2))
            assert rc == 0
            if S2.nevents <= cap:
                break
            for a, b in zip((self.x, self.th, self.c, self.t, self.t_old, self.ba, self.bb, self.Q, self.acc), snap[0]):  # too small: again, larger
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
        return dict(ev, num=int(S.num), nacc=int(S.nacc), nevents=int(S.nevents), nadapt=int(S.nadapt), ndraw_main=int(S.ndraw_main),
                    ndraw_global=int(S.ndraw_global), status=int(S.status), t_event=float(S.t_event), t_last=float(S.t_last), t_state=self.t.copy(),
                    x_final=self.x.copy(), theta_final=self.th.copy(), c_final=self.c.copy(), acc=self.acc.copy())


def bridge(x0, th0, Tend, c, *, L, T, alpha, beta, omega, t0=0.0, adapt=False, factor=1.8, seed=0, flags=RUN_REFERENCE_TAIL, ev_cap=None):
    """One chain in one call.  Returns the dict of Chain.result()."""
    ch = Chain(x0, th0, c, L=L, T=T, alpha=alpha, beta=beta, omega=omega, t0=t0, adapt=adapt, factor=factor, seed=seed, ev_cap=ev_cap)
    ch.run(Tend, flags)
    return ch.result()
