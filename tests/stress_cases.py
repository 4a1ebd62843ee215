"""The draws of the four oldest randomised suites -- tests/test_gpu_stress_parity.py, test_gpu_stress_general.py, test_gpu_stress_sticky.py and
test_gpu_stress_bps.py -- as functions that need no device, with the oracle's chains of every draw.  TEST INFRASTRUCTURE ONLY.

The draws are what those files drew inline until now: the same seeds and the same order of rng calls (tests/test_stress_cases_ref.py pins a
fingerprint per family, so a refactor that shifts a draw fails there, on the CPU).  The same CPU test asserts that every reference chain of
every draw has status 0, which is why the device tests ASSERT it too instead of skipping, and records what the draws reach.

What the census found thin is appended, never replaced: bps_draw(16 ..) and factboomerang_draw(14 ..) come from generators of their own
whose horizon is doubled until the oracle gives every chain 100 events; the old draws stay as they are, thin ones included."""
import functools

import numpy as np
import scipy.sparse as sp

import oracle_lib as O


def _pkg():
    from __graft_entry__ import load_package
    return load_package()


def _csc(G):
    G = sp.csc_matrix(G)
    G.sort_indices()
    return G


def two_hop_max(G):
    A = sp.csc_matrix((np.ones(G.nnz), G.indices, G.indptr), shape=G.shape)
    return int(np.diff(sp.csc_matrix(A @ A).indptr).max())


def col_max(G):
    return int(np.diff(G.indptr).max())


def zigzag_kernel(G, kern="auto"):
    """The event loop select_family (csrc/pdmp_capi.hip) gives a plain ZigZag ensemble below d = 2048: the general kernel beyond one lane per
    member; else a speculative kernel where its geometry holds (zz_spec_supported: |S| <= 32, |G1| <= 15), and the one-event kernel elsewhere
    and under PDMP_KERNEL=seq.  A prefix for the speculative family, whose instantiations have names of their own."""
    if two_hop_max(G) > 64 or col_max(G) > 64:
        return "zz_general_run_kernel"
    if kern == "seq" or two_hop_max(G) > 32 or col_max(G) > 15:
        return "zz_local_run_kernel"
    return "zz_local_spec"


def sticky_kernel(G, kern="auto"):
    if two_hop_max(G) > 64 or col_max(G) > 64:
        return "zz_general_run_kernel"
    if kern == "seq" or two_hop_max(G) > 16 or col_max(G) > 15:
        return "zz_sticky_run_kernel"
    return "zz_sticky_spec_kernel"


# ------------------------------------------------------------------------------------------------------------ test_gpu_stress_parity.py

def _parity_graph(rng):
    pkg = _pkg()
    kind = rng.integers(0, 3)
    if kind == 0:
        n = int(rng.integers(3, 14))
        G = pkg.problems.gmrf_precision(n, eps=float(rng.uniform(0.01, 1.0)))
    elif kind == 1:  # banded: k up to 7, two-hop zone up to 13
        d = int(rng.integers(5, 200))
        w = int(rng.integers(1, 4))
        diags = [np.full(d, 2.0 * w + 1.0 + rng.random())] + [np.full(d - o, -rng.uniform(0.2, 1.0)) for o in range(1, w + 1)]
        G = sp.diags(diags + diags[1:], [0] + list(range(1, w + 1)) + [-o for o in range(1, w + 1)], format="csc")
    else:  # random sparse symmetric, diagonally dominant, small degree
        d = int(rng.integers(8, 120))
        R = sp.random(d, d, density=min(1.5 / d, 0.5), random_state=rng, data_rvs=rng.standard_normal, format="csc")
        A = R + R.T
        G = sp.csc_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=0)).ravel() + 1.0))
    return _csc(G)


PARITY_SLICES_N, PARITY_OPTIONS_N, PARITY_STICKY_N = 12, 14, 8


@functools.lru_cache(maxsize=None)
def parity_slices_draw(case):
    """test_random_slices_and_tiny_traces_zigzag"""
    rng = np.random.default_rng(1000 + case)
    G = _parity_graph(rng)
    d = G.shape[0]
    nch = 3
    x0 = rng.standard_normal((nch, d))
    th0 = rng.choice([-1.0, -0.5, 0.5, 1.0], (nch, d))
    adapt = bool(rng.integers(0, 2))
    c = _pkg().problems.column_norms(G) * (1.2 if not adapt else float(rng.uniform(0.3, 1.0)))
    T = float(rng.uniform(2.0, 12.0)) * min(1.0, 60.0 / d)
    cap = int(rng.integers(8, 64))
    seed = 5000 + case
    cuts = np.sort(rng.uniform(0, T, size=int(rng.integers(1, 6))))
    return dict(case=case, G=G, d=d, nch=nch, x0=x0, th0=th0, adapt=adapt, c=c, T=T, cap=cap, seed=seed, cuts=cuts)


@functools.lru_cache(maxsize=None)
def parity_slices_refs(case):
    P = parity_slices_draw(case)
    return tuple(O.spdmp_zigzag(P["G"], None, P["G"], P["x0"][k], P["th0"][k], P["c"], P["T"], seed=P["seed"] + k, adapt=P["adapt"])
                 for k in range(P["nch"]))


@functools.lru_cache(maxsize=None)
def parity_options_draw(case):
    """test_random_means_bounds_and_refresh_zigzag"""
    rng = np.random.default_rng(3000 + case)
    G = _parity_graph(rng)
    d = G.shape[0]
    nch = 2
    Gb = sp.csc_matrix(0.9 * G) if rng.integers(0, 2) else G
    mu_b = 0.4 * rng.standard_normal(d) if rng.integers(0, 2) else None
    mu_t = (mu_b if (mu_b is not None and rng.integers(0, 2)) else 0.4 * rng.standard_normal(d)) if rng.integers(0, 2) else None
    sig = 0.5 + rng.random(d)
    lam = float(rng.uniform(0.2, 1.5)) if rng.integers(0, 2) else 0.0
    t0 = float(rng.uniform(0.0, 2.0)) if rng.integers(0, 2) else 0.0
    x0 = rng.standard_normal((nch, d))
    th0 = sig * rng.choice([-1.0, 1.0], (nch, d))
    adapt = bool(rng.integers(0, 2))
    c = _pkg().problems.column_norms(G) * (float(rng.uniform(2.5, 4.0)) if not adapt else float(rng.uniform(0.3, 1.5)))
    T = t0 + float(rng.uniform(2.0, 12.0)) * min(1.0, 60.0 / d)
    cap = int(rng.integers(16, 128))
    seed = 3500 + 10 * case
    return dict(case=case, G=G, Gb=Gb, d=d, nch=nch, mu_b=mu_b, mu_t=mu_t, sig=sig, lam=lam, t0=t0, x0=x0, th0=th0, adapt=adapt, c=c, T=T, cap=cap,
                seed=seed)


@functools.lru_cache(maxsize=None)
def parity_options_refs(case):
    P = parity_options_draw(case)
    kw = dict(t0=P["t0"], target_mu=P["mu_t"], adapt=P["adapt"], factor=1.8, sigma=P["sig"])
    if P["lam"] > 0:
        kw["lambda_ref"] = P["lam"]
    return tuple(O.spdmp_zigzag(P["Gb"], P["mu_b"], P["G"], P["x0"][k], P["th0"][k], P["c"], P["T"], seed=P["seed"] + k, **kw) for k in range(P["nch"]))


@functools.lru_cache(maxsize=None)
def parity_sticky_draw(case):
    """test_random_slices_and_tiny_traces_sticky"""
    rng = np.random.default_rng(2000 + case)
    G = _parity_graph(rng)
    d = G.shape[0]
    nch = 2
    x0 = rng.standard_normal((nch, d))
    th0 = rng.choice([-1.0, 1.0], (nch, d))
    c = 1.5 * _pkg().problems.column_norms(G)
    kappa = rng.uniform(0.1, 2.0, d)
    reversible, strong = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    T = float(rng.uniform(2.0, 10.0)) * min(1.0, 60.0 / d)
    cap = int(rng.integers(8, 64))
    seed = 7000 + case
    cuts = np.sort(rng.uniform(0, T, size=int(rng.integers(1, 5))))
    return dict(case=case, G=G, d=d, nch=nch, x0=x0, th0=th0, c=c, kappa=kappa, reversible=reversible, strong=strong, T=T, cap=cap, seed=seed, cuts=cuts)


@functools.lru_cache(maxsize=None)
def parity_sticky_refs(case):
    P = parity_sticky_draw(case)
    return tuple(O.sspdmp_zigzag(P["G"], None, P["G"], P["x0"][k], P["th0"][k], P["c"], P["kappa"], P["T"], seed=P["seed"] + k, adapt=True,
                                 reversible=P["reversible"], strong_upperbounds=P["strong"]) for k in range(P["nch"]))


# ----------------------------------------------------------------------------------------------------------- test_gpu_stress_general.py

def _general_graph(rng, dense):
    pkg = _pkg()
    if dense:  # two-hop sets beyond 64 members: R R' of a sparse R
        d = int(rng.integers(90, 180))
        R = sp.random(d, d, density=float(rng.uniform(0.04, 0.09)), random_state=rng, data_rvs=rng.standard_normal, format="csc")
        G = sp.csc_matrix(R @ R.T + 2.0 * sp.identity(d))
    else:
        kind = rng.integers(0, 3)
        if kind == 0:
            G = pkg.problems.gmrf_precision(int(rng.integers(3, 12)), eps=float(rng.uniform(0.05, 1.0)))
        elif kind == 1:
            G = pkg.problems.maintest_precision(int(rng.integers(4, 40)))
        else:
            d = int(rng.integers(8, 100))
            R = sp.random(d, d, density=min(1.5 / d, 0.5), random_state=rng, data_rvs=rng.standard_normal, format="csc")
            A = R + R.T
            G = A + sp.diags(np.asarray(abs(A).sum(axis=0)).ravel() + 1.0)
    return _csc(G)


FACTBOOMERANG_OLD_N, FACTBOOMERANG_N, WIDE_ZIGZAG_N = 14, 20, 8
MIN_EVENTS_NEW = 100  # what an appended draw's horizon is doubled up to, per chain


def _factboomerang_refs(P):
    return tuple(O.spdmp_zigzag(P["G"], P["mu"], P["G"], P["x0"][k], P["th0"][k], P["c"], P["T"], seed=P["seed"] + k, lambda_ref=P["lam"], rho=P["rho"],
                                sigma=P["sig"], adapt=P["adapt"], factor=1.7, factboomerang=True) for k in range(P["nch"]))


@functools.lru_cache(maxsize=None)
def factboomerang_draw(case):
    """test_random_factboomerang: cases 0..13 as they always were; 14.. the same draw with the horizon doubled until every chain has 100 events."""
    pkg = _pkg()
    rng = np.random.default_rng(8000 + case)
    G = _general_graph(rng, dense=False)
    d = G.shape[0]
    nch = 2
    mu = 0.3 * rng.standard_normal(d) if rng.integers(0, 2) else np.zeros(d)
    sig = 0.5 + rng.random(d) if rng.integers(0, 2) else np.ones(d)
    lam = float(rng.uniform(0.1, 1.0))
    rho = float(rng.uniform(0.0, 0.9)) if rng.integers(0, 2) else 0.0
    x0 = rng.standard_normal((nch, d))
    th0 = sig * rng.standard_normal((nch, d))
    adapt = bool(rng.integers(0, 2))
    c = pkg.problems.column_norms(G) * (float(rng.uniform(2.0, 4.0)) if not adapt else float(rng.uniform(0.2, 1.0)))
    T = float(rng.uniform(4.0, 20.0)) * min(1.0, 40.0 / d)
    cap = int(rng.integers(16, 96))
    seed = 8100 + 10 * case
    cuts = np.sort(rng.uniform(0, T, size=int(rng.integers(0, 4))))
    P = dict(case=case, G=G, d=d, nch=nch, mu=mu, sig=sig, lam=lam, rho=rho, x0=x0, th0=th0, adapt=adapt, c=c, T=T, cap=cap, seed=seed, cuts=cuts)
    if case >= FACTBOOMERANG_OLD_N:
        for _ in range(10):
            rs = _factboomerang_refs(P)
            if any(r["status"] != 0 for r in rs) or min(len(r["events"]) for r in rs) >= MIN_EVENTS_NEW:
                break
            P["T"], P["cuts"] = 2.0 * P["T"], 2.0 * P["cuts"]
    return P


@functools.lru_cache(maxsize=None)
def factboomerang_refs(case):
    return _factboomerang_refs(factboomerang_draw(case))


@functools.lru_cache(maxsize=None)
def wide_zigzag_draw(case):
    """test_random_wide_neighbourhoods_zigzag"""
    pkg = _pkg()
    rng = np.random.default_rng(8500 + case)
    G = _general_graph(rng, dense=True)
    d = G.shape[0]
    nch = 2
    Gb = sp.csc_matrix(0.85 * G) if rng.integers(0, 2) else G
    mu_b = 0.3 * rng.standard_normal(d) if rng.integers(0, 2) else None
    sig = 0.5 + rng.random(d)
    lam = float(rng.uniform(0.2, 1.0)) if rng.integers(0, 2) else 0.0
    x0 = rng.standard_normal((nch, d))
    th0 = sig * rng.choice([-1.0, 1.0], (nch, d))
    adapt = bool(rng.integers(0, 2))
    c = pkg.problems.column_norms(G) * (float(rng.uniform(2.5, 4.0)) if not adapt else float(rng.uniform(0.3, 1.5)))
    T = float(rng.uniform(1.0, 4.0))
    cap = int(rng.integers(16, 128))
    seed = 8600 + 10 * case
    cuts = np.sort(rng.uniform(0, T, size=int(rng.integers(0, 4))))
    return dict(case=case, G=G, Gb=Gb, d=d, nch=nch, mu_b=mu_b, sig=sig, lam=lam, x0=x0, th0=th0, adapt=adapt, c=c, T=T, cap=cap, seed=seed, cuts=cuts)


@functools.lru_cache(maxsize=None)
def wide_zigzag_refs(case):
    P = wide_zigzag_draw(case)
    kw = dict(adapt=P["adapt"], factor=1.6, sigma=P["sig"])
    if P["lam"] > 0:
        kw["lambda_ref"] = P["lam"]
    return tuple(O.spdmp_zigzag(P["Gb"], P["mu_b"], P["G"], P["x0"][k], P["th0"][k], P["c"], P["T"], seed=P["seed"] + k, **kw) for k in range(P["nch"]))


# ------------------------------------------------------------------------------------------------------------ test_gpu_stress_sticky.py

STICKY_OPTIONS_N = 12


@functools.lru_cache(maxsize=None)
def sticky_options_draw(case):
    """test_random_sticky_options"""
    pkg = _pkg()
    rng = np.random.default_rng(9100 + case)
    kind = int(rng.integers(0, 3))
    if kind == 0:
        n = int(rng.integers(4, 30))
        G = pkg.problems.gmrf_precision(n, eps=float(rng.uniform(0.05, 1.0)))
    elif kind == 1:
        d = int(rng.integers(10, 400))
        w = int(rng.integers(1, 3))
        diags = [np.full(d, 2.0 * w + 1.0 + rng.random())] + [np.full(d - o, -rng.uniform(0.2, 1.0)) for o in range(1, w + 1)]
        G = sp.diags(diags + diags[1:], [0] + list(range(1, w + 1)) + [-o for o in range(1, w + 1)], format="csc")
    else:
        d = int(rng.integers(8, 150))
        R = sp.random(d, d, density=min(1.5 / d, 0.5), random_state=rng, data_rvs=rng.standard_normal, format="csc")
        A = R + R.T
        G = sp.csc_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=0)).ravel() + 1.0))
    G = _csc(G)
    d = G.shape[0]
    Gb = sp.csc_matrix(0.9 * G) if rng.integers(0, 2) else G
    mu_b = 0.3 * rng.standard_normal(d) if rng.integers(0, 2) else None
    mu_t = (mu_b if (mu_b is not None and rng.integers(0, 2)) else 0.3 * rng.standard_normal(d)) if rng.integers(0, 2) else None
    nch = 2
    x0 = rng.standard_normal((nch, d))
    th0 = rng.choice([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5], (nch, d))
    adapt = bool(rng.integers(0, 2))
    c = pkg.problems.column_norms(G) * (float(rng.uniform(2.0, 4.0)) if not adapt else float(rng.uniform(0.3, 1.5)))
    kappa = rng.uniform(0.2, 3.0, d)
    rev, strong = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    T = float(rng.uniform(4.0, 30.0)) * min(1.0, 40.0 / d)
    seed = 9300 + 10 * case
    return dict(case=case, kind=kind, G=G, Gb=Gb, d=d, nch=nch, mu_b=mu_b, mu_t=mu_t, x0=x0, th0=th0, adapt=adapt, c=c, kappa=kappa, rev=rev, strong=strong,
                T=T, seed=seed)


@functools.lru_cache(maxsize=None)
def sticky_options_refs(case):
    P = sticky_options_draw(case)
    return tuple(O.sspdmp_zigzag(P["Gb"], P["mu_b"], P["G"], P["x0"][k], P["th0"][k], P["c"], P["kappa"], P["T"], target_mu=P["mu_t"], seed=P["seed"] + k,
                                 adapt=P["adapt"], reversible=P["rev"], strong_upperbounds=P["strong"]) for k in range(P["nch"]))


# --------------------------------------------------------------------------------------------------------------- test_gpu_stress_bps.py

BPS_OLD_N, BPS_N = 16, 24
# what the appended draws must reach, one requirement per draw (the rest of a draw is random): (d, subsample, adapt, local_bound, mean)
_BPS_EXTRA = ((1, False, False, False, True), (1025, False, True, False, False), (None, True, True, False, None), (None, True, False, False, None),
              (None, False, None, True, True), (None, True, True, False, True), (1025, True, False, False, True), (1, True, True, False, False))


def _bps_mass(G, L):
    """B.L of check() in tests/test_gpu_bps_parity.py: the reference's constructor's cholesky(Γ).L, or the explicit factor."""
    pkg = _pkg()
    B = pkg.BouncyParticle(G, np.zeros(G.shape[0]), 1.0, 0.0, **({} if isinstance(L, str) else {"L": L}))
    return B.L


def _bps_refs(P):
    return tuple(O.pdmp_bps(P["G"], P["mu"], P["x0"][k], P["th0"][k], P["c"], P["T"], lambda_ref=P["lam"], rho=P["rho"], adapt=P["adapt"], factor=2.0,
                            seed=P["seed"] + k, ev_cap=20000, mass_L=_bps_mass(P["G"], P["L"]), local_bound=P["local_bound"], subsample=P["subsample"])
                 for k in range(P["nch"]))


@functools.lru_cache(maxsize=None)
def bps_draw(case):
    """test_random_bps_options: cases 0..15 as they always were; 16.. from a generator that forces what the old draws do not reach."""
    pkg = _pkg()
    rng = np.random.default_rng(9500 + case)
    if case >= BPS_OLD_N:
        want_d, want_sub, want_adapt, want_lb, want_mu = _BPS_EXTRA[case - BPS_OLD_N]
        kind = int(rng.integers(0, 3))
        if want_d is not None:
            d, G = want_d, sp.identity(want_d, format="csc")
        elif kind == 0:
            d = int(rng.choice([3, 17, 64, 65, 200]))
            G = sp.identity(d, format="csc")
        elif kind == 1:
            n = int(rng.integers(3, 12))
            G, d = pkg.problems.gmrf_precision(n, eps=float(rng.uniform(0.1, 1.0))), n * n
        else:
            d = int(rng.integers(4, 40))
            G = sp.csc_matrix(sp.diags(rng.uniform(0.5, 2.0, d)))
        G = _csc(G)
        mu = 0.5 * rng.standard_normal(d) if (bool(rng.integers(0, 2)) if want_mu is None else want_mu) else None
        nch = 2
        x0, th0 = rng.standard_normal((nch, d)), rng.standard_normal((nch, d))
        lam = float(rng.choice([0.3, 1.0, 2.5]))
        rho = float(rng.choice([0.0, 0.0, 0.4]))
        adapt = bool(rng.integers(0, 2)) if want_adapt is None else want_adapt
        local_bound, subsample = want_lb, want_sub
        c = float(rng.uniform(0.5, 2.0)) if adapt or local_bound else float(rng.uniform(3.0, 6.0)) * float(np.sqrt(d))
        T = float(rng.uniform(5.0, 25.0)) * min(1.0, 200.0 / d)
        L = "chol" if rng.integers(0, 2) else sp.identity(d, format="csc")
        P = dict(case=case, kind=kind, G=G, d=d, mu=mu, nch=nch, x0=x0, th0=th0, lam=lam, rho=rho, adapt=adapt, local_bound=local_bound, subsample=subsample,
                 c=c, T=T, L=L, seed=9600 + 10 * case)
        for _ in range(10):
            rs = _bps_refs(P)
            if any(r["status"] != 0 for r in rs) or min(r["nevents"] for r in rs) >= MIN_EVENTS_NEW:
                break
            P["T"] = 2.0 * P["T"]
        return P
    kind = int(rng.integers(0, 3))
    if kind == 0:
        d = int(rng.choice([1, 3, 17, 64, 65, 200, 1024, 1025]))
        G = sp.identity(d, format="csc")
    elif kind == 1:
        n = int(rng.integers(3, 12))
        G = pkg.problems.gmrf_precision(n, eps=float(rng.uniform(0.1, 1.0)))
        d = n * n
    else:
        d = int(rng.integers(4, 40))
        G = pkg.problems.maintest_precision(d) if d == 8 else sp.csc_matrix(sp.diags(rng.uniform(0.5, 2.0, d)))
    G = _csc(G)
    mu = 0.5 * rng.standard_normal(d) if rng.integers(0, 2) else None
    nch = 2
    x0, th0 = rng.standard_normal((nch, d)), rng.standard_normal((nch, d))
    lam = float(rng.choice([0.3, 1.0, 2.5]))  # (BouncyParticle needs a strictly positive refreshment rate: the engine refuses 0, as the reference's sampler would never mix)
    rho = float(rng.choice([0.0, 0.0, 0.4])) if lam > 0 else 0.0
    adapt = bool(rng.integers(0, 2))
    local_bound = bool(rng.integers(0, 4) == 0)
    subsample = bool(rng.integers(0, 4) == 0) and not local_bound
    c = float(rng.uniform(0.5, 2.0)) if adapt or local_bound else float(rng.uniform(3.0, 6.0)) * float(np.sqrt(d))
    T = float(rng.uniform(5.0, 25.0)) * min(1.0, 200.0 / d)
    L = "chol" if rng.integers(0, 2) else sp.identity(d, format="csc")
    return dict(case=case, kind=kind, G=G, d=d, mu=mu, nch=nch, x0=x0, th0=th0, lam=lam, rho=rho, adapt=adapt, local_bound=local_bound, subsample=subsample,
                c=c, T=T, L=L, seed=9600 + 10 * case)


@functools.lru_cache(maxsize=None)
def bps_refs(case):
    return _bps_refs(bps_draw(case))
