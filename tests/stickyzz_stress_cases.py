"""The draws of tests/test_gpu_stickyzz_stress.py -- the randomised and the named-edge suite of the barrier ZigZag (stickyzz, src/stickyzz.jl;
zz_barrier_run_kernel, csrc/pdmp_barrier.hip) -- as functions that need no device, with the restatement's chains (tests/ref/stickyzz_ref.c) of
every draw.  TEST INFRASTRUCTURE ONLY.  The pattern is tests/stress_cases.py's: fixed seeds, lru_cached *_draw / *_refs pairs, a census on the
CPU (tests/test_stickyzz_stress_cases_ref.py) that pins a fingerprint per family and asserts what the draws reach.  Draws are appended, never
reseeded or reordered.

A draw is one dict for both families: G (target Γ), Gb (flow Γ), mu_b / mu_t (flow / target mean or None), t0, T, x0, th0 [nch x d], c, adapt,
strong, bars (a list of d plain triples ((lo, hi), (rule_lo, rule_hi), (κ_lo, κ_hi))), cap (trace capacity), cuts (RUN_STOP_BEFORE times in
(t0, T), one of them repeated), seed (chain k runs seed + k)."""
import functools
import hashlib

import numpy as np
import scipy.sparse as sp

import stickyzz_cases as K
import stickyzz_ref_lib as R
from stress_cases import _csc, _parity_graph, _pkg, col_max, sticky_kernel, two_hop_max  # noqa: F401 (re-exported for the tests)

INF = float("inf")
RULE_NAMES = ("sticky", "reflect", "reversible")
FACTOR = 1.5  # stickyzz's default multiplier
MIN_EVENTS, MAX_EVENTS = 200, 20000  # what a family-A horizon is doubled up to per chain, and where the doubling stops as a cap on work
EV_CAP = 1 << 16


def run_refs(P):
    """The restatement's chain of every chain of a draw."""
    return tuple(R.stickyzz(P["t0"], P["x0"][k], P["th0"][k], P["T"], P["c"], P["bars"], gamma=P["Gb"], mu=P["mu_b"], target_gamma=P["G"],
                            target_mu=P["mu_t"], strong_upperbounds=P["strong"], adapt=P["adapt"], factor=FACTOR, seed=P["seed"] + k, ev_cap=EV_CAP)
                 for k in range(P["nch"]))


def fingerprint(P):
    """A hash over the drawn arrays: a refactor that shifts one rng call changes it."""
    h = hashlib.sha256()
    tab = R.barrier_table(P["bars"], P["d"])
    for a in (P["G"].indptr, P["G"].indices, P["G"].data, P["Gb"].data, P["x0"], P["th0"], P["c"], P["cuts"], *tab,
              np.zeros(0) if P["mu_b"] is None else P["mu_b"], np.zeros(0) if P["mu_t"] is None else P["mu_t"]):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(repr((P["d"], P["nch"], P["t0"], P["T"], P["adapt"], P["strong"], P["cap"], P["seed"])).encode())
    return h.hexdigest()[:12]


def thaw_census(r, th0, bars, frozen0):
    """Of one reference chain: the set of (side, rule, κ is a wall) met by a thaw -- side 0 = lower, 1 = upper: the barrier of the RESTORED speed,
    :269 -- and the set of coordinates that started frozen and thawed."""
    cur = np.array(th0, dtype=np.float64)
    saved = np.where(frozen0, cur, 0.0)
    met, thawed0 = set(), set()
    first = np.ones(len(cur), dtype=bool)
    for i, kind, th in zip(r["i"], r["kind"], r["theta"]):
        if kind == R.EV_HIT:
            saved[i] = cur[i]
        elif kind == R.EV_THAW:
            side = int(saved[i] > 0)
            met.add((side, bars[i][1][side], bars[i][2][side] == INF))
            if first[i] and frozen0[i]:
                thawed0.add(int(i))
        first[i] = False
        cur[i] = th
    return met, thawed0


def starts_frozen(P):
    """[nch x d]: x0 on the barrier of θ0's direction (src/stickyzz.jl:201)."""
    lo, hi = np.array([b[0][0] for b in P["bars"]]), np.array([b[0][1] for b in P["bars"]])
    return P["x0"] == np.where(P["th0"] > 0, hi, lo)


def _place_on_barrier(x0, th0, bars, where):
    """x0 with the coordinates `where` ([nch x d] bool) exactly on the barrier of their θ0's direction, where that barrier is finite."""
    lo, hi = np.array([b[0][0] for b in bars]), np.array([b[0][1] for b in bars])
    bar = np.where(th0 > 0, hi, lo)
    return np.where(where & np.isfinite(bar), bar, x0)


def _cuts(rng, n):
    """n fractions of the horizon in (0, 1), one of them repeated, ascending."""
    f = np.sort(rng.uniform(0.05, 0.95, size=n))
    return np.sort(np.append(f, f[int(rng.integers(0, n))]))


# ---------------------------------------------------------------------------------------------------------------- family A: random options

OPTIONS_N = 16
GRAPH_KINDS = ("lattice", "banded", "random_sparse")


def _kappa(rng):
    return INF if rng.integers(0, 4) == 0 else float(np.exp(rng.uniform(np.log(0.05), np.log(20.0))))


def _menu_barrier(rng):
    """One coordinate's barriers: none; one-sided below; one-sided above; a box with each of the nine rule pairs; lo == hi at a level != 0 with
    each rule -- 15 entries, drawn uniformly.  κ per side log-uniform on (0.05, 20), or a wall with probability 1/4."""
    m = int(rng.integers(0, 15))
    kap = (_kappa(rng), _kappa(rng))
    if m == 0:
        return K.NO_BARRIER
    if m == 1:
        return ((-float(rng.uniform(0.5, 1.5)), INF), (RULE_NAMES[int(rng.integers(0, 3))], "reflect"), kap)
    if m == 2:
        return ((-INF, float(rng.uniform(0.4, 1.2))), ("reflect", RULE_NAMES[int(rng.integers(0, 3))]), kap)
    if m < 12:
        return ((-float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.4, 1.2))), (RULE_NAMES[(m - 3) // 3], RULE_NAMES[(m - 3) % 3]), kap)
    level = float(rng.uniform(0.2, 0.8)) * (1.0 if rng.integers(0, 2) else -1.0)
    return ((level, level), (RULE_NAMES[m - 12],) * 2, kap)


@functools.lru_cache(maxsize=None)
def options_draw(case):
    """test_random_barrier_options"""
    pkg = _pkg()
    rng = np.random.default_rng(11000 + case)
    kind = GRAPH_KINDS[int(np.random.default_rng(11000 + case).integers(0, 3))]  # (_parity_graph's own first draw)
    G = _parity_graph(rng)
    d = G.shape[0]
    Gb = sp.csc_matrix(0.9 * G) if rng.integers(0, 2) else G
    mu_b = 0.4 * rng.standard_normal(d) if rng.integers(0, 2) else None
    mu_t = (mu_b if (mu_b is not None and rng.integers(0, 2)) else 0.4 * rng.standard_normal(d)) if rng.integers(0, 2) else None
    t0 = float(rng.uniform(0.0, 3.0)) if rng.integers(0, 2) else 0.0
    adapt = bool(rng.integers(0, 2))
    c = pkg.problems.column_norms(G) * (float(rng.uniform(2.5, 4.0)) if not adapt else float(rng.uniform(0.3, 1.0)))
    strong = bool(rng.integers(0, 2))
    bars = [_menu_barrier(rng) for _ in range(d)]
    nch = int(rng.integers(2, 4))
    x0 = 0.5 * rng.standard_normal((nch, d))
    level = np.array([b[0][0] == b[0][1] for b in bars])
    x0 = np.where(level, x0, K.fit_state(x0, bars))  # (lo == hi is one level met from either side: any start is inside)
    th0 = rng.choice([-1.7, -1.0, -0.5, 0.5, 1.0, 1.7], (nch, d))
    x0 = _place_on_barrier(x0, th0, bars, rng.random((nch, d)) < 0.05)
    cap = int(rng.integers(16, 129))
    frac = _cuts(rng, int(rng.integers(1, 5)))
    seed = 11500 + 10 * case
    P = dict(case=case, kind=kind, G=G, Gb=Gb, d=d, nch=nch, mu_b=mu_b, mu_t=mu_t, t0=t0, x0=x0, th0=th0, adapt=adapt, c=c, strong=strong, bars=bars,
             cap=cap, seed=seed)
    H = 2.0 * min(1.0, 60.0 / d)
    for _ in range(16):
        P["T"], P["cuts"] = t0 + H, t0 + frac * H
        rs = run_refs(P)
        n = [r["nevents"] for r in rs]
        if any(r["status"] != R.REF_OK for r in rs) or min(n) >= MIN_EVENTS or max(n) > MAX_EVENTS:
            break
        H = 2.0 * H
    return P


@functools.lru_cache(maxsize=None)
def options_refs(case):
    return run_refs(options_draw(case))


def what(P):
    """The option dictionary a failure message carries."""
    return dict(case=P["case"], kind=P.get("kind"), d=P["d"], nch=P["nch"], own_bound=P["Gb"] is not P["G"], mu_b=P["mu_b"] is not None,
                mu_t=P["mu_t"] is not None, same_mu=P["mu_t"] is not None and P["mu_t"] is P["mu_b"], t0=P["t0"], T=P["T"], adapt=P["adapt"],
                strong=P["strong"], cap=P["cap"], cuts=len(P["cuts"]))


# ------------------------------------------------------------------------------------------------------------------- family B: named edges

def hub_graph(leaves, rng, extra=True):
    """Hub 0 with leaves 1..leaves and -- extra -- one more node tied to leaf 1; diagonally dominant.  leaves = 62: d = 64, |G1[0]| = 63 and
    |G1 ∪ G2| = 64 for coordinate 0 and for leaf 1.  leaves = 63 without the extra node: |G1[0]| = 64, the width stickyzz refuses."""
    d = leaves + 1 + int(extra)
    A = sp.lil_matrix((d, d))
    w = -rng.uniform(0.1, 0.3, leaves)
    for j in range(1, leaves + 1):
        A[0, j] = A[j, 0] = w[j - 1]
    if extra:
        A[1, d - 1] = A[d - 1, 1] = -0.25
    A = sp.csc_matrix(A)
    return _csc(A + sp.diags(np.asarray(abs(A).sum(axis=0)).ravel() + 1.0))


def _edge(name, G, Gb, bars, x0, th0, c, t0, H, seed, rng, *, mu_b=None, mu_t=None, adapt=False, strong=False, cap=96, ncuts=2):
    d = G.shape[0]
    return dict(case=name, kind=name, G=_csc(G), Gb=_csc(Gb), d=d, nch=x0.shape[0], mu_b=mu_b, mu_t=mu_t, t0=t0, T=t0 + H, x0=x0, th0=th0, adapt=adapt,
                c=np.asarray(c, dtype=np.float64), strong=strong, bars=bars, cap=cap, cuts=t0 + _cuts(rng, ncuts) * H, seed=seed)


def _hub(name, seed, bars_of, *, mu_t_kind, H=20.0, **kw):
    rng = np.random.default_rng(seed)
    G = hub_graph(62, rng)
    d = 64
    mu_b = 0.4 * rng.standard_normal(d)
    mu_t = {"none": None, "same": mu_b, "own": 0.4 * rng.standard_normal(d)}[mu_t_kind]
    bars = bars_of(rng)
    x0 = K.fit_state(0.5 * rng.standard_normal((2, d)), bars)
    th0 = rng.choice([-1.0, 1.0], (2, d))
    c = _pkg().problems.column_norms(G) * (0.5 if kw.get("adapt") else 3.0)
    return _edge(name, G, sp.csc_matrix(0.9 * G), bars, x0, th0, c, 1.5 if name == "hub63_free" else 0.0, H, seed + 100, rng, mu_b=mu_b, mu_t=mu_t, **kw)


BLOCKS_D = (63, 64, 65, 128, 129)
TIES_RULES = ((("sticky", "reflect"), (0.7, INF)), (("reflect", "reflect"), (INF, INF)), (("sticky", "sticky"), (0.7, 0.9)))
EDGE_NAMES = (["hub63_free", "hub63_reversible", "hub63_mixed", "hub63_mixed_strong"] + ["blocks_%d" % d for d in BLOCKS_D]
              + ["ties_%d" % k for k in range(len(TIES_RULES))] + ["level_start_8", "level_start_144", "many_chains"])


@functools.lru_cache(maxsize=None)
def edge_draw(name):
    pkg = _pkg()
    if name == "hub63_free":  # every reflection of the hub re-bounds 63 free members behind the coin: candidate 63
        return _hub(name, 12000, lambda rng: [K.NO_BARRIER] * 64, mu_t_kind="own", adapt=True, H=40.0)
    if name == "hub63_reversible":  # every thaw of the hub: the sign coin plus 63 re-bounds, all 64 candidates
        box0 = ((-0.2, 0.15), ("reversible", "reversible"), (2.0, 3.0))
        return _hub(name, 12001, lambda rng: [box0] + [K.NO_BARRIER] * 63, mu_t_kind="none", adapt=True, H=40.0)
    if name == "hub63_mixed":
        return _hub(name, 12002, lambda rng: K.mixed_barriers(64, rng), mu_t_kind="same", adapt=True)
    if name == "hub63_mixed_strong":
        return _hub(name, 12002, lambda rng: K.mixed_barriers(64, rng), mu_t_kind="none", adapt=True, strong=True)
    if name.startswith("blocks_"):
        d = int(name[7:])
        rng = np.random.default_rng(12100 + d)
        diags = [np.full(d, 5.0 + rng.random())] + [np.full(d - o, -rng.uniform(0.2, 1.0)) for o in (1, 2)]
        G = _csc(sp.diags(diags + diags[1:], [0, 1, 2, -1, -2], format="csc"))
        bars = K.mixed_barriers(d, rng)
        # (mixed_barriers cycles over 8 and leaves coordinate d − 1 without a barrier at d = 65, 129: the last coordinate gets a box of its own)
        bars[d - 1] = ((-0.8, 0.5), ("sticky", "reversible"), tuple(float(rng.uniform(0.3, 1.3)) for _ in range(2)))
        x0 = K.fit_state(0.5 * rng.standard_normal((2, d)), bars)
        th0 = rng.choice([-1.0, 1.0], (2, d))
        mu_b = 0.4 * rng.standard_normal(d)
        return _edge(name, G, G, bars, x0, th0, pkg.problems.column_norms(G), 0.75 if d in (65, 129) else 0.0, 12.0, 12200 + d, rng, mu_b=mu_b,
                     adapt=True)
    if name.startswith("ties_"):  # identical coordinates and walls: bit-equal keys in different key blocks
        rule, kap = TIES_RULES[int(name[5:])]
        d = 130
        rng = np.random.default_rng(12300)
        G = _csc(sp.identity(d, format="csc"))
        even = np.arange(d) % 2 == 0
        x0 = np.where(even, 0.4, -0.9)[None, :].copy()
        th0 = np.where(even, 1.0, -1.0)[None, :].copy()
        return _edge(name, G, G, [((-1.0, 0.5), rule, kap)] * d, x0, th0, np.full(d, 0.01), 0.0, 3.0, 9, rng, cap=128)
    if name.startswith("level_start_"):  # lo == hi met from both sides, x0 on the level: frozen at t0 whatever the sign of θ0
        d = int(name[12:])
        rng = np.random.default_rng(12400 + d)
        G = _csc(K.precision8() if d == 8 else pkg.problems.gmrf_precision(12))
        bars = [((0.3, 0.3), (RULE_NAMES[i % 3],) * 2, tuple(float(rng.uniform(1.0, 3.0)) for _ in range(2))) for i in range(d)]
        x0 = 0.5 * rng.standard_normal((2, d))
        th0 = rng.choice([-1.0, 1.0], (2, d))
        on = set(range(0, d, 3))
        if d == 8:  # two neighbours
            on.add(next(int(r) for r in G.indices[G.indptr[0]:G.indptr[1]] if r != 0))
        else:  # 63 and 64: neighbours on the 12 x 12 lattice, on either side of a key-block boundary
            on.add(64)
        on = np.array(sorted(on))
        x0[:, on] = 0.3
        th0[0, on[:2]], th0[1, on[:2]] = (1.0, -1.0), (-1.0, 1.0)  # (both signs of θ0 among them in every chain)
        P = _edge(name, G, sp.csc_matrix(0.9 * G), bars, x0, th0, 3.0 * pkg.problems.column_norms(G), 2.5, 20.0 if d == 8 else 10.0, 12500 + d, rng,
                  mu_b=0.4 * rng.standard_normal(d), mu_t=0.4 * rng.standard_normal(d), adapt=True)
        P["on_level"] = on
        return P
    if name == "many_chains":  # the d = 8 mixed case of tests/test_gpu_stickyzz_parity.py, 130 chains
        rng = np.random.default_rng(12600)
        G = K.precision8()
        bars = K.mixed_barriers(8)
        x0, th0 = K.state8(130)
        return _edge(name, G, sp.csc_matrix(0.9 * G), bars, K.fit_state(x0, bars), th0, K.c8(G), 0.0, 20.0, 7, rng, mu_b=0.4 * rng.standard_normal(8),
                     adapt=True, cap=64)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def edge_refs(name):
    return run_refs(edge_draw(name))


def refused_hub():
    """The hub with 63 leaves: |G1[0]| = 64 with a two-hop zone of 64 -- not a general-kernel graph by sticky_kernel's rule, refused by the
    barrier sampler's own width check."""
    return hub_graph(63, np.random.default_rng(12700), extra=False)
