"""Hand-made Boomerang traces for the arc pair consumer (pdmp_ensemble_bps_consume_arc_pairs), beside `boom` and `boom_sticky` of
tests/pdmp_consumer_cases.py, whose Case they reuse: one table for tests/test_arc_pairs_ref.py (the C statement, the host mirror and the exact
integrals, no device) and tests/test_gpu_arc_pairs.py (the device against the C statement, through pdmp_debug_bps_trace_append).  TEST
INFRASTRUCTURE ONLY; nothing here touches the device.  Positions and velocities are free numbers (x about μ, θ from N(0, 1)), not a consistent
path, so that a cursor mistake moves a result by O(1); every case is deterministic from its seed.  dt = 0, K = 0: no grid.

    name       what it is
    d1         d = 1, the single pair (0, 0); 9 events in segments of 4 and 5 (the second fills a buffer of 5 exactly).
    sticky130  sticky, d = 130 (mask words of 64, 64 and 2 bits): the first event is (t0, x0, θ0, all free), the masks flip bits 63, 64 and 129
               (and others) between events; 40 events in a buffer of 32, one segment grown in place.
    lists24    d = 24, μ ≠ 0: the pair lists `lists24_255`, `_256`, `_257` have npairs + d = 255, 256 and 257 threads per chain -- under one
               workgroup, exactly one, and two --, every pair given as (i, j) with i >= j.
    edge       d = 5, t0 = 1, μ ≠ 0: two events at one time (τ = 0), then an event before t0 (τ < 0), then τ = 1e-9, τ past 2π and τ past 6π.
    two        2 chains, d = 3; the middle segment gives chain 1 nothing.

LISTS[name] = the case, the pair list and the centre a test runs it with (boom and boom_sticky included: a selection across both mask words
in both orientations).  Every centre is ≠ 0 but d1's."""
import functools

import numpy as np

import pdmp_consumer_cases as PC


def _masks(rng, n, d, flip):
    """[n x d] free masks, row 0 all free; every row flips each bit of `flip` with probability 1/2 and three others"""
    f = np.ones((n, d), dtype=bool)
    for e in range(1, n):
        f[e] = f[e - 1]
        for b in flip:
            if rng.random() < 0.5:
                f[e, b] = ~f[e, b]
        for b in rng.integers(0, d, 3):
            f[e, b] = ~f[e, b]
    return f


def _make(name, seed, d, t0, ts, cuts, cap, sticky=False, flip=(), grow=frozenset()):
    rng = np.random.default_rng(seed)
    nch = len(ts)
    mu = rng.uniform(-1.0, 1.0, d)
    x0, th0 = mu + rng.standard_normal((nch, d)), rng.standard_normal((nch, d))
    xs, ths, fs = [], [], []
    for k, t in enumerate(ts):
        x, th = mu + rng.standard_normal((len(t), d)), rng.standard_normal((len(t), d))
        if sticky:
            x[0], th[0] = x0[k], th0[k]  # (t0, x0, θ0, all free): what the sticky sampler writes first
            fs.append(_masks(rng, len(t), d, flip))
        xs.append(x), ths.append(th)
    return PC.Case(name, d, t0, x0, th0, 0.0, 0, cap, [np.asarray(t, dtype=np.float64) for t in ts], xs, ths, cuts, False,
                   f=fs if sticky else None, mu=mu, grow=grow)


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(900)
    if name == "d1":
        return _make(name, 901, 1, 0.0, [np.cumsum(rng.uniform(0.05, 2.0, 9))], [[0, 4, 9]], 5)
    if name == "sticky130":
        t = np.concatenate([[0.0], np.cumsum(rng.uniform(0.01, 1.2, 39))])
        c = _make(name, 902, 130, 0.0, [t], [[0, 1, 14, 27, 40]], 32, sticky=True, flip=(63, 64, 129), grow=frozenset([2]))
        assert all(len(np.unique(c.f[0][:, b])) == 2 for b in (63, 64, 129))
        return c
    if name == "lists24":
        return _make(name, 903, 24, -0.5, [-0.5 + np.cumsum(rng.uniform(0.05, 1.5, 12))], [[0, 5, 12]], 8)
    if name == "edge":
        t = [1.5, 1.5, 0.75, 0.75 + 1e-9, 7.75, 27.75, 28.0]
        assert t[1] - t[0] == 0 and t[2] < 1.0 and 0 < t[3] - t[2] < 1.1e-9 and t[4] - t[3] > 2 * np.pi and t[5] - t[4] > 6 * np.pi
        return _make(name, 904, 5, 1.0, [t], [[0, 3, 7]], 4)
    if name == "two":
        return _make(name, 905, 3, 0.0, [np.cumsum(rng.uniform(0.1, 1.0, 9)), np.cumsum(rng.uniform(0.1, 1.0, 6))], [[0, 3, 6, 9], [0, 3, 3, 6]], 4)
    return PC.case(name)  # boom, boom_sticky


def _dense(sel):
    """the diagonal and every pair of sel, the off-diagonal ones alternately as (i, j) and (j, i)"""
    a, b = np.tril_indices(len(sel))
    pi, pj = np.asarray(sel)[a], np.asarray(sel)[b]
    swap = (np.arange(len(pi)) % 2 == 1)
    return np.where(swap, pj, pi).astype(np.int64), np.where(swap, pi, pj).astype(np.int64)


def _centre(d, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, d)


@functools.lru_cache(maxsize=None)
def listed(name):
    """(case, pi, pj, centre) of the entry `name` of NAMES"""
    if name.startswith("lists24_"):
        c, n = case("lists24"), int(name[8:]) - 24
        a, b = np.tril_indices(24)  # 300 pairs, i >= j
        keep = np.sort(np.random.default_rng(906).permutation(300)[:n])
        return c, a[keep].astype(np.int64), b[keep].astype(np.int64), _centre(24, 907)
    c = case(name)
    if name == "d1":
        return c, np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64), None
    sel = {"sticky130": [0, 63, 64, 65, 129], "edge": [0, 1, 2, 3, 4], "two": [0, 1, 2], "boom": [0, 7, 31, 63, 64],
           "boom_sticky": [0, 12, 63, 64, 65]}[name]
    pi, pj = _dense(sel)
    return (c,) + (pi, pj) + (_centre(c.d, 908 + c.d),)


NAMES = ["boom", "boom_sticky", "d1", "sticky130", "lists24_255", "lists24_256", "lists24_257", "edge", "two"]


@functools.lru_cache(maxsize=None)
def reference(name, k, s):
    """The C statement on chain k's trace after segment s (computed once, shared by the tests; treat as read-only)"""
    import arc_pairs_ref_lib as AR
    c, pi, pj, cen = listed(name)
    t, x, th, f = c.so_far(k, s)
    return AR.arcs(c.t0, c.x0[k], c.th0[k], t, x, th, c.mu, pi, pj, cen, f=f)
