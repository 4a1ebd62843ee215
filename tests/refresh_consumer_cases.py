"""Hand-made traces for the UNORDERED device trace consumers (Ensemble.refresh_consume_begin, csrc/pdmp_consume.hip): one case table for
tests/test_refresh_consumer_cases_ref.py (the host statements alone, no device) and tests/test_gpu_refresh_consumers.py (the device against
tests/ref/refresh_trace_ref.c, through pdmp_debug_trace_append).  TEST INFRASTRUCTURE ONLY; nothing here touches the device.

A flow with a refresh clock records a refreshed coordinate at its own, stale clock: the trace is sorted within a coordinate only.  These traces
put stale events where a sampler never would on demand: directly behind a written row, at the two ends of a slice, at the end of the trace,
whole chunks of them in front of the first event that passes a grid time.  As in tests/consumer_cases.py positions and velocities are FREE
numbers (x in [0.5, 2], θ in {−1, 0, 1}), so a cursor mistake moves a result by O(1).  No event time is 0 (y / (2t) stays finite) and no trace
starts with an event at or before t0 (the closed form writes row 0 again once the first later event arrives, with the events at or before t0
applied; the reference's iterator emits x0 there -- DESIGN.md §20).  Every case is deterministic from its seed.

A case holds ONE chain: d, t0, x0, θ0 [d], dt, K, trace_capacity, the events (EVENT_DTYPE, trace order), mu ([d]: a FactBoomerang's centre; None: a
ZigZag with λref > 0) and the CUT POINTS of the split feed: segment s is events[cuts[s]:cuts[s + 1]].

    name          what it is
    bsearch       times 1, 9, 2, 3, 4 and a grid point at 5: row 5 applies the first event only (a binary search for the first time > 5 lands
                  behind the last event and applies all five); the trace ends on a stale event: T = 4, npoints from the maximum 9.
    behind_row    a stale event directly behind a written row: the row keeps its bytes, the next row shows the new velocity.
    slice_edges   a stale event as the last of a slice and as the first of the next.
    ends_stale    a longer trace that ends on a stale event far below the maximum.
    cut13         12 events, four of them stale: TEST feeds it cut in two at each of its 13 positions.
    tiny          slices of 0 and 1 events.
    n255 n256 n257 n513   that many events, d = 7, about a third stale; fed whole and in three parts.
    far_split     the first event that passes the first grid time is slot 600: two full chunks and a part lie between pos and the split, with small
                  stale times among them.
    one_coord     300 events of coordinate 0 in a row, all of them stale (behind an event of coordinate 1 at t = 50), then a later event.
    on_grid       events exactly on a grid time (applied before the row) and one ulp past it (the event that opens the row), stale ones among them.
    many_rows     about 300 rows between two events, a stale event between.
    short_grid    K = 6: npoints is not clamped and the Python reader raises.
    neg_t0        t0 = −3.5.
    t0_shift      t0 = 2 and a coordinate whose first own event (a stale one) lies before t0.
    d1 d255 d256 d257   that many coordinates (d = 1 cannot hold a stale event: one coordinate's events keep their order).
    dyadic        times on a lattice of 1/8, x a multiple of 2^-20, dt = 0.25: rows, grid times and the cummean sums are exact in every statement.
    boom          FactBoomerang, μ ≠ 0, d = 5: τ = g − t_cursor from 1e-9 to past 6π.
    boom_dyadic   FactBoomerang on the dyadic lattice (μ a multiple of 1/4): the cummean sums are exact; the rows are not (sin, cos).
"""
import functools
from dataclasses import dataclass

import numpy as np

EVENT_DTYPE = np.dtype([("t", "<f8"), ("i", "<i8"), ("x", "<f8"), ("theta", "<f8")])  # (= _lib.EVENT_DTYPE; the test files assert it)
CHUNK = 256


@dataclass
class Case:
    name: str
    d: int
    t0: float
    x0: np.ndarray
    th0: np.ndarray
    dt: float
    K: int
    trace_capacity: int
    events: np.ndarray
    cuts: list
    mu: object = None
    dyadic: bool = False
    stale: bool = True  # the trace holds events whose time lies below the running maximum before them

    @property
    def nseg(self):
        return len(self.cuts) - 1

    def segment(self, s):
        return self.events[self.cuts[s]:self.cuts[s + 1]]


NAMES = ["bsearch", "behind_row", "slice_edges", "ends_stale", "cut13", "tiny", "n255", "n256", "n257", "n513", "far_split", "one_coord", "on_grid",
         "many_rows", "short_grid", "neg_t0", "t0_shift", "d1", "d255", "d256", "d257", "dyadic", "boom", "boom_dyadic"]
DYADIC = ["bsearch", "behind_row", "dyadic", "boom_dyadic"]
BOOM = ["boom", "boom_dyadic"]


def _events(t, i, x, th):
    ev = np.empty(len(t), dtype=EVENT_DTYPE)
    ev["t"], ev["i"], ev["x"], ev["theta"] = t, i, x, th
    return ev


def _dyadic_x(rng, n):
    return 0.5 + rng.integers(0, 3 * 2 ** 19 + 1, n) * 2.0 ** -20  # multiples of 2^-20 in [0.5, 2]


def _state(rng, d, dyadic):
    return (_dyadic_x(rng, d) if dyadic else rng.uniform(0.5, 2.0, d)), rng.choice([-1.0, 1.0], d)


def _free(rng, n, dyadic):
    return (_dyadic_x(rng, n) if dyadic else rng.uniform(0.5, 2.0, n)), rng.choice([-1.0, 0.0, 1.0], n)


def _times(rng, n, d, t0, step, p_stale, dyadic=False, coords=None):
    """n event times and coordinates: a clock that advances by about `step` per fresh event; a stale event takes a time between its
    coordinate's own last time and the clock (a coordinate's own times never decrease).  The first event is fresh and later than t0."""
    t, i = np.empty(n), np.empty(n, dtype=np.int64)
    clock, own = float(t0), [float(t0)] * d
    for e in range(n):
        j = int(rng.integers(0, d)) if coords is None else int(coords[e])
        if e > 0 and own[j] < clock and rng.random() < p_stale:
            u = rng.random()
            te = own[j] + (np.floor(u * (clock - own[j]) * 8.0) / 8.0 if dyadic else u * (clock - own[j]))
        else:
            clock += (int(rng.integers(1, 4)) / 8.0) if dyadic else step * rng.uniform(0.2, 1.8)
            te = clock
        if te == 0.0:  # (never 0: y / (2t))
            clock += 0.125
            te = clock
        t[e], i[e], own[j] = te, j, te
    return t, i


def _random(name, seed, n, d, t0, dt, K, cap, cuts, step=0.11, p_stale=0.33, dyadic=False, mu=None):
    rng = np.random.default_rng(seed)
    t, i = _times(rng, n, d, t0, step, p_stale, dyadic)
    x0, th0 = _state(rng, d, dyadic)
    x, th = _free(rng, n, dyadic)
    return Case(name, d, t0, x0, th0, dt, K, cap, _events(t, i, x, th), cuts, mu=mu, dyadic=dyadic, stale=d > 1)


def _bsearch():
    rng = np.random.default_rng(201)
    x0, th0 = _state(rng, 3, True)
    x, th = _free(rng, 5, True)
    ev = _events([1.0, 9.0, 2.0, 3.0, 4.0], [0, 1, 0, 2, 0], x, np.where(th == 0.0, 1.0, th))
    return Case("bsearch", 3, 0.0, x0, th0, 5.0, 4, 16, ev, [0, 2, 5], dyadic=True)


def _behind_row():
    rng = np.random.default_rng(202)
    x0, th0 = _state(rng, 2, True)
    x, _ = _free(rng, 4, True)
    # row 1 (g = 1) is written when (1.5, 0) arrives; (0.25, 1) is stale and directly behind it; row 2 is written when (2.5, 0) arrives
    ev = _events([1.5, 0.25, 2.5, 3.5], [0, 1, 0, 1], x, [1.0, -th0[1], -1.0, 1.0])
    return Case("behind_row", 2, 0.0, x0, th0, 1.0, 8, 16, ev, [0, 1, 2, 4], dyadic=True)


def _slice_edges():
    rng = np.random.default_rng(203)
    d, n = 3, 24
    t, i = _times(rng, n, d, 0.0, 0.4, 0.0)
    # events 7 and 8 become stale: 7 is the last of slice [0, 8), 8 the first of slice [8, 16)
    i[7], i[8] = (i[6] + 1) % d, (i[6] + 2) % d
    for e in (7, 8):
        own = t[:e][i[:e] == i[e]]
        t[e] = (own[-1] if len(own) else 0.0) + 0.01
    i[9], t[9] = i[6], t[6] + 0.3
    t[10:] = t[9] + np.cumsum(np.full(n - 10, 0.37))
    x0, th0 = _state(rng, d, False)
    x, th = _free(rng, n, False)
    return Case("slice_edges", d, 0.0, x0, th0, 0.5, 40, 32, _events(t, i, x, th), [0, 8, 16, 24])


def _ends_stale():
    c = _random("ends_stale", 204, 60, 4, 0.0, 0.25, 64, 64, [0, 59, 60], step=0.2)
    ev = c.events
    last = [ev["t"][:-1][ev["i"][:-1] == j].max(initial=0.0) for j in range(c.d)]
    ev["i"][-1] = int(np.argmin(last))  # the coordinate that was hit longest ago
    ev["t"][-1] = min(last) + 1e-3      # far below the maximum
    return c


def _far_split():
    rng = np.random.default_rng(207)
    d, n = 6, 700
    t, i = _times(rng, 600, d, 0.0, 0.0012, 0.4)  # 600 events below the first grid time behind t0 (dt = 1): the clock stays under 0.9
    assert t.max() < 0.9
    t2, i2 = np.array([1.5]), np.array([2])
    t3, i3 = _times(rng, 99, d, 1.5, 0.05, 0.4)
    t3 = np.maximum(t3, 1.5)  # (own times must not fall below the coordinate's earlier ones)
    t, i = np.concatenate([t, t2, t3]), np.concatenate([i, i2, i3])
    x0, th0 = _state(rng, d, False)
    x, th = _free(rng, n, False)
    return Case("far_split", d, 0.0, x0, th0, 1.0, 12, 704, _events(t, i, x, th), [0, 300, 700])


def _one_coord():
    rng = np.random.default_rng(208)
    n = 302
    t = np.concatenate([[50.0], np.sort(rng.uniform(0.1, 30.0, 300)), [60.5]])
    i = np.concatenate([[1], np.zeros(300, dtype=np.int64), [1]])
    x0, th0 = _state(rng, 2, False)
    x, th = _free(rng, n, False)
    return Case("one_coord", 2, 0.0, x0, th0, 1.0, 70, 320, _events(t, i, x, th), [0, 1, 302])


def _on_grid():
    rng = np.random.default_rng(209)
    d, dt, t0 = 3, 0.25, 0.0
    g = lambda k: t0 + dt * k
    up = lambda v: float(np.nextafter(v, np.inf))
    # (time, coordinate): on a grid time; an ulp past one; a stale event ON an earlier grid time and an ulp past one
    te = [(g(2), 0), (up(g(3)), 1), (g(2), 2), (g(5), 0), (up(g(5)), 1), (up(g(2)), 2), (g(8), 0), (up(g(4)), 2), (up(g(9)), 1), (g(9), 2), (g(11), 0)]
    t, i = np.array([a for a, _ in te]), np.array([b for _, b in te])
    x0, th0 = _state(rng, d, True)
    x, th = _free(rng, len(t), True)
    return Case("on_grid", d, t0, x0, th0, dt, 16, 16, _events(t, i, x, th), [0, 3, 6, 11])


def _many_rows():
    rng = np.random.default_rng(210)
    x0, th0 = _state(rng, 3, False)
    x, th = _free(rng, 5, False)
    ev = _events([0.5, 300.2, 0.7, 300.9, 301.4], [0, 1, 2, 0, 2], x, th)
    return Case("many_rows", 3, 0.0, x0, th0, 1.0, 320, 8, ev, [0, 2, 3, 5])


def _t0_shift():
    rng = np.random.default_rng(213)
    d = 3
    x0, th0 = _state(rng, d, False)
    t = [2.5, 1.0, 3.1, 1.7, 3.6, 3.2, 4.4]  # coordinate 1's first own event (1.0) and coordinate 2's (1.7) lie before t0 = 2
    i = [0, 1, 0, 2, 1, 2, 0]
    x, th = _free(rng, len(t), False)
    return Case("t0_shift", d, 2.0, x0, th0, 0.35, 16, 8, _events(t, i, x, th), [0, 2, 4, 7])


def _boom():
    rng = np.random.default_rng(220)
    d, dt, t0 = 5, 0.5, 0.0
    mu = np.array([0.7, -0.4, 0.0, 1.1, -0.9])
    # coordinate 4 is hit once, early: its τ grows past 6π; events 1e-9 before a grid time give the smallest τ; stale events among them
    te = [(0.3, 4), (1.0 - 1e-9, 0), (0.6, 1), (2.2, 2), (1.4, 3), (3.5 - 1e-9, 1), (2.9, 0), (7.25, 2), (4.0, 3), (11.6, 0), (9.0 - 1e-9, 1), (15.1, 3),
          (12.0, 2), (19.7, 0), (19.2, 1), (20.4, 2)]
    t, i = np.array([a for a, _ in te]), np.array([b for _, b in te])
    x0 = mu + rng.uniform(-1.5, 1.5, d)
    th0 = rng.standard_normal(d)
    x = mu[i] + rng.uniform(-1.5, 1.5, len(t))
    th = rng.standard_normal(len(t))
    return Case("boom", d, t0, x0, th0, dt, 48, 16, _events(t, i, x, th), [0, 5, 6, 16], mu=mu)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("n255", "n256", "n257", "n513"):
        n = int(name[1:])
        return _random(name, 300 + n, n, 7, 0.0, 0.5, 128, 520, [0, n // 3, 2 * n // 3 + 1, n])
    if name in ("d1", "d255", "d256", "d257"):
        d = int(name[1:])
        return _random(name, 400 + d, 120, d, 0.3, 0.1, 160, 128, [0, 50, 120], step=0.1)
    if name == "cut13":
        return _random(name, 205, 12, 3, 0.0, 0.25, 24, 16, [0, 12], step=0.3, p_stale=0.4)
    if name == "tiny":
        return _random(name, 206, 9, 3, 0.0, 0.2, 24, 16, [0, 0, 1, 1, 2, 3, 3, 9], step=0.3, p_stale=0.4)
    if name == "short_grid":
        return _random(name, 211, 80, 4, 0.0, 0.25, 6, 96, [0, 30, 80], step=0.2)
    if name == "neg_t0":
        return _random(name, 212, 90, 4, -3.5, 0.25, 64, 96, [0, 45, 90], step=0.15)
    if name == "dyadic":
        return _random(name, 214, 400, 5, 0.0, 0.25, 600, 400, [0, 100, 257, 400], dyadic=True)
    if name == "boom_dyadic":
        return _random(name, 221, 120, 4, 0.0, 0.25, 200, 128, [0, 60, 120], dyadic=True, mu=np.array([0.25, -0.5, 0.0, 1.0]))
    return {"bsearch": _bsearch, "behind_row": _behind_row, "slice_edges": _slice_edges, "ends_stale": _ends_stale, "far_split": _far_split,
            "one_coord": _one_coord, "on_grid": _on_grid, "many_rows": _many_rows, "t0_shift": _t0_shift, "boom": _boom}[name]()


# ---------------------------------------------------------------------------------------------------------------- what the table holds
def stale_events(ev):
    """the events whose time lies below the running maximum of the times before them"""
    t = ev["t"]
    if len(t) < 2:
        return 0
    return int((t[1:] < np.maximum.accumulate(t)[:-1]).sum())


def own_order_kept(ev, d):
    """every coordinate's own event times are non-decreasing (tests/exact_path.py states the property of a refresh trace)"""
    return all(np.all(np.diff(ev["t"][ev["i"] == j]) >= 0) for j in range(d))


@functools.lru_cache(maxsize=None)
def reference(name, upto=None):
    """tests/ref/refresh_trace_ref.c on the first `upto` events (None: all) of the case"""
    import refresh_trace_ref_lib as R
    c = case(name)
    ev = c.events if upto is None else c.events[:upto]
    return R.consume(c.t0, c.x0, c.th0, ev, mu=c.mu, dt=c.dt, K=c.K)
