"""Hand-made trace segments for the device trace consumers (csrc/pdmp_consume.hip): one case table for tests/test_consumer_cases_ref.py (the two
host references alone, no device) and tests/test_gpu_consumers_synthetic.py (the device against them, through pdmp_debug_trace_append).  TEST
INFRASTRUCTURE ONLY; nothing here touches the device.

A sampler's trace has continuous random event times, so it can never put an event exactly at a grid time, 256 events of one coordinate into one
chunk, or two chosen coordinates into one slot of the per-chunk hash table.  These traces do.  Positions and velocities are FREE numbers -- x in
[0.5, 2], θ in {−1, 0, 1}, not a consistent path -- so that a cursor mistake moves a result by O(1), never by a rounding error.  No event time, and
no last event time, is 0 (1/(2T) and y/(2t) stay finite).  Every case is deterministic from its seed.

A case holds d, nchains (1 or 2, a different trace per chain), t0, x0, θ0 [nchains x d], dt, K, trace_capacity, the per-chain event arrays
(EVENT_DTYPE) and the CUT POINTS at which the trace is fed: chain k's segment s is events[k][cuts[k][s]:cuts[k][s + 1]]; after a segment listed
in `grow` the trace is NOT reset, so the next one is appended behind it and consume() starts in the middle of the buffer.

    name          what it is
    one           d = 1, t0 = 0, 1100 events at multiples of 1/8 with repeats, dt = 0.25, K = 200; segments of 256, 257, 1, 255 and 331 events.
                  Events 240..511 share ONE time, a grid time, and event 512 comes later: the 257-event segment [256, 513) reaches the consumer as one
                  chunk of exactly 256 events before that row, and with d = 1 a chunk is a dependency chain of 256 -- the bound of the ordered-rounds
                  loop, met with nothing to spare; the row behind it shows the position of the chunk's LAST event.
    few           d = 3, t0 = −1.5, 700 events on the same time lattice (negative times, never 0); the segment [100, 400) is grown in two appends
                  with a consume() after each and no reset between them.
    row255/6/7    d = 255 / 256 / 257, t0 = 0.3, dt = 0.1, 513 events; each time is g = t0 + dt·k exactly, or nextafter(g, ±inf), about a third
                  each, several events per time.  The oracle steps t += dt and so stands an ulp beside these g: trace.py is the only reference.
    sparse        d = 300, 2 chains, 40 events each over [0, 50], dt = 0.05, K = 1100: many rows between two events, a third of the coordinates
                  never hit; one segment gives chain 0 events and chain 1 none.
    clash         d = 5000, one 768-event segment, dt so large that only row 0 exists: the consumer's chunks are the 256-aligned ones.  i ≠ j share
                  a slot of the hash table (((i·0x9E3779B1) mod 2^32) >> 20); chunk 0 holds i, j, i, j, i at thread slots 251..255 -- thread 255's id
                  is the table's "contested" mark --, chunk 1 holds them at slots 0..4 and chunk 2 in its middle, between unrelated coordinates.
    short_grid    `one` with K = 8: the grid runs out in the middle of the first segment, every later chunk is a full 256.
    on_grid_end   d = 4; the last event of every segment lies exactly on a grid time, the next segment starts with another event at that time and
                  goes past it; so does the last event of the trace (npoints).
    sticky        SAMPLER_STICKY_ZIGZAG, d = 4: freezes (θ = 0 with x = 0.0 or −0.0) and thaws (x = ±0.0, θ ≠ 0); coordinate 3 is hit rarely, so
                  it has long stuck and long free stretches, some between a 0.0 and a −0.0.
    sub           d = 40, segments of 0, 1, 255, 256, 257 and 600 events for subtrace: J = [], all of 0..d−1 and a strict subset; t0 = 0.75.

DYADIC cases (all but row*, sparse, clash): times are multiples of 1/8, dt = 0.25 and x is a multiple of 2^-20, so the oracle's stepping
(x += θ·Δt event by event, t += dt) is exact and oracle/trace_oracle.c and trace.py agree BIT FOR BIT; elsewhere x is a full-precision double.
"""
import functools
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

EVENT_DTYPE = np.dtype([("t", "<f8"), ("i", "<i8"), ("x", "<f8"), ("theta", "<f8")])  # (= _lib.EVENT_DTYPE; both test files assert it)
HASH_MULT, HASH_SHIFT = 0x9E3779B1, 20  # consume_events_kernel's table: 12 bits of the coordinate's multiplicative hash
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
    events: list
    cuts: list
    dyadic: bool
    grow: frozenset = frozenset()
    sticky: bool = False
    J: list = field(default_factory=list)      # sub: the index sets
    pair: tuple = ()                           # clash: (i, j)
    groups: tuple = ()                         # clash: (chunk, first thread slot) of every i, j, i, j, i group

    @property
    def nchains(self):
        return len(self.events)

    @property
    def nseg(self):
        return len(self.cuts[0]) - 1

    def segment(self, k, s):
        return self.events[k][self.cuts[k][s]:self.cuts[k][s + 1]]

    def so_far(self, k, s):
        """chain k's trace after segment s has been fed"""
        return self.events[k][:self.cuts[k][s + 1]]


NAMES = ["one", "few", "row255", "row256", "row257", "sparse", "clash", "short_grid", "on_grid_end", "sticky", "sub"]
DYADIC = ["one", "few", "short_grid", "on_grid_end", "sticky", "sub"]


def hash_slot(i):
    return ((int(i) * HASH_MULT) & 0xFFFFFFFF) >> HASH_SHIFT


def _events(t, i, x, th):
    ev = np.empty(len(t), dtype=EVENT_DTYPE)
    ev["t"], ev["i"], ev["x"], ev["theta"] = t, i, x, th
    return ev


def _dyadic_x(rng, n):
    return 0.5 + rng.integers(0, 3 * 2 ** 19 + 1, n) * 2.0 ** -20  # multiples of 2^-20 in [0.5, 2]


def _state(rng, nch, d, dyadic):
    x0 = _dyadic_x(rng, nch * d) if dyadic else rng.uniform(0.5, 2.0, nch * d)
    return x0.reshape(nch, d), rng.choice([-1.0, 1.0], (nch, d))


def _lattice_times(rng, n, t0, p=(0.5, 0.38, 0.12), burst=None):
    """n non-decreasing multiples of 1/8 behind t0, never 0; events burst[0]..burst[1]−1 share one time"""
    steps = rng.choice([0, 1, 2], n, p=p)
    steps[0] = 1
    if burst:
        steps[burst[0] + 1:burst[1]] = 0
        steps[burst[1]] = max(steps[burst[1]], 1)  # (the event behind them comes later)
        steps[burst[0]] += int(steps[:burst[0] + 1].sum() + round(t0 * 8)) % 2  # (their time is a multiple of 1/4: with dt = 0.25 a grid time)
    e = np.cumsum(steps)
    t = t0 + e / 8.0
    zero = np.flatnonzero(t == 0.0)
    if len(zero):  # (step over the lattice point 0)
        t[zero[0]:] += 0.125
    assert np.all(np.diff(t) >= 0) and not np.any(t == 0.0) and t[0] > t0
    return t


def _one(K):
    rng = np.random.default_rng(101)
    n = 1100
    t = _lattice_times(rng, n, 0.0, p=(0.66, 0.28, 0.06), burst=(240, 512))
    x0, th0 = _state(rng, 1, 1, True)
    ev = _events(t, np.zeros(n, dtype=np.int64), _dyadic_x(rng, n), rng.choice([-1.0, 0.0, 1.0], n))
    return Case("one" if K == 200 else "short_grid", 1, 0.0, x0, th0, 0.25, K, 400, [ev], [[0, 256, 513, 514, 769, 1100]], True)


def _few():
    rng = np.random.default_rng(102)
    n = 700
    t = _lattice_times(rng, n, -1.5)
    x0, th0 = _state(rng, 1, 3, True)
    ev = _events(t, rng.integers(0, 3, n), _dyadic_x(rng, n), rng.choice([-1.0, 0.0, 1.0], n))
    return Case("few", 3, -1.5, x0, th0, 0.25, 300, 400, [ev], [[0, 100, 250, 400, 700]], True, grow=frozenset([1]))


def _row(d):
    rng = np.random.default_rng(1000 + d)
    n, t0, dt = 513, 0.3, 0.1
    k = 1 + np.cumsum(rng.choice([0, 1, 2], n, p=[0.6, 0.3, 0.1]))
    side = rng.integers(-1, 2, n)
    order = np.lexsort((side, k))
    k, side = k[order], side[order]
    g = t0 + dt * k.astype(np.float64)  # the device's and trace.py's grid time, bit for bit
    t = np.where(side == 0, g, np.where(side < 0, np.nextafter(g, -np.inf), np.nextafter(g, np.inf)))
    i = rng.integers(0, d, n)
    i[:6] = [d - 1, 0, d - 1, 254, min(255, d - 1), d - 1]  # the row loop's last thread and its second trip
    x0, th0 = _state(rng, 1, d, False)
    ev = _events(t, i, rng.uniform(0.5, 2.0, n), rng.choice([-1.0, 0.0, 1.0], n))
    return Case("row%d" % d, d, t0, x0, th0, dt, 300, 300, [ev], [[0, 256, 513]], False)


def _sparse():
    rng = np.random.default_rng(104)
    d, n = 300, 40
    x0, th0 = _state(rng, 2, d, False)
    evs = []
    for _ in range(2):
        t = np.sort(rng.uniform(0.5, 50.0, n))
        evs.append(_events(t, rng.integers(0, 200, n), rng.uniform(0.5, 2.0, n), rng.choice([-1.0, 0.0, 1.0], n)))
    return Case("sparse", d, 0.0, x0, th0, 0.05, 1100, 64, evs, [[0, 10, 20, 30, 40], [0, 10, 20, 20, 40]], False)


def _clash():
    rng = np.random.default_rng(105)
    d, n = 5000, 768
    seen = {}
    pair = None
    for i in range(17, d):  # the first two coordinates behind 16 that share a slot
        s = hash_slot(i)
        if s in seen:
            pair = (seen[s], i)
            break
        seen[s] = i
    a, b = pair
    others = np.array([q for q in range(d) if hash_slot(q) != hash_slot(a)])
    i = rng.choice(others, n)
    groups = ((0, 251), (1, 0), (2, 100))
    for c, s in groups:
        i[c * CHUNK + s:c * CHUNK + s + 5] = [a, b, a, b, a]
    t = np.sort(rng.uniform(0.5, 40.0, n))
    x0, th0 = _state(rng, 1, d, False)
    ev = _events(t, i, rng.uniform(0.5, 2.0, n), rng.choice([-1.0, 0.0, 1.0], n))
    return Case("clash", d, 0.0, x0, th0, 1000.0, 2, 768, [ev], [[0, 768]], False, pair=pair, groups=groups)


def _on_grid_end():
    rng = np.random.default_rng(106)
    d, n = 4, 120
    cuts = [0, 30, 31, 75, 120]
    t = _lattice_times(rng, n, 0.0, p=(0.3, 0.5, 0.2))
    for c in cuts[1:]:  # the segment's last event ON a grid time (a multiple of 1/4), the next segment's first event at the same time
        shift = (-(t[c - 1] * 8.0)) % 2.0 / 8.0
        t[c - 1:] += shift
        if c < n:
            t[c:] += t[c - 1] - t[c]
    assert np.all(np.diff(t) >= 0)
    x0, th0 = _state(rng, 1, d, True)
    i = rng.integers(0, d, n)
    for c in cuts[1:-1]:
        i[c] = (i[c - 1] + 1) % d  # (another coordinate at the same time)
    ev = _events(t, i, _dyadic_x(rng, n), rng.choice([-1.0, 0.0, 1.0], n))
    return Case("on_grid_end", d, 0.0, x0, th0, 0.25, 200, 64, [ev], [cuts], True)


def _sticky():
    rng = np.random.default_rng(107)
    d, n = 4, 320
    t = _lattice_times(rng, n, 0.0, p=(0.3, 0.5, 0.2))
    i = rng.choice(d, n, p=[0.45, 0.35, 0.15, 0.05])
    x = _dyadic_x(rng, n)
    th = rng.choice([-1.0, 1.0], n)
    kind = rng.choice(3, n, p=[0.4, 0.3, 0.3])  # 0 an ordinary event, 1 a freeze (x = ±0.0, θ = 0), 2 a thaw (x = ±0.0, θ ≠ 0)
    zero = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    x = np.where(kind > 0, zero, x)
    th = np.where(kind == 1, 0.0, th)
    x0, th0 = _state(rng, 1, d, True)
    return Case("sticky", d, 0.0, x0, th0, 0.25, 200, 256, [_events(t, i, x, th)], [[0, 100, 101, 320]], True, sticky=True)


def _sub():
    rng = np.random.default_rng(108)
    d, n = 40, 1369
    t = _lattice_times(rng, n, 0.75, p=(0.8, 0.15, 0.05))
    x0, th0 = _state(rng, 1, d, True)
    ev = _events(t, rng.integers(0, d, n), _dyadic_x(rng, n), rng.choice([-1.0, 0.0, 1.0], n))
    J = [[], list(range(d)), [1, 5, 6, 17, 39]]
    return Case("sub", d, 0.75, x0, th0, 0.25, 200, 600, [ev], [[0, 0, 1, 256, 512, 769, 1369]], True, J=J)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("one", "short_grid"):
        return _one(200 if name == "one" else 8)
    if name.startswith("row"):
        return _row(int(name[3:]))
    return {"few": _few, "sparse": _sparse, "clash": _clash, "on_grid_end": _on_grid_end, "sticky": _sticky, "sub": _sub}[name]()


# ---------------------------------------------------------------------------------------------------------------- what the table holds
def grid_times(c, n):
    return c.t0 + c.dt * np.arange(n, dtype=np.float64)


def grid_hits(c, k):
    """events of chain k whose time is, bit for bit, a grid time t0 + dt·r with r < K"""
    g = grid_times(c, c.K)
    return int(np.isin(c.events[k]["t"], g).sum())


def same_time_events(c, k):
    t = c.events[k]["t"]
    return int((t[1:] == t[:-1]).sum())


def consumer_chunks(c, k):
    """The chunks consume_events_kernel takes of chain k's events, as (first, last + 1) global index pairs: within a call the events up to the
    next unwritten grid row (t <= g), 256 at a time, then the row if a later event of the call lies behind it; once the grid has run out, the rest."""
    ev = c.events[k]
    out = []
    row, pos = 0, 0
    for s in range(c.nseg):
        end = c.cuts[k][s + 1]
        if pos >= end:
            continue
        while True:
            want = row < c.K
            split = pos + int(np.searchsorted(ev["t"][pos:end], c.t0 + c.dt * row, side="right")) if want else end
            out += [(b, min(b + CHUNK, split)) for b in range(pos, split, CHUNK)]
            pos = split
            if not want or split >= end:
                break
            row += 1
    return out


def longest_chain(c, k):
    """the longest run of events of one coordinate inside one of the consumer's chunks (each waits for the one before it: the ordered rounds)"""
    best = 0
    for a, b in consumer_chunks(c, k):
        if b > a:
            best = max(best, int(np.bincount(c.events[k]["i"][a:b]).max()))
    return best


def empty_rows(c, k):
    """grid rows before the last event that no event lies between them and the row before"""
    t = c.events[k]["t"]
    g = grid_times(c, c.K)
    g = g[g < t[-1]]
    n = np.searchsorted(t, g, side="right")
    return int((np.diff(n) == 0).sum())


def never_hit(c, k):
    return int(c.d - len(np.unique(c.events[k]["i"])))


# ---------------------------------------------------------------------------------------------------------------- references of mean(Ξ)
def mean_loop(t0, x0, ev):
    """mean(Ξ) in the device's documented arithmetic: per coordinate y += (x_prev + x_k)·(t_k − t_prev) in event order, float64, no fused
    multiply-add, scaled ONCE by 1/(2T); and the number of events per coordinate"""
    d = len(x0)
    y = [0.0] * d
    tp = [float(t0)] * d
    xp = [float(v) for v in x0]
    cnt = np.zeros(d, dtype=np.int64)
    for t, i, x in zip(ev["t"].tolist(), ev["i"].tolist(), ev["x"].tolist()):
        y[i] += (xp[i] + x) * (t - tp[i])
        tp[i], xp[i] = t, x
        cnt[i] += 1
    T = float(ev["t"][-1])
    s = 1 / (2 * T)
    return np.array([v * s for v in y]), cnt


def mean_exact(t0, x0, ev):
    """The exact rational mean of the same float inputs, per coordinate, and Σ|term_i|/(2T) (as floats, rounded once)"""
    d = len(x0)
    y = [Fraction(0)] * d
    a = [Fraction(0)] * d
    tp = [Fraction(float(t0))] * d
    xp = [Fraction(float(v)) for v in x0]
    for t, i, x in zip(ev["t"].tolist(), ev["i"].tolist(), ev["x"].tolist()):
        t, x = Fraction(t), Fraction(x)
        term = (xp[i] + x) * (t - tp[i])
        y[i] += term
        a[i] += abs(term)
        tp[i], xp[i] = t, x
    T2 = 2 * Fraction(float(ev["t"][-1]))
    return [v / T2 for v in y], [v / abs(T2) for v in a]
