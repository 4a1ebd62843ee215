"""Hand-made PDMPTrace segments for the device consumers of the Bouncy Particle family (csrc/pdmp_consume_bps.hip), in the manner of
tests/consumer_cases.py: one case table for tests/test_pdmp_consumer_cases_ref.py (trace.py against the sequential C reference, no device) and
tests/test_gpu_bps_consumers.py (the device against the C reference, through pdmp_debug_bps_trace_append).  TEST INFRASTRUCTURE ONLY; nothing here
touches the device.

A sampler's trace has continuous random event times: it never puts an event exactly on a grid time, two events at one time, or a chosen bit
into a free mask.  These traces do.  Positions and velocities are FREE numbers -- x in [0.5, 2] (or about μ), θ in {−1, 0, 1} or N(0, 1), not
a consistent path -- so that a cursor mistake moves a result by O(1), never by a rounding error.  Every case is deterministic from its seed.

A case holds d, nchains (a different trace per chain), t0, x0, θ0 [nchains x d], dt, K, trace_capacity, per chain t [n], x, θ [n x d] (and f
[n x d] bool where sticky), μ [d] for a Boomerang, and the CUT POINTS at which the trace is fed: chain k's segment s is events
cuts[k][s]:cuts[k][s + 1]; after a segment listed in `grow` the trace is NOT reset.  A sticky ensemble's set_state_bps writes the event
(t0, x0, θ0, all free) itself: a sticky case's trace begins with exactly that event and the device test appends what follows it.

    name        what it is
    one         d = 1, t0 = 0, 600 events at multiples of 1/8 with repeats (events 200..260 share ONE time, a grid time), dt = 0.25, K = 400;
                segments of 0, 1, 300 and 299 events.
    short_grid  `one` with K = 8: the grid runs out inside the first long segment, npoints > K.
    neg         d = 5, t0 = −1.5, an event at exactly t = 0 (cummean divides by 0 there: ±inf, the same on both sides); the segment [40, 160)
                is grown in two appends with a consume() after each and no reset between them.
    on_grid_end d = 4; the last event of every segment lies exactly on a grid time, the next segment starts with another event at that time.
    d63/64/65   d = 63 / 64 / 65 (one strip with a tail, one full strip, a second strip of one lane), t0 = 0.3, dt = 0.1; every event time is
                g = t0 + dt·k exactly or nextafter(g, ±inf), several events per time.  Full-precision x.
    sparse      d = 7, 2 chains, 12 events each over [0, 50], dt = 0.05, K = 1100: hundreds of rows between two events; one segment gives
                chain 0 events and chain 1 none.
    sticky130   sticky, d = 130 (strips of 64, 64 and 2), t0 = 0: the first event is (t0, x0, θ0, all free) -- cummean's 0/0 --, the masks flip
                bits 63, 64 and 129 (and others) between events; a grown segment.
    boom        Boomerang, d = 65, μ ≠ 0, dt = 0.37: events sit 1e-9 ... 1e-1 before grid times (τ from 1e-9 up) and gaps of 7 and 20 between
                events put τ past 2π.
    boom_sticky sticky Boomerang, d = 66.
    c1024       sticky, d = 1024 (16 strips: every word of the mask), 2 chains of about 20 events.

DYADIC cases (one, short_grid, neg, on_grid_end, sticky130): times are multiples of 1/8, dt = 0.25, x a multiple of 2^-20 and θ in {−1, 0, 1}:
every product and sum of the consumers is exact, so trace.py and the C reference agree BIT FOR BIT whatever the order of summation.
"""
import functools
from dataclasses import dataclass

import numpy as np


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
    t: list
    x: list
    th: list
    cuts: list
    dyadic: bool
    f: list = None
    mu: np.ndarray = None
    grow: frozenset = frozenset()

    @property
    def nchains(self):
        return len(self.t)

    @property
    def sticky(self):
        return self.f is not None

    @property
    def nseg(self):
        return len(self.cuts[0]) - 1

    def segment(self, k, s):
        """(t, x, θ, f) of chain k's segment s"""
        a, b = self.cuts[k][s], self.cuts[k][s + 1]
        return self.t[k][a:b], self.x[k][a:b], self.th[k][a:b], (self.f[k][a:b] if self.sticky else None)

    def so_far(self, k, s):
        """chain k's trace after segment s has been fed"""
        b = self.cuts[k][s + 1]
        return self.t[k][:b], self.x[k][:b], self.th[k][:b], (self.f[k][:b] if self.sticky else None)


NAMES = ["one", "short_grid", "neg", "on_grid_end", "d63", "d64", "d65", "sparse", "sticky130", "boom", "boom_sticky", "c1024"]
DYADIC = ["one", "short_grid", "neg", "on_grid_end", "sticky130"]


def _dyadic_x(rng, shape):
    return 0.5 + rng.integers(0, 3 * 2 ** 19 + 1, shape) * 2.0 ** -20  # multiples of 2^-20 in [0.5, 2]


def _state(rng, nch, d, dyadic):
    x0 = _dyadic_x(rng, (nch, d)) if dyadic else rng.uniform(0.5, 2.0, (nch, d))
    return x0, rng.choice([-1.0, 1.0], (nch, d))


def _xs(rng, n, d, dyadic):
    return (_dyadic_x(rng, (n, d)) if dyadic else rng.uniform(0.5, 2.0, (n, d))), rng.choice([-1.0, 0.0, 1.0], (n, d))


def _lattice_times(rng, n, t0, p=(0.5, 0.38, 0.12), burst=None, skip_zero=True):
    """n non-decreasing multiples of 1/8 behind t0; events burst[0]..burst[1]−1 share one time, a multiple of 1/4"""
    steps = rng.choice([0, 1, 2], n, p=p)
    steps[0] = 1
    if burst:
        steps[burst[0] + 1:burst[1]] = 0
        steps[burst[1]] = max(steps[burst[1]], 1)
        steps[burst[0]] += int(steps[:burst[0] + 1].sum() + round(t0 * 8)) % 2
    t = t0 + np.cumsum(steps) / 8.0
    zero = np.flatnonzero(t == 0.0)
    if skip_zero and len(zero):
        t[zero[0]:] += 0.125
    assert np.all(np.diff(t) >= 0) and t[0] > t0
    return t


def _one(K):
    rng = np.random.default_rng(201)
    n = 600
    t = _lattice_times(rng, n, 0.0, p=(0.66, 0.28, 0.06), burst=(200, 260))
    x0, th0 = _state(rng, 1, 1, True)
    x, th = _xs(rng, n, 1, True)
    return Case("one" if K == 400 else "short_grid", 1, 0.0, x0, th0, 0.25, K, 320, [t], [x], [th], [[0, 0, 1, 301, 600]], True)


def _neg():
    rng = np.random.default_rng(202)
    n, d, t0 = 260, 5, -1.5
    t = _lattice_times(rng, n, t0, skip_zero=False)
    j = int(np.searchsorted(t, 0.0))
    t[j:] += 0.0 - t[j]  # an event at exactly t = 0, the rest shifted with it
    assert t[j] == 0.0 and np.all(np.diff(t) >= 0) and 0 < j < 40
    x0, th0 = _state(rng, 1, d, True)
    x, th = _xs(rng, n, d, True)
    return Case("neg", d, t0, x0, th0, 0.25, 300, 160, [t], [x], [th], [[0, 40, 100, 160, 260]], True, grow=frozenset([1]))


def _on_grid_end():
    rng = np.random.default_rng(203)
    d, n = 4, 120
    cuts = [0, 30, 31, 75, 120]
    t = _lattice_times(rng, n, 0.0, p=(0.3, 0.5, 0.2))
    for c in cuts[1:]:  # the segment's last event ON a grid time (a multiple of 1/4), the next segment's first event at the same time
        t[c - 1:] += (-(t[c - 1] * 8.0)) % 2.0 / 8.0
        if c < n:
            t[c:] += t[c - 1] - t[c]
    assert np.all(np.diff(t) >= 0) and all((t[c - 1] * 4.0) % 1.0 == 0.0 for c in cuts[1:])
    x0, th0 = _state(rng, 1, d, True)
    x, th = _xs(rng, n, d, True)
    return Case("on_grid_end", d, 0.0, x0, th0, 0.25, 200, 64, [t], [x], [th], [cuts], True)


def _row(d):
    rng = np.random.default_rng(2000 + d)
    n, t0, dt = 120, 0.3, 0.1
    k = 1 + np.cumsum(rng.choice([0, 1, 2], n, p=[0.6, 0.3, 0.1]))
    side = rng.integers(-1, 2, n)
    order = np.lexsort((side, k))
    k, side = k[order], side[order]
    g = t0 + dt * k.astype(np.float64)  # the device's grid time, bit for bit
    t = np.where(side == 0, g, np.where(side < 0, np.nextafter(g, -np.inf), np.nextafter(g, np.inf)))
    x0, th0 = _state(rng, 1, d, False)
    x, th = _xs(rng, n, d, False)
    return Case("d%d" % d, d, t0, x0, th0, dt, 100, 80, [t], [x], [th], [[0, 50, 120]], False)


def _sparse():
    rng = np.random.default_rng(204)
    d, n = 7, 12
    x0, th0 = _state(rng, 2, d, False)
    ts, xs, ths = [], [], []
    for _ in range(2):
        ts.append(np.sort(rng.uniform(0.5, 50.0, n)))
        x, th = _xs(rng, n, d, False)
        xs.append(x)
        ths.append(th)
    return Case("sparse", d, 0.0, x0, th0, 0.05, 1100, 16, ts, xs, ths, [[0, 3, 6, 9, 12], [0, 3, 6, 6, 12]], False)


def _masks(rng, n, d, flip):
    """[n x d] free masks, row 0 all free; every row flips the bits of `flip` with probability 1/2 each and a few others"""
    f = np.ones((n, d), dtype=bool)
    for e in range(1, n):
        f[e] = f[e - 1]
        for b in flip:
            if rng.random() < 0.5:
                f[e, b] = ~f[e, b]
        for b in rng.integers(0, d, 3):
            f[e, b] = ~f[e, b]
    return f


def _sticky130():
    rng = np.random.default_rng(205)
    d, n = 130, 220
    t = np.concatenate([[0.0], _lattice_times(rng, n - 1, 0.0, skip_zero=False)])
    x0, th0 = _state(rng, 1, d, True)
    x, th = _xs(rng, n, d, True)
    x[0], th[0] = x0[0], th0[0]  # (t0, x0, θ0, all free): what the sticky sampler writes first
    f = _masks(rng, n, d, (63, 64, 129))
    assert all(len(np.unique(f[:, b])) == 2 for b in (63, 64, 129))
    return Case("sticky130", d, 0.0, x0, th0, 0.25, 200, 160, [t], [x], [th], [[0, 1, 2, 90, 150, 220]], True, f=[f], grow=frozenset([3]))


def _boom(d, sticky):
    rng = np.random.default_rng(206 + d)
    t0, dt = 0.25, 0.37
    # events a little before grid times (τ of the next row: 1e-9 ... 1e-1), then long gaps (τ beyond 2π and 6π), then ordinary ones
    ks = np.arange(2, 20, 2)
    t = [t0 + dt * k - 10.0 ** -(9 - q) for q, k in enumerate(ks)]
    t += [t[-1] + 7.0, t[-1] + 27.0]
    t = np.array(t + list(t[-1] + np.cumsum(rng.uniform(0.01, 1.5, 40))))
    if sticky:
        t = np.concatenate([[t0], t])
    n = len(t)
    mu = rng.uniform(-1.0, 1.0, d)
    x0 = (mu + rng.standard_normal(d))[None]
    th0 = rng.standard_normal((1, d))
    x = mu + rng.standard_normal((n, d))
    th = rng.standard_normal((n, d))
    f = None
    if sticky:
        x[0], th[0] = x0[0], th0[0]
        f = [_masks(rng, n, d, (0, 63, 64, d - 1))]
    cut = [0, 1, 6, n] if sticky else [0, 5, n]
    return Case("boom_sticky" if sticky else "boom", d, t0, x0, th0, dt, 260, 64, [t], [x], [th], [cut], False, f=f, mu=mu)


def _c1024():
    rng = np.random.default_rng(208)
    d, n = 1024, 21
    x0, th0 = _state(rng, 2, d, False)
    ts, xs, ths, fs = [], [], [], []
    for k in range(2):
        t = np.concatenate([[0.5], 0.5 + np.sort(rng.uniform(0.0, 6.0, n - 1))])
        x, th = _xs(rng, n, d, False)
        x[0], th[0] = x0[k], th0[k]
        f = np.ones((n, d), dtype=bool)
        f[1:] = rng.random((n - 1, d)) < 0.7
        ts.append(t), xs.append(x), ths.append(th), fs.append(f)
    return Case("c1024", d, 0.5, x0, th0, 0.2, 40, 24, ts, xs, ths, [[0, 1, 8, 21], [0, 1, 12, 21]], False, f=fs)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("one", "short_grid"):
        return _one(400 if name == "one" else 8)
    if name in ("d63", "d64", "d65"):
        return _row(int(name[1:]))
    if name.startswith("boom"):
        return _boom(66 if name == "boom_sticky" else 65, name == "boom_sticky")
    return {"neg": _neg, "on_grid_end": _on_grid_end, "sparse": _sparse, "sticky130": _sticky130, "c1024": _c1024}[name]()


@functools.lru_cache(maxsize=None)
def reference(name, k, s):
    """The C reference on chain k's trace after segment s (computed once, shared by the tests; treat as read-only)"""
    import pdmp_trace_ref_lib as R
    c = case(name)
    t, x, th, f = c.so_far(k, s)
    return R.consume(c.t0, c.x0[k], c.th0[k], t, x, th, f=f, mu=c.mu, dt=c.dt, K=c.K)
