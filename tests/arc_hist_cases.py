"""The case table of the arc histogram consumer (pdmp_ensemble_bps_consume_arc_hist): the hand-made Boomerang traces of tests/arc_pairs_cases.py
(boom, boom_sticky, d1, sticky130, edge, two: τ = 0, τ < 0, τ = 1e-9, τ past 2π and 6π, μ ≠ 0, masks flipping bits 63, 64 and 129, buffers smaller
than the trace, a segment grown in place) with bin lists, and hand-made pieces of its own.  One table for tests/test_arc_hist_ref.py (the C
statement, the host mirror and the exact occupation, no device) and tests/test_gpu_arc_hist.py (the device against the C statement, through
pdmp_debug_bps_trace_append).  TEST INFRASTRUCTURE ONLY; nothing here touches the device.

    entry            trace      list
    boom_62          boom       5 coordinates across both mask words, 62 bins on [−2.5, 2.5): a row of 64 slots (one per lane)
    boom_sticky_63   boom_sticky  5 coordinates, 63 bins on [−2.75, 2.75): 65 slots (the second register slot of lane 0 alone)
    d1_1, d1_2       d1         m = 1, 1 and 2 bins
    d1_4096          d1         m = 1, 4096 bins: the long-row walk in global memory
    sticky130_all    sticky130  all 130 coordinates (33 workgroups of four wavefronts, the last half empty), 2 bins
    sticky130_126    sticky130  5 coordinates, 126 bins: 128 slots, the longest row kept in registers
    edge_127         edge       all 5 coordinates, 127 bins: 129 slots, the shortest row walked in global memory
    sticky130_127    sticky130  5 coordinates, 127 bins: the sticky walk in global memory -- coordinates that are not free add their rest time to a
                                slot that an arc of the same coordinate adds to before and after
    sticky130_4096   sticky130  2 coordinates, 4096 bins on [−30, 30): the sticky walk in global memory over 65 rounds of 64 slots
    rest0_127        rest0      127 bins: the walk in global memory with a free coordinate at rest (R == 0)
    two_63           two        2 chains, m = 3, 63 bins; the middle segment gives chain 1 nothing
    d1_inside        d1         a range of width 0.1 about μ: wholly inside the sweep of the arcs, most time in the two outer slots
    edge_never       edge       coordinate 0 with a range far below the path, coordinate 1 far above it: one outer slot takes everything
    d1_onebin        d1         2 bins on [−100, 300): the path stays inside the single bin [−100, 100)
    rest0            (own)      d = 2, not sticky: coordinate 0 sits at μ with θ = 0 on three of six pieces (free, u = p = 0: at rest)
    tangent          (own)      3 chains of one piece each: μ = 0, u = 1, p = 0, τ = π/2, π and 2π as doubles, 4 bins on [−1, 1): the edges ±1.0
                                are exact tangencies (z = ±1 in exact and in double arithmetic alike), 0.5 gives acos(0.5) = π/3 per crossing;
                                the slots are known by hand (TANGENT_SLOTS, in units of π/6)

Apart from the exact tangencies every (piece, edge) keeps 1 − |z| >= 2^-20 or |z| > 1 (tests/test_arc_hist_ref.py asserts it with mpmath)."""
import functools
import math

import numpy as np

import arc_pairs_cases as AC
import pdmp_consumer_cases as PC


def _rest0():
    rng = np.random.default_rng(931)
    mu = np.array([0.25, -0.5])
    t = np.cumsum(rng.uniform(0.2, 2.5, 6))
    x0, th0 = mu + rng.standard_normal((1, 2)), rng.standard_normal((1, 2))
    x, th = mu + rng.standard_normal((6, 2)), rng.standard_normal((6, 2))
    x0[0, 0], th0[0, 0] = mu[0], 0.0
    for e in (1, 2):  # (the cursor of the pieces 2 and 3)
        x[e, 0], th[e, 0] = mu[0], 0.0
    return PC.Case("rest0", 2, 0.0, x0, th0, 0.0, 0, 8, [t], [x], [th], [[0, 3, 6]], False, mu=mu)


def _tangent():
    taus = [math.pi / 2, math.pi, 2 * math.pi]
    return PC.Case("tangent", 1, 0.0, np.ones((3, 1)), np.zeros((3, 1)), 0.0, 0, 4, [np.array([v]) for v in taus], [np.ones((1, 1))] * 3,
                   [np.zeros((1, 1))] * 3, [[0, 1]] * 3, False, mu=np.zeros(1))


# the tangent case's rows in units of π/6: x = cos s from 1; on a quarter turn it spends π/3 above 0.5 and π/6 in [0, 0.5)
TANGENT_SLOTS = [[0, 0, 0, 1, 2, 0], [0, 2, 1, 1, 2, 0], [0, 4, 2, 2, 4, 0]]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "rest0":
        return _rest0()
    if name == "tangent":
        return _tangent()
    return AC.case(name)


_LISTS = {
    "boom_62": ("boom", [0, 7, 31, 63, 64], -2.5, 2.5, 62),
    "boom_sticky_63": ("boom_sticky", [0, 12, 63, 64, 65], -2.75, 2.75, 63),
    "d1_1": ("d1", [0], -1.0, 1.5, 1),
    "d1_2": ("d1", [0], -1.0, 1.5, 2),
    "d1_4096": ("d1", [0], -3.0, 3.0, 4096),
    "sticky130_all": ("sticky130", None, -1.0, 1.25, 2),
    "sticky130_126": ("sticky130", [0, 63, 64, 65, 129], -3.0, 3.0, 126),
    "edge_127": ("edge", [0, 1, 2, 3, 4], -2.0, 3.0, 127),
    "sticky130_127": ("sticky130", [0, 63, 64, 65, 129], -3.0, 3.0, 127),
    "sticky130_4096": ("sticky130", [64, 129], -30.0, 30.0, 4096),
    "rest0_127": ("rest0", [0, 1], -2.0, 2.0, 127),
    "two_63": ("two", [2, 0, 1], -2.0, 2.0, 63),
    "d1_inside": ("d1", [0], "mu-0.05", "mu+0.05", 2),
    "edge_never": ("edge", [0, 1], [-50.0, 40.0], [-40.0, 50.0], 2),
    "d1_onebin": ("d1", [0], -100.0, 300.0, 2),
    "rest0": ("rest0", [0, 1], -2.0, 2.0, 5),
    "tangent": ("tangent", [0], -1.0, 1.0, 4),
}
NAMES = list(_LISTS)


@functools.lru_cache(maxsize=None)
def listed(name):
    """(case, coords [m], lo [m], hi [m], bins) of the entry `name` of NAMES"""
    cname, coords, lo, hi, bins = _LISTS[name]
    c = case(cname)
    coords = np.arange(c.d, dtype=np.int64) if coords is None else np.asarray(coords, dtype=np.int64)
    if isinstance(lo, str):
        lo, hi = c.mu[coords] - 0.05, c.mu[coords] + 0.05
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), coords.shape))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64), coords.shape))
    return c, coords, lo, hi, bins


@functools.lru_cache(maxsize=None)
def reference(name, k, s):
    """The C statement on chain k's trace after segment s: (H, Z, T_last) (computed once, shared by the tests; treat as read-only)"""
    import arc_hist_ref_lib as AH
    c, coords, lo, hi, bins = listed(name)
    t, x, th, f = c.so_far(k, s)
    return AH.arcs(c.t0, c.x0[k], c.th0[k], t, x, th, c.mu, coords, lo, hi, bins, f=f)
