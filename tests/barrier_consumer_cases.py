"""Hand-made traces of a barrier ZigZag (stickyzz) with the values its consumers must return WRITTEN OUT BY HAND: one table for
tests/test_barrier_consumers_host.py (trace.barrier_occupation / barrier_start and the other host mirrors, no device) and
tests/test_gpu_barrier_consumers.py (the device consumers behind Ensemble.barrier_consume_begin, through pdmp_debug_trace_append).  TEST
INFRASTRUCTURE ONLY; nothing here touches the device.

d = 4, 2 chains, t0 = 0, grid step 1, T_last = 4 for both chains: every time, position, sum and mean (y / (2 T_last) = y / 8) is a dyadic
number, exact in float64 whatever the order of operations, so every comparison is for equality.

    coordinate   barriers (lo, hi)    chain 0                                           chain 1
    0            (−1, 2), walls       hi wall at t = 2 (hit and thaw at one time),      STARTS FROZEN on lo (θ0 < 0), thaws at 0.75,
                                      lo wall at t = 4 = T_last                         hi wall at 3.75
    1            (−0.5, 1.5)          STARTS FROZEN on hi (θ0 > 0), thaws at 1.5,       hits hi at 1.5, thaws (reflected) at 2.5, an ordinary
                                      hits lo at 3.5, thaws at 3.875                    reflection at 4 = T_last
    2            (0.5, 0.5): a level  met from ABOVE at 0.5 (counts as lo), thaws at    met from BELOW at 0.5 (counts as hi), thaws at 2,
                                      1, reflects at 2.125 (off the grid), met from     reflects at 3, met from above at 4: still frozen at
                                      below at 3.25 (hi), thaws at 3.75                 the last event, for no time
    3            (−1, 1)              hits lo at 1.25; ANOTHER θ = 0 event at 2.25      NO EVENT
                                      (behind θ_c = 0: time counts, no hit); still
                                      frozen at the last event: extended to T_last

Events lie exactly on grid times (t = 1, 2, and the last ones at 4).  Each chain is fed in two segments; the cut falls between a wall's hit and
its thaw, so the cursors, sides and counts carry across a consume() in the middle of the pair."""
import numpy as np

EVENT_DTYPE = np.dtype([("t", "<f8"), ("i", "<i8"), ("x", "<f8"), ("theta", "<f8")])  # (= _lib.EVENT_DTYPE; the tests assert it)
INF = float("inf")

D, NCHAINS, T0, DT, K, TRACE_CAPACITY = 4, 2, 0.0, 1.0, 8, 16
# ((lo, hi), (rule_lo, rule_hi), (κ_lo, κ_hi)): what tests/stickyzz_ref_lib.barrier_table and trace.barrier_start take
BARRIERS = [((-1.0, 2.0), ("reflect", "reflect"), (INF, INF)),
            ((-0.5, 1.5), ("sticky", "reflect"), (1.0, 1.0)),
            ((0.5, 0.5), ("sticky", "sticky"), (1.0, 1.0)),
            ((-1.0, 1.0), ("sticky", "sticky"), (0.5, 0.5))]
X0 = np.array([[0.0, 1.5, 1.0, 0.25], [-1.0, 0.0, 0.0, 0.5]])
TH0 = np.array([[1.0, 1.0, -1.0, -1.0], [-1.0, 1.0, 1.0, -0.25]])
TH_EFF = np.array([[1.0, 0.0, -1.0, -1.0], [0.0, 1.0, 1.0, -0.25]])  # barrier_start: 0 where x0 lies on the barrier of θ0's direction
SIDE0 = np.array([[1, 1, 0, 0], [0, 1, 1, 0]])

_EVENTS = [
    [(0.5, 2, 0.5, 0.0), (1.0, 2, 0.5, -1.0), (1.25, 3, -1.0, 0.0), (1.5, 1, 1.5, -1.0), (2.0, 0, 2.0, 0.0), (2.0, 0, 2.0, -1.5),
     (2.125, 2, -0.625, 1.0), (2.25, 3, -1.0, -0.0), (3.25, 2, 0.5, 0.0), (3.5, 1, -0.5, 0.0), (3.75, 2, 0.5, 1.0), (3.875, 1, -0.5, 1.0),
     (4.0, 0, -1.0, 0.0), (4.0, 0, -1.0, 1.5)],
    [(0.5, 2, 0.5, 0.0), (0.75, 0, -1.0, 1.0), (1.5, 1, 1.5, 0.0), (2.0, 2, 0.5, 1.0), (2.5, 1, 1.5, -1.0), (3.0, 2, 1.5, -1.0),
     (3.75, 0, 2.0, 0.0), (3.75, 0, 2.0, -1.0), (4.0, 1, 0.0, 1.0), (4.0, 2, 0.5, 0.0)],
]
EVENTS = [np.array(e, dtype=EVENT_DTYPE) for e in _EVENTS]
CUTS = [[0, 5, 14], [0, 7, 10]]  # chain k's segment s is EVENTS[k][CUTS[k][s]:CUTS[k][s + 1]]: between the hit and the thaw of a wall
NSEG = 2
T_LAST = np.array([4.0, 4.0])

# ---- by hand: occupation
FROZEN_LO = np.array([[0.0, 0.375, 0.5, 2.75], [0.75, 0.0, 0.0, 0.0]])  # chain 0, coordinate 3: 1.0 between its two θ = 0 events + (4 − 2.25)
FROZEN_HI = np.array([[0.0, 1.5, 0.5, 0.0], [0.0, 1.0, 1.5, 0.0]])
HITS_LO = np.array([[1, 1, 1, 1], [0, 0, 1, 0]], dtype=np.uint64)
HITS_HI = np.array([[1, 0, 1, 0], [1, 1, 1, 0]], dtype=np.uint64)
# ---- by hand: y_i = Σ (x_prev + x_k)(t_k − t_prev) over i's events, and mean = y / (2 T_last)
Y = np.array([[6.0, 6.125, 1.46875, -2.9375], [1.5, 7.5, 5.75, 0.0]])
MEAN = Y / 8.0
# ---- by hand: collect(discretize(Ξ, 1.0)) from the start (t0, x0, θ_eff): the grid times before T_last, events with t <= g applied
GRID_T = np.array([0.0, 1.0, 2.0, 3.0])
GRID_X = np.array([[[0.0, 1.5, 1.0, 0.25], [1.0, 1.5, 0.5, -0.75], [2.0, 1.0, -0.5, -1.0], [0.5, 0.0, 0.25, -1.0]],
                   [[-1.0, 0.0, 0.0, 0.5], [-0.75, 1.0, 0.5, 0.25], [0.25, 1.5, 0.5, 0.0], [1.25, 1.0, 1.5, -0.25]]])


def segment(k, s):
    return EVENTS[k][CUTS[k][s]:CUTS[k][s + 1]]


def so_far(k, s):
    """chain k's trace after segment s has been fed"""
    return EVENTS[k][:CUTS[k][s + 1]]
