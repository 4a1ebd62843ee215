"""Trace consumers, mirroring src/trace.jl for FactTrace (what every caller of spdmp does next with Ξ).

Events are structured arrays (t, i, x, theta) with 0-based i.  Host side only: these are the callers' post-processing
(SURVEY.md 8f1), not part of the device hot path.  Everything is vectorised over EVENTS (no interpreter loop per event): a
coordinate's path depends on its own events only -- between two of them it flows freely (linearly, or by the FactBoomerang's
rotation about μ_i) -- so the events are grouped per coordinate once (stable sort) and every consumer is a handful of array
operations; the only Python loops left run over coordinates (collect / discretize), never over events.  The reference moves
all coordinates step by step (x += θ·Δt per event); the closed forms used here agree with it to rounding.
"""
import numpy as np

from .flows import Boomerang, FactBoomerang, FactTrace, PDMPTrace


def _is_boom(tr):
    return isinstance(tr.F, FactBoomerang)


def _free_flow(tr, j, x, th, tau):
    """State of coordinate(s) j a time tau after (x, θ): linear (src/dynamics.jl:11-15) or the rotation about μ_j (:29-36)."""
    if _is_boom(tr):
        mu = tr.F.μ[j]
        s, c = np.sin(tau), np.cos(tau)
        return (x - mu) * c + th * s + mu, -(x - mu) * s + th * c
    return x + th * tau, th + 0.0 * tau


def _prev_same_coordinate(tr):
    """For every event k (in trace order; with a refresh clock the trace is sorted within a coordinate only, which is all this needs): time,
    position and velocity the coordinate had after ITS previous event (the initial state for its first one)."""
    ev = tr.events
    n = len(ev)
    i = ev["i"].astype(np.int64)
    order = np.argsort(i, kind="stable")  # by coordinate, time order kept inside a coordinate
    si = i[order]
    prev_sorted = np.empty(n, dtype=np.int64)
    if n:
        prev_sorted[0] = -1
        prev_sorted[1:] = np.where(si[1:] == si[:-1], order[:-1], -1)
    prev = np.empty(n, dtype=np.int64)
    prev[order] = prev_sorted
    has = prev >= 0
    pc = np.maximum(prev, 0)
    tp = np.where(has, ev["t"][pc], tr.t0)
    xp = np.where(has, ev["x"][pc], tr.x0[i])
    thp = np.where(has, ev["theta"][pc], tr.θ0[i])
    return i, tp, xp, thp


def _groups(tr):
    """Events grouped per coordinate: (order, ptr) with order[ptr[j]:ptr[j+1]] the event indices of coordinate j in trace order (= its time
    order, also where a refresh clock leaves the trace as a whole unsorted)."""
    i = tr.events["i"].astype(np.int64)
    order = np.argsort(i, kind="stable")
    ptr = np.zeros(tr.x0.size + 1, dtype=np.int64)
    np.cumsum(np.bincount(i, minlength=tr.x0.size), out=ptr[1:])
    return order, ptr


def _states_at(tr, times, upto=None):
    """x_j(times[r]) for every coordinate j: [len(times) x d].  upto[r] = number of leading events (trace order) applied at row r;
    None: every event with t <= times[r]."""
    ev = tr.events
    d = tr.x0.size
    order, ptr = _groups(tr)
    out = np.empty((len(times), d))
    for j in range(d):
        own = order[ptr[j]:ptr[j + 1]]
        if upto is None:
            pos = np.searchsorted(ev["t"][own], times, side="right") - 1
        else:
            pos = np.searchsorted(own, upto - 1, side="right") - 1
        has = pos >= 0
        k = own[np.maximum(pos, 0)] if len(own) else np.zeros(len(times), dtype=np.int64)
        if len(own):
            tl = np.where(has, ev["t"][k], tr.t0)
            xl = np.where(has, ev["x"][k], tr.x0[j])
            thl = np.where(has, ev["theta"][k], tr.θ0[j])
        else:
            tl, xl, thl = tr.t0, tr.x0[j], tr.θ0[j]
        out[:, j] = _free_flow(tr, j, xl, thl, times - tl)[0]
    return out


def collect(tr: FactTrace):
    """collect(Ξ): (t, x) pairs of Base.iterate(FT::FactTrace), src/trace.jl:44-63 -- the initial state, the state after each
    event but the last (which is never applied, :56), and that state once more: 1 + length(events) entries (:42)."""
    ev = tr.events
    n = len(ev)
    if n == 0:
        return np.array([tr.t0]), tr.x0[None].copy()
    ts = np.concatenate([[tr.t0], ev["t"][:n - 1], [ev["t"][n - 2] if n > 1 else tr.t0]])
    upto = np.concatenate([[0], np.arange(1, n), [n - 1]])
    return ts, _states_at(tr, ts, upto=upto)


def _discretize_pdmp(tr: PDMPTrace, dt):
    """collect(discretize(Ξ::PDMPTrace, dt)) -- src/trace.jl:102-106,129-150: the grid t0, t0+dt, ... up to (excluding) the
    last event time; between events the state flows from the latest event (linear, or the Boomerang rotation about μ).
    Closed form per grid point (the reference accumulates dt steps)."""
    d = len(tr.x0)
    if len(tr.t) == 0:
        return np.array([tr.t0]), tr.x0[None].copy()
    n = int(np.ceil((tr.t[-1] - tr.t0) / dt)) + 1  # (+ 1: the quotient of a last event an ulp past a grid time rounds to that grid point's index)
    grid = tr.t0 + dt * np.arange(n)
    grid = grid[grid < tr.t[-1]]
    te = np.concatenate([[tr.t0], tr.t])
    X = np.vstack([tr.x0[None], tr.x.reshape(-1, d)])
    TH = np.vstack([tr.θ0[None], tr.θ.reshape(-1, d)])
    idx = np.searchsorted(te, grid, side="right") - 1
    tau = (grid - te[idx])[:, None]
    if isinstance(tr.F, Boomerang):
        mu = tr.F.μ
        xs = (X[idx] - mu) * np.cos(tau) + TH[idx] * np.sin(tau) + mu
    else:
        xs = X[idx] + TH[idx] * tau
    if tr.f is not None:  # a sticky trace: smove_forward!(…, f, …) moves the free coordinates only (src/ss_not_fact.jl:78-97)
        Fm = np.vstack([np.asarray(tr.f0, dtype=bool)[None], np.asarray(tr.f, dtype=bool).reshape(-1, d)])
        xs = np.where(Fm[idx], xs, X[idx])
    return grid, xs


def discretize_1d(events, flow, dt):
    """discretize(x::Vector, Flow::Union{ZigZag1d, Boomerang1d}, dt) -- src/discretise.jl:10-42, the skeleton of the 1-d samplers to a
    trajectory: the clock advances by dt inside a segment (the step that would cross the next event is shortened and the remainder carried
    into the following segment, :28-29), the state flows by move_forward from the previous grid point (src/dynamics.jl:66-68,79-82), the last
    segment is not emitted (:18) and the final clock / position is appended (:40).  events: structured (t, x, theta).  Returns (t, x)."""
    from .flows import Boomerang1d
    boom = isinstance(flow, Boomerang1d)
    mu = flow.μ if boom else 0.0
    n = len(events)
    ts, xs = [0.0], [float(events["x"][0])]
    clock, dt_cur = 0.0, float(dt)
    xi, th = float(events["x"][0]), float(events["theta"][0])

    def move(tau, clock, xi, th):
        if boom:
            s, c = np.sin(tau), np.cos(tau)
            return clock + tau, (xi - mu) * c + th * s + mu, -(xi - mu) * s + th * c
        return tau + clock, xi + th * tau, th

    k = 0
    while k < n - 2:
        tau_next = float(events["t"][k + 1])
        while clock + dt_cur <= tau_next:
            if th == 0.0:
                clock += dt_cur
            else:
                clock, xi, th = move(dt_cur, clock, xi, th)
            ts.append(clock)
            xs.append(xi)
            dt_cur = float(dt)
        dt_cur = dt_cur - (tau_next - clock)
        if th == 0.0:
            clock = tau_next
        else:
            clock, xi, th = move(tau_next - clock, clock, xi, th)
        k += 1
        xi, th = float(events["x"][k]), float(events["theta"][k])
    ts.append(clock)
    xs.append(xi)
    return np.array(ts), np.array(xs)


def discretize(tr, dt):
    """collect(discretize(Ξ, dt)): positions on the grid t0, t0+dt, ... -- src/trace.jl:94-125 (FactTrace: a grid point is
    emitted while it lies before the last event; events at or before a grid time are applied), :129-150 (PDMPTrace)."""
    if isinstance(tr, PDMPTrace):
        return _discretize_pdmp(tr, dt)
    ev = tr.events
    if len(ev) == 0:
        return np.array([tr.t0]), tr.x0[None].copy()
    # The reference consumes the events IN TRACE ORDER and stops at the first one later than the grid time (:111-113).  A refresh
    # of a coordinate whose clock lags (src/sfact.jl:84-85: the refreshed i is not moved to t′) is recorded with its stale time, so a
    # trace with λref > 0 is not sorted; the number of events applied at grid time g is the first index whose time exceeds g,
    # i.e. a search in the running maximum of the event times.
    tmax = np.maximum.accumulate(ev["t"])
    n = int(np.ceil((tmax[-1] - tr.t0) / dt)) + 1
    grid = tr.t0 + dt * np.arange(n)
    grid = grid[grid < tmax[-1]]
    if len(grid) == 0:
        grid = np.array([tr.t0])
    return grid, _states_at(tr, grid, upto=np.searchsorted(tmax, grid, side="right"))


def _mean_pdmp(tr: PDMPTrace):
    """Statistics.mean(Ξ::PDMPTrace) -- src/trace.jl:229-246, restated as written: Σ (x + x₂)(t₂ − t) over consecutive events divided
    by the LAST event time T -- the reference omits the ½ of the trapezoid rule here (its cummean, :248-266, has it), so this is
    twice the time average of the interpolated path."""
    d = len(tr.x0)
    X = np.vstack([tr.x0[None], np.asarray(tr.x).reshape(-1, d)])
    te = np.concatenate([[tr.t0], tr.t])
    y = ((X[:-1] + X[1:]) * np.diff(te)[:, None]).sum(0)
    return y / tr.t[-1]


def _segment_integrals(tr):
    """Per event k of coordinate i: Δt since i's previous event and the reference's trapezoid term (x_prev + x_k)·Δt, where x_k is
    the RECORDED position (src/trace.jl:191-195; for a ZigZag the path between two events of i is the chord, so this is exact)."""
    i, tp, xp, _ = _prev_same_coordinate(tr)
    ev = tr.events
    dt = ev["t"] - tp
    return i, dt, (xp + ev["x"]) * dt, xp


def cummean(tr):
    """cummean(Ξ) -- src/trace.jl:203-225 (FactTrace: per coordinate the running (t, ∫x/(2t))) and :248-266 (PDMPTrace: the
    running vector y/(2t) after every event).  Returns a list of (t, y) array pairs per coordinate, resp. an [n x d] array."""
    if isinstance(tr, PDMPTrace):
        d = len(tr.x0)
        X = np.vstack([tr.x0[None], np.asarray(tr.x).reshape(-1, d)])
        te = np.concatenate([[tr.t0], tr.t])
        y = np.cumsum((X[:-1] + X[1:]) * np.diff(te)[:, None], axis=0)
        return y / (2.0 * te[1:, None])
    ev = tr.events
    _, _, term, _ = _segment_integrals(tr)
    order, ptr = _groups(tr)
    out = []
    for j in range(tr.x0.size):
        own = order[ptr[j]:ptr[j + 1]]
        t = ev["t"][own]
        y = np.cumsum(term[own]) / (2 * t) if len(own) else np.empty(0)
        out.append((np.concatenate([[tr.t0], t]), np.concatenate([[tr.x0[j]], y])))
    return out


def mean(tr):
    """mean(Ξ): time average of the piecewise-linear path per coordinate -- src/trace.jl:182-200 (FactTrace), :229-246 (PDMPTrace).  A FactTrace
    is taken in trace order, so traces with a refresh clock (λref > 0, FactBoomerang) are served as the reference serves them: T is the time of
    the LAST event, which need not be the largest; the FactBoomerang gets the same trapezoid between recorded positions (:194).  cummean and
    discretize likewise; Ensemble.refresh_consume_begin opens their device twins."""
    if isinstance(tr, PDMPTrace):
        return _mean_pdmp(tr)
    ev = tr.events
    i, _, term, _ = _segment_integrals(tr)
    T = ev["t"][-1]
    return np.bincount(i, weights=term * (1 / (2 * T)), minlength=tr.x0.size)  # (summed per coordinate in event order, like :191-196)


def moments(tr: FactTrace, T_end=None):
    """Exact time averages of x_i and x_i² over [t0, T_end] (segments of coordinate i between ITS events, linear flow);
    the tail after a coordinate's last event is extrapolated with its last velocity.  Used by the tests and the ESS validation."""
    ev = tr.events
    d = tr.x0.size
    if T_end is None:
        T_end = ev["t"][-1]
    keep = ev["t"] <= T_end
    sub = FactTrace(tr.F, tr.t0, tr.x0, tr.θ0, ev[keep])
    i, tp, xa, tha = _prev_same_coordinate(sub)
    e = sub.events
    dt = e["t"] - tp
    xb = xa + tha * dt
    s1 = np.bincount(i, weights=dt * (xa + xb) / 2, minlength=d)
    s2 = np.bincount(i, weights=dt * (xa * xa + xa * xb + xb * xb) / 3, minlength=d)
    # the open segment after each coordinate's last event
    tl, xl, thl = np.full(d, tr.t0), tr.x0.astype(np.float64).copy(), tr.θ0.astype(np.float64).copy()
    if len(e):
        order, ptr = _groups(sub)
        last = order[np.maximum(ptr[1:] - 1, 0)]
        has = ptr[1:] > ptr[:-1]
        tl = np.where(has, e["t"][last], tl)
        xl = np.where(has, e["x"][last], xl)
        thl = np.where(has, e["theta"][last], thl)
    dt = T_end - tl
    xb = xl + thl * dt
    s1 += dt * (xl + xb) / 2
    s2 += dt * (xl * xl + xl * xb + xb * xb) / 3
    L = T_end - tr.t0
    m = s1 / L
    return m, s2 / L - m * m


def path_moments(tr: PDMPTrace, T):
    """(∫_{t0}^{T} x dt, ∫_{t0}^{T} x² dt) of the path a PDMPTrace describes, [d] each, in closed form per segment: between two events
    the state flows freely from the earlier one's (x, θ) -- linearly for a BouncyParticle (src/dynamics.jl:11-15), by the rotation about
    F.μ for a Boomerang (:29-36).  Past the last event the path goes on from that event's (x, θ) (the caller guarantees that T lies
    before the next one); events after T are cut off.  The host statement of pdmp_ensemble_bps_moments (mean = ∫x/(T − t0))."""
    d = len(tr.x0)
    X = np.vstack([np.asarray(tr.x0, dtype=np.float64)[None], np.asarray(tr.x, dtype=np.float64).reshape(-1, d)])
    TH = np.vstack([np.asarray(tr.θ0, dtype=np.float64)[None], np.asarray(tr.θ, dtype=np.float64).reshape(-1, d)])
    te = np.concatenate([[tr.t0], np.asarray(tr.t, dtype=np.float64)])
    end = np.minimum(np.append(te[1:], np.inf), T)
    tau = np.maximum(end - te, 0.0)[:, None]
    if isinstance(tr.F, Boomerang):
        m = np.asarray(tr.F.μ, dtype=np.float64)[None]
        A = X - m
        s, c = np.sin(tau), np.cos(tau)
        rot = A * s + TH * (1.0 - c)
        j1 = m * tau + rot
        j2 = m * m * tau + 2.0 * m * rot + A * A * (tau / 2 + s * c / 2) + TH * TH * (tau / 2 - s * c / 2) + A * TH * s * s
    else:
        j1 = tau * (X + TH * tau / 2)
        j2 = tau * (X * X + X * TH * tau + TH * TH * tau * tau / 3)
    return j1.sum(0), j2.sum(0)


def subtrace(tr: FactTrace, J):
    """subtrace(Ξ, J): trace of the subvector x[J] -- src/trace.jl:275-290."""
    J = np.asarray(J, dtype=np.int64)
    assert np.all(np.diff(J) > 0)
    ev = tr.events
    if len(J) == 0:  # (nothing to look up in: no event is kept)
        return FactTrace(tr.F, tr.t0, tr.x0[J].copy(), tr.θ0[J].copy(), ev[:0].copy())
    loc = np.searchsorted(J, ev["i"])
    loc_c = np.minimum(loc, len(J) - 1)
    keep = J[loc_c] == ev["i"]
    sub = ev[keep].copy()
    sub["i"] = loc_c[keep]
    return FactTrace(tr.F, tr.t0, tr.x0[J].copy(), tr.θ0[J].copy(), sub)


def inclusion_prob(tr: FactTrace):
    """inclusion_prob(Ξ): fraction of time each coordinate is non-zero -- src/trace.jl:161-178.  A sticky PDMPTrace (one carrying f):
    the fraction of [t0, T_last] each coordinate is free, from the recorded masks."""
    if isinstance(tr, PDMPTrace):
        if tr.f is None:
            raise TypeError("inclusion_prob of a PDMPTrace needs the free masks of a sticky sampler (sspdmp)")
        d = len(tr.x0)
        te = np.concatenate([[tr.t0], np.asarray(tr.t, dtype=np.float64)])
        Fm = np.vstack([np.asarray(tr.f0, dtype=bool)[None], np.asarray(tr.f, dtype=bool).reshape(-1, d)])
        if len(te) < 2 or not te[-1] > tr.t0:
            return Fm[0].astype(np.float64)
        return (Fm[:-1] * np.diff(te)[:, None]).sum(0) / (te[-1] - tr.t0)
    ev = tr.events
    i, dt, _, xp = _segment_integrals(tr)
    T = ev["t"][-1]
    return np.bincount(i, weights=((xp != 0) | (ev["x"] != 0)) * dt / T, minlength=tr.x0.size)


def _barrier_levels(barriers, d):
    """(lo, hi) [d] of a list of d StickyBarriers -- or plain ((lo, hi), rules, κ) triples --, or of one for all coordinates"""
    def one(b):
        return hasattr(b, "x") or (isinstance(b, tuple) and len(b) == 3 and isinstance(b[1], tuple) and isinstance(b[1][0], str))

    bl = [barriers] * d if one(barriers) else list(barriers)
    if len(bl) != d:
        raise ValueError("barriers: a list of %d StickyBarriers, or one for all coordinates" % d)
    x = [b.x if hasattr(b, "x") else b[0] for b in bl]
    return np.array([float(v[0]) for v in x]), np.array([float(v[1]) for v in x])


def barrier_start(x0, θ0, barriers):
    """(θ_eff, side0) of a stickyzz start (src/stickyzz.jl:198-208): a coordinate whose x0[i] equals the barrier in the direction of θ0[i] -- the
    upper one for θ0[i] > 0, else the lower one -- starts frozen.  θ_eff is θ0 with 0 there: the velocities of the path the chain travels, and
    the start (t0, x0, θ_eff) the device consumers of a barrier ensemble work from (Ensemble.barrier_consume_begin).  The host mirrors (mean,
    discretize, cummean, pair_integrals, conditional_trace) agree with them on FactTrace(F, t0, x0, θ_eff, events); on the trace a sampler
    returns, which records θ0 like the reference's Trace(t′, x0, v0), they extrapolate a frozen start with a speed it never had.  side0 [.. x d]:
    1 where θ0 > 0 (upper barrier), else 0.  x0 / θ0 may carry a leading chain axis."""
    x0 = np.asarray(x0, dtype=np.float64)
    θ0 = np.asarray(θ0, dtype=np.float64)
    lo, hi = _barrier_levels(barriers, x0.shape[-1])
    up = θ0 > 0
    frozen = x0 == np.where(up, hi, lo)
    return np.where(frozen, 0.0, θ0), up.astype(np.int64)


def barrier_occupation(Ξ, t0, x0, θ0, barriers):
    """(frozen_lo, frozen_hi [d] float64, hits_lo, hits_hi [d] uint64, T_last): how long each coordinate of a stickyzz / sspdmp2 trace sat
    frozen (θ = 0) on its lower and on its upper barrier over [t0, T_last], and how often it hit each -- raw sums, the caller divides; the
    host mirror of Ensemble.barrier_consume_occupation, bit for bit (DESIGN.md "Barrier occupation").  Ξ: a FactTrace or its events; (t0,
    x0, θ0): the start as the sampler was given it (θ0 ≠ 0 everywhere; barrier_start tells which coordinates start frozen, and on which side).

    Per coordinate, a cursor (t_c, θ_c) from (t0, θ_eff) and a side s from side0; for each of its events (t, x, θ) in trace order:
    θ_c == 0: z[s] += t − t_c;  θ == 0 and θ_c ≠ 0 (a hit): s = upper iff θ_c > 0, n[s] += 1;  then the cursor takes (t, θ).  A θ == 0 event
    behind θ_c == 0 counts nothing.  −0.0 counts as 0.  A coordinate still frozen at the end is extended to T_last, the last event time of the
    whole trace (t0 without events).  A wall's hit and thaw at one time: one hit, no time.  Sums run sequentially per coordinate in float64."""
    ev = Ξ.events if isinstance(Ξ, FactTrace) else Ξ
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1)
    d = x0.size
    th_eff, side0 = barrier_start(x0, np.asarray(θ0, dtype=np.float64).reshape(-1), barriers)
    tc = [float(t0)] * d
    thc = [float(v) for v in th_eff]
    side = [int(s) for s in side0]
    z = [[0.0, 0.0] for _ in range(d)]
    n = np.zeros((d, 2), dtype=np.uint64)
    for t, i, th in zip(ev["t"].tolist(), ev["i"].tolist(), ev["theta"].tolist()):
        if thc[i] == 0.0:
            z[i][side[i]] += t - tc[i]
        if th == 0.0 and thc[i] != 0.0:
            side[i] = 1 if thc[i] > 0.0 else 0
            n[i, side[i]] += np.uint64(1)
        tc[i], thc[i] = t, th
    T_last = float(ev["t"][-1]) if len(ev) else float(t0)
    out = np.array([[z[i][s] + ((T_last - tc[i]) if (thc[i] == 0.0 and s == side[i]) else 0.0) for s in (0, 1)] for i in range(d)]).reshape(d, 2)
    return out[:, 0].copy(), out[:, 1].copy(), n[:, 0].copy(), n[:, 1].copy(), T_last


def _dot_wave64(A, B):
    """Row-wise dot(A[r], B[r]) in the one order the device and the oracle sum in (dot_wave64, oracle/pdmp_oracle.c): lane l adds the
    products of elements l, l + 64, ... in order, then the lanes are combined by the xor butterfly 1, 2, 4, 8, 16, 32."""
    A, B = np.broadcast_arrays(np.atleast_2d(A), np.atleast_2d(B))
    m, k = A.shape
    ns = max((k + 63) // 64, 1)
    P = np.zeros((m, ns * 64))
    P[:, :k] = A * B
    P = P.reshape(m, ns, 64)
    part = np.zeros((m, 64))
    for s in range(ns):
        part = part + P[:, s]
    lanes = np.arange(64)
    for off in (1, 2, 4, 8, 16, 32):
        part = part + part[:, lanes ^ off]
    return part[:, 0]


def _states_before(tr, times):
    """x_j(times[r]) for every coordinate j from j's last event with t < times[r] (strictly), else from (t0, x0_j, θ0_j): [len(times) x d]."""
    ev = tr.events
    d = tr.x0.size
    order, ptr = _groups(tr)
    out = np.empty((len(times), d))
    for j in range(d):
        own = order[ptr[j]:ptr[j + 1]]
        tl, xl, thl = tr.t0, tr.x0[j], tr.θ0[j]
        if len(own):
            pos = np.searchsorted(ev["t"][own], times, side="left") - 1
            has = pos >= 0
            k = own[np.maximum(pos, 0)]
            tl = np.where(has, ev["t"][k], tr.t0)
            xl = np.where(has, ev["x"][k], tr.x0[j])
            thl = np.where(has, ev["theta"][k], tr.θ0[j])
        out[:, j] = xl + thl * (times - tl)
    return out


def _conditional_fact(tr, p, n):
    ev = tr.events
    d = tr.x0.size
    S = np.flatnonzero(n != 0)
    if len(ev) == 0:
        return np.empty(0), np.empty((0, d))
    loc = np.full(d, -1, dtype=np.int64)
    loc[S] = np.arange(len(S))
    l = loc[ev["i"].astype(np.int64)]
    sel = np.flatnonzero(l >= 0)  # the events of S; piece m opens at the (m − 1)-th of them (piece 0 at t0)
    M = len(sel)
    last = np.zeros((M + 1, len(S)), dtype=np.int64)  # per piece and list position: 1 + the latest event of S that set it, 0: the initial state
    last[np.arange(1, M + 1), l[sel]] = np.arange(1, M + 1)
    last = np.maximum.accumulate(last, axis=0)
    has = last > 0
    k = sel[np.maximum(last - 1, 0)] if M else np.zeros_like(last)
    Tc = np.where(has, ev["t"][k], tr.t0)
    Xc = np.where(has, ev["x"][k], tr.x0[S][None])
    THc = np.where(has, ev["theta"][k], tr.θ0[S][None])
    t_b = np.concatenate([[tr.t0], ev["t"][sel]])
    xs = Xc + THc * (t_b[:, None] - Tc)
    g = _dot_wave64(n[S][None], p[S][None] - xs)
    h = _dot_wave64(n[S][None], THc)
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = g / h
    s = t_b + tau
    t_close = np.concatenate([ev["t"][sel], [ev["t"][-1]]])  # the next event of S (inclusive, src/condition.jl:42), else the last event of the trace
    hit = (tau > 0) & (t_close >= s)
    return s[hit], _states_before(tr, s[hit])


def _conditional_pdmp(tr, p, n):
    d = len(tr.x0)
    t = np.asarray(tr.t, dtype=np.float64)
    if len(t) == 0:
        return np.empty(0), np.empty((0, d))
    tc = np.concatenate([[tr.t0], t[:-1]])
    Xc = np.vstack([np.asarray(tr.x0, dtype=np.float64)[None], np.asarray(tr.x, dtype=np.float64).reshape(-1, d)[:-1]])
    THc = np.vstack([np.asarray(tr.θ0, dtype=np.float64)[None], np.asarray(tr.θ, dtype=np.float64).reshape(-1, d)[:-1]])
    g = _dot_wave64(p[None] - Xc, n[None])
    h = _dot_wave64(THc, n[None])
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = g / h
        hit = (tau > 0) & (tc + tau < t)  # (strict, src/condition.jl:63)
    rows = Xc[hit] + THc[hit] * tau[hit, None]
    if tr.f is not None:  # smove_forward!(τ, t, x, θ, f, F) moves the free coordinates only (src/ss_not_fact.jl:78-86)
        f0 = np.ones(d, dtype=bool) if tr.f0 is None else np.asarray(tr.f0, dtype=bool)
        Fm = np.vstack([f0[None], np.asarray(tr.f, dtype=bool).reshape(-1, d)[:-1]])
        rows = np.where(Fm[hit], rows, Xc[hit])
    return (tc + tau)[hit], rows


def conditional_trace(tr, p, n):
    """collect(conditional_trace(Ξ, (p, n))) -- src/condition.jl: the points (t [m], X [m x d]) where the path crosses the hyperplane
    {x : ⟨x − p, n⟩ = 0}, in closed form and with at most one hit per linear piece (DESIGN.md "Conditional trace" states the contract; the
    reference moves the state to every hit and event and agrees to rounding, apart from crossings it emits twice).

    FactTrace (time-ordered: no refresh clock): a piece runs between two events of the coordinates S = supp n; from the cursors of S as of its
    start t_b, τ = Σ n_k (p_k − x_k(t_b)) / Σ n_k θ_k and s = t_b + τ; a hit iff τ > 0 and the next event of S, or else the last event of the
    trace, lies at or after s.  The row is every coordinate's line from its last event strictly before s.
    PDMPTrace: per event, from the state before it, τ = ⟨p − x, n⟩ / ⟨θ, n⟩; a hit iff τ > 0 and t + τ lies strictly before the event; frozen
    coordinates of a sticky trace stay where they are.  Sums run in the 64-lane order of the device.  Boomerang flows: TypeError (the
    reference's hittingtime has no method for them, src/condition.jl:18)."""
    if isinstance(tr.F, (Boomerang, FactBoomerang)):
        raise TypeError("conditional_trace: hittingtime has no method for the Boomerang flows (src/condition.jl:18)")
    d = len(tr.x0)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1)
    n = np.ascontiguousarray(n, dtype=np.float64).reshape(-1)
    if p.size != d or n.size != d:
        raise ValueError("conditional_trace: p and n have the trace's dimension %d" % d)
    if not (np.all(np.isfinite(p)) and np.all(np.isfinite(n)) and np.any(n != 0)):
        raise ValueError("conditional_trace: p and n are finite and n is not zero")
    if isinstance(tr, PDMPTrace):
        return _conditional_pdmp(tr, p, n)
    return _conditional_fact(tr, p, n)


def _pair_piece(a, b, vi, vj, tau):
    """∫_0^τ (a + vi·u)(b + vj·u) du in the one grouping of the contract (tests/ref/pairs_ref.c; symmetric in (i, j) bit for bit)."""
    return tau * (a * b + tau * (0.5 * (a * vj + b * vi) + tau * ((vi * vj) / 3.0)))


def _line_piece(a, vi, tau):
    return tau * (a + 0.5 * (vi * tau))


def _seq_sum(pieces):
    """0.0 + p_0 + p_1 + ... added one after the other, as an accumulator does (np.cumsum is that loop; the leading 0.0 matters for −0.0)."""
    return float(np.cumsum(np.concatenate([[0.0], pieces]))[-1])


def _pairs_fact(tr, pi, pj, c):
    ev = tr.events
    d = tr.x0.size
    order, ptr = _groups(tr)
    T_last = float(ev["t"][-1]) if len(ev) else float(tr.t0)
    own = [order[ptr[j]:ptr[j + 1]] for j in range(d)]

    def cursors(j, cnt):
        """t, x, θ of coordinate j after its first cnt[k] events (0: the initial state)"""
        if not len(own[j]):
            return np.full(len(cnt), float(tr.t0)), np.full(len(cnt), tr.x0[j]), np.full(len(cnt), tr.θ0[j])
        has = cnt > 0
        k = own[j][np.maximum(cnt - 1, 0)]
        return np.where(has, ev["t"][k], tr.t0), np.where(has, ev["x"][k], tr.x0[j]), np.where(has, ev["theta"][k], tr.θ0[j])

    S = np.empty(len(pi))
    for k, (i, j) in enumerate(zip(pi, pj)):
        idx = own[i] if i == j else np.sort(np.concatenate([own[i], own[j]]))  # the events of either coordinate, in trace order
        is_i = ev["i"][idx] == i
        ci_cnt = np.cumsum(is_i) - is_i  # events of i before each of them
        cj_cnt = ci_cnt if i == j else np.cumsum(~is_i) - (~is_i)
        # ... and once more behind the last, for the close at T_last
        ci_cnt = np.concatenate([ci_cnt, [len(own[i])]]).astype(np.int64)
        cj_cnt = np.concatenate([cj_cnt, [len(own[j])]]).astype(np.int64)
        t1 = np.concatenate([ev["t"][idx], [T_last]])
        ti, xi, thi = cursors(i, ci_cnt)
        tj, xj, thj = cursors(j, cj_cnt)
        s0 = np.where(ti > tj, ti, tj)
        a = (xi - c[i]) + thi * (s0 - ti)
        b = (xj - c[j]) + thj * (s0 - tj)
        S[k] = _seq_sum(_pair_piece(a, b, thi, thj, t1 - s0))
    J = np.empty(d)
    for j in range(d):
        cnt = np.arange(len(own[j]) + 1, dtype=np.int64)
        tc, xc, thc = cursors(j, cnt)
        t1 = np.concatenate([ev["t"][own[j]], [T_last]])
        J[j] = _seq_sum(_line_piece(xc - c[j], thc, t1 - tc))
    return S, J, T_last


def _pairs_pdmp(tr, pi, pj, c):
    d = len(tr.x0)
    t = np.asarray(tr.t, dtype=np.float64).reshape(-1)
    m = len(t)
    T_last = float(t[-1]) if m else float(tr.t0)
    tc = np.concatenate([[tr.t0], t[:-1]])[:m]
    Xc = np.vstack([np.asarray(tr.x0, dtype=np.float64)[None], np.asarray(tr.x, dtype=np.float64).reshape(-1, d)[:-1]])[:m]
    Vc = np.vstack([np.asarray(tr.θ0, dtype=np.float64)[None], np.asarray(tr.θ, dtype=np.float64).reshape(-1, d)[:-1]])[:m]
    if tr.f is not None:  # a coordinate that is not free keeps x
        f0 = np.ones(d, dtype=bool) if tr.f0 is None else np.asarray(tr.f0, dtype=bool)
        Fm = np.vstack([f0[None], np.asarray(tr.f, dtype=bool).reshape(-1, d)[:-1]])[:m]
        Vc = np.where(Fm, Vc, 0.0)
    tau = t - tc
    A = Xc - c[None]
    S = np.array([_seq_sum(_pair_piece(A[:, i], A[:, j], Vc[:, i], Vc[:, j], tau)) for i, j in zip(pi, pj)])
    J = np.array([_seq_sum(_line_piece(A[:, j], Vc[:, j], tau)) for j in range(d)])
    return S, J, T_last


def _pair_list(d, pi, pj, center):
    pi = np.ascontiguousarray(pi, dtype=np.int64).reshape(-1)
    pj = np.ascontiguousarray(pj, dtype=np.int64).reshape(-1)
    if pi.size != pj.size or pi.size < 1:
        raise ValueError("pair_integrals: pi and pj list at least one pair, one entry each")
    if pi.min() < 0 or pj.min() < 0 or pi.max() >= d or pj.max() >= d:
        raise ValueError("pair_integrals: a pair has an index outside [0, %d)" % d)
    key = np.minimum(pi, pj) * d + np.maximum(pi, pj)
    if len(np.unique(key)) != len(key):
        raise ValueError("pair_integrals: a pair is listed twice (either orientation counts)")
    c = np.zeros(d) if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(-1)
    if c.size != d or not np.all(np.isfinite(c)):
        raise ValueError("pair_integrals: the centre has the trace's dimension %d and is finite" % d)
    return pi, pj, c


def pair_integrals(tr, pi, pj, center=None):
    """(S [npairs], J [d], T_last): the exact path integrals S_k = ∫ (x_i − c_i)(x_j − c_j) dt of the pairs (i, j) = (pi[k], pj[k]) and
    J_i = ∫ (x_i − c_i) dt of every coordinate over [t0, T_last], T_last the trace's last event time -- the host mirror of the device's pair
    consumers (Ensemble.consume_pairs / bps_consume_pairs), bit for bit the sequential statement tests/ref/pairs_ref.c (DESIGN.md "Pair
    integrals").  A FactTrace (time-ordered: no refresh clock): the integrand of a pair is a product of two lines whose pieces end at the
    events of either coordinate; a PDMPTrace: every event ends a piece of every pair, frozen coordinates of a sticky trace stay where they
    are.  Boomerang flows: TypeError (the product of two rotations is another integral)."""
    if isinstance(tr.F, (Boomerang, FactBoomerang)):
        raise TypeError("pair_integrals: on a Boomerang flow the product of two rotations is another integral than that of two lines")
    pi, pj, c = _pair_list(len(tr.x0), pi, pj, center)
    if isinstance(tr, PDMPTrace):
        return _pairs_pdmp(tr, pi, pj, c)
    return _pairs_fact(tr, pi, pj, c)


_H = float.fromhex
_SIN_POLY = [_H(v) for v in ("-0x1.5555555555549p-3", "0x1.111111110f8a6p-7", "-0x1.a01a019c161d5p-13", "0x1.71de357b1fe7dp-19",
                             "-0x1.ae5e68a2b9cebp-26", "0x1.5d93a5acfd57cp-33")]
_COS_POLY = [_H(v) for v in ("0x1.555555555554cp-5", "-0x1.6c16c16c15177p-10", "0x1.a01a019cb1590p-16", "-0x1.27e4f809c52adp-22",
                             "0x1.1ee9ebdb4b1c4p-29", "-0x1.8fae9be8838d4p-37")]
_PIO2 = [_H(v) for v in ("0x1.921fb54400000p+0", "0x1.0b4611a600000p-34", "0x1.3198a2e000000p-69", "0x1.b839a252049c1p-104")]
_INVPIO2 = _H("0x1.45f306dc9c883p-1")


def _pdmp_sincos(x):
    """(sin x, cos x) as pdmp_sincos of include/pdmp_detmath.h computes them, bit for bit (every operation below is one correctly rounded
    double operation of that function, in its order): the Cody-Waite reduction by π/2 in three 33-bit pieces and a tail, then the two
    polynomial kernels.  NaN beyond |x| <= 2^30 and for a non-finite x.  Vectorised over x."""
    x = np.asarray(x, dtype=np.float64)
    ok = np.abs(x) <= 2.0 ** 30  # (False for NaN)
    xs = np.where(ok, x, 0.0)
    n = np.trunc(xs * _INVPIO2 + np.where(xs < 0, -0.5, 0.5)).astype(np.int64)
    nl = np.fmod(n, 0x100000)  # (the sign of n, as C's %)
    fn, fnh, fnl = n.astype(np.float64), (n - nl).astype(np.float64), nl.astype(np.float64)
    r = xs - fnh * _PIO2[0]
    r = r - fnl * _PIO2[0]
    r = r - fnh * _PIO2[1]
    r = r - fnl * _PIO2[1]
    r = r - fnh * _PIO2[2]
    r = r - fnl * _PIO2[2]
    r = r - fn * _PIO2[3]
    z = r * r
    S1, S2, S3, S4, S5, S6 = _SIN_POLY
    sr = r + (z * r) * (S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))))
    C1, C2, C3, C4, C5, C6 = _COS_POLY
    cr = (1.0 - 0.5 * z) + z * (z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6))))))
    q = n & 3
    s = np.select([q == 0, q == 1, q == 2], [sr, cr, -sr], -cr)
    c = np.select([q == 0, q == 1, q == 2], [cr, -sr, -cr], sr)
    return np.where(ok, s, np.nan), np.where(ok, c, np.nan)


def _seq_sum_columns(P):
    """_seq_sum of every column of P [m x k]"""
    return np.cumsum(np.vstack([np.zeros((1, P.shape[1])), P]), axis=0)[-1]


def arc_pair_integrals(tr, pi, pj, center=None):
    """(S [npairs], J [d], T_last) as pair_integrals, for the PDMPTrace of a Boomerang, sticky or not: between two events a free coordinate
    rotates about F.μ, x(s) − z = u·cos s + p·sin s + m with u = x_c − μ, p = θ_c, m = μ − z (a coordinate that is not free: u = p = 0,
    m = x_c − z), and a pair's piece is a combination of the integrals of cos², sin², sin·cos, cos and sin over the piece.  The host mirror of
    Ensemble.bps_consume_arc_pairs, bit for bit the sequential statement tests/ref/arc_pairs_ref.c (DESIGN.md "Pair integrals of arcs").  Any
    other trace: TypeError (pair_integrals takes the straight-line flows)."""
    if not (isinstance(tr, PDMPTrace) and isinstance(tr.F, Boomerang)):
        raise TypeError("arc_pair_integrals: the PDMPTrace of a Boomerang (pair_integrals takes the traces of the straight-line flows)")
    d = len(tr.x0)
    pi, pj, z = _pair_list(d, pi, pj, center)
    t = np.asarray(tr.t, dtype=np.float64).reshape(-1)
    m = len(t)
    T_last = float(t[-1]) if m else float(tr.t0)
    mu = np.asarray(tr.F.μ, dtype=np.float64).reshape(-1)
    tc = np.concatenate([[tr.t0], t[:-1]])[:m]
    Xc = np.vstack([np.asarray(tr.x0, dtype=np.float64)[None], np.asarray(tr.x, dtype=np.float64).reshape(-1, d)[:-1]])[:m]
    Pc = np.vstack([np.asarray(tr.θ0, dtype=np.float64)[None], np.asarray(tr.θ, dtype=np.float64).reshape(-1, d)[:-1]])[:m]
    U, M = Xc - mu[None], np.broadcast_to((mu - z)[None], Xc.shape)
    if tr.f is not None:  # a coordinate that is not free stays where it is
        f0 = np.ones(d, dtype=bool) if tr.f0 is None else np.asarray(tr.f0, dtype=bool)
        Fm = np.vstack([f0[None], np.asarray(tr.f, dtype=bool).reshape(-1, d)[:-1]])[:m]
        U, Pc, M = np.where(Fm, U, 0.0), np.where(Fm, Pc, 0.0), np.where(Fm, M, Xc - z[None])
    tau = t - tc
    s, c = _pdmp_sincos(tau)
    h = s * c
    Icc, Iss, Isc, Ic = 0.5 * (tau + h), 0.5 * (tau - h), 0.5 * (s * s), s
    with np.errstate(divide="ignore", invalid="ignore"):
        Is = np.where(c > 0, (s * s) / (1.0 + c), 1.0 - c)
    G = U * Ic[:, None] + Pc * Is[:, None]
    S = np.empty(len(pi))
    for k, (i, j) in enumerate(zip(pi, pj)):
        S[k] = _seq_sum((((U[:, i] * U[:, j]) * Icc + (Pc[:, i] * Pc[:, j]) * Iss) + (U[:, i] * Pc[:, j] + U[:, j] * Pc[:, i]) * Isc)
                        + ((M[:, i] * G[:, j] + M[:, j] * G[:, i]) + (M[:, i] * M[:, j]) * tau))
    J = _seq_sum_columns(G + M * tau[:, None])
    return S, J, T_last


def covariance(pi, pj, S, J, L, pooled=True, center=None):
    """(cov, mean) from pair integrals: cov a symmetric scipy.sparse matrix [d x d] with S_ij / L − (J_i / L)(J_j / L) at the listed pairs, mean
    = J / L + center.  S [n x npairs], J [n x d], L [n] (the run lengths T_last − t0) of n chains -- or one chain's S [npairs], J [d], L.
    pooled=True: one matrix from ΣS / ΣL − (ΣJ / ΣL)(ΣJ / ΣL)ᵀ (raw integrals pool exactly across chains and ranks); pooled=False: a list of
    n (cov, mean) pairs."""
    import scipy.sparse as sp
    pi = np.asarray(pi, dtype=np.int64).reshape(-1)
    pj = np.asarray(pj, dtype=np.int64).reshape(-1)
    S, J = np.atleast_2d(np.asarray(S, dtype=np.float64)), np.atleast_2d(np.asarray(J, dtype=np.float64))
    L = np.asarray(L, dtype=np.float64).reshape(-1)
    d = J.shape[1]
    c = np.zeros(d) if center is None else np.asarray(center, dtype=np.float64).reshape(-1)

    def one(s, j, l):
        m = j / l
        v = s / l - m[pi] * m[pj]
        off = pi != pj
        M = sp.coo_matrix((np.concatenate([v, v[off]]), (np.concatenate([pi, pj[off]]), np.concatenate([pj, pi[off]]))), shape=(d, d))
        return M.tocsr(), m + c

    if pooled:
        return one(S.sum(axis=0), J.sum(axis=0), L.sum())
    return [one(S[k], J[k], L[k]) for k in range(S.shape[0])]


def histogram_edges(lo, hi, bins):
    """[m x (bins + 1)]: the edges e_0 = lo, e_k = lo + w·k, e_bins = hi, w = (hi − lo) / bins, of the contract (tests/ref/hist_ref.c)."""
    lo = np.atleast_1d(np.asarray(lo, dtype=np.float64))
    hi = np.atleast_1d(np.asarray(hi, dtype=np.float64))
    w = (hi - lo) / float(bins)
    E = lo[:, None] + w[:, None] * np.arange(bins + 1, dtype=np.float64)[None]
    E[:, 0], E[:, bins] = lo, hi
    return E


def _hist_row(a, v, tau, E):
    """(H [B + 2], Z) of the pieces (a, v, tau) [n] of one coordinate, in their order; E [B + 1] its edges.  The contract's piece: tau <= 0
    adds nothing; at rest (v == 0 or a + v·tau == a) tau goes to the slot of a; otherwise every bin gets (min(xh, e_k+1) − max(xl, e_k))·r
    where that is positive, r = tau / (xh − xl).  Sums run sequentially over the pieces."""
    B = len(E) - 1
    keep = tau > 0.0
    a, v, tau = a[keep], v[keep], tau[keep]
    b = a + v * tau
    rest = (v == 0.0) | (b == a)
    Ex = np.concatenate([[-np.inf], E, [np.inf]])
    H = np.zeros(B + 2)
    for s in range(0, len(a), 4096):  # (pieces x bins at a time)
        sl = slice(s, s + 4096)
        xl, xh = np.minimum(a[sl], b[sl]), np.maximum(a[sl], b[sl])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = tau[sl] / (xh - xl)
            o = np.minimum(xh[:, None], Ex[None, 1:]) - np.maximum(xl[:, None], Ex[None, :-1])
            C = np.where(o > 0.0, o * r[:, None], 0.0)
        at = np.searchsorted(E, a[sl], side="right")  # slot of a: 0 below lo, B + 1 at or above hi (−0.0 compares as 0)
        C[rest[sl]] = 0.0
        C[np.flatnonzero(rest[sl]), at[rest[sl]]] = tau[sl][rest[sl]]
        H = np.cumsum(np.vstack([H[None], C]), axis=0)[-1]
    return H, _seq_sum(tau[v == 0.0])


def _hist_fact(tr, coords, E):
    ev = tr.events
    order, ptr = _groups(tr)
    T_last = float(ev["t"][-1]) if len(ev) else float(tr.t0)
    H, Z = np.empty((len(coords), E.shape[1] + 1)), np.empty(len(coords))
    for s, j in enumerate(coords):
        own = order[ptr[j]:ptr[j + 1]]
        tc = np.concatenate([[tr.t0], ev["t"][own]])
        xc = np.concatenate([[tr.x0[j]], ev["x"][own]])
        thc = np.concatenate([[tr.θ0[j]], ev["theta"][own]])
        t1 = np.concatenate([ev["t"][own], [T_last]])  # (the last piece: closed at T_last)
        H[s], Z[s] = _hist_row(xc, thc, t1 - tc, E[s])
    return H, Z, T_last


def _hist_pdmp(tr, coords, E):
    d = len(tr.x0)
    t = np.asarray(tr.t, dtype=np.float64).reshape(-1)
    m = len(t)
    T_last = float(t[-1]) if m else float(tr.t0)
    tc = np.concatenate([[tr.t0], t[:-1]])[:m]
    Xc = np.vstack([np.asarray(tr.x0, dtype=np.float64)[None], np.asarray(tr.x, dtype=np.float64).reshape(-1, d)[:-1]])[:m]
    Vc = np.vstack([np.asarray(tr.θ0, dtype=np.float64)[None], np.asarray(tr.θ, dtype=np.float64).reshape(-1, d)[:-1]])[:m]
    if tr.f is not None:  # a coordinate that is not free keeps x
        f0 = np.ones(d, dtype=bool) if tr.f0 is None else np.asarray(tr.f0, dtype=bool)
        Fm = np.vstack([f0[None], np.asarray(tr.f, dtype=bool).reshape(-1, d)[:-1]])[:m]
        Vc = np.where(Fm, Vc, 0.0)
    H, Z = np.empty((len(coords), E.shape[1] + 1)), np.empty(len(coords))
    for s, j in enumerate(coords):
        H[s], Z[s] = _hist_row(Xc[:, j], Vc[:, j], t - tc, E[s])
    return H, Z, T_last


def marginal_histogram(tr, coords, lo, hi, bins):
    """(H [m x (bins + 2)], Z [m], T_last): the exact time each listed coordinate of the path spends in each of `bins` bins of its own range
    [lo, hi) (scalars broadcast; coords None: all), with slot 0 the time below lo and slot bins + 1 the time at or above hi; Z the time it
    rested (velocity 0) -- the host mirror of the device's histogram consumers (Ensemble.consume_hist / bps_consume_hist), the contract of
    tests/ref/hist_ref.c in numpy (DESIGN.md "Marginal histograms").  A FactTrace (time-ordered: no refresh clock): a coordinate moves on a
    line between ITS events, the last piece is closed at the trace's last event time T_last; a PDMPTrace: every coordinate moves on a line
    between consecutive events, frozen coordinates of a sticky trace stay where they are, nothing behind the last event.  Σ_k H[s, k] =
    T_last − t0 to rounding.  Boomerang flows: TypeError (an arc is not a line)."""
    if isinstance(tr.F, (Boomerang, FactBoomerang)):
        raise TypeError("marginal_histogram: on a Boomerang flow a coordinate moves on an arc between two events, not on a line")
    d = len(tr.x0)
    coords = np.arange(d, dtype=np.int64) if coords is None else np.ascontiguousarray(coords, dtype=np.int64).reshape(-1)
    bins = int(bins)
    if coords.size < 1 or coords.min() < 0 or coords.max() >= d or len(np.unique(coords)) != coords.size:
        raise ValueError("marginal_histogram: coords lists at least one coordinate of [0, %d), each once" % d)
    if not 1 <= bins <= 4096:
        raise ValueError("marginal_histogram: bins is in 1..4096")
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), coords.shape)
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), coords.shape)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)):
        raise ValueError("marginal_histogram: the ranges are finite with lo < hi")
    E = histogram_edges(lo, hi, bins)
    if isinstance(tr, PDMPTrace):
        return _hist_pdmp(tr, coords, E)
    return _hist_fact(tr, coords, E)


_TWO_PI = 6.28318530717958623200e+00  # 2π as the one double constant of the contract


def _arc_hist_row(xc, thc, free, mu, tau, E):
    """(H [B + 2], Z) of the pieces (x_c, θ_c, free, tau) [n] of one coordinate of a Boomerang about mu, in their order; E [B + 1] its edges.
    The contract's piece (tests/ref/arc_hist_ref.c) with numpy's arctan2 and arccos in the place of pdmp_atan2 and pdmp_acos."""
    B = len(E) - 1
    keep = tau > 0.0
    xc, thc, free, tau = xc[keep], thc[keep], free[keep], tau[keep]
    u = xc - mu
    R = np.where(free, np.sqrt(u * u + thc * thc), 0.0)
    rest = R == 0.0
    Ex = np.concatenate([[-np.inf], E, [np.inf]])
    H = np.zeros(B + 2)
    for s in range(0, len(xc), 1024):  # (pieces x edges at a time)
        sl = slice(s, s + 1024)
        Rs, ts = np.where(rest[sl], 1.0, R[sl])[:, None], tau[sl][:, None]
        psi0 = -np.arctan2(thc[sl], u[sl])[:, None]
        psi1 = psi0 + ts
        n0, n1 = np.floor(psi0 / _TWO_PI), np.floor(psi1 / _TWO_PI)
        r0, r1 = psi0 - _TWO_PI * n0, psi1 - _TWO_PI * n1
        z = (Ex[None] - mu) / Rs
        alpha = np.arccos(np.clip(z, -1.0, 1.0))
        L = _TWO_PI - 2.0 * alpha
        below = (n1 * L + np.clip(r1 - alpha, 0.0, L)) - (n0 * L + np.clip(r0 - alpha, 0.0, L))
        below = np.where(z >= 1.0, ts, np.where(z <= -1.0, 0.0, below))
        C = np.maximum(below[:, 1:] - below[:, :-1], 0.0)
        at = np.searchsorted(E, xc[sl], side="right")  # slot of x_c: 0 below lo, B + 1 at or above hi
        C[rest[sl]] = 0.0
        C[np.flatnonzero(rest[sl]), at[rest[sl]]] = tau[sl][rest[sl]]
        H = np.cumsum(np.vstack([H[None], C]), axis=0)[-1]
    return H, _seq_sum(tau[rest])


def arc_marginal_histogram(tr, coords, lo, hi, bins):
    """(H [m x (bins + 2)], Z [m], T_last) as marginal_histogram, for the PDMPTrace of a Boomerang, sticky or not: between two events a free
    coordinate is the arc x(s) = μ + u·cos s + p·sin s about F.μ (u = x_c − μ, p = θ_c), and the time it spends below a level is a closed form
    in acos and atan2, so the histogram is exact as it is for lines; a coordinate that is not free, or with u = p = 0, rests (Z counts both).
    The host mirror of Ensemble.bps_consume_arc_hist: the contract of tests/ref/arc_hist_ref.c in numpy, with numpy's arctan2 and arccos, so
    it agrees with the device to rounding, not bit for bit (DESIGN.md "Marginal histograms of arcs").  Σ_k H[s, k] = T_last − t0 to rounding.
    Any other trace: TypeError (marginal_histogram takes the straight-line flows)."""
    if not (isinstance(tr, PDMPTrace) and isinstance(tr.F, Boomerang)):
        raise TypeError("arc_marginal_histogram: the PDMPTrace of a Boomerang (marginal_histogram takes the traces of the straight-line flows)")
    d = len(tr.x0)
    coords = np.arange(d, dtype=np.int64) if coords is None else np.ascontiguousarray(coords, dtype=np.int64).reshape(-1)
    bins = int(bins)
    if coords.size < 1 or coords.min() < 0 or coords.max() >= d or len(np.unique(coords)) != coords.size:
        raise ValueError("arc_marginal_histogram: coords lists at least one coordinate of [0, %d), each once" % d)
    if not 1 <= bins <= 4096:
        raise ValueError("arc_marginal_histogram: bins is in 1..4096")
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), coords.shape)
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), coords.shape)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)):
        raise ValueError("arc_marginal_histogram: the ranges are finite with lo < hi")
    E = histogram_edges(lo, hi, bins)
    t = np.asarray(tr.t, dtype=np.float64).reshape(-1)
    m = len(t)
    T_last = float(t[-1]) if m else float(tr.t0)
    mu = np.broadcast_to(np.asarray(tr.F.μ, dtype=np.float64).reshape(-1), (d,))
    tc = np.concatenate([[tr.t0], t[:-1]])[:m]
    Xc = np.vstack([np.asarray(tr.x0, dtype=np.float64)[None], np.asarray(tr.x, dtype=np.float64).reshape(-1, d)[:-1]])[:m]
    Pc = np.vstack([np.asarray(tr.θ0, dtype=np.float64)[None], np.asarray(tr.θ, dtype=np.float64).reshape(-1, d)[:-1]])[:m]
    Fm = np.ones((m, d), dtype=bool)
    if tr.f is not None:  # a coordinate that is not free stays where it is
        f0 = np.ones(d, dtype=bool) if tr.f0 is None else np.asarray(tr.f0, dtype=bool)
        Fm = np.vstack([f0[None], np.asarray(tr.f, dtype=bool).reshape(-1, d)[:-1]])[:m]
    H, Z = np.empty((len(coords), bins + 2)), np.empty(len(coords))
    for s, j in enumerate(coords):
        H[s], Z[s] = _arc_hist_row(Xc[:, j], Pc[:, j], Fm[:, j], mu[j], t - tc, E[s])
    return H, Z, T_last


def histogram_quantiles(H, lo, hi, q):
    """Quantiles of marginal histograms: H [.. x m x (B + 2)] rows as marginal_histogram / Ensemble.consume_histogram return them (per chain or
    pooled), lo / hi [m] or scalars, q a probability or a list of them.  Returns [.. x m x len(q)] (the last axis dropped for a scalar q): the
    piecewise-linear CDF of the bins -- the mass of a bin spread evenly over it, the outer slots counted but not resolved -- inverted at
    q·Σ_k H[k].  nan where the requested mass lies in an outer slot (below lo or at or above hi: widen the range), or in a row without mass."""
    H = np.asarray(H, dtype=np.float64)
    B = H.shape[-1] - 2
    scalar = np.ndim(q) == 0
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    rows = H.reshape(-1, B + 2)
    m = H.shape[-2] if H.ndim > 1 else 1
    E = histogram_edges(np.broadcast_to(np.asarray(lo, dtype=np.float64), (m,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (m,)), B)
    out = np.full((rows.shape[0], qs.size), np.nan)
    for r, row in enumerate(rows):
        e = E[r % m]
        cdf = np.concatenate([[0.0], np.cumsum(row)])  # cdf[k + 1]: the mass below e_k, k = 0 .. B; cdf[B + 2]: all of it
        total = cdf[-1]
        if not total > 0.0:
            continue
        inner = cdf[1:B + 2]  # the CDF at the edges e_0 .. e_B
        if not inner[-1] > inner[0]:
            continue
        for c, p in enumerate(qs):
            mass = p * total
            if inner[0] <= mass <= inner[-1]:  # the smallest x with CDF(x) >= mass: in the bin k − 1 with inner[k − 1] < mass <= inner[k]
                k = int(np.searchsorted(inner, mass, side="left"))
                out[r, c] = e[0] if k == 0 else e[k - 1] + (e[k] - e[k - 1]) * ((mass - inner[k - 1]) / (inner[k] - inner[k - 1]))
    out = out.reshape(H.shape[:-1] + (qs.size,))
    return out[..., 0] if scalar else out


def faber_schauder_path(ξ, s, L, T):
    """dotψ(ξ, s, L, T) of research/diffusion_bridge/faberschauder.jl:16-24, vectorised: the bridge X_s of the Faber-Schauder coefficients ξ
    ([d] or [n x d], d = (2 << L) + 1, e.g. the rows of discretize(Ξ, dt)) at the times s (scalar or [m], 0 <= s < T).  Returns [m], or
    [n x m] for a stack of coefficient vectors."""
    ξ = np.asarray(ξ, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    L = int(L)
    if ξ.shape[-1] != (2 << L) + 1:
        raise ValueError("ξ has %d coefficients, level L = %d has %d" % (ξ.shape[-1], L, (2 << L) + 1))
    sv = np.atleast_1d(s)
    if np.any(sv < 0) or np.any(sv >= T):
        raise ValueError("out of bounds")  # faberschauder.jl:17
    X = np.atleast_2d(ξ)
    sT = np.sqrt(T)
    r = (sv / sT)[None, :] * X[:, -1:] + (sT * (1 - sv / T))[None, :] * X[:, :1]
    for lev in range(L + 1):
        p2 = float(1 << (L - lev))
        j = np.floor(sv / T * p2).astype(np.int64) * (2 << lev) + (1 << lev)
        lam = (sT * 0.5 - np.abs(np.fmod(sv * p2, T) / sT - sT * 0.5)) / np.sqrt(p2)  # Λ(s, L − lev, T), :3-6
        r = r + X[:, j] * lam[None, :]
    if ξ.ndim == 1:
        return r[0] if s.ndim else r[0, 0]
    return r if s.ndim else r[:, 0]


def lower_index(n):
    """(rows, cols) of the packed lower triangle of an n x n matrix, column by column: 𝕀 of casestudies/precision/precision.jl:39 (0-based).
    Coordinate i = c n − c (c − 1)/2 + (r − c) is entry (rows[i], cols[i]); d = n (n + 1)/2."""
    n = int(n)
    cols, rows = np.triu_indices(n)  # row-major upper triangle of the transpose == column-major lower triangle
    return rows.astype(np.int64), cols.astype(np.int64)


def pack_lower(L):
    """transform(L, 𝕀) = L[𝕀] (precision.jl:18): the lower triangle of L ([n x n], or a stack [... x n x n]) as the coordinate vector u."""
    L = np.asarray(L, dtype=np.float64)
    r, c = lower_index(L.shape[-1])
    return L[..., r, c]


def unpack_lower(u, n=None):
    """backform(u, 𝕀) (precision.jl:11-17): the lower-triangular matrix of the coordinate vector u ([d], or a stack [... x d])."""
    u = np.asarray(u, dtype=np.float64)
    d = u.shape[-1]
    if n is None:
        n = int(round((np.sqrt(8 * d + 1) - 1) / 2))
    if n * (n + 1) // 2 != d:
        raise ValueError("u has %d coordinates: not n (n + 1)/2 for n = %d" % (d, n))
    r, c = lower_index(n)
    L = np.zeros(u.shape[:-1] + (n, n))
    L[..., r, c] = u
    return L
