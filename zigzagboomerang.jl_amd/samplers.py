"""Host-side mirror of the reference's sampler entry points for the device-resident hot path.

    spdmp(∇ϕ, t0, x0, θ0, T, c, F::ZigZag, args...; factor=1.8, adapt=false, seed) = Ξ, (t, x, θ), (acc, num), c
                                                                        (src/sfact.jl:162-163,211,214)

Differences forced by the C ABI: `∇ϕ, args...` is replaced by an enumerated `target` (GaussianTarget);
coordinates are 0-based; x0/θ0 may be [nchains, d] to run an ensemble (outputs then carry a leading chain
axis).  Everything else -- argument order, keyword names, the 4-tuple returned, the error raised when the
bound `c` is too small with adapt=false -- follows the reference.
"""
import copy

import numpy as np
import scipy.sparse as sp

from . import _lib
from .engine import Ensemble
from .flows import (Boomerang, Boomerang1d, BouncyParticle, DiffusionBridgeTarget, ExtendedForm, FactBoomerang, LocalBound, FactTrace, GaussianTarget,
                    GaussianTarget1d, LogisticRegressionTarget, LogisticTarget, PDMPTrace, PrecisionCholeskyTarget, StickyBarriers, ZigZag, ZigZag1d)

DEFAULT_SEED = 0x5EED0000


def _drain(ens, events):
    cnt = ens.counters()
    for k in range(ens.nchains):
        n = int(cnt["ntrace"][k])
        if n:
            events[k].append(ens.trace(k, 0, n, counters=cnt))
    ens.trace_reset()


def _consume_capacity(consume, trace, trace_capacity):
    """The trace capacity of a Bouncy Particle run: with consume=... the events are written to the device buffer even where trace=False."""
    if consume is None:
        return trace_capacity if trace else 0
    if not isinstance(consume, dict) or set(consume) - {"dt", "points", "condition", "hits", "cov", "center", "hist"}:
        raise TypeError("consume=dict(dt=..., points=...[, condition=(p, n), hits=K][, cov=P, center=c][, hist=dict(coords=..., lo=..., hi=..., bins=B)])")
    if trace_capacity <= 0:
        raise ValueError("consume=... reads the device trace buffer: trace_capacity must be positive")
    return trace_capacity


def _condition_of(consume):
    """(p, n, K) of consume=dict(..., condition=(p, n), hits=K) -- the conditional trace on the device, K rows reserved per chain -- or None."""
    if consume is None or "condition" not in consume:
        if consume is not None and "hits" in consume:
            raise TypeError("consume=dict(hits=K) goes with condition=(p, n)")
        return None
    p, n = consume["condition"]
    hits = int(consume.get("hits", 0))
    if hits < 1:
        raise ValueError("consume=dict(condition=(p, n), hits=K) reserves K >= 1 rows per chain")
    return p, n, hits


def _pairs_of(consume, d):
    """(pi, pj, center) of consume=dict(..., cov=P[, center=c]) -- the pair integrals on the device -- or None.  P: a sparse matrix (its
    structural lower triangle plus the whole diagonal), "diag", or a (pi, pj) tuple of 0-based index lists."""
    if consume is None or "cov" not in consume:
        if consume is not None and "center" in consume:
            raise TypeError("consume=dict(center=c) goes with cov=P")
        return None
    P = consume["cov"]
    if isinstance(P, str):
        if P != "diag":
            raise ValueError('consume=dict(cov=P): P is a sparse matrix, "diag" or a (pi, pj) tuple')
        pi = pj = np.arange(d, dtype=np.int64)
    elif isinstance(P, tuple):
        pi, pj = (np.asarray(v, dtype=np.int64).reshape(-1) for v in P)
    else:
        import scipy.sparse as sp
        A = sp.coo_matrix(P)
        if A.shape != (d, d):
            raise ValueError("consume=dict(cov=P): P is %d x %d" % (d, d))
        low = A.row > A.col
        key = np.unique(A.row[low].astype(np.int64) * d + A.col[low])  # (row-major, duplicates of an unsummed COO matrix once)
        pi = np.concatenate([np.arange(d, dtype=np.int64), key // d])
        pj = np.concatenate([np.arange(d, dtype=np.int64), key % d])
    return pi, pj, consume.get("center")


def _hist_of(consume, d):
    """(coords, lo, hi, bins) of consume=dict(..., hist=dict(coords=..., lo=..., hi=..., bins=B)) -- the marginal histograms on the device -- or
    None.  coords=None: all of d; scalars for lo / hi broadcast over the listed coordinates."""
    if consume is None or "hist" not in consume:
        return None
    h = consume["hist"]
    if not isinstance(h, dict) or set(h) - {"coords", "lo", "hi", "bins"} or not {"lo", "hi", "bins"} <= set(h):
        raise TypeError("consume=dict(hist=dict(coords=..., lo=..., hi=..., bins=B))")
    coords = np.arange(d, dtype=np.int64) if h.get("coords") is None else np.asarray(h["coords"], dtype=np.int64).reshape(-1)
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(h["lo"], dtype=np.float64), coords.shape))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(h["hi"], dtype=np.float64), coords.shape))
    return coords, lo, hi, int(h["bins"])


def _admits(consume):
    """a consume= whose keys alone admit it on every target: cov=P or hist=dict(...)"""
    return isinstance(consume, dict) and ("cov" in consume or "hist" in consume)


def _hist_result(out, hist, histogram, single):
    """hist_coords [m], hist_edges [m x (B + 1)], hist_H [nchains x m x (B + 2)], hist_Z [nchains x m]: with out["T"] what
    trace.histogram_quantiles takes"""
    from .trace import histogram_edges
    coords, lo, hi, bins = hist
    out["hist_coords"], out["hist_edges"] = coords, histogram_edges(lo, hi, bins)
    out["hist_H"], out["hist_Z"], _ = histogram()
    if single:
        out["hist_H"], out["hist_Z"] = out["hist_H"][0], out["hist_Z"][0]


def _pairs_result(out, pairs, integrals):
    """pairs = (pi, pj), pair_S [nchains x npairs], pair_J [nchains x d]: with out["T"] what trace.covariance takes"""
    out["pairs"] = (pairs[0], pairs[1])
    out["pair_S"], out["pair_J"], _ = integrals()


def _condition_result(out, conditioned, nchains):
    """hit_t, hit_x (per chain: a chain has its own number of hits) and nhits [nchains] -- a value above hits=K: later hits were dropped"""
    res = [conditioned(k) for k in range(nchains)]
    out["hit_t"], out["hit_x"] = [r[0] for r in res], [r[1] for r in res]
    out["nhits"] = np.array([r[2] for r in res], dtype=np.int64)


def _consume_result(ens, consume, single, sticky):
    """The extra element of a consume=... run: dict(mean, T, grid_t, grid_x[, inclusion][, hit_t, hit_x, nhits]) from the device consumers;
    grid_t / grid_x (and hit_t / hit_x) are per chain (a chain's grid ends before ITS last event), None without points."""
    mean, T = ens.bps_consume_mean()
    out = dict(mean=mean, T=T, grid_t=None, grid_x=None)
    if sticky:
        out["inclusion"] = ens.bps_consume_inclusion()[0]
    if _condition_of(consume) is not None:
        _condition_result(out, ens.bps_consume_conditioned, ens.nchains)
    pairs = _pairs_of(consume, ens.d)
    if int(consume.get("points", 0)) > 0:
        grids = [ens.bps_consume_discretized(k) for k in range(ens.nchains)]
        out["grid_t"], out["grid_x"] = [g[0] for g in grids], [g[1] for g in grids]
    if single:
        out = {k: (v if v is None else v[0]) for k, v in out.items()}
    if pairs is not None:
        _pairs_result(out, pairs, ens.bps_consume_pair_integrals)
        if single:
            out["pair_S"], out["pair_J"] = out["pair_S"][0], out["pair_J"][0]
    if _hist_of(consume, ens.d) is not None:
        _hist_result(out, _hist_of(consume, ens.d), ens.bps_consume_histogram, single)
    return out


def _split_G(GF, G):
    """spdmp(∇ϕ, t0, x0, θ0, T, c, F) or spdmp(∇ϕ, t0, x0, θ0, T, c, G, F) as in the reference (src/sfact.jl:162,214); G may also be a keyword."""
    if GF and isinstance(GF[-1], ExtendedForm):  # SelfMoving() as args[1] (src/sfact.jl:57-68): the device targets that need it carry it in their type
        GF = GF[:-1]
    if len(GF) == 1:
        return G, GF[0]
    if len(GF) == 2 and G is None:
        return GF[0], GF[1]
    raise TypeError("expected spdmp(target, t0, x0, θ0, T, c, [G,] F[, SelfMoving()], ...)")


def spdmp(target, t0, x0, θ0, T, c, *GF, factor=1.8, adapt=False, adaptscale=False, seed=DEFAULT_SEED, device=0,
          trace_capacity=None, trace=True, tracked=False, G=None, consume=None):
    """Local ZigZag: spdmp(∇ϕ, t0, x0, θ0, T, c, [G,] F::ZigZag, args...) (src/sfact.jl:162,214); without G: G = Matched().
    Returns Ξ, (t, x, θ), (acc, num), c like the reference (:211).

    A trailing SelfMoving() / ExtendedForm() is accepted as in spdmp(∇ϕmoving, ..., F, SelfMoving(), args...) (:68).  With a
    DiffusionBridgeTarget this is research/diffusion_bridge/diffbridge.jl:32-33: spdmp(target, 0.0, ξ0, θ0, T′, c, ZigZag(I, 0), SelfMoving(),
    adapt=True) with ξ0, θ0, c of problems.diffusion_bridge_problem.

    consume=dict(dt=..., points=...) (DiffusionBridgeTarget; engine-only keyword): the device consumers (pdmp_ensemble_consume_*) run over
    every slice before its buffer is recycled and a fifth element is returned: dict(mean, T, grid_t, grid_x) -- trace.mean(Ξ), the last
    event time and trace.discretize(Ξ, dt) on at most `points` rows (grid_t / grid_x None without points), per chain as in pdmp.  With
    condition=(p, n), hits=K in the dict it also holds hit_t, hit_x, nhits: trace.conditional_trace(Ξ, p, n), at most K rows per chain
    (problems.bridge_point_condition gives the (p, n) of a bridge through a point).
    consume=dict(dt=..., points=...) is also admitted where the flow has a refresh clock -- a ZigZag with λref > 0 or a FactBoomerang, on any device
    target: the unordered device consumers (Ensemble.refresh_consume_begin) then run over every slice and the same dict(mean, T, grid_t, grid_x) is
    returned; with trace=False the events are consumed without being copied.  cov, hist and condition in the dict raise TypeError on such a flow.
    consume=dict(cov=P[, center=c]) (any device target with a ZigZag without refresh clock; also on sspdmp and pdmp): the exact pair integrals of the path, kept on the
    device slice by slice -- P a sparse matrix (its structural lower triangle plus the diagonal), "diag" or a (pi, pj) tuple; the element gains
    pairs = (pi, pj), pair_S [npairs] and pair_J [d] per chain, which with T (L = T − t0) is what trace.covariance takes.
    consume=dict(hist=dict(coords=None, lo=..., hi=..., bins=B)) (any device target with a ZigZag; also on sspdmp, pdmp, stickyzz and sspdmp2): the
    exact marginal histograms of the path -- the time each listed coordinate (None: all) spends in each of B bins of [lo, hi) (scalars broadcast),
    below and above -- kept on the device slice by slice; the element gains hist_coords [m], hist_edges [m x (B + 1)], hist_H [m x (B + 2)] and
    hist_Z [m] (the time at rest) per chain: trace.histogram_quantiles(hist_H, lo, hi, q) gives medians and credible intervals.

    G: the neighbourhoods a proposal moves before its gradient is taken (:82,171-179) -- a sparse matrix whose column patterns are the
    G[i] (e.g. the target's Γ when the bounding F.Γ is sparser) or a sequence of index arrays; G[i] ⊇ G1[i] = pattern of F.Γ[:, i] is
    asserted as in the reference (:177).

    adaptscale=True (src/sfact.jl:86-99) tunes σ in the refresh branch.  Like the reference, a single-chain call mutates
    F.σ in place; for an ensemble every chain's tuned σ is the `σ` of the flow attached to its trace (Ξ[k].F.σ).

    tracked=True (engine-only keyword): the tracked-gradient evaluation of the same process (pdmp_ensemble_set_gradient_tracking) -- the
    engine's fast path (what bench.py's headline times: 2.5 x the rate of the default on C3).  It is NOT the reference's arithmetic: the sums
    Γ[:,i]·x and Γ[:,i]·θ are carried along instead of gathered, so event times and positions agree with the default to ~1e-13 (tested to 1e-9),
    and indices, outcomes and counters are identical until such a difference flips a thinning test or the order of two almost simultaneous
    events: measured 3 of 4096 chains by T = 20 on the 128 x 128 lattice (6e-10 per proposal; tests/test_gpu_track_horizon.py).  A chain that
    has left is still a realisation of the same process, and the tracked arithmetic itself is pinned bit for bit by the oracle's
    spdmp_zigzag_tracked.  The default (False) follows the reference's evaluation order bit for bit; PdmpError(UNSUPPORTED) where no tracked
    kernel serves the graph / options."""
    G, F = _split_G(GF, G)
    return _zigzag(_lib.SAMPLER_ZIGZAG_LOCAL, target, t0, x0, θ0, T, c, F, factor, adapt, seed, device, trace_capacity, trace,
                   adaptscale=adaptscale, tracked=tracked, G=G, consume=consume)


def pdmp(target, *args, factor=1.8, adapt=False, subsample=None, seed=DEFAULT_SEED, device=0, trace_capacity=None, trace=True,
         moments=False, oscn=False, consume=None):
    """pdmp(∇ϕ, t0, x0, θ0, T, c, F, ...) -- the d-dimensional drivers, see _pdmp_nd -- or, with a 1-d flow as the sixth argument,
    pdmp(∇ϕ, x, θ, T, c, Flow::Union{ZigZag1d, Boomerang1d}; adapt=false, factor=2.0) -> Ξ, acc/num  (src/zigzagboom1d.jl:34-67)."""
    if len(args) == 5 and isinstance(args[4], (ZigZag1d, Boomerang1d)):
        if subsample or moments or oscn or consume is not None:
            raise TypeError("subsample, moments and consume are keywords of the non-factorised pdmp (BouncyParticle / Boomerang)")
        x0, θ0, T, c, Flow = args
        return _pdmp_1d(target, x0, θ0, T, c, Flow, 2.0 if factor == 1.8 else factor, adapt, seed, device, trace_capacity)
    if len(args) != 6:
        raise TypeError("expected pdmp(target, t0, x0, θ0, T, c, F, ...) or pdmp(target, x, θ, T, c, Flow1d, ...)")
    return _pdmp_nd(target, *args, factor=factor, adapt=adapt, subsample=subsample, seed=seed, device=device, trace_capacity=trace_capacity,
                    trace=trace, moments=moments, oscn=oscn, consume=consume)


def _pdmp_1d(target, x0, θ0, T, c, Flow, factor, adapt, seed, device, trace_capacity):
    """The 1-d samplers as an ensemble (one chain per lane, pdmp_1d_run): scalars run one chain and return (Ξ, acc/num) like the reference
    (:66), arrays of starting points run len(x0) chains (seeds seed + k) and return lists.  Ξ: structured array of (t, x, theta), the first
    entry being (0, x0, θ0) (:36).  c may be a scalar or one value per chain."""
    import ctypes as C
    if not isinstance(target, GaussianTarget1d):
        raise TypeError("the 1-d samplers take a GaussianTarget1d (∇ϕ(x) = (x − μ)/σ² + noise (rand() − 0.5), test/test1d.jl:9-10)")
    scalar = np.ndim(x0) == 0
    x0 = np.atleast_1d(np.asarray(x0, dtype=np.float64))
    n = len(x0)
    θ0 = np.broadcast_to(np.asarray(θ0, dtype=np.float64), (n,))
    cc = np.broadcast_to(np.asarray(c, dtype=np.float64), (n,))
    cap = int(trace_capacity) if trace_capacity else int(max(1024, min(1 << 20, 4 * max(float(T), 1.0))))
    boom = isinstance(Flow, Boomerang1d)
    cfg = _lib.Config1d(C.sizeof(_lib.Config1d), int(device), 1 if boom else 0, int(bool(adapt)), float(factor), n, cap, float(target.μ),
                        float(target.σ2), float(target.noise), Flow.Σ if boom else 1.0, Flow.μ if boom else 0.0, Flow.λref if boom else 1.0)
    st = np.zeros(n, dtype=_lib.STATE1D_DTYPE)
    st["x"], st["theta"], st["c"] = x0, θ0, cc
    seeds = np.uint64(seed) + np.arange(n, dtype=np.uint64)
    ev = np.empty((n, cap), dtype=_lib.EVENT1D_DTYPE)
    nev = np.zeros(n, dtype=np.int64)
    L = _lib.load()
    parts = [[] for _ in range(n)]
    while True:
        _lib.check(L.pdmp_1d_run(C.byref(cfg), st.ctypes.data, seeds.ctypes.data, float(T), ev.ctypes.data, nev.ctypes.data))
        for k in range(n):
            if nev[k]:
                parts[k].append(ev[k, :nev[k]].copy())
        if np.any(st["status"] == _lib.CHAIN_BOUND_VIOLATED):
            raise RuntimeError("Tuning parameter `c` too small.")  # :55
        if not _lib.needs_rerun(st["status"]):
            break
    Ξ = [np.concatenate(p) for p in parts]
    ratio = st["acc"] / np.maximum(st["num"], 1)
    return (Ξ[0], float(ratio[0])) if scalar else (Ξ, ratio)


def _pdmp_nd(target, t0, x0, θ0, T, c, F, *, factor=1.8, adapt=False, subsample=None, seed=DEFAULT_SEED, device=0,
             trace_capacity=None, trace=True, moments=False, oscn=False, consume=None):
    """pdmp(∇ϕ, t0, x0, θ0, T, c, F::ZigZag, args...) = spdmp(..., All(), ...) (src/sfact.jl:236): every proposal moves
    ALL coordinates (no sparsity assumption on ∇ϕ); same return value as spdmp.

    pdmp(∇ϕ!, t0, x0, θ0, T, c, B::BouncyParticle; adapt, factor=2.0) (src/not_fact_samplers.jl:117,395-396) when F is a
    BouncyParticle: the target is ∇ϕ!(y, x) = B.Γ(x − B.μ) (pass target=None) or a GaussianTarget of its own -- ab(…GlobalBound…) then
    keeps the flow's B.Γ, B.μ while gradient, rate and reflection use the target's (src/not_fact_samplers.jl:26-28,122) --, c is the scalar of GlobalBound(c) or a
    LocalBound(c) (src/not_fact_samplers.jl:29-31; the second derivative v = θ'Γθ is the Gaussian target's own);
    `subsample` as in the reference (:53,90); returns Ξ::PDMPTrace, (t, x, θ), (acc, num), c.

    moments=True (BouncyParticle / Boomerang, engine-only keyword): a fifth element dict(mean, var, T) -- the exact time averages
    ∫x dt/(T − t0) and ∫x² dt/(T − t0) − mean² over [t0, T] kept by the event loop (pdmp_ensemble_set_bps_moments), [n x d] or [d]; the
    first four elements are bit for bit those of moments=False.  With trace=False no event is written at all.

    consume=dict(dt=..., points=...) (BouncyParticle / Boomerang, the speed-recorded form included; engine-only keyword): the device consumers
    (pdmp_ensemble_bps_consume_*) run over every slice before its buffer is recycled, and one more element is returned: dict(mean, T, grid_t,
    grid_x) -- trace.mean(Ξ), the last event time, and trace.discretize(Ξ, dt) on a grid of at most `points` rows (ValueError if the run
    passes it; grid_t / grid_x are None without points), [n x ...] or squeezed for a single chain, the grids one array per chain.  The
    earlier elements are bit for bit those without the keyword.  With trace=False the events are still written to the device buffer and
    consumed, but never copied to the host; trace_capacity=0 raises.  With condition=(p, n), hits=K in the dict (event-recorded
    BouncyParticle and its sticky form) the element also holds hit_t, hit_x -- trace.conditional_trace(Ξ, p, n), at most K rows per chain --
    and nhits, the number of hits found (above K: the later ones were dropped).  With cov=P[, center=c] it holds pairs, pair_S and pair_J,
    what trace.covariance takes: of lines on a BouncyParticle (trace.pair_integrals), of arcs about μ on a Boomerang
    (trace.arc_pair_integrals), sticky forms included.

    pdmp(dϕ, ∇ϕ!, t0, x0, θ0, T, c::LocalBound, B::BouncyParticle; oscn=false, adapt=false, factor=2.0) (src/not_fact_samplers.jl:336-384),
    the speed-recorded driver: B.Γ is None (BouncyParticle(None, None, λref, ρ, L=..., U=...)), target is a GaussianTarget or a
    LogisticRegressionTarget (dϕ and ∇ϕ! are its two directional derivatives and its gradient), c a LocalBound.  An integer T is a number of
    samples, a float an end time.  The trace holds one record per 1/λref of speed-time and does not begin with (t0, x0, θ0); subsample defaults to True here and
    subsample=False raises the reference's ArgumentError (:338)."""
    if isinstance(F, BouncyParticle) and F.Γ is None:
        if not isinstance(target, (GaussianTarget, LogisticRegressionTarget)):
            raise TypeError("BouncyParticle(missing, missing, ...): target must be a GaussianTarget (dϕ, ∇ϕ! of Γt(x − μt)) or a "
                            "LogisticRegressionTarget")
        if not isinstance(c, LocalBound):
            raise TypeError("pdmp(dϕ, ∇ϕ!, ..., c::LocalBound, flow::BouncyParticle): pass c as LocalBound(c)")
        if subsample is not None and not subsample:
            raise ValueError("`subsample=true` required.")  # ArgumentError, :338
        if moments:
            raise TypeError("moments is a keyword of the event-recorded pdmp (a BouncyParticle with a Γ, or a Boomerang)")
        return _bps_modern(target, t0, x0, θ0, T, c, F, 2.0 if factor == 1.8 else factor, adapt, seed, device, trace_capacity, trace, oscn,
                           consume=consume)
    if oscn:
        raise TypeError("oscn is a keyword of the speed-recorded pdmp (BouncyParticle(None, None, ...), c::LocalBound)")
    subsample = bool(subsample)
    if isinstance(F, BouncyParticle):
        if target is not None and not isinstance(target, GaussianTarget):
            raise TypeError("BouncyParticle: target is None (∇ϕ!(y, x) = B.Γ(x − B.μ)) or a GaussianTarget of its own")
        return _bps(t0, x0, θ0, T, c, F, 2.0 if factor == 1.8 else factor, adapt, seed, device, trace_capacity, trace,
                    target=target, subsample=subsample, moments=moments, consume=consume)
    if isinstance(F, Boomerang):  # pdmp(∇ϕ!, t0, x0, θ0, T, c, B::Boomerang) (test/maintest.jl:139-154); target = GaussianTarget
        if not isinstance(target, GaussianTarget):
            raise TypeError("Boomerang: target must be a GaussianTarget (∇ϕ!(y, x) = Γ(x − μ))")
        return _bps(t0, x0, θ0, T, c, F, 2.0 if factor == 1.8 else factor, adapt, seed, device, trace_capacity, trace,
                    target=target, subsample=subsample, moments=moments, consume=consume)
    if subsample or moments or consume is not None:
        raise TypeError("subsample, moments and consume are keywords of the non-factorised pdmp (BouncyParticle / Boomerang)")
    return _zigzag(_lib.SAMPLER_ZIGZAG_ALL, target, t0, x0, θ0, T, c, F, factor, adapt, seed, device, trace_capacity, trace)


def sspdmp(target, t0, x0, θ0, T, c, *GFκ, reversible=False, strong_upperbounds=False, factor=None, adapt=False,
           seed=DEFAULT_SEED, device=0, trace_capacity=None, trace=True, G=None, consume=None):
    """Sticky ZigZag: sspdmp(∇ϕ, t0, x0, θ0, T, c, [G,] F::ZigZag, κ, args...; reversible, strong_upperbounds, factor=1.5,
    adapt) (src/ss_fact.jl:159-160,217) -> Ξ, (t, x, θ), (acc, num), c with scalar acc, num (:175,214).  G as in spdmp (:167-172).

    With a PrecisionCholeskyTarget this is casestudies/precision/precision.jl:82: sspdmp(target, t0, x0, θ0, T, c, ZigZag(diag Γ̂, μ̂), κ;
    adapt=True) with the inputs of problems.precision_cholesky_problem (the column of a coordinate, the script's G, is the target's own);
    consume=dict(dt=..., points=...) then appends dict(mean, T, grid_t, grid_x, inclusion) from the device consumers.

    Sticky Bouncy Particle / Boomerang: sspdmp(∇ϕ!, t0, x0, θ0, T, c, Flow::Union{BouncyParticle, Boomerang}, κ, args...;
    strong_upperbounds, adapt, factor=2.0) (src/ss_not_fact.jl:182-201) -> Ξ, (t, x, θ), (acc, num), c.  Ξ is a PDMPTrace carrying f0 and f
    ([events x d] bool, True = free); its first event is (t0, x0, θ0, all free) (:189).  target as in pdmp: None (∇ϕ!(y, x) = B.Γ(x − B.μ))
    or a GaussianTarget for a BouncyParticle, a GaussianTarget for a Boomerang.  κ: [d] or a scalar.  No G, no `reversible`.
    consume=dict(dt=..., points=...) as in pdmp; the extra element also holds `inclusion`, trace.inclusion_prob(Ξ).

    factor=None is each signature's own default: 1.5 for a ZigZag, 2.0 for a BouncyParticle / Boomerang; a value given is used as given."""
    if len(GFκ) == 2 and isinstance(GFκ[0], (BouncyParticle, Boomerang)):
        if G is not None or reversible:
            raise TypeError("sspdmp(..., Flow::Union{BouncyParticle, Boomerang}, κ): no G and no `reversible` (src/ss_not_fact.jl:182-183)")
        F = GFκ[0]
        if isinstance(F, Boomerang) and not isinstance(target, GaussianTarget):
            raise TypeError("Boomerang: target must be a GaussianTarget (∇ϕ!(y, x) = Γ(x − μ))")
        if isinstance(F, BouncyParticle) and target is not None and not isinstance(target, GaussianTarget):
            raise TypeError("BouncyParticle: target is None (∇ϕ!(y, x) = B.Γ(x − B.μ)) or a GaussianTarget of its own")
        return _bps(t0, x0, θ0, T, c, F, 2.0 if factor is None else factor, adapt, seed, device, trace_capacity, trace, target=target,
                    sticky=(GFκ[1], strong_upperbounds), consume=consume)
    if consume is not None and not _admits(consume) and not isinstance(target, PrecisionCholeskyTarget):
        raise TypeError("consume is a keyword of the sticky BouncyParticle / Boomerang and of a PrecisionCholeskyTarget, or with cov=P or hist=dict(...) "
                        "(elsewhere the ZigZag's device consumers are Ensemble.consume_*)")
    if len(GFκ) not in (2, 3):
        raise TypeError("expected sspdmp(target, t0, x0, θ0, T, c, [G,] F, κ, ...)")
    G, F = _split_G(GFκ[:-1], G)
    κ = GFκ[-1]
    return _zigzag(_lib.SAMPLER_STICKY_ZIGZAG, target, t0, x0, θ0, T, c, F, 1.5 if factor is None else factor, adapt, seed, device,
                   trace_capacity, trace, sticky=(np.asarray(κ, dtype=np.float64), reversible, strong_upperbounds), G=G, consume=consume)


def stickyzz(target, t0, x0, θ0, T, c, F, barriers, *, strong_upperbounds=False, adapt=False, factor=1.5, seed=DEFAULT_SEED, device=0,
             trace_capacity=None, trace=True, details=False, consume=None):
    """The ZigZag with sticky and reflecting barriers: stickyzz(u0, target::StructuredTarget, flow::StickyFlow(F), upper_bounds::
    StickyUpperBounds(G, G1, Γ, c; adapt, strong, multiplier=factor), barriers, EndTime(T)) (src/stickyzz.jl:176-218) with G = G1 = the pattern of
    F.Γ, in the call shape of the other samplers.  barriers: a list of d StickyBarriers, or one for all coordinates.  Returns
    Ξ, t′, (t, x, θ), (acc, num) like the reference (:217); x0 / θ0 may be [nchains, d] (outputs then carry a leading chain axis).  Box
    constraints, truncated Gaussians, positivity constraints, sticking at any level with its own stickiness on either side.

    details=True (engine-only keyword) appends a dict: c (the bounds after adaptation), frozen (v == 0 and v_old != 0) and θ_saved (v_old).

    consume=dict(dt=..., points=...[, cov=P, center=c][, condition=(p, n), hits=K]) (engine-only keyword): the device consumers
    (Ensemble.barrier_consume_begin) run over every slice before its buffer is recycled, and a dict is appended behind everything else: mean,
    T, grid_t, grid_x as in spdmp, frozen_lo / frozen_hi (the time each coordinate sat frozen on its lower / upper barrier) and hits_lo /
    hits_hi (how often it hit each) -- trace.barrier_occupation, raw sums over [t0, T] --, plus pairs / pair_S / pair_J and hit_t / hit_x /
    nhits where asked for.  The consumers follow the path the chain travelled -- a coordinate that starts on the barrier of its θ0 starts with
    θ = 0 --, i.e. the host mirrors on FactTrace(F, t0, x0, trace.barrier_start(x0, θ0, barriers)[0], Ξ.events), not on the returned Ξ, which
    records θ0 like the reference's Trace(t′, x0, v0).  With trace=False the events are written to the device buffer and consumed, never
    copied to the host.  Without the keyword, returns and behaviour are unchanged."""
    if not isinstance(F, ZigZag) or isinstance(F, FactBoomerang):
        raise TypeError("stickyzz takes F::ZigZag (StickyFlow(F), src/stickyzz.jl:28-30)")
    d = np.asarray(x0).shape[-1]
    if isinstance(barriers, StickyBarriers):
        barriers = [barriers] * d
    barriers = list(barriers)
    if len(barriers) != d or not all(isinstance(b, StickyBarriers) for b in barriers):
        raise TypeError("barriers: a list of d StickyBarriers, or one for all coordinates")
    tab = (np.array([b.x[0] for b in barriers]), np.array([b.x[1] for b in barriers]),
           np.array([_lib.BARRIER_RULES[b.rule[0]] for b in barriers], dtype=np.int32),
           np.array([_lib.BARRIER_RULES[b.rule[1]] for b in barriers], dtype=np.int32),
           np.array([b.κ[0] for b in barriers]), np.array([b.κ[1] for b in barriers]), strong_upperbounds)
    return _zigzag(_lib.SAMPLER_BARRIER_ZIGZAG, target, t0, x0, θ0, T, c, F, factor, adapt, seed, device, trace_capacity, trace,
                   barriers=tab, details=details, consume=consume)


def sspdmp2(target, t0, x0, θ0, T, c, G, Z, κ, *, strong_upperbounds=False, adapt=False, factor=1.5, seed=DEFAULT_SEED, device=0,
            trace_capacity=None, trace=True, consume=None):
    """sspdmp2(∇ϕ2, t, x0, v0, T, c, ::Nothing, Z, κ, args...; strong_upperbounds, adapt, factor=1.5) (src/stickyzz.jl:323-339): the sticky
    ZigZag written with the barrier framework -- barriers (0, 0), (:sticky, :sticky), (κ[i], κ[i]) on every coordinate.  Returns (trace, acc)
    like the reference (:338), acc being the pair (acc, num).  consume=... as in stickyzz: (trace, acc, consumed); the posterior inclusion
    probability is 1 − (frozen_lo + frozen_hi) / (T − t0)."""
    if G is not None:
        raise TypeError("sspdmp2(∇ϕ2, t, x0, v0, T, c, ::Nothing, Z, κ, ...): the seventh argument is None (src/stickyzz.jl:323)")
    d = np.asarray(x0).shape[-1]
    κ = np.broadcast_to(np.asarray(κ, dtype=np.float64), (d,))
    barriers = [StickyBarriers((0.0, 0.0), ("sticky", "sticky"), (κ[i], κ[i])) for i in range(d)]
    Ξ, _, _, acc, *consumed = stickyzz(target, t0, x0, θ0, T, c, Z, barriers, strong_upperbounds=strong_upperbounds, adapt=adapt, factor=factor,
                                       seed=seed, device=device, trace_capacity=trace_capacity, trace=trace, consume=consume)
    return (Ξ, acc, *consumed)


class Partition:
    """Partition(nt, n) (src/parallel.jl:4-31): n coordinates in nt chunks of k = n ÷ nt; pt(i) -> (chunk, offset), pt(chunk, offset) -> i
    (0-based here)."""

    def __init__(self, nt, n):
        self.nt, self.n, self.k = int(nt), int(n), int(n) // int(nt)

    def __len__(self):
        return self.nt

    def __call__(self, *a):
        if len(a) == 1:
            return divmod(int(a[0]), self.k)
        return int(a[0]) * self.k + int(a[1])


def partition_tables(F, target, G=None):
    """The flow tables of a partitioned run: (Fu, mask).  Fu is F with its bounding Γ spread over G's pattern (explicit zeros where Γ has no
    entry) and mask [nnz] uint8 flags Γ's own structural entries, G1, among them -- what Ensemble.set_flow and Ensemble.run_partitioned take.
    G: None = the pattern of F.Γ (src/parallel.jl:113-115), or a sparse matrix whose pattern ⊇ F.Γ's (G ⊇ G1, :119) and ⊇ the target's."""
    def pattern(A):  # structural pattern (explicit zeros count, as in Julia's rowvals / nzrange)
        A = sp.csc_matrix(A)
        B = sp.csc_matrix((np.ones(A.nnz), A.indices.copy(), A.indptr.copy()), shape=A.shape)
        B.sort_indices()
        B.sum_duplicates()
        B.data[:] = 1.0
        return B

    Gb = F.Γ
    d = Gb.shape[0]
    own = pattern(Gb)
    pg = own if G is None else pattern(G)
    U = (pg + own + pattern(target.Γ)).tocsc()
    U.sort_indices()
    if U.nnz != pg.nnz:
        raise ValueError("G must contain the patterns of F.Γ (G ⊇ G1, src/parallel.jl:119) and of the target")
    cols = np.repeat(np.arange(d), np.diff(U.indptr))
    rows = U.indices
    mask = np.asarray(own[rows, cols]).reshape(-1) != 0
    vals = np.asarray(sp.csc_matrix(Gb)[rows, cols]).reshape(-1)
    Γu = sp.csc_matrix((vals, rows.copy(), U.indptr.copy()), shape=Gb.shape)
    Fu = copy.copy(F)
    Fu.Γ = Γu  # (not through __post_init__: explicit zeros must stay)
    return Fu, mask.astype(np.uint8)


def parallel_spdmp(partition, target, t0, x0, θ0, T, c, G, F, *, factor=1.8, adapt=False, Δ=0.1, seed=DEFAULT_SEED, device=0,
                   trace_capacity=None, trace=True):
    """parallel_spdmp(partition, ∇ϕ, t0, x0, θ0, T, c, G, F::ZigZag; factor=1.8, adapt=false, Δ=0.1) (src/parallel.jl:104-175):
    the local ZigZag with the coordinates cut into len(partition) chunks, one worker per chunk and a coordinator -- on the device one
    WAVEFRONT per chunk (pdmp_ensemble_run_partitioned).  F.Γ is the bounding precision: its pattern G1 must not leave the chunks
    ("Upper bounds may not depend across chunks.", :124-127).  G: None = the pattern of F.Γ (:113-115), or a sparse matrix whose pattern
    ⊇ F.Γ's and ⊇ the target's gives the neighbourhoods that are moved before a gradient (test/testparallel.jl:49 passes the target's).
    Returns Ξ (sorted by time, :167), (t, x, θ), (acc, num); with adapt=True a numpy `c` is updated in place like the reference's."""
    if not isinstance(F, ZigZag) or isinstance(F, FactBoomerang):
        raise TypeError("the device path of parallel_spdmp supports F::ZigZag")
    if not isinstance(target, GaussianTarget):
        raise TypeError("target must be a GaussianTarget")
    K = len(partition) if not np.isscalar(partition) else int(partition)
    x0 = np.asarray(x0, dtype=np.float64)
    θ0 = np.asarray(θ0, dtype=np.float64)
    single = x0.ndim == 1
    X0, TH0 = np.atleast_2d(x0), np.atleast_2d(θ0)
    nch, d = X0.shape
    Fu, mask = partition_tables(F, target, G)
    cc = np.asarray(c, dtype=np.float64)
    seeds = (np.uint64(seed) + np.arange(nch, dtype=np.uint64)) if np.isscalar(seed) else np.asarray(seed, np.uint64)
    if trace_capacity is None:
        trace_capacity = int(min(max(4096, 4.0 * d * max(T - t0, 1.0)), 1 << 24))
    cap = trace_capacity if trace else 0
    ens = Ensemble(nch, d, sampler=_lib.SAMPLER_ZIGZAG_LOCAL, adapt=adapt, factor=factor, device=device, trace_capacity=cap)
    try:
        ens.set_flow(Fu)
        ens.set_target(target)
        ens.set_state(t0, X0, TH0, cc, seeds)
        ens.run_partitioned(T, K, Δ, mask)
        cnt = ens.counters()
        if np.any(cnt["status"] == _lib.CHAIN_BOUND_VIOLATED):
            raise RuntimeError("Tuning parameter `c` too small.")  # src/parallel.jl:42
        if np.any(cnt["status"] == _lib.CHAIN_TRACE_FULL):
            raise RuntimeError("trace_capacity too small for a partitioned run (it is not resumable): %d events" % int(cnt["nevents"].max()))
        events = [[] for _ in range(nch)]
        if trace:
            _drain(ens, events)
        fs = ens.final_state()
    finally:
        ens.close()
    traces = []
    for k_ in range(nch):
        ev = np.concatenate(events[k_]) if events[k_] else np.empty(0, dtype=_lib.EVENT_DTYPE)
        ev = ev[np.argsort(ev["t"], kind="stable")]  # sort!(Ξ.events, by=ev->ev[1]), :167
        traces.append(FactTrace(F, t0, X0[k_].copy(), TH0[k_].copy(), ev))
    acc, num = cnt["nacc"].astype(np.int64), cnt["num"].astype(np.int64)
    if adapt and single and isinstance(c, np.ndarray) and c.dtype == np.float64:
        c[:] = fs["c"][0]  # adapt!(c, i, factor) acts on the caller's vector
    if single:
        return traces[0], (fs["t"][0], fs["x"][0], fs["theta"][0]), (int(acc[0]), int(num[0]))
    return traces, (fs["t"], fs["x"], fs["theta"]), (acc, num)


def _pattern_of(G, d):
    """G as a CSC pattern: a sparse matrix (explicit zeros count, like rowvals / nzrange) or a sequence of index arrays / (i, indices) pairs."""
    if sp.issparse(G):
        G = sp.csc_matrix(G)
        return sp.csc_matrix((np.ones(G.nnz), G.indices.copy(), G.indptr.copy()), shape=G.shape)
    cols = [np.asarray(g[1] if isinstance(g, tuple) else g, dtype=np.int64) for g in G]
    if len(cols) != d:
        raise ValueError("G needs one neighbourhood per coordinate")
    indptr = np.concatenate([[0], np.cumsum([len(g) for g in cols])])
    P = sp.csc_matrix((np.ones(int(indptr[-1])), np.concatenate(cols) if cols else np.empty(0, np.int64), indptr), shape=(d, d))
    P.sort_indices()
    return P


def _zigzag(sampler, target, t0, x0, θ0, T, c, F, factor, adapt, seed, device, trace_capacity, trace, sticky=None,
            adaptscale=False, tracked=False, G=None, barriers=None, details=False, consume=None):
    if not isinstance(F, (ZigZag, FactBoomerang)):
        raise TypeError("the device path supports F::ZigZag and F::FactBoomerang")
    if not isinstance(target, (GaussianTarget, LogisticTarget, DiffusionBridgeTarget, PrecisionCholeskyTarget)):
        raise TypeError("target must be one of the device-resident families (GaussianTarget, LogisticTarget, DiffusionBridgeTarget, PrecisionCholeskyTarget)")
    if isinstance(target, PrecisionCholeskyTarget) and sticky is None:
        raise TypeError("PrecisionCholeskyTarget is a target of sspdmp (the sticky ZigZag of casestudies/precision/precision.jl)")
    # a flow with a refresh clock (a ZigZag with λref > 0, a FactBoomerang) leaves a trace that is sorted within a coordinate only: the unordered
    # consumers (Ensemble.refresh_consume_begin) serve it, with mean and the grid alone
    refresh = barriers is None and sticky is None and (isinstance(F, FactBoomerang) or F.λref > 0)
    if consume is not None and refresh:
        if not isinstance(consume, dict) or set(consume) & {"cov", "center", "hist", "condition", "hits"}:
            raise TypeError("consume=dict(dt=..., points=...) on a flow with a refresh clock (a ZigZag with λref > 0, a FactBoomerang): cov, hist and "
                            "condition walk a time-ordered trace and are not available there")
    elif consume is not None and barriers is None and not isinstance(target, (DiffusionBridgeTarget, PrecisionCholeskyTarget)) and not _admits(consume):
        raise TypeError("consume is a keyword of spdmp with a DiffusionBridgeTarget and of sspdmp with a PrecisionCholeskyTarget, or with cov=P or "
                        "hist=dict(...) (elsewhere the ZigZag's device consumers are Ensemble.consume_*)")
    x0 = np.asarray(x0, dtype=np.float64)
    θ0 = np.asarray(θ0, dtype=np.float64)
    single = x0.ndim == 1
    X0 = np.atleast_2d(x0)
    TH0 = np.atleast_2d(θ0)
    nch, d = X0.shape
    local_bound = isinstance(c, LocalBound)  # spdmp(∇ϕ, t0, x0, θ0, T, C::LocalBound, F, args...), src/local.jl:95-149
    c = np.asarray(c.c if local_bound else c, dtype=np.float64)
    seeds = (np.uint64(seed) + np.arange(nch, dtype=np.uint64)) if np.isscalar(seed) else np.asarray(seed, np.uint64)
    if trace_capacity is None:
        # ~0.8 reflections per coordinate per unit time on the GMRF; generous first guess, refilled on demand
        trace_capacity = int(min(max(1024, 2.0 * d * max(T - t0, 1.0)), 1 << 22))
    cap = _consume_capacity(consume, trace, trace_capacity)
    ens = Ensemble(nch, d, sampler=sampler, adapt=adapt, factor=factor, device=device,
                   trace_capacity=cap)
    try:
        ens.set_flow(F)
        if G is not None:
            try:
                ens.set_neighbourhood(_pattern_of(G, d))
            except _lib.PdmpError as exc:
                if "does not contain G1" in str(exc) or "must contain G1" in str(exc):
                    raise AssertionError("all(a.second ⊇ b.second for (a,b) in zip(G, G1)) -- src/sfact.jl:177") from exc
                raise
        ens.set_target(target)
        if sticky is not None:
            ens.set_sticky(*sticky)
        if barriers is not None:
            ens.set_barriers(*barriers)
        if adaptscale:
            ens.set_adaptscale(True)
        if local_bound:
            ens.set_local_bound(True)
        if tracked:
            ens.set_gradient_tracking(True)
        ens.set_state(t0, X0, TH0, c, seeds)
        if consume is not None:
            begin = ens.refresh_consume_begin if refresh else ens.consume_begin if barriers is None else ens.barrier_consume_begin
            begin(float(consume.get("dt", 0.0)), int(consume.get("points", 0)))
            if _condition_of(consume) is not None:
                ens.consume_condition(*_condition_of(consume))
            if _pairs_of(consume, d) is not None:
                ens.consume_pairs(*_pairs_of(consume, d))
            if _hist_of(consume, d) is not None:
                ens.consume_hist(*_hist_of(consume, d))
        events = [[] for _ in range(nch)]
        while True:
            ens.run(T, _lib.RUN_REFERENCE_TAIL)
            cnt = ens.counters()
            if np.any(cnt["status"] == _lib.CHAIN_BOUND_VIOLATED):
                raise RuntimeError("Tuning parameter `c` too small.")  # src/sfact.jl:124
            if isinstance(target, PrecisionCholeskyTarget) and np.any(cnt["status"] == _lib.CHAIN_STALLED):
                # (the reference would go on to evaluate N/0: the affine bound let a diagonal of L run into 0 -- a tuning failure like the one above)
                k = int(np.flatnonzero(cnt["status"] == _lib.CHAIN_STALLED)[0])
                raise RuntimeError("PrecisionCholeskyTarget: chain %d stalled at t = %g: a diagonal coordinate L[c, c] reached 0 (or a coordinate was "
                                   "started at x = 0 with θ = 0); the bound c is too small for the −N/L[c, c] term" % (k, float(cnt["t_last"][k])))
            if consume is not None:
                ens.consume()
            if trace:
                _drain(ens, events)
            elif consume is not None:
                ens.trace_reset()
            if not _lib.needs_rerun(cnt["status"]):  # (both resume with the next run)
                break
        consumed = None
        if consume is not None:
            mean, Tl = ens.consume_mean()
            consumed = dict(mean=mean, T=Tl, grid_t=None, grid_x=None)
            if isinstance(target, PrecisionCholeskyTarget):
                consumed["inclusion"] = ens.consume_inclusion()[0]  # trace.inclusion_prob(Ξ): the posterior probability of L[r, c] != 0
            if barriers is not None:
                occ = ens.barrier_consume_occupation()
                consumed.update(frozen_lo=occ[0], frozen_hi=occ[1], hits_lo=occ[2], hits_hi=occ[3])
            if int(consume.get("points", 0)) > 0:
                grids = [ens.consume_discretized(k) for k in range(nch)]
                consumed["grid_t"], consumed["grid_x"] = [g[0] for g in grids], [g[1] for g in grids]
            if _condition_of(consume) is not None:
                _condition_result(consumed, ens.consume_conditioned, nch)
            if single:
                consumed = {k: (v if v is None else v[0]) for k, v in consumed.items()}
            if _pairs_of(consume, d) is not None:
                _pairs_result(consumed, _pairs_of(consume, d), ens.consume_pair_integrals)
                if single:
                    consumed["pair_S"], consumed["pair_J"] = consumed["pair_S"][0], consumed["pair_J"][0]
            if _hist_of(consume, d) is not None:
                _hist_result(consumed, _hist_of(consume, d), ens.consume_histogram, single)
        fs = ens.final_state()
        cnt = ens.counters()
        sig = ens.final_sigma() if adaptscale else None
        fb = ens.final_barrier() if barriers is not None else None
    finally:
        ens.close()
    traces = []
    for k in range(nch):
        ev = np.concatenate(events[k]) if events[k] else np.empty(0, dtype=_lib.EVENT_DTYPE)
        Fk = F
        if sig is not None:
            if single:
                F.σ[:] = sig[0]  # the reference mutates F.σ (src/sfact.jl:90,97)
            else:
                Fk = copy.copy(F)
                Fk.σ = sig[k].copy()
        traces.append(FactTrace(Fk, t0, X0[k].copy(), TH0[k].copy(), ev))
    num = cnt["num"].astype(np.int64)
    c_out = fs["c"] if adapt else np.broadcast_to(c, (nch, d)).copy()
    acc = cnt["nacc"].astype(np.int64) if sticky is not None else fs["acc"]  # sticky: scalar acc (src/ss_fact.jl:175)
    if barriers is not None:  # Ξ, t′, u, acc (src/stickyzz.jl:217): acc::AcceptanceDiagnostics is the scalar pair
        acc = cnt["nacc"].astype(np.int64)
        tp = cnt["t_last"].astype(np.float64)
        extra = dict(c=c_out, frozen=fb["frozen"], θ_saved=fb["theta_saved"])
        tail = () if consumed is None else (consumed,)
        if single:
            out = traces[0], float(tp[0]), (fs["t"][0], fs["x"][0], fs["theta"][0]), (int(acc[0]), int(num[0]))
            return out + (({k: v[0] for k, v in extra.items()},) if details else ()) + tail
        return (traces, tp, (fs["t"], fs["x"], fs["theta"]), (acc, num)) + ((extra,) if details else ()) + tail
    tail = () if consumed is None else (consumed,)
    if single:
        return (traces[0], (fs["t"][0], fs["x"][0], fs["theta"][0]), (acc[0], int(num[0])), c_out[0]) + tail
    return (traces, (fs["t"], fs["x"], fs["theta"]), (acc, num), c_out) + tail


def _bps_modern(target, t0, x0, θ0, T, c, B, factor, adapt, seed, device, trace_capacity, trace, oscn, consume=None):
    """The speed-recorded Bouncy Particle on the device (pdmp_ensemble_set_flow_bps_modern): one chain per row of x0."""
    c = float(np.asarray(c.c, dtype=np.float64).reshape(-1)[0])
    x0 = np.asarray(x0, dtype=np.float64)
    θ0 = np.asarray(θ0, dtype=np.float64)
    single = x0.ndim == 1
    X0, TH0 = np.atleast_2d(x0), np.atleast_2d(θ0)
    nch, d = X0.shape
    seeds = (np.uint64(seed) + np.arange(nch, dtype=np.uint64)) if np.isscalar(seed) else np.asarray(seed, np.uint64)
    count = isinstance(T, (int, np.integer)) and not isinstance(T, bool)  # `T isa Int`: a number of samples
    if count and T < 0:
        raise ValueError("a sample count T must not be negative")
    if trace_capacity is None:
        want = int(T) if count else int(4 * B.λref * max(float(T) - t0, 1.0))
        trace_capacity = int(min(max(64, want), (1 << 28) // max(2 * d, 1)))
    cap = _consume_capacity(consume, trace, trace_capacity)
    ens = Ensemble(nch, d, sampler=_lib.SAMPLER_BPS, adapt=adapt, factor=factor, device=device, trace_capacity=cap)
    ts, xs, ths = [[] for _ in range(nch)], [[] for _ in range(nch)], [[] for _ in range(nch)]
    try:
        ens.set_flow_bps_modern(B.λref, B.ρ, B.U, oscn)
        ens.set_target(target)
        if B.L is not None:
            ens.set_mass_cholesky(B.L)
        ens.set_state_bps(t0, X0, TH0, c, seeds)
        if consume is not None:
            ens.bps_consume_begin(consume.get("dt", 0.0), consume.get("points", 0))
            if _condition_of(consume) is not None:
                ens.bps_consume_condition(*_condition_of(consume))
            if _pairs_of(consume, ens.d) is not None:
                ens.bps_consume_pairs(*_pairs_of(consume, ens.d))
            if _hist_of(consume, ens.d) is not None:
                ens.bps_consume_hist(*_hist_of(consume, ens.d))
        if count:
            ens.set_bps_record_limit(int(T))
        T_end = float("inf") if count else float(T)
        while not (count and int(T) == 0):
            ens.run(T_end, _lib.RUN_REFERENCE_TAIL)
            cnt = ens.counters()
            if np.any(cnt["status"] == _lib.CHAIN_BOUND_VIOLATED):
                raise RuntimeError("Tuning parameter `c` too small.")  # :230, :262
            if np.any(cnt["status"] == _lib.CHAIN_STALLED):
                raise AssertionError("Δrec > 0.0")  # :239
            if consume is not None:
                ens.bps_consume()
            if trace:
                for k in range(nch):
                    if cnt["ntrace"][k]:
                        a, b_, c_ = ens.bps_trace(k, counters=cnt)
                        ts[k].append(a)
                        xs[k].append(b_)
                        ths[k].append(c_)
            if trace or consume is not None:
                ens.trace_reset()
            if not _lib.needs_rerun(cnt["status"]):
                break
        fs = ens.bps_final_state()
        cnt = ens.counters()
        consumed = None if consume is None else _consume_result(ens, consume, single, False)
    finally:
        ens.close()
    traces = []
    for k in range(nch):
        if ts[k]:
            traces.append(PDMPTrace(B, t0, X0[k].copy(), TH0[k].copy(), np.concatenate(ts[k]), np.concatenate(xs[k]), np.concatenate(ths[k])))
        else:
            traces.append(PDMPTrace(B, t0, X0[k].copy(), TH0[k].copy(), np.empty(0), np.empty((0, d)), np.empty((0, d))))
    acc, num = cnt["nacc"].astype(np.int64), cnt["num"].astype(np.int64)
    if single:
        out = traces[0], (fs["t"][0], fs["x"][0], fs["theta"][0]), (int(acc[0]), int(num[0])), fs["c"][0]
    else:
        out = traces, (fs["t"], fs["x"], fs["theta"]), (acc, num), fs["c"]
    return out if consume is None else out + (consumed,)


def _bps(t0, x0, θ0, T, c, B, factor, adapt, seed, device, trace_capacity, trace, target=None, subsample=False, moments=False, sticky=None,
         consume=None):
    local_bound = isinstance(c, LocalBound)
    if local_bound:
        c = float(np.asarray(c.c, dtype=np.float64).reshape(-1)[0])
    x0 = np.asarray(x0, dtype=np.float64)
    θ0 = np.asarray(θ0, dtype=np.float64)
    single = x0.ndim == 1
    X0, TH0 = np.atleast_2d(x0), np.atleast_2d(θ0)
    nch, d = X0.shape
    seeds = (np.uint64(seed) + np.arange(nch, dtype=np.uint64)) if np.isscalar(seed) else np.asarray(seed, np.uint64)
    if trace_capacity is None:
        trace_capacity = int(min(max(256, 64 * max(T - t0, 1.0)), (1 << 28) // max(2 * d, 1)))
    cap = _consume_capacity(consume, trace, trace_capacity)
    ens = Ensemble(nch, d, sampler=_lib.SAMPLER_BPS, adapt=adapt, factor=factor, device=device, trace_capacity=cap)
    try:
        if isinstance(B, Boomerang):
            ens.set_flow_boomerang(target, B)
        else:
            ens.set_flow_bps(B)
            if target is not None:  # ∇ϕ! of its own; ab(…GlobalBound…) keeps B.Γ, B.μ (src/not_fact_samplers.jl:26-28,122)
                ens.set_target(target)
        if local_bound or subsample:
            ens.set_bps_options(local_bound, subsample)
        if moments:
            ens.set_bps_moments(2)
        if sticky is not None:
            ens.set_bps_sticky(*sticky)
        ens.set_state_bps(t0, X0, TH0, float(c), seeds)
        if consume is not None:
            ens.bps_consume_begin(consume.get("dt", 0.0), consume.get("points", 0))
            if _condition_of(consume) is not None:
                ens.bps_consume_condition(*_condition_of(consume))
            if _pairs_of(consume, ens.d) is not None:  # (a Boomerang's pieces are arcs: another integral, the same accumulators)
                (ens.bps_consume_arc_pairs if isinstance(B, Boomerang) else ens.bps_consume_pairs)(*_pairs_of(consume, ens.d))
            if _hist_of(consume, ens.d) is not None:  # (likewise: the occupation time of an arc is another closed form, the rows are the same)
                (ens.bps_consume_arc_hist if isinstance(B, Boomerang) else ens.bps_consume_hist)(*_hist_of(consume, ens.d))
        fs_ = [[] for _ in range(nch)]
        ts = [[] for _ in range(nch)]
        xs = [[] for _ in range(nch)]
        ths = [[] for _ in range(nch)]
        J = None
        # moments: every chain paused before its first event at or past T (the moments are read there), then the reference's tail --
        # the same events in the same order as one reference-tail run
        for flags in ((_lib.RUN_STOP_BEFORE, _lib.RUN_REFERENCE_TAIL) if moments else (_lib.RUN_REFERENCE_TAIL,)):
            while True:
                ens.run(T, flags)
                cnt = ens.counters()
                if np.any(cnt["status"] == _lib.CHAIN_BOUND_VIOLATED):
                    if sticky is not None:  # (either error(...) of src/ss_not_fact.jl:129-132,160)
                        raise RuntimeError("Tuning parameter `c` too small, or a coordinate froze away from 0 (|x[i]| > 1e-8).")
                    raise RuntimeError("Tuning parameter `c` too small.")  # src/not_fact_samplers.jl:82
                if consume is not None:
                    ens.bps_consume()
                if trace:
                    for k in range(nch):
                        if cnt["ntrace"][k]:
                            a, b_, c_ = ens.bps_trace(k, counters=cnt)
                            ts[k].append(a)
                            xs[k].append(b_)
                            ths[k].append(c_)
                            if sticky is not None:
                                fs_[k].append(ens.bps_trace_free(k, counters=cnt))
                if trace or consume is not None:
                    ens.trace_reset()
                if not _lib.needs_rerun(cnt["status"]):  # (both resume with the next run)
                    break
            if flags == _lib.RUN_STOP_BEFORE:
                J = ens.bps_moments(T)
        fs = ens.bps_final_state()
        cnt = ens.counters()
        consumed = None if consume is None else _consume_result(ens, consume, single, sticky is not None)
    finally:
        ens.close()
    traces = []
    for k in range(nch):
        if ts[k]:
            traces.append(PDMPTrace(B, t0, X0[k].copy(), TH0[k].copy(), np.concatenate(ts[k]), np.concatenate(xs[k]),
                                    np.concatenate(ths[k])))
        else:
            traces.append(PDMPTrace(B, t0, X0[k].copy(), TH0[k].copy(), np.empty(0), np.empty((0, d)), np.empty((0, d))))
        if sticky is not None:
            traces[-1].f0 = np.ones(d, dtype=bool)
            traces[-1].f = np.concatenate(fs_[k]) if fs_[k] else np.empty((0, d), dtype=bool)
    acc, num = cnt["nacc"].astype(np.int64), cnt["num"].astype(np.int64)
    if single:
        out = traces[0], (fs["t"][0], fs["x"][0], fs["theta"][0]), (int(acc[0]), int(num[0])), fs["c"][0]
    else:
        out = traces, (fs["t"], fs["x"], fs["theta"]), (acc, num), fs["c"]
    if moments:
        mean = J[0] / (T - t0)
        var = J[1] / (T - t0) - mean * mean
        if single:
            mean, var = mean[0], var[0]
        out = out + (dict(mean=mean, var=var, T=T),)
    return out if consume is None else out + (consumed,)
