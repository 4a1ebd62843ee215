"""The one-wave forms of the one-proposal-per-lane tracked kernel keep their draws in a ring of 128 doubles in LDS (-m gpu): every uniform of a
launch is produced once, 64 at a time, and a block of 64 is flushed into the ring as far as the iteration's window of 128 draws has moved on -- in
most iterations only partly.  Three chains put the launch on the target rule (about 34 proposals, about 90 draws per iteration), so blocks of 64 are
crossed and left half flushed all the time; launches that resume at draw counts that are no multiple of 64 (a lowered count limit, a trace segment
that fills up, a slice boundary) restart the ring at the chain's own draw count.  Every case forces the one-wave form on its own ensemble and holds
the complete trace, the final state and the counters of every chain to the oracle's tracked evaluation, bit for bit."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu


def _run_and_collect(pkg, e, slices):
    """Run the slices (T, flag) to their ends through every pause, the trace drained and recycled after every launch; the concatenated trace of every
    chain, and how many launches it took."""
    L = pkg._lib
    got = [[] for _ in range(e.nchains)]
    launches = 0
    for T, flag in slices:
        for _ in range(100000):
            e.run(T, flag)
            launches += 1
            cn = e.counters()
            for k in range(e.nchains):
                got[k].append(e.trace(k, counters=cn))
            e.trace_reset()
            if not L.needs_rerun(cn["status"]):
                break
        else:
            raise AssertionError("the run did not end")
    return [np.concatenate(g) for g in got], launches


def _check(pkg, e, evs, refs):
    cn = e.counters()
    fs = e.final_state()
    assert np.all(cn["status"] == pkg._lib.CHAIN_OK), cn["status"]
    for k, r in enumerate(refs):
        assert r["status"] == 0
        ev = evs[k]
        assert len(ev) == len(r["events"]), (k, len(ev), len(r["events"]))
        for f in ("i", "t", "x", "theta"):
            assert np.array_equal(ev[f], r["events"][f]), (k, f)
        assert int(cn["num"][k]) == r["num"] and int(cn["nacc"][k]) == r["nacc"] and int(cn["ndraw_main"][k]) == r["ndraw_main"], k
        assert np.array_equal(fs["t"][k], r["t"]) and np.array_equal(fs["x"][k], r["x"]) and np.array_equal(fs["theta"][k], r["theta"]), k
        assert np.array_equal(fs["acc"][k], r["acc"]), k


def _synthetic(pkg, G, c, nch, cap, seed0, limit):
    d = G.shape[0]
    e = pkg.Ensemble(nch, d, trace_capacity=cap)
    e.debug_set_helper_wave(0)
    if limit:
        pkg._lib.check(e._L.pdmp_debug_set_launch_count_limit(e._h, limit))
    e.set_flow(pkg.ZigZag(G, np.zeros(d)))
    e.set_target(pkg.GaussianTarget(G))
    e.set_gradient_tracking(True)
    e.set_state_synthetic(0.0, c, seed0)
    return e


@pytest.fixture(scope="module")
def lattice48(gpu_pkg):
    """The 48 x 48 lattice, three chains, and the oracle's tracked runs to T = 4 with the reference's tail (computed once, read only)."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(48)
    d = G.shape[0]
    c = pkg.problems.column_norms(G)
    seed0 = 1300
    refs = []
    for k in range(3):
        x0, th0 = O.synthetic_state(seed0 + k, d)
        refs.append(O.spdmp_zigzag(G, None, G, x0, th0, c, 4.0, seed=seed0 + k, tracked=True))
    return G, c, seed0, refs


@pytest.mark.parametrize("limit", [100, 333, 3000])
def test_lattice_resumed_at_odd_draw_counts(gpu_pkg, lattice48, limit):
    """A launch ends once it has used `limit` draws -- wherever inside a block of 64 that falls -- and a trace segment of 700 events fills up in
    between: every resumed launch starts its ring at its own draw count."""
    pkg = gpu_pkg
    G, c, seed0, refs = lattice48
    with _synthetic(pkg, G, c, 3, 700, seed0, limit) as e:
        evs, launches = _run_and_collect(pkg, e, [(4.0, pkg._lib.RUN_REFERENCE_TAIL)])
        assert e.kernel_name() == "zz_local_trackp_kernel"
        assert launches > max(len(r["events"]) for r in refs) // 700  # (the trace filled up)
        assert launches > min(r["ndraw_main"] for r in refs) // (limit + 128) // 2  # (... and the count limit paused the launches)
        assert any(r["ndraw_main"] % 64 for r in refs)
        _check(pkg, e, evs, refs)


def test_random_graph(gpu_pkg):
    """LAT = false: an accepted event takes up to nine draws, and the groups of eight have few lanes without a member."""
    pkg = gpu_pkg
    G = pkg.problems.random_sparse_precision(2048, 8)
    d = G.shape[0]
    c = pkg.problems.column_norms(G)
    seed0, T = 1400, 2.0
    refs = []
    for k in range(3):
        x0, th0 = O.synthetic_state(seed0 + k, d)
        refs.append(O.spdmp_zigzag(G, None, G, x0, th0, c, T, seed=seed0 + k, tracked=True))
    with _synthetic(pkg, G, c, 3, max(len(r["events"]) for r in refs) + 64, seed0, 333) as e:
        evs, launches = _run_and_collect(pkg, e, [(T, pkg._lib.RUN_REFERENCE_TAIL)])
        assert e.kernel_name() == "zz_local_trackp_kernel<LAT=false>"
        assert launches > 10
        _check(pkg, e, evs, refs)


def test_two_slices_without_a_limit(gpu_pkg):
    """T = 1, then 2, stopping before T, the trace recycled in between: the second launch's ring starts at the draw count the first one left."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(48)
    d = G.shape[0]
    c = pkg.problems.column_norms(G)
    seed0 = 1500
    refs = []
    for k in range(3):
        x0, th0 = O.synthetic_state(seed0 + k, d)
        refs.append(O.spdmp_zigzag(G, None, G, x0, th0, c, 2.0, seed=seed0 + k, stop_before_T=True, tracked=True))
    with _synthetic(pkg, G, c, 3, 3 * d, seed0, 0) as e:
        evs, launches = _run_and_collect(pkg, e, [(1.0, pkg._lib.RUN_STOP_BEFORE), (2.0, pkg._lib.RUN_STOP_BEFORE)])
        assert e.kernel_name() == "zz_local_trackp_kernel" and launches == 2
        _check(pkg, e, evs, refs)


def test_flow_mean_equal_to_the_targets(gpu_pkg):
    """Z = ZigZag(Γ, μ) with a target of the same mean (track_mean = 2): Γ[:,i]·μ enters the bound of every re-bounded proposal."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(48)
    d = G.shape[0]
    rng = np.random.default_rng(3)
    mu = 0.3 * rng.standard_normal(d)
    nch, T, seed0 = 3, 1.5, 77
    x0 = rng.standard_normal((nch, d))
    th0 = rng.choice([-1.0, 1.0], (nch, d))
    c = 3.0 * pkg.problems.column_norms(G)
    refs = [O.spdmp_zigzag(G, mu, G, x0[k], th0[k], c, T, seed=seed0 + k, target_mu=mu, tracked=True) for k in range(nch)]
    with pkg.Ensemble(nch, d, trace_capacity=max(len(r["events"]) for r in refs) + 64) as e:
        e.debug_set_helper_wave(0)
        pkg._lib.check(e._L.pdmp_debug_set_launch_count_limit(e._h, 333))
        e.set_flow(pkg.ZigZag(G, mu))
        e.set_target(pkg.GaussianTarget(G, mu))
        e.set_gradient_tracking(True)
        e.set_state(0.0, x0, th0, c, np.arange(nch, dtype=np.uint64) + np.uint64(seed0))
        evs, launches = _run_and_collect(pkg, e, [(T, pkg._lib.RUN_REFERENCE_TAIL)])
        assert e.kernel_name() == "zz_local_trackp_kernel" and launches > 10
        assert min(len(r["events"]) for r in refs) > 500
        _check(pkg, e, evs, refs)


def test_big_form(gpu_pkg):
    """d = 129 x 129 > 16384: zz_local_trackp_big_kernel, whose ring lies behind 8192 block bounds."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(129)
    d = G.shape[0]
    c = pkg.problems.column_norms(G)
    seed0, T = 1600, 0.05
    refs = []
    for k in range(2):
        x0, th0 = O.synthetic_state(seed0 + k, d)
        refs.append(O.spdmp_zigzag(G, None, G, x0, th0, c, T, seed=seed0 + k, tracked=True))
    with _synthetic(pkg, G, c, 2, max(len(r["events"]) for r in refs) + 64, seed0, 3000) as e:
        evs, launches = _run_and_collect(pkg, e, [(T, pkg._lib.RUN_REFERENCE_TAIL)])
        assert e.kernel_name() == "zz_local_trackp_big_kernel"
        assert launches > 1
        assert min(len(r["events"]) for r in refs) > 100
        _check(pkg, e, evs, refs)
