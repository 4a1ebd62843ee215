"""Wave priority by rank of progress and the one-pass head of the one-proposal-per-lane tracked kernel (-m gpu).

The one-wave forms of zz_local_trackp_kernel (up to d = 16384) post every chain's progress through the launch on a board in device memory and give the
wave of a SIMD that is furthest behind the top priority (pdmp_engine.hpp: PrioLag; pdmp_debug_set_prio_policy: 0 = the turns every other event
loop takes, 1 = by rank); and the forms of 2048 block bounds build their level 1 from ONE coalesced pass over the chain's pairs.  Neither may change
a committed event, a float or a draw: every case holds the complete trace, the final state and the counters to the oracle's tracked evaluation with
tolerance 0, or the two policies to each other, across launches that start at t_begin > 0, pauses (a new epoch each), a T that makes the progress
meaningless, a chain that returns before its loop, and the forms that keep the turns."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
SEED0 = 1700


def _run_and_collect(pkg, e, slices):
    """Run the slices (T, flag) to their ends through every pause, the trace drained and recycled after every launch: the concatenated trace of every
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


def _check(pkg, e, evs, refs, chains=None):
    cn = e.counters()
    fs = e.final_state()
    assert np.all(cn["status"] == pkg._lib.CHAIN_OK), cn["status"]
    for k, r in zip(range(len(refs)) if chains is None else chains, refs):
        assert r["status"] == 0
        ev = evs[k]
        assert len(ev) == len(r["events"]), (k, len(ev), len(r["events"]))
        for f in ("i", "t", "x", "theta"):
            assert np.array_equal(ev[f], r["events"][f]), (k, f)
        assert int(cn["num"][k]) == r["num"] and int(cn["nacc"][k]) == r["nacc"] and int(cn["ndraw_main"][k]) == r["ndraw_main"], k
        assert np.array_equal(fs["t"][k], r["t"]) and np.array_equal(fs["x"][k], r["x"]) and np.array_equal(fs["theta"][k], r["theta"]), k
        assert np.array_equal(fs["acc"][k], r["acc"]), k


def _synthetic(pkg, G, c, nch, cap, seed0, policy, helper=0, limit=0):
    d = G.shape[0]
    e = pkg.Ensemble(nch, d, trace_capacity=cap)
    e.debug_set_helper_wave(helper)
    e.debug_set_prio_policy(policy)
    if limit:
        pkg._lib.check(e._L.pdmp_debug_set_launch_count_limit(e._h, limit))
    e.set_flow(pkg.ZigZag(G, np.zeros(d)))
    e.set_target(pkg.GaussianTarget(G))
    e.set_gradient_tracking(True)
    e.set_state_synthetic(0.0, c, seed0)
    return e


def _oracle(G, c, seed, T, **kw):
    x0, th0 = O.synthetic_state(seed, G.shape[0])
    return O.spdmp_zigzag(G, None, G, x0, th0, c, T, seed=seed, tracked=True, **kw)


@pytest.fixture(scope="module")
def lattice48(gpu_pkg):
    """The 48 x 48 lattice, three chains, and the oracle's tracked runs to T = 2 stopping before T (computed once, read only)."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(48)
    c = pkg.problems.column_norms(G)
    return G, c, [_oracle(G, c, SEED0 + k, 2.0, stop_before_T=True) for k in range(3)]


@pytest.mark.parametrize("policy", [1, 0])
def test_two_slices(gpu_pkg, lattice48, policy):
    """T = 1, then 2: the second launch starts at t_begin > 0 with a new epoch."""
    pkg = gpu_pkg
    G, c, refs = lattice48
    with _synthetic(pkg, G, c, 3, 3 * G.shape[0], SEED0, policy) as e:
        evs, launches = _run_and_collect(pkg, e, [(1.0, pkg._lib.RUN_STOP_BEFORE), (2.0, pkg._lib.RUN_STOP_BEFORE)])
        assert e.kernel_name() == "zz_local_trackp_kernel" and launches == 2
        _check(pkg, e, evs, refs)


def test_switch_takes_three_values(gpu_pkg, lattice48):
    pkg = gpu_pkg
    G, c, _ = lattice48
    with _synthetic(pkg, G, c, 1, 0, SEED0, -1) as e:
        for bad in (-2, 2):
            with pytest.raises(pkg._lib.PdmpError):
                e.debug_set_prio_policy(bad)


def test_four_waves_per_simd(gpu_pkg):
    """4096 chains: every SIMD holds four of them from start to end and its board row has four live words.  Counters, final states and traces of all
    chains are the same under both policies; chains 0, 2047 and 4095 are the oracle's."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(48)
    c = pkg.problems.column_norms(G)
    nch, T, cap = 4096, 0.25, 1024
    res = {}
    for policy in (0, 1):
        with _synthetic(pkg, G, c, nch, cap, SEED0, policy) as e:
            e.run(T, pkg._lib.RUN_STOP_BEFORE)
            assert e.kernel_name() == "zz_local_trackp_kernel"
            cn = e.counters()
            assert np.all(cn["status"] == pkg._lib.CHAIN_OK)
            res[policy] = (cn, e.final_state(), [e.trace(k, counters=cn) for k in range(nch)])
    (c0, f0, t0), (c1, f1, t1) = res[0], res[1]
    for f in ("status", "num", "nacc", "nevents", "ntrace", "ndraw_main", "t_last"):
        assert np.array_equal(c0[f], c1[f]), f
    for f in ("t", "x", "theta", "acc"):
        assert np.array_equal(f0[f], f1[f]), f
    for k in range(nch):
        assert np.array_equal(t0[k], t1[k]), k
    assert min(len(t) for t in t1) > 100 and max(len(t) for t in t1) < cap
    for k in (0, 2047, 4095):
        r = _oracle(G, c, SEED0 + k, T, stop_before_T=True)
        assert r["status"] == 0 and len(t1[k]) == len(r["events"]) and int(c1["num"][k]) == r["num"] and int(c1["ndraw_main"][k]) == r["ndraw_main"]
        for f in ("i", "t", "x", "theta"):
            assert np.array_equal(t1[k][f], r["events"][f]), (k, f)
        assert np.array_equal(f1["t"][k], r["t"]) and np.array_equal(f1["x"][k], r["x"]) and np.array_equal(f1["theta"][k], r["theta"])
        assert np.array_equal(f1["acc"][k], r["acc"])


def test_pauses_and_a_run_that_has_nothing_to_do(gpu_pkg, lattice48):
    """A trace segment of 700 events and a count limit of 333 draws: dozens of launches, each with its own epoch and t_begin.  Then the same T once
    more: no chain has a proposal left before T, nothing changes."""
    pkg = gpu_pkg
    G, c, refs = lattice48
    with _synthetic(pkg, G, c, 3, 700, SEED0, 1, limit=333) as e:
        evs, launches = _run_and_collect(pkg, e, [(2.0, pkg._lib.RUN_STOP_BEFORE)])
        assert e.kernel_name() == "zz_local_trackp_kernel" and launches > 24
        _check(pkg, e, evs, refs)
        cn0, fs0 = e.counters(), e.final_state()
        e.run(2.0, pkg._lib.RUN_STOP_BEFORE)
        cn1, fs1 = e.counters(), e.final_state()
        assert np.all(cn1["status"] == pkg._lib.CHAIN_OK)
        for f in ("num", "nacc", "nevents", "ntrace", "ndraw_main", "t_last"):
            assert np.array_equal(cn0[f], cn1[f]), f
        for f in ("t", "x", "theta", "acc"):
            assert np.array_equal(fs0[f], fs1[f]), f


def test_huge_T(gpu_pkg, lattice48):
    """T = 1e300: the progress is 0 from start to end; the launch ends when its 300 trace slots are full, under either policy with the same events."""
    pkg = gpu_pkg
    G, c, _ = lattice48
    res = {}
    for policy in (0, 1):
        with _synthetic(pkg, G, c, 3, 300, SEED0, policy) as e:
            e.run(1e300, pkg._lib.RUN_REFERENCE_TAIL)
            cn = e.counters()
            assert np.all(cn["status"] == pkg._lib.CHAIN_TRACE_FULL), cn["status"]
            res[policy] = (cn, [e.trace(k, counters=cn) for k in range(3)])
    for f in ("num", "nacc", "nevents", "ntrace", "ndraw_main", "t_last"):
        assert np.array_equal(res[0][0][f], res[1][0][f]), f
    for k in range(3):
        assert len(res[1][1][k]) == 300 and np.array_equal(res[0][1][k], res[1][1][k]), k


def _violation_case(pkg):
    """48 x 48, three chains with bounds c = 1e-12: chains 0 and 2 start near the mode, where the margin c is thousands of ulps of every rate; chain 1
    starts a million times further out, where c is below an ulp of its rates and the bound holds or fails by rounding."""
    G = pkg.problems.gmrf_precision(48)
    d = G.shape[0]
    rng = np.random.default_rng(17)
    x0 = rng.standard_normal((3, d))
    x0[1] *= 1e6
    th0 = rng.choice([-1.0, 1.0], (3, d))
    c = np.full(d, 1e-12)
    return G, x0, th0, c


def test_violated_chain_returns_before_its_loop(gpu_pkg):
    pkg = gpu_pkg
    G, x0, th0, c = _violation_case(pkg)
    d = G.shape[0]
    seed0, T1, T = 1800, 0.5, 1.0
    refs = [O.spdmp_zigzag(G, None, G, x0[k], th0[k], c, T, seed=seed0 + k, stop_before_T=True, tracked=True) for k in range(3)]
    assert refs[0]["status"] == 0 and refs[2]["status"] == 0 and refs[1]["status"] == O.ORC_BOUND_VIOLATED
    assert refs[1]["t"].max() < T1  # (violated inside the first slice)
    with pkg.Ensemble(3, d, trace_capacity=4 * d) as e:
        e.debug_set_helper_wave(0)
        e.debug_set_prio_policy(1)
        e.set_flow(pkg.ZigZag(G, np.zeros(d)))
        e.set_target(pkg.GaussianTarget(G))
        e.set_gradient_tracking(True)
        e.set_state(0.0, x0, th0, c, np.arange(3, dtype=np.uint64) + np.uint64(seed0))
        e.run(T1, pkg._lib.RUN_STOP_BEFORE)
        assert e.kernel_name() == "zz_local_trackp_kernel"
        cn1, fs1 = e.counters(), e.final_state()
        assert list(cn1["status"]) == [pkg._lib.CHAIN_OK, pkg._lib.CHAIN_BOUND_VIOLATED, pkg._lib.CHAIN_OK]
        ev1 = e.trace(1, counters=cn1)
        e.run(T, pkg._lib.RUN_STOP_BEFORE)  # (chain 1 returns before the loop: it never touches the board)
        cn, fs = e.counters(), e.final_state()
        assert list(cn["status"]) == [pkg._lib.CHAIN_OK, pkg._lib.CHAIN_BOUND_VIOLATED, pkg._lib.CHAIN_OK]
        for f in ("num", "nacc", "nevents", "ntrace", "ndraw_main", "t_last"):
            assert cn[f][1] == cn1[f][1], f
        for f in ("t", "x", "theta", "acc"):
            assert np.array_equal(fs[f][1], fs1[f][1]), f
        r = refs[1]
        assert int(cn["num"][1]) == r["num"] and len(ev1) == len(r["events"]) and np.array_equal(ev1["t"], r["events"]["t"])
        assert np.array_equal(fs["x"][1], r["x"]) and np.array_equal(fs["t"][1], r["t"])
        for k in (0, 2):
            r = refs[k]
            ev = e.trace(k, counters=cn)
            assert len(ev) == len(r["events"]) and int(cn["num"][k]) == r["num"] and int(cn["ndraw_main"][k]) == r["ndraw_main"], k
            for f in ("i", "t", "x", "theta"):
                assert np.array_equal(ev[f], r["events"][f]), (k, f)
            assert np.array_equal(fs["t"][k], r["t"]) and np.array_equal(fs["x"][k], r["x"]) and np.array_equal(fs["theta"][k], r["theta"]), k
            assert np.array_equal(fs["acc"][k], r["acc"]), k


def test_random_graph(gpu_pkg):
    """LAT = false: the other instantiation of the one-wave form, same head, same policy."""
    pkg = gpu_pkg
    G = pkg.problems.random_sparse_precision(2048, 8)
    c = pkg.problems.column_norms(G)
    seed0, T = 1900, 2.0
    refs = [_oracle(G, c, seed0 + k, T) for k in range(3)]
    with _synthetic(pkg, G, c, 3, max(len(r["events"]) for r in refs) + 64, seed0, 1) as e:
        evs, launches = _run_and_collect(pkg, e, [(T, pkg._lib.RUN_REFERENCE_TAIL)])
        assert e.kernel_name() == "zz_local_trackp_kernel<LAT=false>" and launches == 1
        _check(pkg, e, evs, refs)


def test_big_form_keeps_its_head_and_its_turns(gpu_pkg):
    """d = 129 x 129 > 16384: 8192 block bounds, two passes over the pairs, priority in turns whatever the switch says."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(129)
    c = pkg.problems.column_norms(G)
    seed0, T = 2000, 0.05
    refs = [_oracle(G, c, seed0 + k, T) for k in range(2)]
    with _synthetic(pkg, G, c, 2, max(len(r["events"]) for r in refs) + 64, seed0, 1) as e:
        evs, _ = _run_and_collect(pkg, e, [(T, pkg._lib.RUN_REFERENCE_TAIL)])
        assert e.kernel_name() == "zz_local_trackp_big_kernel"
        assert min(len(r["events"]) for r in refs) > 100
        _check(pkg, e, evs, refs)


def test_two_ensembles_alive_at_once(gpu_pkg, lattice48):
    """Every ensemble has a board and an epoch counter of its own: runs of two ensembles in turn."""
    pkg = gpu_pkg
    G, c, refs = lattice48
    d = G.shape[0]
    with _synthetic(pkg, G, c, 3, 3 * d, SEED0, 1) as a, _synthetic(pkg, G, c, 3, 3 * d, SEED0, 1) as b:
        ev = {id(a): [[] for _ in range(3)], id(b): [[] for _ in range(3)]}
        for T in (0.5, 1.0, 1.5, 2.0):
            for e in (a, b):
                e.run(T, pkg._lib.RUN_STOP_BEFORE)
                cn = e.counters()
                assert np.all(cn["status"] == pkg._lib.CHAIN_OK)
                for k in range(3):
                    ev[id(e)][k].append(e.trace(k, counters=cn))
                e.trace_reset()
        for e in (a, b):
            _check(pkg, e, [np.concatenate(g) for g in ev[id(e)]], refs)


def test_two_wave_form_takes_the_new_head(gpu_pkg, lattice48):
    pkg = gpu_pkg
    G, c, refs = lattice48
    with _synthetic(pkg, G, c, 3, 3 * G.shape[0], SEED0, 1, helper=1) as e:
        evs, launches = _run_and_collect(pkg, e, [(2.0, pkg._lib.RUN_STOP_BEFORE)])
        assert e.kernel_name() == "zz_local_trackp2_kernel" and launches == 1
        _check(pkg, e, evs, refs)
