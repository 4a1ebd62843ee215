"""The common path of the one-proposal-per-lane tracked kernel's iteration without the instructions that computed nothing (-m gpu): the re-basing
of the level-1 bounds ends its iteration (the next one reads the new bounds back), the selection's mask pass takes the sign bit of a difference,
and a candidate's eight pair loads are issued by every lane, without a branch around each.  None of it may show in what a chain computes: every
case forces the form on its own ensemble and holds the complete trace, the final state and the counters of every chain to the oracle's tracked
evaluation, bit for bit.

The base of the bounds lags the front by at most 0.25 of process time, so a launch over three units re-bases at least ten times, wherever its
pauses and slice ends fall; a launch shorter than 0.25 never does.  The mask pass is also called alone, by a probe of the parity build, on a table
of thresholds and entries around them."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

P_INFBITS = 0x7F7FFFF8
SELECT_P_MASK32 = 11  # include/pdmp_debug.h: PDMP_SELECT_P_MASK32


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


def _synthetic(pkg, G, c, nch, cap, seed0, helper, t0=0.0):
    d = G.shape[0]
    e = pkg.Ensemble(nch, d, trace_capacity=cap)
    e.debug_set_helper_wave(helper)
    e.set_flow(pkg.ZigZag(G, np.zeros(d)))
    e.set_target(pkg.GaussianTarget(G))
    e.set_gradient_tracking(True)
    e.set_state_synthetic(t0, c, seed0)
    return e


def _refs(G, c, nch, seed0, T, t0=0.0, stop_before=False):
    out = []
    for k in range(nch):
        x0, th0 = O.synthetic_state(seed0 + k, G.shape[0])
        out.append(O.spdmp_zigzag(G, None, G, x0, th0, c, T, t0=t0, seed=seed0 + k, stop_before_T=stop_before, tracked=True))
    return out


def _name(helper, lat=True):
    return ("zz_local_trackp2_kernel" if helper else "zz_local_trackp_kernel") + ("" if lat else "<LAT=false>")


def _cap(refs):
    return max(len(r["events"]) for r in refs) + 64


SEED48, T48 = 2100, 3.0


@pytest.fixture(scope="module")
def lattice48(gpu_pkg):
    """The 48 x 48 lattice, three chains, and the oracle's tracked runs to T = 3 stopping before T and with the reference's tail (computed once,
    read only)."""
    G = gpu_pkg.problems.gmrf_precision(48)
    c = gpu_pkg.problems.column_norms(G)
    return G, c, {False: _refs(G, c, 3, SEED48, T48), True: _refs(G, c, 3, SEED48, T48, stop_before=True)}


@pytest.mark.parametrize("helper", [0, 1])
@pytest.mark.parametrize("stop_before", [True, False])
def test_rebasing_inside_a_launch(gpu_pkg, lattice48, helper, stop_before):
    """One launch from 0 to 3: the base moves up at least ten times inside it."""
    pkg = gpu_pkg
    G, c, refs = lattice48
    flag = pkg._lib.RUN_STOP_BEFORE if stop_before else pkg._lib.RUN_REFERENCE_TAIL
    with _synthetic(pkg, G, c, 3, _cap(refs[stop_before]), SEED48, helper) as e:
        evs, launches = _run_and_collect(pkg, e, [(T48, flag)])
        assert e.kernel_name() == _name(helper) and launches == 1
        assert min(len(r["events"]) for r in refs[stop_before]) > 1000
        _check(pkg, e, evs, refs[stop_before])


@pytest.mark.parametrize("helper", [0, 1])
@pytest.mark.parametrize("cap", [700, 150])
def test_rebasing_next_to_launch_ends(gpu_pkg, lattice48, helper, cap):
    """The same run in ten slices of 0.3 with a trace segment of 700 events, and of 150, which fills up inside every slice: slice ends and pauses
    fall at arbitrary distances from an iteration that re-bases, and the launch after one starts from the pairs again."""
    pkg = gpu_pkg
    G, c, refs = lattice48
    slices = [(0.3 * k, pkg._lib.RUN_STOP_BEFORE) for k in range(1, 10)] + [(T48, pkg._lib.RUN_STOP_BEFORE)]
    with _synthetic(pkg, G, c, 3, cap, SEED48, helper) as e:
        evs, launches = _run_and_collect(pkg, e, slices)
        assert e.kernel_name() == _name(helper)
        assert launches >= max(10, max(len(r["events"]) for r in refs[True]) // cap)
        _check(pkg, e, evs, refs[True])


@pytest.mark.parametrize("helper", [0, 1])
def test_rebasing_between_pauses_of_one_slice(gpu_pkg, lattice48, helper):
    """One slice to T = 3 with the reference's tail and a trace segment of 700 events: every resumed launch re-bases on its own."""
    pkg = gpu_pkg
    G, c, refs = lattice48
    with _synthetic(pkg, G, c, 3, 700, SEED48, helper) as e:
        evs, launches = _run_and_collect(pkg, e, [(T48, pkg._lib.RUN_REFERENCE_TAIL)])
        assert e.kernel_name() == _name(helper)
        assert launches > max(len(r["events"]) for r in refs[False]) // 700  # (the trace filled up)
        _check(pkg, e, evs, refs[False])


@pytest.mark.parametrize("helper", [0, 1])
def test_start_time_five(gpu_pkg, helper):
    """t0 = 5: the first keys lie before t0 (the reference's initial keys carry no t0), the base starts below them and is moved past t0 by the
    first re-basing."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(48)
    c = pkg.problems.column_norms(G)
    seed0, t0, T = 2200, 5.0, 6.5
    refs = _refs(G, c, 3, seed0, T, t0=t0)
    with _synthetic(pkg, G, c, 3, _cap(refs), seed0, helper, t0=t0) as e:
        evs, launches = _run_and_collect(pkg, e, [(T, pkg._lib.RUN_REFERENCE_TAIL)])
        assert e.kernel_name() == _name(helper) and launches == 1
        assert min(len(r["events"]) for r in refs) > 500
        _check(pkg, e, evs, refs)


@pytest.mark.parametrize("helper", [0, 1])
def test_random_graph(gpu_pkg, helper):
    """LAT = false: a random symmetric pattern with at most six entries per column at d = 2048 -- the loads without a branch and the re-basing
    that ends its iteration on the generic instantiation."""
    pkg = gpu_pkg
    G = pkg.problems.random_sparse_precision(2048, 6)
    c = pkg.problems.column_norms(G)
    seed0, T = 2300, 2.0
    refs = _refs(G, c, 3, seed0, T)
    with _synthetic(pkg, G, c, 3, _cap(refs), seed0, helper) as e:
        evs, launches = _run_and_collect(pkg, e, [(T, pkg._lib.RUN_REFERENCE_TAIL)])
        assert e.kernel_name() == _name(helper, lat=False) and launches == 1
        assert min(len(r["events"]) for r in refs) > 500
        _check(pkg, e, evs, refs)


@pytest.mark.parametrize("helper", [0, 1])
def test_odd_lattice(gpu_pkg, helper):
    """47 x 47: 277 blocks, no multiple of 64 -- most of the 2048 level-1 entries are the empty pattern, and the mask pass meets it in every lane."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(47)
    c = pkg.problems.column_norms(G)
    seed0, T = 2400, 2.0
    refs = _refs(G, c, 3, seed0, T)
    with _synthetic(pkg, G, c, 3, _cap(refs), seed0, helper) as e:
        evs, launches = _run_and_collect(pkg, e, [(T, pkg._lib.RUN_REFERENCE_TAIL)])
        assert e.kernel_name() == _name(helper) and launches == 1
        assert min(len(r["events"]) for r in refs) > 500
        _check(pkg, e, evs, refs)


def test_big_form(gpu_pkg):
    """d = 129 x 129 > 16384: zz_local_trackp_big_kernel re-bases its four chunks of 2048 bounds and ends the iteration in the same way."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(129)
    c = pkg.problems.column_norms(G)
    seed0, T = 2500, 0.5
    refs = _refs(G, c, 2, seed0, T)
    with _synthetic(pkg, G, c, 2, _cap(refs), seed0, 0) as e:
        evs, launches = _run_and_collect(pkg, e, [(T, pkg._lib.RUN_REFERENCE_TAIL)])
        assert e.kernel_name() == "zz_local_trackp_big_kernel" and launches == 1
        assert min(len(r["events"]) for r in refs) > 1000
        _check(pkg, e, evs, refs)


def test_mask_pass_on_a_table(gpu_pkg_parity):
    """p_mask32, the helper the loop calls, against numpy's kk <= thr bit for bit: every threshold of the table with every entry of the table at
    every one of the 32 positions, the other 31 entries alternating between 0 (always within) and 0x7f7fffff (never)."""
    thrs = [7, 8, 0x3F000000, P_INFBITS - 1]
    rows = []
    for thr in thrs:
        for ent in (0, thr - 1, thr, thr + 1, P_INFBITS, 0x7F7FFFFF):
            for pos in range(32):
                rows.append((thr, ent, pos))
    a, b, c = (np.array(v, dtype=np.float64) for v in zip(*rows))
    dev = gpu_pkg_parity._lib.queue_eval(SELECT_P_MASK32, a, b, c)[0]
    j = np.arange(32)
    for (thr, ent, pos), got in zip(rows, dev):
        kk = np.where(j == pos, ent, np.where(j & 1, 0, 0x7F7FFFFF)).astype(np.uint64)
        want = int(((kk <= thr).astype(np.uint64) << j.astype(np.uint64)).sum())
        assert int(got) == want, (hex(thr), hex(ent), pos, hex(int(got)), hex(want))
