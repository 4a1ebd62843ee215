"""zz_partitioned_run_kernel (csrc/pdmp_partition.hip) on every row of tests/partition_cases.py, against the oracle's restatement of the reference's
parallel_spdmp (oracle/pdmp_oracle.c orc_parallel_spdmp) -- bit for bit, end states included -- against itself (a second run), and against the
path its own trace describes (no oracle).  The ensemble is driven directly, with the tables samplers.parallel_spdmp builds, so that a violated
bound and a full trace are read back instead of raised (-m gpu)."""
import numpy as np
import pytest
import scipy.sparse as sp

import oracle_lib as O
import partition_cases as PC

pytestmark = pytest.mark.gpu


def _sorted(ev):
    return ev[np.lexsort((ev["i"], ev["t"]))]  # by time (exactly tied times: by coordinate), whatever order the waves wrote them in


def device_run(pkg, c):
    """One launch of the case on a fresh ensemble: per chain the time-sorted trace, the final state and the counters."""
    L = pkg._lib
    F = pkg.ZigZag(c.Gb, np.zeros(c.d) if c.mu_b is None else c.mu_b)
    target = pkg.GaussianTarget(c.Gt, c.mu_t)
    Fu, mask = pkg.samplers.partition_tables(F, target, c.Gfull)
    ens = pkg.Ensemble(c.nchains, c.d, sampler=L.SAMPLER_ZIGZAG_LOCAL, adapt=c.adapt, factor=c.factor, trace_capacity=c.trace_capacity)
    try:
        ens.set_flow(Fu)
        ens.set_target(target)
        ens.set_state(c.t0, c.x0, c.th0, c.c, np.uint64(c.seed) + np.arange(c.nchains, dtype=np.uint64))
        ens.run_partitioned(c.T, c.K, c.delta, mask)
        cnt = ens.counters()
        evs = [_sorted(ens.trace(k, 0, int(cnt["ntrace"][k]), counters=cnt)) if c.trace_capacity and cnt["ntrace"][k]
               else np.empty(0, dtype=L.EVENT_DTYPE) for k in range(c.nchains)]
        fs = ens.final_state()
    finally:
        ens.close()
    return dict(cnt=cnt, events=evs, fs=fs)


_FIRST = {}


def first_run(pkg, name):
    if name not in _FIRST:
        _FIRST[name] = device_run(pkg, PC.case(name))
    return _FIRST[name]


def _status(pkg, c):
    L = pkg._lib
    return {PC.OK: L.CHAIN_OK, PC.VIOLATED: L.CHAIN_BOUND_VIOLATED, PC.TRACE_FULL: L.CHAIN_TRACE_FULL}[c.expect]


@pytest.mark.parametrize("name", PC.NAMES)
def test_device_equals_the_oracle(gpu_pkg, name):
    """Events, final (t, x, θ), num, nacc, status, rounds and the adapted c, bit for bit; acc[i] = the events of coordinate i."""
    c = PC.case(name)
    dev = first_run(gpu_pkg, name)
    for k in range(c.nchains):
        r = PC.reference(name, k)
        oe = _sorted(r["events"])
        cnt, ev, fs = dev["cnt"][k], dev["events"][k], dev["fs"]
        print("%-15s chain %d: events %d / %d, num %d / %d, rounds %d / %d, status %d" %
              (name, k, int(cnt["nevents"]), len(oe), int(cnt["num"]), r["num"], int(cnt["nrefresh"]), r["rounds"], int(cnt["status"])))
        assert int(cnt["status"]) == _status(gpu_pkg, c)
        assert (int(cnt["status"]) == gpu_pkg._lib.CHAIN_BOUND_VIOLATED) == (r["status"] == O.ORC_BOUND_VIOLATED)
        assert int(cnt["num"]) == r["num"] and int(cnt["nacc"]) == r["nacc"] and int(cnt["nrefresh"]) == r["rounds"]
        assert np.array_equal(fs["t"][k], r["t"]) and np.array_equal(fs["x"][k], r["x"]) and np.array_equal(fs["theta"][k], r["theta"])
        assert np.array_equal(fs["c"][k], r["c"])
        assert np.array_equal(fs["acc"][k], np.bincount(oe["i"], minlength=c.d))
        assert int(cnt["nevents"]) == len(oe) == r["nacc"]
        if c.expect == PC.TRACE_FULL:
            # which events were kept depends on the waves' timing: they are trace_capacity distinct events of the oracle's
            assert int(cnt["ntrace"]) == c.trace_capacity == len(ev) == 64
            kept, all_ = set(map(tuple, ev.tolist())), set(map(tuple, oe.tolist()))
            assert len(kept) == c.trace_capacity and kept <= all_
        elif c.trace_capacity == 0:
            assert int(cnt["ntrace"]) == 0 and len(ev) == 0 and int(cnt["nevents"]) == int(cnt["nacc"])
        else:
            assert int(cnt["ntrace"]) == len(oe) == len(ev) and len(oe) >= PC.MIN_EVENTS
            for f in ("i", "t", "x", "theta"):
                assert np.array_equal(ev[f], oe[f]), f
            assert np.array_equal(fs["acc"][k], np.bincount(ev["i"], minlength=c.d))


@pytest.mark.parametrize("name", PC.NAMES)
def test_second_run_equals_the_first(gpu_pkg, name):
    """The same case once more on a fresh ensemble: sorted events, state and counters byte for byte (the workers of a round share no data; an
    ordering missing between the waves would show here).  A full trace keeps whichever events came first: their number is compared."""
    c = PC.case(name)
    a, b = first_run(gpu_pkg, name), device_run(gpu_pkg, c)
    assert a["cnt"].tobytes() == b["cnt"].tobytes()
    for f in ("t", "x", "theta", "acc", "c"):
        assert a["fs"][f].tobytes() == b["fs"][f].tobytes(), f
    for k in range(c.nchains):
        if c.expect == PC.TRACE_FULL:
            assert len(a["events"][k]) == len(b["events"][k])
        else:
            assert a["events"][k].tobytes() == b["events"][k].tobytes()


@pytest.mark.parametrize("name", PC.NAMES)
def test_device_trace_is_on_its_own_path(gpu_pkg, name):
    """PC.check_path on the device's trace and final state: rationals, no oracle.  (A trace that overflowed or was not kept describes no path:
    there the final state is held to the path of the initial state alone where a coordinate has no event.)"""
    c = PC.case(name)
    dev = first_run(gpu_pkg, name)
    for k in range(min(c.nchains, 2)):
        cnt, ev, fs = dev["cnt"][k], dev["events"][k], dev["fs"]
        m = int(cnt["num"]) + int(cnt["nevents"]) + 1
        if int(cnt["ntrace"]) != int(cnt["nevents"]):
            still = fs["acc"][k] == 0  # coordinates without an event: straight from (t0, x0)
            assert still.any()
            idx = np.flatnonzero(still)
            PC.check_path(c.t0, c.x0[k][idx], c.th0[k][idx], ev[:0], fs["t"][k][idx], fs["x"][k][idx], fs["theta"][k][idx], m)
            continue
        worst = PC.check_path(c.t0, c.x0[k], c.th0[k], ev, fs["t"][k], fs["x"][k], fs["theta"][k], m)
        print("%-15s chain %d: largest error / bound = %.2e" % (name, k, worst))


# ------------------------------------------------------------------------------------------------------------------------------ refusals

def _lds_bytes(K, nbc):
    """zz_partitioned_lds_bytes (csrc/pdmp_partition.hip): block minima f64 and their lanes u16 per block, 56 bytes of round state per chunk, 32 more."""
    return K * nbc * 8 + K * (3 * 8 + 2 * 8 + 4 * 4) + 16 + K * nbc * 2 + 16


def _refused(pkg, code, call, *a):
    with pytest.raises(pkg._lib.PdmpError) as ei:
        call(*a)
    assert ei.value.code == code, str(ei.value)


def test_refusals_leave_the_ensemble_usable(gpu_pkg):
    """K = 0, 17, d % K != 0, Δ = 0, a mask slot outside the bound pattern that carries a bound value, a 65-entry column: each a status, and the
    valid run that follows on the same ensemble is the oracle's."""
    pkg, L = gpu_pkg, gpu_pkg._lib
    d, K, T, delta, seed = 16 * 17, 16, 4.0, 0.1, 901
    Gt = PC.tridiagonal(d)
    Gb = PC.chunk_diagonal(Gt, K)
    rng = np.random.default_rng(seed)
    x0, th0 = rng.standard_normal(d), rng.choice([-1.0, 1.0], d)
    c = 2.0 * PC.column_norms(Gt)
    r = O.parallel_spdmp(Gb, None, Gt, x0, th0, c, T, K, delta, seed=seed)
    assert r["status"] == O.ORC_OK and len(r["events"]) > 100
    target = pkg.GaussianTarget(Gt)
    Fu, mask = pkg.samplers.partition_tables(pkg.ZigZag(Gb, np.zeros(d)), target, Gt)
    bad_mask = mask.copy()
    slot = np.flatnonzero((mask != 0) & (Fu.Γ.data != 0))[1]
    bad_mask[slot] = 0
    # a column of 65 entries inside one chunk of 136 (K = 2)
    W = sp.lil_matrix((d, d))
    W.setdiag(70.0)
    W[1:65, 0] = 0.1
    W[0, 1:65] = 0.1
    W = PC._csc(W)
    assert np.diff(W.indptr).max() == 65
    ens = pkg.Ensemble(1, d, sampler=L.SAMPLER_ZIGZAG_LOCAL, trace_capacity=4096)

    def fresh(F=Fu, tg=target):
        ens.set_flow(F)
        ens.set_target(tg)
        ens.set_state(0.0, x0[None], th0[None], c, np.array([seed], dtype=np.uint64))

    def valid_run_is_the_oracles():
        ens.run_partitioned(T, K, delta, mask)
        cnt = ens.counters()
        ev = _sorted(ens.trace(0, counters=cnt))
        assert int(cnt["status"][0]) == L.CHAIN_OK and ev.tobytes() == _sorted(r["events"]).tobytes()
        assert np.array_equal(ens.final_state()["x"][0], r["x"])

    try:
        for code, args in ((L.PDMP_ERR_INVALID, (T, 0, delta, mask)), (L.PDMP_ERR_INVALID, (T, 17, delta, mask)),
                           (L.PDMP_ERR_INVALID, (T, 3, delta, mask)), (L.PDMP_ERR_INVALID, (T, K, 0.0, mask)),
                           (L.PDMP_ERR_INVALID, (T, K, delta, bad_mask))):
            fresh()
            _refused(pkg, code, ens.run_partitioned, *args)
            valid_run_is_the_oracles()  # (no set_state in between: the refusal left the fresh state alone)
        Fw, mw = pkg.samplers.partition_tables(pkg.ZigZag(W, np.zeros(d)), pkg.GaussianTarget(W), None)
        fresh(Fw, pkg.GaussianTarget(W))
        _refused(pkg, L.PDMP_ERR_UNSUPPORTED, ens.run_partitioned, T, 2, delta, mw)
        fresh()
        valid_run_is_the_oracles()
    finally:
        ens.close()


def test_lds_limit(gpu_pkg):
    """The chunk queues of a workgroup must fit 64 KiB of LDS.  From zz_partitioned_lds_bytes: at K = 16 the first nbc beyond it is 404, so
    k = 403·64 + 1 is refused; the same d as ONE chunk (nbc = 6449, 64578 bytes) fits and runs, and equals the oracle."""
    pkg, L = gpu_pkg, gpu_pkg._lib
    nbc = next(n for n in range(1, 1 << 12) if _lds_bytes(16, n) > 64 * 1024)
    assert nbc == 404 and _lds_bytes(16, nbc - 1) <= 64 * 1024
    k = (nbc - 1) * 64 + 1
    d = 16 * k
    assert _lds_bytes(1, -(-d // 64)) <= 64 * 1024
    T, delta, seed = 0.002, 0.0005, 77
    Gt = PC.tridiagonal(d)
    rng = np.random.default_rng(seed)
    x0, th0 = rng.standard_normal(d), rng.choice([-1.0, 1.0], d)
    c = 2.0 * PC.column_norms(Gt)
    ens = pkg.Ensemble(1, d, sampler=L.SAMPLER_ZIGZAG_LOCAL, trace_capacity=1 << 14)
    try:
        ens.set_flow(pkg.ZigZag(PC.chunk_diagonal(Gt, 16), np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(PC.chunk_diagonal(Gt, 16)))
        ens.set_state(0.0, x0[None], th0[None], c, np.array([seed], dtype=np.uint64))
        _refused(pkg, L.PDMP_ERR_UNSUPPORTED, ens.run_partitioned, T, 16, delta)
        ens.run_partitioned(T, 1, delta)
        cnt = ens.counters()
        ev = _sorted(ens.trace(0, counters=cnt))
        fs = ens.final_state()
    finally:
        ens.close()
    Gc = PC.chunk_diagonal(Gt, 16)
    r = O.parallel_spdmp(Gc, None, Gc, x0, th0, c, T, 1, delta, seed=seed)
    assert int(cnt["status"][0]) == L.CHAIN_OK and r["status"] == O.ORC_OK and len(r["events"]) > 100
    assert ev.tobytes() == _sorted(r["events"]).tobytes() and np.array_equal(fs["x"][0], r["x"]) and np.array_equal(fs["t"][0], r["t"])
    assert int(cnt["num"][0]) == r["num"] and int(cnt["nrefresh"][0]) == r["rounds"]
