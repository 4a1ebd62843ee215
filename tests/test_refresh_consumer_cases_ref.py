"""The host statements of the FactTrace consumers on the unsorted hand-made traces of tests/refresh_consumer_cases.py, held to each other without a
device: trace.py (vectorised numpy), tests/ref/refresh_trace_ref.c (the closed form in the arithmetic of the unordered walk of
csrc/pdmp_consume.hip, and the reference's iterator restated step by step) and oracle/trace_oracle.c (the iterator for the linear flow).
tests/test_gpu_refresh_consumers.py then holds the device to the closed form bit for bit.

ZigZag rows: trace.discretize equals the closed form bit for bit, grid times always; both agree with the oracle's stepping within the atol of
tests/test_gpu_consumers.py (times 1e-10, rows 1e-9), bit for bit on the dyadic cases.  mean / cummean: rtol = 1e-12, atol = 1e-15.
FactBoomerang rows: the closed form (pdmp_sincos, one rotation from the cursor) against the step-by-step restatement (libm, every event a
rotation of every coordinate, backward steps included) within SINCOS_ABS · max(|x − μ| + |θ|) · steps -- the form and constant of
test_boomerang_rows_within_the_sincos_bound (tests/test_pdmp_consumer_cases_ref.py), times the number of rotations an entry went through."""
import numpy as np
import pytest

import oracle_lib as O
import refresh_consumer_cases as RC
import refresh_trace_ref_lib as R
from test_detmath_accuracy import SINCOS_ABS

TOL = dict(rtol=1e-12, atol=1e-15)  # the project's tolerance for mean / cummean (tests/test_gpu_consumers_synthetic.py)
ORACLE_T, ORACLE_X = 1e-10, 1e-9    # tests/test_gpu_consumers.py: the device's grid against oracle_lib.trace_discretize


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def oracle_discretize(c):
    """oracle/trace_oracle.c::orc_trace_discretize on the case's trace (oracle_lib.trace_discretize sizes its buffers by the LAST event's time,
    which on a trace that ends on a stale event is not the largest)"""
    import ctypes as C
    et, ei, ex, eth = O._ev_arrays(c.events)
    x0, th0 = np.ascontiguousarray(c.x0, dtype=np.float64), np.ascontiguousarray(c.th0, dtype=np.float64)
    cap = int((et.max() - c.t0) / c.dt) + 8
    ts, xs = np.empty(cap), np.empty((cap, c.d))
    L = O.lib()
    L.orc_trace_discretize.restype = C.c_int64
    L.orc_trace_discretize.argtypes = [C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_double, C.c_int64, C.c_void_p, C.c_void_p]
    q = L.orc_trace_discretize(c.d, float(c.t0), x0.ctypes.data, th0.ctypes.data, et.size, et.ctypes.data, ei.ctypes.data, ex.ctypes.data, eth.ctypes.data,
                               float(c.dt), cap, ts.ctypes.data, xs.ctypes.data)
    assert 0 < q <= cap
    return ts[:q].copy(), xs[:q].copy()


def host_trace(pkg, c, upto=None):
    F = pkg.FactBoomerang(np.eye(c.d), c.mu, 0.1) if c.mu is not None else None
    return pkg.FactTrace(F, c.t0, c.x0, c.th0, c.events if upto is None else c.events[:upto])


def test_the_table_holds_what_it_says():
    assert RC.EVENT_DTYPE.itemsize == 32
    for name in RC.NAMES:
        c = RC.case(name)
        ev = c.events
        assert c.dyadic == (name in RC.DYADIC) and (c.mu is not None) == (name in RC.BOOM)
        assert RC.own_order_kept(ev, c.d), name                      # the property the consumers rely on (tests/exact_path.py)
        assert (RC.stale_events(ev) > 0) == c.stale, name            # every row with stale events in it has them
        assert c.stale == (name != "d1")
        assert ev["t"][0] > c.t0 and not np.any(ev["t"] == 0.0)
        assert c.cuts[0] == 0 and c.cuts[-1] == len(ev) <= c.trace_capacity and np.all(np.diff(c.cuts) >= 0)
        assert (RC.reference(name)["npoints"] > c.K) == (name == "short_grid")
    b = RC.case("bsearch")
    assert b.events["t"].tolist() == [1.0, 9.0, 2.0, 3.0, 4.0] and b.t0 + b.dt == 5.0
    r = RC.reference("bsearch")
    assert r["npoints"] == 2 and r["T"] == 4.0 and r["t_max"] == 9.0  # the trace ends on a stale event
    assert np.searchsorted(b.events["t"], 5.0, side="right") == 5      # (what a binary search makes of it: all five events)
    j = int(b.events["i"][0])  # row 5 shows the first event only: coordinate j from it, the others from (t0, x0, θ0)
    want = b.x0 + b.th0 * 5.0
    want[j] = b.events["x"][0] + b.events["theta"][0] * (5.0 - 1.0)
    assert same_bits(r["grid"][1], want)
    c = RC.case("behind_row")
    r = RC.reference("behind_row")
    assert same_bits(r["grid"][1, 1], c.x0[1] + c.th0[1] * 1.0)                                      # the stale event is not in the row before it
    assert same_bits(r["grid"][2, 1], c.events["x"][1] + c.events["theta"][1] * (2.0 - 0.25))        # ... and is in the next
    assert c.events["theta"][1] == -c.th0[1] and same_bits(RC.reference("behind_row", 1)["grid"][1], r["grid"][1])
    c = RC.case("slice_edges")
    tm = np.maximum.accumulate(c.events["t"])
    assert c.cuts[1] == 8 and c.events["t"][7] < tm[6] and c.events["t"][8] < tm[7]
    for name in ("ends_stale", "d256"):
        r = RC.reference(name)
        assert r["T"] == RC.case(name).events["t"][-1] < r["t_max"]
    assert sorted(np.diff(RC.case("tiny").cuts))[:4] == [0, 0, 0, 1]
    assert [len(RC.case(n).events) for n in ("n255", "n256", "n257", "n513")] == [255, 256, 257, 513]
    assert [RC.case(n).d for n in ("d1", "d255", "d256", "d257")] == [1, 255, 256, 257]
    c = RC.case("far_split")
    first = int(np.argmax(c.events["t"] > c.t0 + c.dt))
    assert first == 600 and RC.stale_events(c.events[:600]) > 100
    c = RC.case("one_coord")
    assert np.all(c.events["i"][1:301] == 0) and np.all(c.events["t"][1:301] < c.events["t"][0])
    c = RC.case("on_grid")
    g = c.t0 + c.dt * np.arange(c.K)
    assert np.isin(c.events["t"], g).sum() >= 5 and np.isin(c.events["t"], np.nextafter(g, np.inf)).sum() >= 5
    assert RC.reference("many_rows")["npoints"] > 300
    assert RC.case("neg_t0").t0 < 0
    c = RC.case("t0_shift")
    assert c.t0 == 2.0 and c.events["t"][c.events["i"] == 1][0] < c.t0
    c = RC.case("boom")
    assert np.any(c.mu != 0)
    tau = []  # τ of every entry of every row: g − (the coordinate's cursor time)
    ct = np.full(c.d, c.t0)
    k = 0
    for t2, i in zip(c.events["t"], c.events["i"]):
        while c.t0 + c.dt * k < t2:
            tau += list(c.t0 + c.dt * k - ct)
            k += 1
        ct[i] = t2
    assert 0 < min(abs(v) for v in tau if v != 0.0) < 2e-9 and max(tau) > 6 * np.pi


@pytest.mark.parametrize("name", RC.NAMES)
def test_trace_py_agrees_with_the_c_statement(pkg, name):
    c = RC.case(name)
    for upto in sorted({len(c.events)} | set(c.cuts[1:])):
        if upto == 0:
            r = RC.reference(name, 0)
            assert r["npoints"] == 1 and r["T"] == c.t0 and same_bits(r["grid"][0], c.x0) and not r["grid"][1:].any()
            continue
        r = RC.reference(name, upto)
        ev = c.events[:upto]
        tr = host_trace(pkg, c, upto)
        assert r["T"] == ev["t"][-1] and r["t_max"] == ev["t"].max()
        assert np.allclose(pkg.trace.mean(tr), r["mean"], **TOL)
        cm = pkg.trace.cummean(tr)
        for j in range(c.d):
            own = ev["i"] == j
            assert same_bits(cm[j][0][1:], r["cummean_t"][own]) and np.allclose(cm[j][1][1:], r["cummean_y"][own], **TOL)
        if c.dyadic:  # (the sums are exact; mean scales them by 1/(2T) once here and term by term there)
            assert all(same_bits(cm[j][1][1:], r["cummean_y"][ev["i"] == j]) for j in range(c.d))
        grid, X = pkg.trace.discretize(tr, c.dt)
        n = min(r["npoints"], c.K)
        assert len(grid) == r["npoints"] and same_bits(grid[:n], r["grid_t"])  # grid times: always bit for bit
        assert not r["grid"][n:].any()
        if c.mu is None:
            assert same_bits(X[:n], r["grid"][:n])
        else:  # (np.sin / np.cos against pdmp_sincos: the values are held by test_boomerang_rows_against_the_iterator)
            assert np.allclose(X[:n], r["grid"][:n], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", [n for n in RC.NAMES if n not in RC.BOOM])
def test_zigzag_rows_agree_with_the_oracle_iterator(name):
    """oracle/trace_oracle.c::orc_trace_discretize restates Base.iterate(::Discretize{<:FactTrace}) line by line and takes unsorted traces as it
    is: the same rows at the same times, the same number of them."""
    c = RC.case(name)
    r = RC.reference(name)
    ts, xs = oracle_discretize(c)
    n = min(r["npoints"], c.K)
    assert len(ts) == r["npoints"]
    assert np.allclose(ts[:n], r["grid_t"], rtol=0, atol=ORACLE_T) and np.allclose(xs[:n], r["grid"][:n], rtol=0, atol=ORACLE_X)
    if c.dyadic:
        assert same_bits(ts[:n], r["grid_t"]) and same_bits(xs[:n], r["grid"][:n])
    assert np.allclose(r["mean"], O.trace_mean(c.t0, c.x0, c.events), **TOL)
    ot, oy = O.trace_cummean(c.t0, c.x0, c.events)
    assert same_bits(ot, r["cummean_t"]) and same_bits(oy, r["cummean_y"])


def test_the_step_by_step_iterator_is_the_oracle_on_the_linear_flow():
    """ref_refresh_steps with mu = NULL is orc_trace_discretize in other words: bit for bit, on every ZigZag row of the table"""
    for name in RC.NAMES:
        c = RC.case(name)
        if c.mu is not None:
            continue
        ts, xs = oracle_discretize(c)
        st, sx, _ = R.steps(c.t0, c.x0, c.th0, c.events, c.dt)
        assert same_bits(st, ts) and same_bits(sx, xs), name


@pytest.mark.parametrize("name", RC.BOOM)
def test_boomerang_rows_against_the_iterator(name):
    """The closed form (one pdmp_sincos rotation from the coordinate's cursor) against the reference's iterator restated step by step (libm's
    sin / cos; every step rotates every coordinate, a stale event steps back and on again).  Entry by entry:
        |row(closed form) − row(iterator)| <= SINCOS_ABS · M · max(steps, 1),
    SINCOS_ABS = 2.5e-16 the absolute error tests/test_detmath_accuracy.py holds pdmp_sincos to, M = the largest |x − μ| + |θ| over the initial
    state and the events (the maximum norm, as in test_boomerang_rows_within_the_sincos_bound), steps = the move_forward! calls the entry went
    through since its coordinate's last event.

    Measured (the test prints them): boom -- largest difference 3.11e-15, largest error / bound 0.30 (8.88e-16 after 3 steps against
    2.5e-16 · 4.00 · 3 = 3.0e-15); boom_dyadic -- largest difference 1.33e-15, largest error / bound 0.26 (6.66e-16 after 3 steps against
    2.5e-16 · 3.49 · 3 = 2.6e-15)."""
    c = RC.case(name)
    r = RC.reference(name)
    ts, xs, steps = R.steps(c.t0, c.x0, c.th0, c.events, c.dt, mu=c.mu)
    n = min(r["npoints"], c.K)
    assert len(ts) == r["npoints"] and np.allclose(ts[:n], r["grid_t"], rtol=0, atol=ORACLE_T)
    M = max(float(np.max(np.abs(c.x0 - c.mu) + np.abs(c.th0))), float(np.max(np.abs(c.events["x"] - c.mu[c.events["i"]]) + np.abs(c.events["theta"]))))
    err = np.abs(xs[:n] - r["grid"][:n])
    bound = SINCOS_ABS * M * np.maximum(steps[:n], 1)
    at = np.unravel_index(np.argmax(err / bound), err.shape)
    print("%s: largest |closed form - iterator| = %.3g; largest error / bound = %.3g (error %.3g, %d steps, bound %.3g * %.3g * steps = %.3g)"
          % (name, err.max(), (err / bound).max(), err[at], steps[:n][at], SINCOS_ABS, M, bound[at]))
    assert np.all(err <= bound), (float((err / bound).max()), at)
    assert err.max() > 0.0  # (the two sides do differ: the comparison is not vacuous)
