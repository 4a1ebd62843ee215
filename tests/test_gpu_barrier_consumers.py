"""The device trace consumers of a barrier ensemble (stickyzz / sspdmp2: Ensemble.barrier_consume_begin, csrc/pdmp_consume.hip) and the barrier
occupation (-m gpu): (a) the hand-made table of tests/barrier_consumer_cases.py through pdmp_debug_trace_append, (b) real runs consumed slice
by slice against the host mirrors of zigzagboomerang.jl_amd/trace.py applied to the trace copied out slice by slice, (c) calls and refusals,
(d) the consume= keyword of stickyzz and sspdmp2.

The host mirrors take the trace started at (t0, x0, θ_eff) -- trace.barrier_start: θ = 0 where a coordinate starts frozen --, the path the
chain travelled.  mean: the device scales the summed trapezoid terms once, trace.mean scales every term; bit for bit it is held to the host loop
in the device's documented arithmetic (tests/consumer_cases.mean_loop, as tests/test_gpu_consumers_synthetic.py does) and to trace.mean within
that file's tolerance; on the dyadic case table all three agree bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sp

import barrier_consumer_cases as B
import consumer_cases as CC
import stickyzz_cases as K
import stickyzz_ref_lib as R

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-12, atol=1e-15)  # tests/test_gpu_consumers_synthetic.py's tolerance for mean against trace.py


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def open_ens(pkg, p, cap, seed):
    """A barrier ensemble in the start state of problem p: nothing has run"""
    L = pkg._lib
    nch, d = p["x0"].shape
    ens = pkg.Ensemble(nch, d, sampler=L.SAMPLER_BARRIER_ZIGZAG, factor=1.5, trace_capacity=cap)
    ens.set_flow(pkg.ZigZag(p["G"], np.zeros(d)))
    ens.set_target(pkg.GaussianTarget(p["Gt"], p["mu_t"]))
    ens.set_barriers(*R.barrier_table(p["bar"], d))
    ens.set_state(p["t0"], p["x0"], p["th0"], p["c"], np.uint64(seed) + np.arange(nch, dtype=np.uint64))
    return ens


def table_problem():
    G = sp.identity(B.D, format="csc")
    return dict(G=G, Gt=G, mu_t=None, bar=B.BARRIERS, t0=B.T0, x0=B.X0, th0=B.TH0, c=np.ones(B.D))


def problem(name):
    if name in ("box1d", "sticky1d"):
        one, two = sp.csc_matrix(np.array([[1.0]])), sp.csc_matrix(np.array([[2.0]]))
        return dict(G=one, Gt=two, mu_t=np.array([0.9]), bar=K.BOX_1D if name == "box1d" else K.STICKY_1D, t0=0.0,
                    x0=np.array([[1.0], [0.3], [1.0]]), th0=np.array([[0.8], [-1.0], [-0.8]]), c=np.array([20.0]), T=300.0, dt=0.5)
    G = K.precision8()
    bar = K.mixed_barriers(8)
    x0, th0 = K.state8(3)
    x0 = K.fit_state(x0, bar)
    x0[:, 4] = np.where(th0[:, 4] > 0, 0.5, -1.0)  # coordinate 4 starts frozen on the barrier of its direction ((−1, 0.5), sticky)
    return dict(G=0.9 * G, Gt=G, mu_t=None, bar=bar, t0=0.0, x0=x0, th0=th0, c=K.c8(G), T=30.0, dt=0.25)


def run_sliced(pkg, ens, T, each_slice=None):
    """run -> consume -> copy the slice out -> reset, until every chain is past T; returns the events per chain and the number of slices"""
    L = pkg._lib
    parts = [[] for _ in range(ens.nchains)]
    nslices = 0
    while True:
        ens.run(T)
        cnt = ens.counters()
        assert not np.any(cnt["status"] == L.CHAIN_BOUND_VIOLATED)
        ens.consume()
        for k in range(ens.nchains):
            parts[k].append(ens.trace(k, counters=cnt))
        if each_slice is not None:
            each_slice(nslices, cnt)
        ens.trace_reset()
        nslices += 1
        if not L.needs_rerun(cnt["status"]):
            break
    return [np.concatenate(p) for p in parts], nslices


def check_against_mirrors(pkg, ens, p, events, grid):
    """mean, T, grid and occupation of every chain against the host mirrors on the θ_eff-started trace"""
    mean, T = ens.consume_mean()
    zl, zh, nl, nh, To = ens.barrier_consume_occupation()
    th_eff, _ = pkg.trace.barrier_start(p["x0"], p["th0"], p["bar"])
    for k, ev in enumerate(events):
        tr = pkg.FactTrace(None, p["t0"], p["x0"][k], th_eff[k], ev)
        assert T[k] == To[k] == ev["t"][-1]
        loop, _ = CC.mean_loop(p["t0"], p["x0"][k], ev)
        assert same_bits(mean[k], loop) and np.allclose(mean[k], pkg.trace.mean(tr), **TOL)
        hzl, hzh, hnl, hnh, hT = pkg.trace.barrier_occupation(ev, p["t0"], p["x0"][k], p["th0"][k], p["bar"])
        assert same_bits(zl[k], hzl) and same_bits(zh[k], hzh) and np.array_equal(nl[k], hnl) and np.array_equal(nh[k], hnh) and hT == To[k]
        if grid:
            gt, gx = ens.consume_discretized(k)
            ht, hx = pkg.trace.discretize(tr, p["dt"])
            assert same_bits(gt, ht) and same_bits(gx, hx) and len(gt) > 20
    return zl, zh, nl, nh


# ------------------------------------------------------------------------------------------------------------------ (a) the case table
def test_case_table_through_trace_append(gpu_pkg):
    pkg = gpu_pkg
    assert B.EVENT_DTYPE == pkg._lib.EVENT_DTYPE
    p = table_problem()
    with open_ens(pkg, p, B.TRACE_CAPACITY, 1) as ens:
        ens.barrier_consume_begin(B.DT, B.K)
        ens.consume_cummean(True)
        cm = [[] for _ in range(B.NCHAINS)]
        for s in range(B.NSEG):
            for k in range(B.NCHAINS):
                ens.debug_trace_append(k, B.segment(k, s))
            ens.consume()
            mean, T = ens.consume_mean()
            zl, zh, nl, nh, To = ens.barrier_consume_occupation()
            for k in range(B.NCHAINS):
                ev = B.so_far(k, s)
                tr = pkg.FactTrace(None, B.T0, B.X0[k], B.TH_EFF[k], ev)
                assert T[k] == To[k] == ev["t"][-1]
                assert same_bits(mean[k], CC.mean_loop(B.T0, B.X0[k], ev)[0]) and np.allclose(mean[k], pkg.trace.mean(tr), **TOL)
                if s == B.NSEG - 1:  # (1 / (2 T_last) = 1/8: scaling every term or the sum is the same number)
                    assert same_bits(mean[k], pkg.trace.mean(tr))
                gt, gx = ens.consume_discretized(k)
                ht, hx = pkg.trace.discretize(tr, B.DT)
                assert same_bits(gt, ht) and same_bits(gx, hx)
                hz = pkg.trace.barrier_occupation(ev, B.T0, B.X0[k], B.TH0[k], B.BARRIERS)
                assert same_bits(zl[k], hz[0]) and same_bits(zh[k], hz[1]) and np.array_equal(nl[k], hz[2]) and np.array_equal(nh[k], hz[3])
                seg = B.segment(k, s)
                cm[k].append(ens.consume_cummean_pairs(k, len(seg)))
                assert np.array_equal(ens.subtrace(k, [1, 3])["t"], seg["t"][np.isin(seg["i"], [1, 3])])
            ens.trace_reset()
        # the hand values
        assert same_bits(mean, B.MEAN) and same_bits(T, B.T_LAST)
        assert same_bits(zl, B.FROZEN_LO) and same_bits(zh, B.FROZEN_HI) and np.array_equal(nl, B.HITS_LO) and np.array_equal(nh, B.HITS_HI)
        assert nl.dtype == nh.dtype == np.uint64
        for k in range(B.NCHAINS):
            gt, gx = ens.consume_discretized(k)
            assert same_bits(gt, B.GRID_T) and same_bits(gx, B.GRID_X[k])
            # cummean: the pairs beside the events, coordinate by coordinate those of trace.cummean
            ct = np.concatenate([c[0] for c in cm[k]])
            cy = np.concatenate([c[1] for c in cm[k]])
            want = pkg.trace.cummean(pkg.FactTrace(None, B.T0, B.X0[k], B.TH_EFF[k], B.EVENTS[k]))
            for j in range(B.D):
                own = B.EVENTS[k]["i"] == j
                assert same_bits(ct[own], want[j][0][1:]) and same_bits(cy[own], want[j][1][1:])


# ------------------------------------------------------------------------------------------------------------------ (b) real runs
@pytest.mark.parametrize("name", ["box1d", "sticky1d", "d8"])
def test_real_runs_slice_by_slice(gpu_pkg, name):
    """trace_capacity = 64: several slices, so cursors, sides and counts carry across them"""
    pkg = gpu_pkg
    p = problem(name)
    with open_ens(pkg, p, 64, 7) as ens:
        ens.barrier_consume_begin(p["dt"], int(p["T"] / p["dt"]) + 64)
        events, nslices = run_sliced(pkg, ens, p["T"])
        assert nslices >= 3 and ens.kernel_name() == "zz_barrier_run_kernel"
        zl, zh, nl, nh = check_against_mirrors(pkg, ens, p, events, grid=True)
    assert np.all((nl + nh).sum(axis=1) > 5)
    if name == "box1d":
        assert not zl.any() and not zh.any()  # walls: hits, no time
    else:
        assert np.all((zl + zh).sum(axis=1) > 0)
    if name == "d8":  # the frozen start counts from t0 on the side of θ0; a coordinate without barriers never freezes
        up = p["th0"][:, 4] > 0
        assert np.all(np.where(up, zh[:, 4], zl[:, 4]) > 0) and not zl[:, 0].any() and not nh[:, 0].any()


def test_long_1d_run_fills_whole_chunks_of_one_coordinate(gpu_pkg):
    """d = 1, trace_capacity = 1024 and a run of more than 1024 events, no grid: the first slice reaches the consumer as full chunks of 256
    events of ONE coordinate, the fully serialised ordered rounds (with hit / thaw pairs at one time among them)."""
    pkg = gpu_pkg
    p = problem("box1d")
    p["T"] = 1500.0
    with open_ens(pkg, p, 1024, 7) as ens:
        ens.barrier_consume_begin()
        first = []
        events, nslices = run_sliced(pkg, ens, p["T"], each_slice=lambda s, cnt: first.append(cnt["ntrace"].copy()) if s == 0 else None)
        assert nslices >= 2 and np.all(first[0] == 1024)
        check_against_mirrors(pkg, ens, p, events, grid=False)


def test_pairs_and_condition_on_the_d8_run(gpu_pkg):
    """cov="diag" and the condition x_3 = x_5 beside the consumers: trace.pair_integrals / trace.conditional_trace on the θ_eff-started trace.
    hits=K lies above the count of the reference trace itself (computed on the CPU from the restatement), so no hit is dropped."""
    pkg = gpu_pkg
    p = problem("d8")
    d = 8
    th_eff, _ = pkg.trace.barrier_start(p["x0"], p["th0"], p["bar"])
    pt, nn = np.zeros(d), np.zeros(d)
    nn[3], nn[5] = 1.0, -1.0
    Khits = 256
    want_hits = []
    for k in range(3):
        r = R.stickyzz(0.0, p["x0"][k], p["th0"][k], p["T"], p["c"], p["bar"], gamma=p["G"], target_gamma=p["Gt"], seed=7 + k)
        ev = np.zeros(len(r["t"]), dtype=pkg._lib.EVENT_DTYPE)
        ev["t"], ev["i"], ev["x"], ev["theta"] = r["t"], r["i"], r["x"], r["theta"]
        want_hits.append(pkg.trace.conditional_trace(pkg.FactTrace(None, 0.0, p["x0"][k], th_eff[k], ev), pt, nn))
        assert 0 < len(want_hits[k][0]) < Khits
    with open_ens(pkg, p, 64, 7) as ens:
        ens.barrier_consume_begin()
        ens.consume_condition(pt, nn, Khits)
        ens.consume_pairs(np.arange(d), np.arange(d))
        events, nslices = run_sliced(pkg, ens, p["T"])
        assert nslices >= 3
        S, J, Tl = ens.consume_pair_integrals()
        for k, ev in enumerate(events):
            tr = pkg.FactTrace(None, 0.0, p["x0"][k], th_eff[k], ev)
            hS, hJ, hT = pkg.trace.pair_integrals(tr, np.arange(d), np.arange(d))
            assert same_bits(S[k], hS) and same_bits(J[k], hJ) and Tl[k] == hT
            t, x, nhits = ens.consume_conditioned(k)
            ht, hx = pkg.trace.conditional_trace(tr, pt, nn)
            assert nhits == len(ht) == len(want_hits[k][0]) < Khits
            assert same_bits(t, ht) and same_bits(x, hx) and same_bits(t, want_hits[k][0]) and same_bits(x, want_hits[k][1])
        check_against_mirrors(pkg, ens, p, events, grid=False)


# ------------------------------------------------------------------------------------------------------------------ (c) calls and refusals
def test_calls_and_refusals(gpu_pkg):
    pkg = gpu_pkg
    L = pkg._lib

    def code(fn):
        with pytest.raises(L.PdmpError) as ei:
            fn()
        return ei.value.code, str(ei.value)

    p = problem("d8")
    G = p["Gt"]
    for sampler, kw in ((L.SAMPLER_ZIGZAG_LOCAL, {}), (L.SAMPLER_STICKY_ZIGZAG, dict(factor=1.5))):  # not a barrier ensemble
        with pkg.Ensemble(1, 8, sampler=sampler, trace_capacity=64, **kw) as e:
            e.set_flow(pkg.ZigZag(G, np.zeros(8)))
            e.set_target(pkg.GaussianTarget(G, None))
            if sampler == L.SAMPLER_STICKY_ZIGZAG:
                e.set_sticky(np.ones(8))
            e.set_state(0.0, p["x0"][:1], p["th0"][:1], p["c"], np.array([1], dtype=np.uint64))
            assert code(lambda: e.barrier_consume_begin())[0] == L.PDMP_ERR_INVALID
            assert code(lambda: e.barrier_consume_occupation())[0] == L.PDMP_ERR_INVALID
            e.consume_begin()  # (its own entry still serves it)
            assert code(lambda: e.barrier_consume_occupation())[0] == L.PDMP_ERR_INVALID
    with open_ens(pkg, p, 64, 7) as e:
        assert code(lambda: e.barrier_consume_occupation())[0] == L.PDMP_ERR_INVALID  # before begin
        c, msg = code(lambda: e.consume_begin())
        assert c == L.PDMP_ERR_UNSUPPORTED and "pdmp_ensemble_barrier_consume_begin" in msg
        assert code(lambda: e.barrier_consume_begin(0.5, -1))[0] == L.PDMP_ERR_INVALID
        assert code(lambda: e.barrier_consume_begin(0.0, 4))[0] == L.PDMP_ERR_INVALID
        e.barrier_consume_begin(0.5, 8)
        assert code(lambda: e.consume_async())[0] == L.PDMP_ERR_UNSUPPORTED
        c, msg = code(lambda: e.consume_inclusion())
        assert c == L.PDMP_ERR_UNSUPPORTED and "pdmp_ensemble_barrier_consume_occupation" in msg
        assert code(lambda: e.barrier_consume_occupation(2, 2))[0] == L.PDMP_ERR_INVALID  # a range outside the ensemble
        assert code(lambda: e.barrier_consume_occupation(-1, 1))[0] == L.PDMP_ERR_INVALID
        zl, zh, nl, nh, T = e.barrier_consume_occupation(1, 2)  # nothing consumed yet: zeros, T_last = t0
        assert zl.shape == nh.shape == (2, 8) and not zl.any() and not zh.any() and not nl.any() and not nh.any() and np.all(T == 0.0)
        st = e._L.pdmp_ensemble_barrier_consume_occupation(e._h, 0, 3, None, None, None, None, None)  # every output may be NULL
        assert st == 0
        e.run(1.0)
        assert code(lambda: e.barrier_consume_begin())[0] == L.PDMP_ERR_INVALID  # after the first run
    with pkg.Ensemble(1, 8, sampler=L.SAMPLER_BARRIER_ZIGZAG, factor=1.5, trace_capacity=0) as e:
        e.set_flow(pkg.ZigZag(p["G"], np.zeros(8)))
        e.set_target(pkg.GaussianTarget(G, None))
        e.set_barriers(*R.barrier_table(p["bar"], 8))
        e.set_state(0.0, p["x0"][:1], p["th0"][:1], p["c"], np.array([1], dtype=np.uint64))
        assert code(lambda: e.barrier_consume_begin())[0] == L.PDMP_ERR_INVALID  # no trace buffer


def test_a_read_between_slices_leaves_the_final_values_unchanged(gpu_pkg):
    pkg = gpu_pkg
    p = problem("d8")
    out = []
    for read in (False, True):
        mids = []
        with open_ens(pkg, p, 64, 7) as ens:
            ens.barrier_consume_begin()
            _, nslices = run_sliced(pkg, ens, p["T"], each_slice=(lambda s, cnt: mids.append(ens.barrier_consume_occupation())) if read else None)
            out.append(ens.barrier_consume_occupation())
        if read:  # the reads in between saw the chains advance and the sums grow
            assert len(mids) == nslices >= 3 and np.all(np.diff([m[4] for m in mids], axis=0) >= 0) and np.all(mids[-1][4] > mids[0][4])
            tot = [(m[0] + m[1]).sum() for m in mids]
            assert np.all(np.diff(tot) >= 0) and tot[-1] > tot[0]
            assert all(a.tobytes() == b.tobytes() for a, b in zip(mids[-1], out[-1]))  # (the last of them is the final read)
    for a, b in zip(*out):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------ (d) the samplers' keyword
def same_result(a, b):
    assert a.keys() == b.keys()
    for f in a:
        if isinstance(a[f], (list, tuple)):
            assert len(a[f]) == len(b[f]) and all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a[f], b[f])), f
        else:
            assert (a[f] is None and b[f] is None) or np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), f


def test_stickyzz_consume_keyword(gpu_pkg):
    pkg = gpu_pkg
    p = problem("d8")
    d = 8
    pt, nn = np.zeros(d), np.zeros(d)
    nn[3], nn[5] = 1.0, -1.0
    args = (pkg.GaussianTarget(p["Gt"], None), 0.0, p["x0"], p["th0"], p["T"], p["c"], pkg.ZigZag(p["G"], np.zeros(d)), K.barriers_for(pkg, p["bar"], d))
    cons = dict(dt=0.25, points=200, cov="diag", condition=(pt, nn), hits=256)
    plain = pkg.stickyzz(*args, seed=7, trace_capacity=64)
    full = pkg.stickyzz(*args, seed=7, trace_capacity=64, consume=cons)
    assert len(plain) == 4 and len(full) == 5
    for k in range(3):  # the earlier elements are those without the keyword
        assert full[0][k].events.tobytes() == plain[0][k].events.tobytes()
    assert np.array_equal(full[1], plain[1]) and all(np.array_equal(u, v) for u, v in zip(full[3], plain[3]))
    res = full[4]
    assert set(res) == {"mean", "T", "grid_t", "grid_x", "frozen_lo", "frozen_hi", "hits_lo", "hits_hi", "pairs", "pair_S", "pair_J", "hit_t", "hit_x",
                        "nhits"}
    assert res["mean"].shape == res["frozen_lo"].shape == res["frozen_hi"].shape == res["hits_lo"].shape == res["hits_hi"].shape == (3, d)
    assert res["T"].shape == (3,) and res["hits_lo"].dtype == np.uint64 and res["pair_S"].shape == res["pair_J"].shape == (3, d)
    th_eff, _ = pkg.trace.barrier_start(p["x0"], p["th0"], p["bar"])
    for k in range(3):
        ev = full[0][k].events
        hz = pkg.trace.barrier_occupation(full[0][k], 0.0, p["x0"][k], p["th0"][k], p["bar"])
        assert same_bits(res["frozen_lo"][k], hz[0]) and same_bits(res["frozen_hi"][k], hz[1])
        assert np.array_equal(res["hits_lo"][k], hz[2]) and np.array_equal(res["hits_hi"][k], hz[3]) and res["T"][k] == hz[4]
        tr = pkg.FactTrace(None, 0.0, p["x0"][k], th_eff[k], ev)
        ht, hx = pkg.trace.discretize(tr, 0.25)
        assert same_bits(res["grid_t"][k], ht) and same_bits(res["grid_x"][k], hx) and res["grid_x"][k].shape[1] == d
        assert res["nhits"][k] == len(res["hit_t"][k]) < 256 and res["hit_x"][k].shape == (res["nhits"][k], d)
    same_result(res, pkg.stickyzz(*args, seed=7, trace_capacity=64, trace=False, consume=cons)[4])
    # one chain, details and the keyword: the dict comes last, squeezed
    one = pkg.stickyzz(args[0], 0.0, p["x0"][0], p["th0"][0], p["T"], p["c"], args[6], args[7], seed=7, trace_capacity=64, details=True,
                       consume=dict(dt=0.25, points=200))
    assert len(one) == 6 and set(one[4]) == {"c", "frozen", "θ_saved"} and one[5]["frozen_lo"].shape == (d,) and one[5]["grid_x"].shape[1] == d
    assert same_bits(one[5]["frozen_lo"], res["frozen_lo"][0]) and same_bits(one[5]["mean"], res["mean"][0])
    with pytest.raises(TypeError):
        pkg.stickyzz(*args, seed=7, consume=dict(step=0.25))
    with pytest.raises(ValueError):
        pkg.stickyzz(*args, seed=7, trace_capacity=0, consume=dict())


def test_sspdmp2_consume_keyword(gpu_pkg):
    """1 − (frozen_lo + frozen_hi) / (T_last − t0), the posterior inclusion probability, equals the same quantity from the returned trace"""
    pkg = gpu_pkg
    G = K.precision8()
    x0, th0 = K.state8(3)
    kap = np.linspace(0.4, 1.8, 8)
    args = (pkg.GaussianTarget(G, None), 0.0, x0, th0, 30.0, K.c8(G), None, pkg.ZigZag(0.9 * G, np.zeros(8)), kap)
    tr0, acc0 = pkg.sspdmp2(*args, seed=7, trace_capacity=64)
    tr, acc, res = pkg.sspdmp2(*args, seed=7, trace_capacity=64, consume=dict(dt=0.5, points=80))
    assert all(tr[k].events.tobytes() == tr0[k].events.tobytes() for k in range(3)) and all(np.array_equal(u, v) for u, v in zip(acc, acc0))
    assert set(res) == {"mean", "T", "grid_t", "grid_x", "frozen_lo", "frozen_hi", "hits_lo", "hits_hi"}
    bar = [((0.0, 0.0), ("sticky", "sticky"), (k, k)) for k in kap]
    incl = 1.0 - (res["frozen_lo"] + res["frozen_hi"]) / (res["T"] - 0.0)[:, None]
    for k in range(3):
        zl, zh, nl, nh, T = pkg.trace.barrier_occupation(tr[k], 0.0, x0[k], th0[k], bar)
        assert same_bits(incl[k], 1.0 - (zl + zh) / (T - 0.0)) and np.all((incl[k] > 0) & (incl[k] < 1))
        assert np.array_equal(res["hits_lo"][k] + res["hits_hi"][k], np.bincount(tr[k].events["i"][tr[k].events["theta"] == 0], minlength=8))
    off = pkg.sspdmp2(*args, seed=7, trace_capacity=64, trace=False, consume=dict(dt=0.5, points=80))
    assert len(off) == 3 and all(len(t.events) == 0 for t in off[0])
    same_result(res, off[2])
