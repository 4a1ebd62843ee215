"""The Cholesky factor of a precision matrix under the sticky ZigZag (casestudies/precision/precision.jl) on gfx950 -- zz_precision_run_kernel,
csrc/pdmp_precision.inc -- against its CPU restatement (tests/ref/precision_ref.c), bit for bit, through the C ABI and the public sspdmp
(-m gpu)."""
import numpy as np
import pytest
import scipy.sparse as sp

import precision_ref_lib as R
from precision_cases import DIAGONAL_FREEZE, N2, lower_index, n2_flow, random_case, stalled_input

pytestmark = pytest.mark.gpu


def flow(pkg, gam, mu):
    return pkg.ZigZag(sp.diags(np.asarray(gam, dtype=np.float64), format="csc"), np.asarray(mu, dtype=np.float64))


def device_run(pkg, a, c, kappa, seeds, TP, *, gamma0=0.0, adapt=False, factor=1.5, reversible=False, strong=False, cap=1 << 14, slices=()):
    """Every chain to T through the C ABI: PDMP_RUN_STOP_BEFORE to each of `slices`, then the reference tail; the trace is drained whenever a
    launch returns.  Returns (events per chain, counters, final state with θf, launches)."""
    Lb = pkg._lib
    x0, th0 = np.atleast_2d(a["x0"]), np.atleast_2d(a["th0"])
    nch, d = x0.shape
    events = [[] for _ in range(nch)]
    launches = 0
    with pkg.Ensemble(nch, d, sampler=Lb.SAMPLER_STICKY_ZIGZAG, adapt=adapt, factor=factor, trace_capacity=cap) as ens:
        ens.set_flow(flow(pkg, a["gam"], a["mu"]))
        ens.set_target(pkg.PrecisionCholeskyTarget(a["YY"], a["N"], gamma0))
        ens.set_sticky(np.broadcast_to(np.asarray(kappa, dtype=np.float64), (d,)), reversible, strong)
        ens.set_state(0.0, x0, th0, np.broadcast_to(np.asarray(c, dtype=np.float64), (d,)), seeds)
        for Tk, flags in [(s, Lb.RUN_STOP_BEFORE) for s in slices] + [(TP, Lb.RUN_REFERENCE_TAIL)]:
            while True:
                ens.run(Tk, flags)
                launches += 1
                cnt = ens.counters()
                for k in range(nch):
                    if cnt["ntrace"][k]:
                        events[k].append(ens.trace(k, counters=cnt))
                ens.trace_reset()
                if not Lb.needs_rerun(cnt["status"]):
                    break
        assert ens.kernel_name() == "zz_precision_run_kernel"
        cnt, fs = ens.counters(), ens.final_state()
        fs.update(ens.final_sticky())
    ev = [np.concatenate(e) if e else np.empty(0, dtype=Lb.EVENT_DTYPE) for e in events]
    return ev, cnt, fs, launches


def same_bytes(a, b):
    """equal as BYTES: −0.0 is not +0.0 here (a coordinate frozen while going down sits at −0.0 until a thaw moves it by θ·0), and no NaN equals itself"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def compare(ev, cnt, fs, refs):
    """events, num, nacc, nevents, draw counts, status, final (t, x, θ, θf), the flags f and the adapted c: byte for byte."""
    for k, r in enumerate(refs):
        assert int(cnt["status"][k]) == r["status"], (k, int(cnt["status"][k]), r["status"])
        assert len(ev[k]) == r["nevents"] == len(r["t"]), (k, len(ev[k]), r["nevents"])
        for f in ("i", "t", "x", "theta"):
            assert same_bytes(ev[k][f], r[f]), (k, f, int(np.argmax(np.ascontiguousarray(ev[k][f]).view(np.uint64) != r[f].view(np.uint64))))
        got = tuple(int(cnt[f][k]) for f in ("num", "nacc", "nevents", "ndraw_main", "ndraw_global"))
        assert got == (r["num"], r["nacc"], r["nevents"], r["ndraw_main"], 0), (k, got)
        assert same_bytes(fs["t"][k], r["t_state"]) and same_bytes(fs["x"][k], r["x_final"]) and same_bytes(fs["theta"][k], r["theta_final"]), k
        assert same_bytes(fs["theta_f"][k], r["thf_final"]) and same_bytes(fs["c"][k], r["c_final"]) and np.array_equal(fs["acc"][k], r["f_final"]), k
        assert np.array_equal(fs["frozen"][k], (r["x_final"] == 0) & (r["theta_final"] == 0))
        assert cnt["t_last"][k] == r["t_last"]


def pair(pkg, a, TP, seed, *, c=1.0, kappa=0.5, gamma0=0.0, adapt=True, factor=1.5, reversible=False, strong=False, **kw):
    x0, th0 = np.atleast_2d(a["x0"]), np.atleast_2d(a["th0"])
    nch = x0.shape[0]
    seeds = np.uint64(seed) + np.arange(nch, dtype=np.uint64)
    out = device_run(pkg, a, c, kappa, seeds, TP, gamma0=gamma0, adapt=adapt, factor=factor, reversible=reversible, strong=strong, **kw)
    refs = [R.precision(a["YY"], a["N"], x0[k], th0[k], TP, c, a["gam"], a["mu"], kappa, gamma0=gamma0, adapt=adapt, factor=factor,
                        reversible=reversible, strong_upperbounds=strong, seed=int(seeds[k])) for k in range(nch)]
    compare(out[0], out[1], out[2], refs)
    return out, refs


def n2_case(nch=6):
    gam, mu = n2_flow()
    rng = np.random.default_rng(2)
    x0 = mu[None, :] + 0.1 * rng.standard_normal((nch, 3))
    return dict(YY=N2["YY"], N=N2["N"], gam=gam, mu=mu, x0=x0, th0=rng.choice([-1.0, 1.0], size=(nch, 3)), n=2, d=3)


@pytest.fixture(scope="module")
def case5():
    return random_case(5, 40, 505, 4)


def test_n1_a_lone_diagonal(gpu_pkg):
    """d = 1: L11 alone, ϕ = ½ YY L² − N log L.  It reflects off the −N/u wall and never freezes."""
    a = random_case(1, 8, 101, 4)
    _, refs = pair(gpu_pkg, a, 200.0, 11)
    assert all(r["status"] == R.REF_OK and r["nevents"] > 100 and np.all(r["theta"] != 0) and r["x"].min() > 0 for r in refs)


def test_n2_the_statistical_case(gpu_pkg):
    """YY = [[12, 1.5], [1.5, 9]], N = 10, κ = 1 (tests/test_precision_ref.py holds this law to its closed form), six chains to T = 20."""
    _, refs = pair(gpu_pkg, n2_case(), 20.0, 21, kappa=1.0)
    assert all(r["status"] == R.REF_OK and r["nevents"] > 40 for r in refs) and sum(int((r["theta"] == 0).sum()) for r in refs) > 10


def test_n5(gpu_pkg, case5):
    _, refs = pair(gpu_pkg, case5, 30.0, 31)
    assert all(r["status"] == R.REF_OK and r["nevents"] > 300 and (r["theta"] == 0).sum() > 10 for r in refs)


def test_n64_every_lane_and_33_key_blocks(gpu_pkg):
    """d = 2080: column 0 has a member in every lane, the queue has 33 blocks; T for about 2000 events per chain."""
    a = random_case(64, 200, 6464, 4)
    _, refs = pair(gpu_pkg, a, 0.15, 41, c=10.0)
    assert all(r["status"] == R.REF_OK and 1200 < r["nevents"] < 4000 for r in refs)
    assert all(len(np.unique(r["i"])) > 600 and r["i"].max() >= 2016 for r in refs)


def test_n5_across_launches(gpu_pkg, case5, monkeypatch):
    """Three PDMP_RUN_STOP_BEFORE slices, a trace buffer of 4 events that fills and is drained, and the count-limit pause: the bytes of the
    restatement's one-shot run each time (compare() inside pair())."""
    pkg = gpu_pkg
    (_, _, _, n1), refs = pair(pkg, case5, 30.0, 31, slices=(2.0, 11.5, 11.75))
    assert n1 == 4 and all(r["nevents"] > 300 for r in refs)
    (_, _, _, n2), _ = pair(pkg, case5, 6.0, 32, cap=4)
    assert n2 > 20
    monkeypatch.setenv("PDMP_LAUNCH_COUNT_LIMIT", "300")
    (_, _, _, n3), refs = pair(pkg, case5, 30.0, 31)
    assert n3 > 5 and min(r["ndraw_main"] for r in refs) > 5 * 300


def test_n5_adapt_grows_c_and_fixed_c_is_violated(gpu_pkg, case5):
    """adapt from c = 1e-3: c must grow (and acc, num restart at every growth); the same start without adapt ends BOUND_VIOLATED after the
    same events and draws, and the public call raises the reference's error."""
    pkg = gpu_pkg
    (_, _, fs, _), refs = pair(pkg, case5, 10.0, 51, c=1e-3, adapt=True)
    assert all(r["status"] == R.REF_OK and r["nadapt"] > 5 for r in refs) and np.all(fs["c"].max(axis=1) > 1e-3)
    (_, cnt, _, _), refs = pair(pkg, case5, 10.0, 51, c=1e-3, adapt=False)
    assert all(r["status"] == R.REF_BOUND_VIOLATED for r in refs) and np.all(cnt["status"] == pkg._lib.CHAIN_BOUND_VIOLATED)
    a = case5
    with pytest.raises(RuntimeError, match="too small"):
        pkg.sspdmp(pkg.PrecisionCholeskyTarget(a["YY"], a["N"]), 0.0, a["x0"][0], a["th0"][0], 10.0, np.full(15, 1e-3), flow(pkg, a["gam"], a["mu"]),
                   np.full(15, 0.5), seed=51)


@pytest.mark.parametrize("kw", [dict(reversible=True), dict(strong=True), dict(reversible=True, strong=True, gamma0=0.3), dict(gamma0=0.3)],
                         ids=["reversible", "strong", "rev_strong_g0", "g0"])
def test_n5_keywords(gpu_pkg, case5, kw):
    _, refs = pair(gpu_pkg, case5, 20.0, 61, **kw)
    assert all(r["status"] == R.REF_OK and r["nevents"] > 200 and (r["theta"] == 0).sum() > 5 for r in refs)
    if kw.get("reversible"):  # a coordinate frozen at −0.0 whose coin sends it up thaws at +0.0 (x + θ·0): compare() sees the sign bit
        r = refs[0]
        thaw = np.flatnonzero((r["x"] == 0) & (r["theta"] != 0))
        assert np.any(np.signbit(r["x"][thaw]) != np.signbit(r["x"][[np.flatnonzero((r["i"] == r["i"][q]) & (r["t"] < r["t"][q]))[-1] for q in thaw]]))


def test_n5_diagonal_freeze_stalls(gpu_pkg):
    """precision_cases.stalled_input: the freeze of L11 is popped -- PDMP_CHAIN_STALLED with the restatement's counts, nothing of L11 changed."""
    pkg = gpu_pkg
    a = stalled_input()
    case = dict(a, x0=a["x0"][None, :], th0=a["th0"][None, :])
    (ev, cnt, fs, _), refs = pair(pkg, case, 5.0, a["seed"], c=a["c"], kappa=a["kappa"], adapt=False)
    assert refs[0]["status"] == R.REF_STALLED and int(cnt["status"][0]) == pkg._lib.CHAIN_STALLED
    assert (int(cnt["nevents"][0]), int(cnt["num"][0]), int(cnt["ndraw_main"][0])) == (DIAGONAL_FREEZE["nevents"], DIAGONAL_FREEZE["num"], DIAGONAL_FREEZE["ndraw_main"])
    assert fs["acc"][0, 0] == 1 and fs["theta"][0, 0] < 0 and fs["x"][0, 0] > 0
    with pytest.raises(RuntimeError, match="stalled at t = 0.59875"):  # the public call says so instead of returning a trace that stops short of T
        pkg.sspdmp(pkg.PrecisionCholeskyTarget(a["YY"], a["N"]), 0.0, a["x0"], a["th0"], 5.0, a["c"], flow(pkg, a["gam"], a["mu"]), a["kappa"], seed=a["seed"])


def test_public_call_and_consumers(gpu_pkg, case5):
    """sspdmp(target, 0.0, x0, θ0, T, c, ZigZag(diag Γ̂, μ̂), κ; adapt=True) returns the reference's tuple, bit for bit the restatement's.  With
    consume=dict(dt, points) the device consumers add mean, inclusion and the grid: consume_mean / consume_inclusion equal trace.mean /
    trace.inclusion_prob of the copied trace (tests/test_gpu_consumers.py's tolerances), the grid equals trace.discretize bit for bit.  The
    path-integral calls are refused."""
    pkg = gpu_pkg
    Lb = pkg._lib
    a, T = case5, 30.0
    F, kappa, c = flow(pkg, a["gam"], a["mu"]), np.full(15, 0.5), np.ones(15)
    tgt = pkg.PrecisionCholeskyTarget(a["YY"], a["N"])
    tr, (t, x, th), (acc, num), cc = pkg.sspdmp(tgt, 0.0, a["x0"][:2], a["th0"][:2], T, c, F, kappa, adapt=True, seed=81)
    refs = [R.precision(a["YY"], a["N"], a["x0"][k], a["th0"][k], T, c, a["gam"], a["mu"], kappa, adapt=True, seed=81 + k) for k in range(2)]
    for k, r in enumerate(refs):
        for f in ("i", "t", "x", "theta"):
            assert same_bytes(tr[k].events[f], r[f])
        assert same_bytes(t[k], r["t_state"]) and same_bytes(x[k], r["x_final"]) and same_bytes(th[k], r["theta_final"])
        assert (int(acc[k]), int(num[k])) == (r["nacc"], r["num"]) and np.array_equal(cc[k], r["c_final"]) and r["nadapt"] > 0
    dt, K = 0.37, 96
    out = pkg.sspdmp(tgt, 0.0, a["x0"][:2], a["th0"][:2], T, c, F, kappa, adapt=True, seed=81, trace_capacity=100, consume=dict(dt=dt, points=K))
    assert len(out) == 5 and all(out[0][k].events.tobytes() == tr[k].events.tobytes() for k in range(2)) and len(tr[0].events) > 300
    for k in range(2):
        grid, X = pkg.trace.discretize(tr[k], dt)
        assert len(grid) > 40 and np.array_equal(out[4]["grid_t"][k], grid) and np.array_equal(out[4]["grid_x"][k], X)
        assert np.allclose(out[4]["mean"][k], pkg.trace.mean(tr[k]), rtol=1e-12, atol=1e-15) and out[4]["T"][k] == tr[k].events["t"][-1]
        inc = pkg.trace.inclusion_prob(tr[k])
        assert np.allclose(out[4]["inclusion"][k], inc, rtol=1e-12, atol=1e-15)
        r_, c_ = lower_index(5)
        # the diagonal never sits at 0 (inclusion_prob counts a coordinate up to its own last event: just short of 1); off-diagonals do
        assert np.all(inc[r_ == c_] > 0.99) and np.all(tr[k].events["x"][np.isin(tr[k].events["i"], np.flatnonzero(r_ == c_))] > 0) and inc[r_ != c_].min() < 0.9
        L = pkg.trace.unpack_lower(out[4]["mean"][k])
        assert L.shape == (5, 5) and np.array_equal(pkg.trace.pack_lower(L), out[4]["mean"][k]) and np.all(np.triu(L, 1) == 0)
    with pkg.Ensemble(1, 15, sampler=Lb.SAMPLER_STICKY_ZIGZAG, adapt=True, trace_capacity=4096) as ens:  # the C ABI's consumer calls, one launch
        ens.set_flow(F)
        ens.set_target(tgt)
        ens.set_sticky(kappa)
        ens.set_state(0.0, a["x0"][:1], a["th0"][:1], c, np.array([81], dtype=np.uint64))
        ens.consume_begin()
        ens.run(T, Lb.RUN_STOP_BEFORE)
        ens.consume()
        ev = ens.trace(0)
        one = pkg.FactTrace(F, 0.0, a["x0"][0], a["th0"][0], ev)
        m, Tl = ens.consume_mean()
        p, Tp = ens.consume_inclusion()
        assert 300 < len(ev) < 4096 and Tl[0] == Tp[0] == ev["t"][-1]
        assert np.allclose(m[0], pkg.trace.mean(one), rtol=1e-12, atol=1e-15) and np.allclose(p[0], pkg.trace.inclusion_prob(one), rtol=1e-12, atol=1e-15)
        for call in (lambda: ens.path_integrals(1.0, np.arange(15)), lambda: ens.batch_means(0.0, 1.0), lambda: ens.ess_begin(1.0)):
            with pytest.raises(Lb.PdmpError) as ei:
                call()
            assert ei.value.code == Lb.PDMP_ERR_UNSUPPORTED and "precision-cholesky" in str(ei.value), str(ei.value)


def test_refusals(gpu_pkg, case5):
    """Every refusal of pdmp_ensemble_set_target_precision_cholesky and of set_state under it, by status and the word in the message."""
    pkg = gpu_pkg
    Lb = pkg._lib
    a = case5
    n, d = 5, 15
    x0, th0, c, seeds, kappa = a["x0"][:2], a["th0"][:2], np.ones(d), np.array([3, 4], dtype=np.uint64), np.full(d, 0.5)
    tgt = pkg.PrecisionCholeskyTarget(a["YY"], a["N"])

    def refused(fn, code, word):
        with pytest.raises(Lb.PdmpError) as ei:
            fn()
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    def fresh(F=None, sampler=Lb.SAMPLER_STICKY_ZIGZAG, dd=d, **kw):
        e = pkg.Ensemble(2, dd, sampler=sampler, trace_capacity=64, **kw)
        e.set_flow(flow(pkg, a["gam"], a["mu"]) if F is None else F)
        return e

    inf, nan = float("inf"), float("nan")
    with fresh() as e:  # the arguments
        refused(lambda: e.set_target(pkg.PrecisionCholeskyTarget(np.eye(4), 10.0)), Lb.PDMP_ERR_INVALID, "n (n + 1)/2")
        refused(lambda: Lb.check(e._L.pdmp_ensemble_set_target_precision_cholesky(e._h, 0, a["YY"].ctypes.data, 10.0, 0.0)), Lb.PDMP_ERR_INVALID, "n = 0")
        for bad in (0.0, -1.0, inf, nan):
            refused(lambda: e.set_target(pkg.PrecisionCholeskyTarget(a["YY"], bad)), Lb.PDMP_ERR_INVALID, "N = ")
        for bad in (-0.1, inf, nan):
            refused(lambda: e.set_target(pkg.PrecisionCholeskyTarget(a["YY"], 10.0, bad)), Lb.PDMP_ERR_INVALID, "gamma0")
        Y2 = a["YY"].copy()
        Y2[3, 1] = nan
        refused(lambda: e.set_target(pkg.PrecisionCholeskyTarget(Y2, 10.0)), Lb.PDMP_ERR_INVALID, "not finite")
        Y2 = a["YY"].copy()
        Y2[1, 3] = np.nextafter(Y2[1, 3], inf)
        refused(lambda: e.set_target(pkg.PrecisionCholeskyTarget(Y2, 10.0)), Lb.PDMP_ERR_INVALID, "symmetric")
        e.set_target(tgt)
        e.set_sticky(kappa)
        for bad in (0.0, -0.2, nan):
            xb = x0.copy()
            xb[1, 5] = bad  # L22 of the second chain
            refused(lambda: e.set_state(0.0, xb, th0, c, seeds), Lb.PDMP_ERR_UNSUPPORTED, "diagonal")
        refused(lambda: e.set_state_synthetic(0.0, c, 1), Lb.PDMP_ERR_UNSUPPORTED, "explicit state")
        e.set_state(0.0, x0, th0, c, seeds)
        refused(lambda: e.set_target(tgt), Lb.PDMP_ERR_INVALID, "state exists")  # a state already exists
        e.run(1.0, Lb.RUN_STOP_BEFORE)
        assert e.kernel_name() == "zz_precision_run_kernel"
    with fresh() as e:  # the later target call wins
        e.set_target(tgt)
        e.set_target(pkg.GaussianTarget(sp.identity(d, format="csc"), None))
        e.set_sticky(kappa)
        e.set_state(0.0, x0, th0, c, seeds)
        e.run(8.0)
        assert e.kernel_name() != "zz_precision_run_kernel"
        fs, st = e.final_state(), e.final_sticky()  # pdmp_ensemble_final_sticky on an ordinary sticky ensemble: a frozen coordinate has a saved speed
        assert np.array_equal(st["frozen"], (fs["x"] == 0) & (fs["theta"] == 0)) and st["frozen"].sum() > 0
        assert st["theta_f"].shape == (2, d) and np.all(st["theta_f"][st["frozen"]] != 0)
    with pkg.Ensemble(2, d, sampler=Lb.SAMPLER_ZIGZAG_LOCAL, trace_capacity=64) as e:
        refused(lambda: e.final_sticky(), Lb.PDMP_ERR_INVALID, "PDMP_SAMPLER_STICKY_ZIGZAG")
    for sampler in (Lb.SAMPLER_ZIGZAG_LOCAL, Lb.SAMPLER_ZIGZAG_ALL, Lb.SAMPLER_BARRIER_ZIGZAG):  # another sampler
        with fresh(sampler=sampler) as e:
            refused(lambda: e.set_target(tgt), Lb.PDMP_ERR_INVALID, "PDMP_SAMPLER_STICKY_ZIGZAG")
    with pkg.Ensemble(2, d, sampler=Lb.SAMPLER_BPS, trace_capacity=64) as e:
        refused(lambda: e.set_target(tgt), Lb.PDMP_ERR_INVALID, "PDMP_SAMPLER_STICKY_ZIGZAG")
    n65 = 65
    d65 = n65 * (n65 + 1) // 2
    with pkg.Ensemble(1, d65, sampler=Lb.SAMPLER_STICKY_ZIGZAG, trace_capacity=64) as e:  # beyond one column member per lane
        e.set_flow(pkg.ZigZag(sp.identity(d65, format="csc"), np.zeros(d65)))
        refused(lambda: e.set_target(pkg.PrecisionCholeskyTarget(np.eye(n65), 10.0)), Lb.PDMP_ERR_UNSUPPORTED, "n = 65")

    def state_refused(e, word):
        e.set_target(tgt)
        e.set_sticky(kappa)
        refused(lambda: e.set_state(0.0, x0, th0, c, seeds), Lb.PDMP_ERR_UNSUPPORTED, word)

    tri = sp.diags([np.full(d - 1, 0.1), np.ones(d), np.full(d - 1, 0.1)], [-1, 0, 1], format="csc")
    with fresh(F=pkg.ZigZag(tri, np.zeros(d))) as e:
        state_refused(e, "diagonal")
    neg = a["gam"].copy()
    neg[7] = -1.0
    with fresh(F=flow(pkg, neg, a["mu"])) as e:
        state_refused(e, "positive")
    with fresh() as e:
        e.set_neighbourhood(tri)
        state_refused(e, "set_neighbourhood")
    with fresh() as e:
        e.set_gradient_tracking(True)
        state_refused(e, "gradient tracking")
    with fresh() as e:
        e.set_local_bound(True)
        state_refused(e, "LocalBound")
    with fresh(F=pkg.ZigZag(sp.diags(a["gam"], format="csc"), a["mu"], λref=0.5)) as e:  # a refresh clock: no sticky ensemble gets as far as a state with one
        e.set_target(tgt)
        refused(lambda: e.set_sticky(kappa), Lb.PDMP_ERR_UNSUPPORTED, "refresh")
        refused(lambda: e.set_adaptscale(True), Lb.PDMP_ERR_UNSUPPORTED, "adaptscale")
        refused(lambda: e.set_state(0.0, x0, th0, c, seeds), Lb.PDMP_ERR_INVALID, "set_sticky")
    with fresh() as e:  # ... unless the flow is set again after set_sticky: set_state then names the refresh clock
        e.set_sticky(kappa)
        e.set_flow(pkg.ZigZag(sp.diags(a["gam"], format="csc"), a["mu"], λref=0.5))
        e.set_target(tgt)
        refused(lambda: e.set_state(0.0, x0, th0, c, seeds), Lb.PDMP_ERR_UNSUPPORTED, "refresh clock")
