"""The speed-recorded Bouncy Particle on the logistic-regression target on gfx950 (csrc/pdmp_bps_logit.inc) vs its sequential restatement
(tests/ref/bps_logistic_ref.c), through the C ABI's Python binding and the Python pdmp (-m gpu): records (t, x, θ), the counters num, nacc,
nrefresh, nevents, ndraw_main, the status and the final (t, x, θ, c), bit for bit, for every chain checked."""
import numpy as np
import pytest
import scipy.sparse as sp

import bps_logistic_ref_lib as B
import modern_bps_ref_lib as M
from test_gpu_modern_bps_parity import INF, Collector, compare, same

pytestmark = pytest.mark.gpu

KERNEL = "bps_logit_run_kernel"


def sparse_design(n, d, rng, density=None):
    """A sparse n x d design in which some rows have one entry, the last column (d >= 3) has none at all, and one entry is an explicit zero."""
    density = min(1.0, 3.0 / d) if density is None else density
    D = rng.standard_normal((n, d)) * (rng.random((n, d)) < density)
    for i in range(0, n, 3):  # rows with exactly one entry
        D[i] = 0.0
        D[i, (7 * i) % d] = 0.5 + rng.random()
    for i in range(n):  # no empty row
        if not D[i].any():
            D[i, i % d] = -0.7
    if d >= 3:
        D[:, d - 1] = 0.0
        for i in range(n):
            if not D[i].any():
                D[i, 0] = 0.9
    A = sp.csc_matrix(D)
    A.sort_indices()
    A.data[len(A.data) // 2] = 0.0  # an explicit zero: stays in the pattern
    return A


def problem(d, n, seed, A=None, form="I", L=None, oscn=False, rho=0.9, lam=1.0, nch=3, gamma0=0.7, m=None, y=None, t0=0.0, xscale=0.3):
    rng = np.random.default_rng(seed)
    A = sparse_design(n, d, rng) if A is None else A
    m = rng.integers(1, 4, n).astype(np.float64) if m is None else np.asarray(m, dtype=np.float64)
    y = np.floor(rng.random(n) * (m + 1)) if y is None else np.asarray(y, dtype=np.float64)
    return dict(d=d, n=n, A=A, y=y, m=m, gamma0=gamma0, form=form, L=L if form == "L" else None,
                u=(0.5 + rng.random(d) * 1.5) if form == "U" else None, oscn=oscn, rho=rho, lam=lam, t0=t0,
                x0=xscale * rng.standard_normal((nch, d)), th0=rng.standard_normal((nch, d)),
                seeds=np.uint64(3000 + seed) + np.arange(nch, dtype=np.uint64))


def ref_runs(P, T, c, adapt=False, factor=2.0, chains=None):
    return [B.pdmp(P["t0"], P["x0"][k], P["th0"][k], T, c, A=P["A"], y=P["y"], m=P["m"], gamma0=P["gamma0"], lambda_ref=P["lam"], rho=P["rho"],
                   L=P["L"], u_diag=P["u"], oscn=P["oscn"], adapt=adapt, factor=factor, seed=int(P["seeds"][k]), ev_cap=4096)
            for k in (range(len(P["x0"])) if chains is None else chains)]


def open_ensemble(pkg, P, c, cap=64, adapt=False, factor=2.0):
    nch, d = P["x0"].shape
    ens = pkg.Ensemble(nch, d, sampler=pkg._lib.SAMPLER_BPS, adapt=adapt, factor=factor, trace_capacity=cap)
    try:
        ens.set_flow_bps_modern(P["lam"], P["rho"], P["u"], P["oscn"])
        ens.set_target(pkg.LogisticRegressionTarget(P["A"], P["y"], P["m"], P["gamma0"]))
        if P["L"] is not None:
            ens.set_mass_cholesky(P["L"])
        ens.set_state_bps(P["t0"], P["x0"], P["th0"], c, P["seeds"])
    except Exception:
        ens.close()
        raise
    return ens


def one_run(pkg, P, n, c, adapt=False, factor=2.0, cap=64):
    with open_ensemble(pkg, P, c, cap=cap, adapt=adapt, factor=factor) as ens:
        ens.set_bps_record_limit(n)
        col = Collector(pkg, ens)
        col.drive(INF, pkg._lib.RUN_REFERENCE_TAIL)
        assert ens.kernel_name() == KERNEL
        return col.result()


C0 = 30.0  # LocalBound(c): large enough for every problem here without adapt


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("d", [1, 7, 64, 65, 129, 1024])
def test_slot_boundaries(gpu_pkg, d, n):
    """1, 2, 4 and 16 slots per lane with full and partial last slots, crossed with the observation counts around one LDS pass per lane; a
    sparse design; L = I.  30 records of 2 chains."""
    P = problem(d, n, 100 * d + n, nch=2)
    refs = ref_runs(P, 30, C0, adapt=True)
    assert all(r["status"] == B.REF_OK and r["num"] > 10 and r["nrefresh"] > 2 for r in refs)
    compare(one_run(gpu_pkg, P, 30, C0, adapt=True), refs)


@pytest.fixture(scope="module")
def flow_design():
    return sparse_design(130, 100, np.random.default_rng(77), density=0.08)


@pytest.mark.parametrize("form,oscn,rho", [("L", False, 0.9), ("U", False, 0.9), ("I", True, 0.0), ("I", True, 0.9), ("I", True, 1.0)])
def test_flow_forms(gpu_pkg, flow_design, form, oscn, rho):
    d, n = 100, 130
    rng = np.random.default_rng(8)
    Ls = sp.diags([0.8 + 0.4 * rng.random(d), 0.3 * rng.standard_normal(d - 1), 0.2 * rng.standard_normal(d - 7)], [0, -1, -7], format="csc")
    Ls.sort_indices()
    P = problem(d, n, 21, A=flow_design, form=form, L=sp.csc_matrix(Ls), oscn=oscn, rho=rho)
    refs = ref_runs(P, 40, C0, adapt=True)
    assert all(r["status"] == B.REF_OK and r["nacc"] > 5 and r["nrefresh"] > 3 for r in refs)
    if oscn:
        assert all((r["noscn_draws"] == 0) == (rho == 1.0) for r in refs)
    compare(one_run(gpu_pkg, P, 40, C0, adapt=True), refs)


@pytest.mark.parametrize("case", ["m015", "y0", "ym", "gamma0", "eta750"])
def test_data_forms(gpu_pkg, case):
    d, n = 7, 65
    rng = np.random.default_rng(31)
    A = sparse_design(n, d, rng)
    kw = {}
    if case == "m015":
        kw["m"] = np.array([0.0, 1.0, 5.0])[np.arange(n) % 3]
    elif case == "y0":
        kw["m"] = rng.integers(1, 4, n)
        kw["y"] = np.zeros(n)
    elif case == "ym":
        kw["m"] = rng.integers(1, 4, n)
        kw["y"] = kw["m"]
    elif case == "gamma0":
        kw["gamma0"] = 0.0
    P = problem(d, n, 32, A=A, **kw)
    if case == "eta750":  # two rows scaled so that |η| passes 750 during the run, starting below it: p reaches exactly 1 on one, 0 on the other
        D = A.toarray()
        D[4], D[5] = 0.0, 0.0
        D[4, 2], D[5, 3] = 800.0, 800.0
        P["A"] = sp.csc_matrix(D)
        P["x0"][:, 2], P["th0"][:, 2] = np.array([0.9, 0.92, 0.93]), np.array([1.0, 0.8, 0.6])
        P["x0"][:, 3], P["th0"][:, 3] = -np.array([0.9, 0.92, 0.93]), -np.array([1.0, 0.8, 0.6])
        P["y"][4], P["m"][4] = 2.0, 2.0  # (all successes: nothing but the prior holds η back on the way up)
        P["y"][5], P["m"][5] = 0.0, 2.0  # (no success: nor on the way down)
    refs = ref_runs(P, 40, C0, adapt=True)
    assert all(r["status"] == B.REF_OK and r["num"] > 10 for r in refs)
    if case == "eta750":
        # every chain starts below 750 on both rows; on the way down exp(−η) is +Inf from the setup on (η < −709.8: p = 0 exactly), and on the
        # way up the records (one per unit of time: the path between them is not seen here) show η past 750 on two of the three chains
        assert np.all(np.abs(800.0 * P["x0"][:, 2:4]) < 750) and np.all(800.0 * P["x0"][:, 3] < -709.8)
        assert sum((800.0 * r["x"][:, 2]).max() > 750 for r in refs) >= 2
    compare(one_run(gpu_pkg, P, 40, C0, adapt=True), refs)


@pytest.fixture(scope="module", params=["I", "U", "oscn"])
def resumption_case(request, flow_design):
    form = request.param
    P = problem(100, 130, 50, A=flow_design, form="U" if form == "U" else "I", oscn=form == "oscn")
    T = 30.0 if form != "U" else 4.0
    refs = ref_runs(P, T, C0)
    assert all(r["status"] == B.REF_OK and 20 <= r["nevents"] <= 200 for r in refs)
    return P, T, refs


def test_resume_stop_before_slices(gpu_pkg, resumption_case):
    """Slices end between two records: an η gathered afresh at the start of a launch, instead of the carried one, fails here."""
    P, T, refs = resumption_case
    L = gpu_pkg._lib
    with open_ensemble(gpu_pkg, P, C0) as ens:
        col = Collector(gpu_pkg, ens)
        for Tk in np.linspace(0.0, T, 8)[1:] - 0.37 * T / 7:
            cnt = col.drive(float(Tk), L.RUN_STOP_BEFORE)
            assert np.all(cnt["t_last"] < Tk) and np.all(cnt["status"] == L.CHAIN_OK)
        col.drive(T, L.RUN_REFERENCE_TAIL)
        assert ens.kernel_name() == KERNEL
        compare(col.result(), refs)


def test_resume_trace_capacity_four(gpu_pkg, resumption_case):
    P, T, refs = resumption_case
    L = gpu_pkg._lib
    with open_ensemble(gpu_pkg, P, C0, cap=4) as ens:
        col = Collector(gpu_pkg, ens)
        col.drive(T, L.RUN_REFERENCE_TAIL)
        assert L.CHAIN_TRACE_FULL in col.statuses and col.launches >= 5
        compare(col.result(), refs)


def test_resume_launch_count_limit_pauses(gpu_pkg, resumption_case):
    P, T, refs = resumption_case
    L = gpu_pkg._lib
    with open_ensemble(gpu_pkg, P, C0, cap=256) as ens:
        L.check(ens._L.pdmp_debug_set_launch_count_limit(ens._h, 300))
        col = Collector(gpu_pkg, ens)
        col.drive(T, L.RUN_REFERENCE_TAIL)
        assert L.CHAIN_PAUSED in col.statuses and col.launches >= 5
        compare(col.result(), refs)


def test_resume_record_limit_raised_in_three_steps(gpu_pkg, resumption_case):
    P, T, _ = resumption_case
    L = gpu_pkg._lib
    refs = ref_runs(P, 36, C0)
    with open_ensemble(gpu_pkg, P, C0) as ens:
        col = Collector(gpu_pkg, ens)
        for step in (12, 24, 36):
            ens.set_bps_record_limit(step)
            cnt = col.drive(INF, L.RUN_REFERENCE_TAIL)
            assert np.all(cnt["nevents"] == step)
        compare(col.result(), refs)


@pytest.mark.parametrize("c", [1e-20, 3e-16])
def test_adapt_and_bound_violated(gpu_pkg, c):
    P = problem(7, 65, 41)
    refs = ref_runs(P, 40, c, adapt=True, factor=2.0)
    assert all(r["status"] == B.REF_OK and r["nviol"] >= 2 and r["c_final"] > c for r in refs)
    compare(one_run(gpu_pkg, P, 40, c, adapt=True, factor=2.0), refs)
    bad = ref_runs(P, 40, c)
    assert all(r["status"] == B.REF_BOUND_VIOLATED and r["nevents"] < 40 for r in bad)
    res = one_run(gpu_pkg, P, 40, c)
    assert np.all(res["cnt"]["status"] == gpu_pkg._lib.CHAIN_BOUND_VIOLATED)
    compare(res, bad)


def lds_problem(n):
    rng = np.random.default_rng(n)
    A = sp.csc_matrix(0.02 * rng.standard_normal((n, 1)))
    return problem(1, n, n, A=A, nch=1, m=np.ones(n), y=(rng.random(n) < 0.5).astype(np.float64))


@pytest.mark.parametrize("n", [4097, 10239])
def test_lds_past_64k_and_largest(gpu_pkg, n):
    """d = 1: 8 + 16 n bytes of LDS -- n = 4097 is the first size past 64 KiB (the kernel opts in), n = 10239 the largest accepted."""
    P = lds_problem(n)
    refs = ref_runs(P, 5, C0, adapt=True)
    assert all(r["status"] == B.REF_OK for r in refs)
    compare(one_run(gpu_pkg, P, 5, C0, adapt=True), refs)


def test_lds_limit_refused(gpu_pkg):
    L = gpu_pkg._lib
    P = lds_problem(10240)
    with pytest.raises(L.PdmpError) as ei:
        open_ensemble(gpu_pkg, P, C0)
    assert ei.value.code == L.PDMP_ERR_UNSUPPORTED and "n = 10240" in str(ei.value) and "163848" in str(ei.value)


def test_refusals(gpu_pkg):
    """Every refusal of the header: its status, and a message naming the cause."""
    pkg = gpu_pkg
    L = pkg._lib
    UNS, INV = L.PDMP_ERR_UNSUPPORTED, L.PDMP_ERR_INVALID
    d, n = 4, 6
    rng = np.random.default_rng(3)
    A, At, arrs = B.design(sp.csc_matrix(rng.standard_normal((n, d)) * (rng.random((n, d)) < 0.6) + np.eye(n, d)))
    y, m = np.ones(n), np.full(n, 2.0)
    x0, th0 = rng.standard_normal((1, d)), rng.standard_normal((1, d))
    seeds = np.array([1], dtype=np.uint64)
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(ens, n_=n, arrs_=None, y_=y, m_=m, g0=0.5):
        a = list(arrs if arrs_ is None else arrs_)
        return ens._L.pdmp_ensemble_set_target_bps_logistic(ens._h, n_, *[ptr(v) for v in a], ptr(y_), ptr(m_), g0)

    def refused(code, word, **kw):
        with pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, trace_capacity=8) as ens:
            ens.set_flow_bps_modern(1.0, 0.9, None, False)
            with pytest.raises(L.PdmpError) as ei:
                L.check(call(ens, **kw))
            assert ei.value.code == code and word in str(ei.value), str(ei.value)

    def changed(k, f):
        a = [v.copy() for v in arrs]
        f(a[k])
        return a

    for k in range(6):
        refused(INV, "null", arrs_=[None if j == k else v for j, v in enumerate(arrs)])
    refused(INV, "null", y_=None)
    refused(INV, "null", m_=None)
    refused(INV, "n = 0", n_=0)
    refused(INV, "n = -3", n_=-3)
    refused(INV, "colptr[0]", arrs_=changed(0, lambda v: v.__setitem__(0, 1)))
    refused(INV, "colptr[0]", arrs_=changed(3, lambda v: v.__setitem__(0, 1)))
    refused(INV, "nnz", arrs_=changed(3, lambda v: v.__setitem__(n, v[n] - 1)))
    refused(INV, "out of range", arrs_=changed(1, lambda v: v.__setitem__(0, n)))
    refused(INV, "out of range", arrs_=changed(4, lambda v: v.__setitem__(0, -1)))
    col = int(np.argmax(np.diff(arrs[0]) >= 2))  # a column of A with two entries: swap them
    q = int(arrs[0][col])
    refused(INV, "ascending", arrs_=changed(1, lambda v: v.__setitem__(slice(q, q + 2), v[q:q + 2][::-1].copy())))
    row = int(np.argmax(np.diff(arrs[3]) >= 1))
    q2 = int(arrs[3][row])
    other = next(j for j in range(d) if j not in arrs[4][arrs[3][row]:arrs[3][row + 1]])
    wrong = changed(4, lambda v: v.__setitem__(slice(arrs[3][row], arrs[3][row + 1]), np.sort(np.r_[v[q2 + 1:arrs[3][row + 1]], other])))
    refused(INV, "transpose", arrs_=wrong)
    for bad_y in (np.where(np.arange(n) == 2, 3.0, y), np.where(np.arange(n) == 2, -1.0, y), np.where(np.arange(n) == 1, np.nan, y)):
        refused(INV, "y[", y_=bad_y)
    for bad_m in (np.where(np.arange(n) == 2, -1.0, m), np.where(np.arange(n) == 0, np.inf, m), np.where(np.arange(n) == 0, np.nan, m)):
        refused(INV, "m[", m_=bad_m)
    for g0 in (-0.1, np.inf, np.nan):
        refused(INV, "gamma0", g0=g0)
    # another sampler; no flow; a state exists
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_ZIGZAG_LOCAL) as ens:
        with pytest.raises(L.PdmpError) as ei:
            L.check(call(ens))
        assert ei.value.code == INV and "PDMP_SAMPLER_BPS" in str(ei.value)
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, trace_capacity=8) as ens:
        with pytest.raises(L.PdmpError) as ei:
            L.check(call(ens))
        assert ei.value.code == INV and "set_flow_bps_modern" in str(ei.value)
        ens.set_flow_bps_modern(1.0, 0.9, None, False)
        with pytest.raises(L.PdmpError) as ei:  # the target is missing: both setters are named
            ens.set_state_bps(0.0, x0, th0, 5.0, seeds)
        assert ei.value.code == INV and "set_target_gaussian_csc" in str(ei.value) and "set_target_bps_logistic" in str(ei.value)
        L.check(call(ens))
        ens.set_state_bps(0.0, x0, th0, 5.0, seeds)
        with pytest.raises(L.PdmpError) as ei:
            L.check(call(ens))
        assert ei.value.code == INV and "set_state_bps" in str(ei.value)
    # flows other than set_flow_bps_modern: UNSUPPORTED at set_state_bps, naming the flow
    T = pkg.LogisticRegressionTarget(A, y, m, 0.5)
    I = sp.identity(d, format="csc")
    for word, setup in (("set_flow_bps", lambda e: e.set_flow_bps(pkg.BouncyParticle(I, np.zeros(d), 1.0))),
                        ("Boomerang", lambda e: e.set_flow_boomerang(pkg.GaussianTarget(I), pkg.Boomerang(I, np.zeros(d), 1.0))),
                        ("sticky", lambda e: (e.set_flow_bps(pkg.BouncyParticle(I, np.zeros(d), 1.0)), e.set_bps_sticky(1.5)))):
        with pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, trace_capacity=8) as ens:
            setup(ens)
            ens.set_target(T)
            with pytest.raises(L.PdmpError) as ei:
                ens.set_state_bps(0.0, x0, th0, 5.0, seeds)
            assert ei.value.code == UNS and word in str(ei.value) and "set_target_bps_logistic" in str(ei.value), str(ei.value)
    # the later of the two target calls wins
    G = sp.csc_matrix(np.diag([1.0, 2.0, 1.5, 0.7]))
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, trace_capacity=8) as ens:
        ens.set_flow_bps_modern(1.0, 0.9, None, False)
        ens.set_target(T)
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_state_bps(0.0, x0, th0, 5.0, seeds)
        ens.set_bps_record_limit(3)
        ens.run(INF)
        assert ens.kernel_name() == "bps_modern_run_kernel"
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, trace_capacity=8) as ens:
        ens.set_flow_bps_modern(1.0, 0.9, None, False)
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_target(T)
        ens.set_state_bps(0.0, x0, th0, 5.0, seeds)
        ens.set_bps_record_limit(3)
        ens.run(INF)
        assert ens.kernel_name() == KERNEL


def test_gaussian_ensemble_after_a_logistic_one_is_unchanged(gpu_pkg):
    """A Gaussian ModernBPS ensemble created after a logistic one in the same process: bit for bit modern_bps_ref's."""
    import test_gpu_modern_bps_parity as G
    P = problem(65, 64, 9)
    one_run(gpu_pkg, P, 10, C0, adapt=True)
    Pg = G.problem(65, 9)
    refs = G.ref_runs(Pg, 30, 5.0)
    assert all(r["status"] == M.REF_OK for r in refs)
    compare(G.one_run(gpu_pkg, Pg, 30, 5.0), refs)


def test_ensemble_width(gpu_pkg):
    """300 chains, d = 10, n = 100: chains 0, 150 and 299 against the restatement, every chain OK with exactly 20 records."""
    nch = 300
    P = problem(10, 100, 77, nch=nch)
    chains = [0, 150, nch - 1]
    refs = ref_runs(P, 20, C0, adapt=True, chains=chains)
    res = one_run(gpu_pkg, P, 20, C0, adapt=True, cap=20)
    assert np.all(res["cnt"]["status"] == gpu_pkg._lib.CHAIN_OK) and np.all(res["cnt"]["nevents"] == 20)
    compare(res, refs, chains=chains)


def test_posterior_envelope_through_pdmp(gpu_pkg):
    """The d = 2 envelope case of tests/test_bps_logistic_ref.py on the device through samplers.pdmp, seeds 0, 1, 2, against the quadrature
    truth; the records are the restatement's; with consume=, the device's mean is trace.mean of the returned trace."""
    pkg = gpu_pkg
    E = B.envelope_case()
    mean, cov = B.posterior_quadrature(E, 8.0, 801)
    seeds = B.ENVELOPE_SEEDS
    nch = len(seeds)
    assert seeds == tuple(range(seeds[0], seeds[0] + nch))
    target = pkg.LogisticRegressionTarget(E["A"], E["y"], E["m"], E["gamma0"])
    Bf = pkg.BouncyParticle(None, None, E["lambda_ref"], E["rho"])
    x0, th0 = np.tile(E["x0"], (nch, 1)), np.tile(E["th0"], (nch, 1))
    tr, (t, x, th), (acc, num), cout = pkg.pdmp(target, 0.0, x0, th0, E["nrec"], pkg.LocalBound(E["c"]), Bf, adapt=True, seed=seeds[0])
    for k, seed in enumerate(seeds):
        r = B.pdmp(0.0, E["x0"], E["th0"], E["nrec"], E["c"], A=E["A"], y=E["y"], m=E["m"], gamma0=E["gamma0"], lambda_ref=E["lambda_ref"],
                   rho=E["rho"], adapt=True, seed=seed)
        assert len(tr[k].t) == E["nrec"]
        assert same(tr[k].t, r["t"]) and same(tr[k].x, r["x"]) and same(tr[k].θ, r["theta"])
        assert (int(acc[k]), int(num[k])) == (r["nacc"], r["num"]) and cout[k] == r["c_final"] and t[k] == r["t_final"]
        m_, cv, bound = B.envelope_stats(tr[k].x, mean, cov)
        print("device, seed %d: mean %.4f cov %.4f bound %.4f" % (seed, m_, cv, bound))
        assert m_ < bound and cv < bound
    out = pkg.pdmp(target, 0.0, x0, th0, 60, pkg.LocalBound(E["c"]), Bf, adapt=True, seed=seeds[0], consume=dict(dt=0.5, points=200))
    tr2, cons = out[0], out[4]
    for k in range(nch):
        assert same(tr2[k].t, tr[k].t[:60]) and same(tr2[k].x, tr[k].x[:60])
        want = pkg.trace.mean(tr2[k])
        assert np.allclose(cons["mean"][k], want, rtol=1e-12, atol=1e-14), (cons["mean"][k], want)
