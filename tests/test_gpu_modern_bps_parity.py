"""The speed-recorded Bouncy Particle on gfx950 (csrc/pdmp_bps_modern.inc) vs the sequential restatement of
src/not_fact_samplers.jl:151-384 (tests/ref/modern_bps_ref.c), through the C ABI's Python binding and the Python pdmp (-m gpu): records
(t, x, θ), counters, status and the final (t, x, θ, c) bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sp

import modern_bps_ref_lib as M
from test_modern_bps_ref import ENVELOPE_SEEDS

pytestmark = pytest.mark.gpu

INF = float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def tridiag(d):
    if d == 1:
        return sp.csc_matrix(np.array([[1.7]]))
    k = np.arange(d)
    G = sp.diags([np.full(d - 1, -0.45), 1.5 + 0.5 * np.cos(k), np.full(d - 1, -0.45)], [-1, 0, 1], format="csc")
    G.sort_indices()
    return sp.csc_matrix(G)


def problem(d, seed, form="I", L=None, oscn=False, rho=0.9, lam=1.0, nch=3, gamma=None, t0=0.0):
    """form "I": the L form with L = I; "L": the L form with the factor L; "U": the diagonal-U form with a non-constant u."""
    rng = np.random.default_rng(seed)
    P = dict(d=d, G=tridiag(d) if gamma is None else gamma, mu=0.3 * rng.standard_normal(d), form=form, L=L if form == "L" else None,
             u=(0.5 + rng.random(d) * 1.5) if form == "U" else None, oscn=oscn, rho=rho, lam=lam, t0=t0,
             x0=rng.standard_normal((nch, d)), th0=rng.standard_normal((nch, d)), seeds=np.uint64(1000 + seed) + np.arange(nch, dtype=np.uint64))
    return P


def ref_runs(P, T, c, adapt=False, factor=2.0, chains=None):
    out = []
    for k in (range(len(P["x0"])) if chains is None else chains):
        out.append(M.pdmp(P["t0"], P["x0"][k], P["th0"][k], T, c, gamma=P["G"], mu=P["mu"], lambda_ref=P["lam"], rho=P["rho"], L=P["L"],
                          u_diag=P["u"], oscn=P["oscn"], adapt=adapt, factor=factor, seed=int(P["seeds"][k]), ev_cap=4096))
    return out


def open_ensemble(pkg, P, c, cap=64, adapt=False, factor=2.0):
    nch, d = P["x0"].shape
    ens = pkg.Ensemble(nch, d, sampler=pkg._lib.SAMPLER_BPS, adapt=adapt, factor=factor, trace_capacity=cap)
    try:
        ens.set_flow_bps_modern(P["lam"], P["rho"], P["u"], P["oscn"])
        ens.set_target(pkg.GaussianTarget(P["G"], P["mu"]))
        if P["L"] is not None:
            ens.set_mass_cholesky(sp.csc_matrix(np.tril(P["L"])) if not sp.issparse(P["L"]) else P["L"])
        ens.set_state_bps(P["t0"], P["x0"], P["th0"], c, P["seeds"])
    except Exception:
        ens.close()
        raise
    return ens


class Collector:
    """Drives an ensemble and keeps every chain's records across drains; counts the launches."""

    def __init__(self, pkg, ens):
        self.L, self.ens = pkg._lib, ens
        self.t = [[] for _ in range(ens.nchains)]
        self.x = [[] for _ in range(ens.nchains)]
        self.th = [[] for _ in range(ens.nchains)]
        self.launches = 0
        self.statuses = set()

    def drive(self, T, flags):
        for _ in range(100000):
            self.ens.run(T, flags)
            self.launches += 1
            cnt = self.ens.counters()
            self.statuses |= set(int(s) for s in cnt["status"])
            for k in range(self.ens.nchains):
                if cnt["ntrace"][k]:
                    a, b, c = self.ens.bps_trace(k, counters=cnt)
                    self.t[k].append(a)
                    self.x[k].append(b)
                    self.th[k].append(c)
            self.ens.trace_reset()
            if not self.L.needs_rerun(cnt["status"]):
                return cnt
        raise AssertionError("the run does not end")

    def result(self):
        d = self.ens.d
        cnt = self.ens.counters()
        fs = self.ens.bps_final_state()
        cat = lambda v, shape: np.concatenate(v) if v else np.empty(shape)
        return dict(cnt=cnt, fs=fs, t=[cat(v, 0) for v in self.t], x=[cat(v, (0, d)) for v in self.x], th=[cat(v, (0, d)) for v in self.th])


def compare(res, refs, chains=None):
    for j, r in enumerate(refs):
        k = j if chains is None else chains[j]
        cnt, fs = res["cnt"], res["fs"]
        assert int(cnt["status"][k]) == r["status"], (k, int(cnt["status"][k]), r["status"])
        for name in ("num", "nacc", "nrefresh", "nevents", "ndraw_main"):
            assert int(cnt[name][k]) == r[name], (k, name, int(cnt[name][k]), r[name])
        assert len(res["t"][k]) == len(r["t"]) == r["nevents"], (k, len(res["t"][k]), r["nevents"])
        assert same(res["t"][k], r["t"]) and same(res["x"][k], r["x"]) and same(res["th"][k], r["theta"]), k
        assert same(fs["t"][k], r["t_final"]) and same(fs["c"][k], r["c_final"]), (k, fs["t"][k], r["t_final"], fs["c"][k], r["c_final"])
        assert same(fs["x"][k], r["x_final"]) and same(fs["theta"][k], r["theta_final"]), k


def one_run(pkg, P, n, c, adapt=False, factor=2.0, cap=64):
    with open_ensemble(pkg, P, c, cap=cap, adapt=adapt, factor=factor) as ens:
        ens.set_bps_record_limit(n)
        col = Collector(pkg, ens)
        col.drive(INF, pkg._lib.RUN_REFERENCE_TAIL)
        assert ens.kernel_name() == "bps_modern_run_kernel"
        return col.result()


@pytest.mark.parametrize("form", ["I", "U"])
@pytest.mark.parametrize("d", [1, 7, 64, 100, 129, 257, 1024])
def test_every_width_and_tail(gpu_pkg, d, form):
    """1, 2 and 16 slots per lane, full and partial last slots, and 4 and 8 with wholly empty trailing slots (d = 129, 257); a tridiagonal target
    with a mean: 40 records of 3 chains.  Every slot count with a Γ that couples slots, `oscn` and a factor: tests/test_gpu_bps_widths.py."""
    P = problem(d, d, form=form, rho=0.9 if d != 64 else 0.0)
    c = 5.0
    refs = ref_runs(P, 40, c)
    assert all(r["status"] == M.REF_OK and r["num"] > 20 and r["nrefresh"] > 3 for r in refs)
    compare(one_run(gpu_pkg, P, 40, c), refs)


def test_mass_factor(gpu_pkg):
    """A sparse lower-triangular L at d = 100 (set_mass_cholesky) and the dense L of the envelope test at d = 8."""
    d = 100
    rng = np.random.default_rng(8)
    Ls = sp.diags([0.8 + 0.4 * rng.random(d), 0.3 * rng.standard_normal(d - 1), 0.2 * rng.standard_normal(d - 7)], [0, -1, -7], format="csc")
    Ls.sort_indices()
    P = problem(d, 21, form="L", L=sp.csc_matrix(Ls))
    refs = ref_runs(P, 40, 5.0)
    assert all(r["status"] == M.REF_OK and r["nacc"] > 10 and r["nrefresh"] > 3 for r in refs)
    compare(one_run(gpu_pkg, P, 40, 5.0), refs)
    E = M.envelope_case(gpu_pkg.problems.maintest_precision(8))
    P = problem(8, 22, form="L", L=E["L"], gamma=E["gamma"])
    refs = ref_runs(P, 60, E["c"])
    assert all(r["status"] == M.REF_OK and r["nacc"] > 10 for r in refs)
    compare(one_run(gpu_pkg, P, 60, E["c"]), refs)


@pytest.mark.parametrize("d", [7, 100])
@pytest.mark.parametrize("rho", [0.0, 0.9, 1.0])
def test_oscn(gpu_pkg, rho, d):
    P = problem(d, 30 + d, oscn=True, rho=rho)
    refs = ref_runs(P, 40, 5.0)
    assert all(r["status"] == M.REF_OK and r["nacc"] > 5 for r in refs)
    assert all((r["noscn_draws"] == 0) == (rho == 1.0) for r in refs)
    compare(one_run(gpu_pkg, P, 40, 5.0), refs)


@pytest.mark.parametrize("form", ["I", "U"])
@pytest.mark.parametrize("c", [1e-20, 3e-16])
def test_adapt_and_bound_violated(gpu_pkg, c, form):
    """c far too small: with adapt it is multiplied up at the same violations as in the restatement; without, every chain ends as
    BOUND_VIOLATED at the same record count with the same state."""
    P = problem(7, 41, form=form)
    refs = ref_runs(P, 40, c, adapt=True, factor=2.0)
    assert all(r["status"] == M.REF_OK and r["nviol"] >= 2 and r["c_final"] > c for r in refs)
    compare(one_run(gpu_pkg, P, 40, c, adapt=True, factor=2.0), refs)
    bad = ref_runs(P, 40, c)
    assert all(r["status"] == M.REF_BOUND_VIOLATED and r["nevents"] < 40 for r in bad)
    res = one_run(gpu_pkg, P, 40, c)
    assert np.all(res["cnt"]["status"] == gpu_pkg._lib.CHAIN_BOUND_VIOLATED)
    compare(res, bad)


@pytest.fixture(scope="module", params=["I", "U", "oscn"])
def resumption_case(request):
    form = request.param
    P = problem(100, 50, form="U" if form == "U" else "I", oscn=form == "oscn")
    T = 30.0 if form != "U" else 4.0
    refs = ref_runs(P, T, 5.0)
    assert all(r["status"] == M.REF_OK and 20 <= r["nevents"] <= 200 for r in refs)
    return P, T, refs


def test_resume_stop_before_slices(gpu_pkg, resumption_case):
    P, T, refs = resumption_case
    L = gpu_pkg._lib
    with open_ensemble(gpu_pkg, P, 5.0) as ens:
        col = Collector(gpu_pkg, ens)
        for Tk in np.linspace(0.0, T, 8)[1:]:
            cnt = col.drive(float(Tk), L.RUN_STOP_BEFORE)
            assert np.all(cnt["t_last"] < Tk) and np.all(cnt["status"] == L.CHAIN_OK)
        col.drive(T, L.RUN_REFERENCE_TAIL)
        compare(col.result(), refs)


def test_resume_trace_capacity_four(gpu_pkg, resumption_case):
    P, T, refs = resumption_case
    L = gpu_pkg._lib
    with open_ensemble(gpu_pkg, P, 5.0, cap=4) as ens:
        col = Collector(gpu_pkg, ens)
        col.drive(T, L.RUN_REFERENCE_TAIL)
        assert L.CHAIN_TRACE_FULL in col.statuses and col.launches >= 5
        compare(col.result(), refs)


def test_resume_launch_count_limit_pauses(gpu_pkg, resumption_case):
    P, T, refs = resumption_case
    L = gpu_pkg._lib
    with open_ensemble(gpu_pkg, P, 5.0, cap=256) as ens:
        L.check(ens._L.pdmp_debug_set_launch_count_limit(ens._h, 300))
        col = Collector(gpu_pkg, ens)
        col.drive(T, L.RUN_REFERENCE_TAIL)
        assert L.CHAIN_PAUSED in col.statuses and col.launches >= 5
        compare(col.result(), refs)


def test_resume_record_limit_raised_in_three_steps(gpu_pkg, resumption_case):
    P, T, _ = resumption_case
    L = gpu_pkg._lib
    n = 36
    refs = ref_runs(P, n, 5.0)
    with open_ensemble(gpu_pkg, P, 5.0) as ens:
        col = Collector(gpu_pkg, ens)
        for step in (12, 24, 36):
            ens.set_bps_record_limit(step)
            cnt = col.drive(INF, L.RUN_REFERENCE_TAIL)
            assert np.all(cnt["nevents"] == step)
        col.drive(INF, L.RUN_REFERENCE_TAIL)  # (the limit is reached: nothing more happens)
        compare(col.result(), refs)
    # T and n together: whichever comes first, per chain
    both = ref_runs(P, (T / 2, 10), 5.0)
    with open_ensemble(gpu_pkg, P, 5.0) as ens:
        ens.set_bps_record_limit(10)
        col = Collector(gpu_pkg, ens)
        col.drive(T / 2, L.RUN_REFERENCE_TAIL)
        compare(col.result(), both)


def test_refusals(gpu_pkg):
    """Every refusal of the header: its status, and a message naming the option."""
    pkg = gpu_pkg
    L = pkg._lib
    d = 8
    G = tridiag(d)
    rng = np.random.default_rng(3)
    x0, th0 = rng.standard_normal((1, d)), rng.standard_normal((1, d))
    seeds = np.array([1], dtype=np.uint64)
    u = 0.5 + rng.random(d)
    Lf = sp.csc_matrix(np.tril(np.eye(d) + 0.1 * rng.standard_normal((d, d))))

    def refused(code, word, setup, d_=d, state=True):
        with pkg.Ensemble(1, d_, sampler=L.SAMPLER_BPS, trace_capacity=8) as ens:
            with pytest.raises(L.PdmpError) as ei:
                setup(ens)
                if state:
                    ens.set_state_bps(0.0, x0, th0, 5.0, seeds)
            assert ei.value.code == code and word in str(ei.value), str(ei.value)

    def base(ens, u_diag=None, oscn=False):
        ens.set_flow_bps_modern(1.0, 0.9, u_diag, oscn)
        ens.set_target(pkg.GaussianTarget(G))

    UNS, INV = L.PDMP_ERR_UNSUPPORTED, L.PDMP_ERR_INVALID
    refused(UNS, "set_bps_moments", lambda e: (base(e), e.set_bps_moments(1)))
    refused(UNS, "set_bps_sticky", lambda e: (base(e), e.set_bps_sticky(1.5)))
    refused(UNS, "subsample", lambda e: (base(e), e.set_bps_options(False, True)))
    refused(UNS, "local_bound", lambda e: (base(e), e.set_bps_options(True, False)))
    refused(UNS, "oscn", lambda e: base(e, u, True))
    refused(UNS, "oscn", lambda e: (base(e, None, True), e.set_mass_cholesky(Lf)))
    refused(UNS, "u_diag", lambda e: (base(e, u), e.set_mass_cholesky(Lf)))
    refused(INV, "set_target_gaussian_csc", lambda e: e.set_flow_bps_modern(1.0, 0.9, None, False))  # the target is missing
    refused(INV, "refreshment rate", lambda e: e.set_flow_bps_modern(0.0, 0.9, None, False), state=False)
    refused(INV, "rho", lambda e: e.set_flow_bps_modern(1.0, 1.5, None, False), state=False)
    for badu in (np.where(np.arange(d) == 3, 0.0, u), np.where(np.arange(d) == 5, np.inf, u), np.where(np.arange(d) == 1, np.nan, u)):
        refused(INV, "u_diag", lambda e, b=badu: e.set_flow_bps_modern(1.0, 0.9, b, False), state=False)
    # d > 1024
    big = 1025
    with pkg.Ensemble(1, big, sampler=L.SAMPLER_BPS, trace_capacity=2) as ens:
        ens.set_flow_bps_modern(1.0, 0.9, None, False)
        ens.set_target(pkg.GaussianTarget(sp.identity(big, format="csc")))
        with pytest.raises(L.PdmpError) as ei:
            ens.set_state_bps(0.0, np.zeros((1, big)), np.ones((1, big)), 5.0, seeds)
        assert ei.value.code == UNS and "1024" in str(ei.value)
    # another sampler; a state exists
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_ZIGZAG_LOCAL) as ens:
        with pytest.raises(L.PdmpError) as ei:
            ens.set_flow_bps_modern(1.0, 0.9, None, False)
        assert ei.value.code == INV and "PDMP_SAMPLER_BPS" in str(ei.value)
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, trace_capacity=8) as ens:
        base(ens)
        ens.set_state_bps(0.0, x0, th0, 5.0, seeds)
        with pytest.raises(L.PdmpError) as ei:
            ens.set_flow_bps_modern(1.0, 0.9, None, False)
        assert ei.value.code == INV and "set_state_bps" in str(ei.value)
    # any set_flow_* clears the setting: the record limit belongs to the modern flow only, and a plain flow runs the plain kernel
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BPS, trace_capacity=64) as ens:
        base(ens)
        ens.set_flow_bps(pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0))
        with pytest.raises(L.PdmpError) as ei:
            ens.set_bps_record_limit(5)
        assert ei.value.code == INV and "set_flow_bps_modern" in str(ei.value)
        ens.set_state_bps(0.0, x0, th0, 0.5, seeds)
        ens.run(2.0)
        assert ens.kernel_name() == "bps_run_kernel"


def test_plain_and_sticky_ensembles_after_a_modern_one_are_unchanged(gpu_pkg):
    import oracle_lib as O
    import sticky_ref_lib as R
    pkg = gpu_pkg
    d = 64
    I = sp.identity(d, format="csc")
    rng = np.random.default_rng(2)
    x0, th0 = rng.standard_normal((2, d)), rng.standard_normal((2, d))
    Bm = pkg.BouncyParticle(None, None, 1.0, 0.9)
    pkg.pdmp(pkg.GaussianTarget(tridiag(d)), 0.0, x0, th0, 10, pkg.LocalBound(5.0), Bm, seed=3)
    B = pkg.BouncyParticle(I, np.zeros(d), 1.0)
    tr, (t, x, th), (acc, num), cout = pkg.pdmp(None, 0.0, x0, th0, 10.0, 1e-3, B, seed=3)
    for k in range(2):
        r = O.pdmp_bps(I, None, x0[k], th0[k], 1e-3, 10.0, lambda_ref=1.0, seed=3 + k, ev_cap=200000)
        assert np.array_equal(tr[k].t, r["t_ev"]) and np.array_equal(tr[k].x, r["x_ev"]) and np.array_equal(tr[k].θ, r["theta_ev"])
        assert (int(acc[k]), int(num[k])) == (r["nacc"], r["num"]) and np.array_equal(x[k], r["x"])
    tr, (t, x, th), (acc, num), cout = pkg.sspdmp(None, 0.0, x0, th0, 5.0, 0.5, B, 1.5, seed=3)
    for k in range(2):
        r = R.sspdmp_notfact(0.0, x0[k], th0[k], 5.0, 0.5, 1.5, flow_kind=0, gamma=I, mu=np.zeros(d), lambda_ref=1.0, seed=3 + k, ev_cap=400000)
        assert r["status"] == R.REF_OK and same(tr[k].t, r["t"]) and same(tr[k].x, r["x"]) and same(tr[k].θ, r["theta"])
        assert np.array_equal(tr[k].f, r["f"]) and (int(acc[k]), int(num[k])) == (r["nacc"], r["num"])


@pytest.mark.parametrize("form", ["L", "U"])
def test_reference_envelope_through_pdmp(gpu_pkg, form):
    """test/maintest.jl:209-242 on the device through samplers.pdmp, on the seeds of the CPU test: the 4-tuple of the reference, the
    records equal to the restatement's, mean|mean(xs)| < 3/√n and mean|cov(xs) − Γ⁻¹| < 3/√n."""
    pkg = gpu_pkg
    E = M.envelope_case(pkg.problems.maintest_precision(8))
    B = pkg.BouncyParticle(None, None, E["lambda_ref"], E["rho"], L=sp.csc_matrix(E["L"]) if form == "L" else None, U=E["u"] if form == "U" else None)
    nch = len(ENVELOPE_SEEDS)
    assert ENVELOPE_SEEDS == tuple(range(ENVELOPE_SEEDS[0], ENVELOPE_SEEDS[0] + nch))
    x0, th0 = np.tile(E["x0"], (nch, 1)), np.tile(E["th0"], (nch, 1))
    tr, (t, x, th), (acc, num), cout = pkg.pdmp(pkg.GaussianTarget(E["gamma"]), 0.0, x0, th0, E["n"], pkg.LocalBound(E["c"]), B,
                                                seed=ENVELOPE_SEEDS[0])
    for k, seed in enumerate(ENVELOPE_SEEDS):
        r = M.pdmp(0.0, E["x0"], E["th0"], E["n"], E["c"], gamma=E["gamma"], lambda_ref=E["lambda_ref"], rho=E["rho"], seed=seed,
                   L=E["L"] if form == "L" else None, u_diag=E["u"] if form == "U" else None)
        assert len(tr[k].t) == E["n"] and len(tr[k]) == E["n"] + 1
        assert same(tr[k].t, r["t"]) and same(tr[k].x, r["x"]) and same(tr[k].θ, r["theta"])
        assert (int(acc[k]), int(num[k])) == (r["nacc"], r["num"]) and cout[k] == r["c_final"] and t[k] == r["t_final"]
        m, cv, bound = M.envelope_stats(tr[k].x, E["gamma"])
        print("device, form %s seed %d: mean %.4f cov %.4f bound %.4f" % (form, seed, m, cv, bound))
        assert m < bound and cv < bound
    # one chain: scalars as the reference returns them; a float T ends past T; subsample=False is the reference's ArgumentError
    tr1, (t1, x1, th1), (a1, n1), c1 = pkg.pdmp(pkg.GaussianTarget(E["gamma"]), 0.0, E["x0"], E["th0"], 25.5, pkg.LocalBound(E["c"]), B,
                                                seed=ENVELOPE_SEEDS[0])
    assert tr1.t[-1] >= 25.5 and np.all(tr1.t[:-1] < 25.5) and t1 == tr1.t[-1] and isinstance(a1, int) and c1 == E["c"]
    assert same(tr1.t, tr[0].t[:len(tr1.t)]) and same(tr1.x, tr[0].x[:len(tr1.t)])
    with pytest.raises(ValueError, match="`subsample=true` required."):
        pkg.pdmp(pkg.GaussianTarget(E["gamma"]), 0.0, E["x0"], E["th0"], 10, pkg.LocalBound(E["c"]), B, subsample=False)


def test_ensemble_width(gpu_pkg):
    """4096 chains at d = 64 for 20 records: the first and the last chain bit for bit, every chain OK with exactly 20 records."""
    nch, d = 4096, 64
    P = problem(d, 77, nch=nch)
    refs = ref_runs(P, 20, 5.0, chains=[0, nch - 1])
    res = one_run(gpu_pkg, P, 20, 5.0, cap=20)
    assert np.all(res["cnt"]["status"] == gpu_pkg._lib.CHAIN_OK) and np.all(res["cnt"]["nevents"] == 20)
    assert all(len(t) == 20 for t in res["t"])
    compare(res, refs, chains=[0, nch - 1])
