"""The two side channels of pdmp_ensemble_run (-m gpu): the phase profile (pdmp_debug_set_phase_profile / pdmp_debug_phase_profile, what
tools/phase_profile.py reads) and the refusals a run raises instead of launching another kernel than the one asked for.

One small ensemble per event-loop kernel family.  Without the profile every family refuses pdmp_debug_phase_profile; with it, the families
whose kernels have a profiling instantiation return their kind (1: the speculative, tracked and one-proposal-per-lane kernels; 2: the general
and logistic kernels) and the others (Bouncy Particle, both sticky kernels, the one-event kernel) still refuse.  pdmp_ensemble_last_run_ms
answers after every run.  The expectations are the behaviour of the dispatch as it was before it was gathered into one selection and one
epilogue; a refused run leaves the kernel name and the timing of the ensemble as they were."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

NO_PROFILE = "no phase profile recorded by the last run"


def _state(ens, pkg, d, nch, c, seed, sigma=None, x0=None):
    rng = np.random.default_rng(seed)
    if x0 is None:
        x0 = rng.standard_normal((nch, d))
    th0 = (np.ones(d) if sigma is None else sigma) * rng.choice([-1.0, 1.0], (nch, d))
    ens.set_state(0.0, x0, th0, c, np.arange(nch, dtype=np.uint64) + np.uint64(500 + seed))


def _lattice(pkg, ens, n=48, tracked=False, mu_f=None, mu_t=None, c_scale=1.0, kappa=None, seed=1):
    G = pkg.problems.gmrf_precision(n, 0.5) if kappa is not None else pkg.problems.gmrf_precision(n)
    d = G.shape[0]
    ens.set_flow(pkg.ZigZag(G, np.zeros(d) if mu_f is None else mu_f))
    ens.set_target(pkg.GaussianTarget(G, mu_t))
    if kappa is not None:
        ens.set_sticky(np.full(d, kappa))
    if tracked:
        ens.set_gradient_tracking(True)
    _state(ens, pkg, d, ens.nchains, c_scale * pkg.problems.column_norms(G), seed)


def _logistic(pkg, ens, ksub=10, tracked=False, seed=4):
    P = pkg.problems.logistic_problem(m=20)
    d = P["p"]
    ens.set_flow(pkg.ZigZag(P["Gdrop"], P["mu"], P["sigma"]))
    ens.set_target(pkg.LogisticTarget(P["A"], P["y"], P["ny"], P["mu"], P["gamma0"], ksub))
    if tracked:
        ens.set_gradient_tracking(True)
    _state(ens, pkg, d, ens.nchains, P["c"], seed, sigma=P["sigma"], x0=np.tile(P["x0"], (ens.nchains, 1)))


def _logistic_d():
    return "logistic"  # (the number of coefficients of problems.logistic_problem: _make asks the problem)


# family -> (library, Ensemble keywords, environment, set-up, (T1, T2), kernel names, kind with the profile on or None, numbers not all zero)
def _cases():
    S = {}
    S["bps"] = ("default", dict(d=16, bps=True), {}, None, (2.0, 4.0), ("bps_run_kernel",), None, None)
    S["general"] = ("default", dict(d=144, adapt=True), {},
                    lambda pkg, e: (_general_local_bound(pkg, e)), (3.0, 6.0), ("zz_general_run_kernel",), 2, True)
    S["logistic_lds"] = ("default", dict(d=_logistic_d(), adapt=True, factor=5.0), {}, lambda pkg, e: _logistic(pkg, e), (2.0, 4.0),
                         ("zz_logistic_lds_kernel",), 2, True)
    # (the tracked-bounds instantiation of the LDS kernel has no profiling form: the buffer comes back as it was cleared)
    S["logistic_lds_tracked"] = ("default", dict(d=_logistic_d(), adapt=True, factor=5.0), {}, lambda pkg, e: _logistic(pkg, e, tracked=True),
                                 (2.0, 4.0), ("zz_logistic_lds_kernel",), 2, False)
    S["logistic_hbm"] = ("default", dict(d=_logistic_d(), adapt=True, factor=5.0, kernel="seq"), {}, lambda pkg, e: _logistic(pkg, e), (2.0, 4.0),
                         ("zz_general_run_kernel",), 2, True)
    S["tracked_lines"] = ("default", dict(d=2304), {"PDMP_HELPER_WAVE": "0", "PDMP_TRACK_LINES": "1"},
                          lambda pkg, e: _lattice(pkg, e, tracked=True), (0.3, 0.6), ("zz_local_trackl_kernel",), 1, True)
    S["tracked_pairs"] = ("default", dict(d=2304), {"PDMP_HELPER_WAVE": "0", "PDMP_TRACK_LINES": "0"},
                          lambda pkg, e: _lattice(pkg, e, tracked=True), (0.3, 0.6), ("zz_local_trackp_kernel",), 1, True)
    S["tracked_pairs_two_waves"] = ("default", dict(d=2304), {"PDMP_HELPER_WAVE": "1", "PDMP_TRACK_LINES": "0"},
                                    lambda pkg, e: _lattice(pkg, e, tracked=True), (0.3, 0.6), ("zz_local_trackp2_kernel",), 1, True)
    S["tracked_groups"] = ("default", dict(d=2304), {"PDMP_TRACK_GROUPS": "1"},
                           lambda pkg, e: _lattice(pkg, e, tracked=True), (0.3, 0.6), ("zz_local_track_kernel",), 1, True)
    S["exactp"] = ("parity", dict(d=2304, kernel="exactp"), {}, lambda pkg, e: _lattice(pkg, e), (0.3, 0.6), ("zz_local_exactp_kernel",), 1, True)
    S["sticky_spec"] = ("default", dict(d=2304, sticky=True, factor=1.5), {}, lambda pkg, e: _lattice(pkg, e, kappa=0.8, c_scale=1.5),
                        (0.3, 0.6), ("zz_sticky_spec_kernel",), None, None)
    S["sticky_run"] = ("default", dict(d=2304, sticky=True, factor=1.5, kernel="seq"), {}, lambda pkg, e: _lattice(pkg, e, kappa=0.8, c_scale=1.5),
                       (0.3, 0.6), ("zz_sticky_run_kernel",), None, None)
    S["spec"] = ("default", dict(d=2304), {}, lambda pkg, e: _lattice(pkg, e), (0.3, 0.6), ("zz_local_spec8_kernel",), 1, True)
    S["spec4"] = ("default", dict(d=2304, kernel="spec4"), {}, lambda pkg, e: _lattice(pkg, e), (0.3, 0.6), ("zz_local_spec_kernel",), 1, True)
    S["one_event"] = ("default", dict(d=2304, kernel="seq"), {}, lambda pkg, e: _lattice(pkg, e), (0.3, 0.6), ("zz_local_run_kernel",), None, None)
    return S


def _general_local_bound(pkg, ens):
    G = pkg.problems.gmrf_precision(12)
    d = G.shape[0]
    ens.set_flow(pkg.ZigZag(G, np.zeros(d)))
    ens.set_target(pkg.GaussianTarget(G))
    ens.set_local_bound(True)
    rng = np.random.default_rng(9)
    _state(ens, pkg, d, ens.nchains, pkg.problems.column_norms(G) * (1.0 + 0.01 * rng.random(d)), 18)


def _make(pkg, kw, nch=2):
    L = pkg._lib
    kw = dict(kw)
    d, kernel = kw.pop("d"), kw.pop("kernel", None)
    if d == "logistic":
        d = pkg.problems.logistic_problem(m=20)["p"]
    if kw.pop("bps", False):
        ens = pkg.Ensemble(nch, d, sampler=L.SAMPLER_BPS, factor=2.0, trace_capacity=4096)
        ens.set_flow_bps(pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0))
        rng = np.random.default_rng(3)
        ens.set_state_bps(0.0, rng.standard_normal((nch, d)), rng.standard_normal((nch, d)), 1e-3, 5 + np.arange(nch, dtype=np.uint64))
        return ens
    if kw.pop("sticky", False):
        kw["sampler"] = L.SAMPLER_STICKY_ZIGZAG
    ens = pkg.Ensemble(nch, d, **kw)
    if kernel is not None:
        ens.debug_set_kernel(kernel)
    return ens


def _refuses_profile(pkg, ens):
    with pytest.raises(pkg._lib.PdmpError) as ei:
        ens.debug_phase_cycles()
    assert ei.value.code == pkg._lib.PDMP_ERR_INVALID and str(ei.value).endswith(": " + NO_PROFILE), str(ei.value)


@pytest.mark.parametrize("family", sorted(_cases()))
def test_phase_profile_and_timing_per_kernel_family(gpu_pkg, gpu_pkg_parity, monkeypatch, family):
    lib, kw, env, setup, (T1, T2), names, kind, nonzero = _cases()[family]
    pkg = gpu_pkg_parity if lib == "parity" else gpu_pkg
    L = pkg._lib
    for k in ("PDMP_KERNEL", "PDMP_HELPER_WAVE", "PDMP_TRACK_LINES", "PDMP_TRACK_GROUPS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with _make(pkg, kw) as ens:
        if setup is not None:
            setup(pkg, ens)
        assert ens.kernel_name() == ""
        # profile off: the run is timed, nothing is recorded
        ens.run(T1, L.RUN_STOP_BEFORE)
        assert ens.kernel_name() in names, ens.kernel_name()
        assert ens.last_run_ms() > 0.0
        _refuses_profile(pkg, ens)
        # profile on
        ens.debug_phase_profile(True)
        _refuses_profile(pkg, ens)  # (switching it on records nothing by itself)
        ens.run(T2, L.RUN_STOP_BEFORE)
        assert ens.kernel_name() in names, ens.kernel_name()
        assert ens.last_run_ms() > 0.0
        if kind is None:
            _refuses_profile(pkg, ens)
        else:
            got, ph = ens.debug_phase_cycles()
            print("%s [%s]: kind %d, numbers %s" % (family, ens.kernel_name(), got, ph.tolist()))
            assert got == kind, (family, got)
            assert ph.shape == (16,) and bool(np.any(ph != 0.0)) == nonzero, (family, ph)
        if family != "bps":
            cnt = ens.counters()
            assert np.all(cnt["status"] == L.CHAIN_OK), cnt["status"]
        # off again: the last profile is dropped, and the next run records none
        ens.debug_phase_profile(False)
        _refuses_profile(pkg, ens)
        ens.run(T2 + (T2 - T1), L.RUN_STOP_BEFORE)
        assert ens.last_run_ms() > 0.0
        _refuses_profile(pkg, ens)


def _refused(pkg, ens, T, text):
    """The run raises PDMP_ERR_UNSUPPORTED with exactly `text`, names no kernel and leaves the ensemble untimed."""
    L = pkg._lib
    with pytest.raises(L.PdmpError) as ei:
        ens.run(T, L.RUN_STOP_BEFORE)
    assert ei.value.code == L.PDMP_ERR_UNSUPPORTED, str(ei.value)
    assert str(ei.value).endswith(": " + text), str(ei.value)
    assert ens.kernel_name() == ""
    with pytest.raises(L.PdmpError) as ei:
        ens.last_run_ms()
    assert ei.value.code == L.PDMP_ERR_INVALID and "no run has been launched" in str(ei.value)


@pytest.mark.parametrize("form", ["lines", "pairs", "groups"])
def test_refusal_proposal_dump_under_tracking(gpu_pkg, monkeypatch, form):
    pkg = gpu_pkg
    monkeypatch.setenv("PDMP_HELPER_WAVE", "0")
    monkeypatch.setenv("PDMP_TRACK_LINES", "1" if form == "lines" else "0")
    monkeypatch.setenv("PDMP_TRACK_GROUPS", "1" if form == "groups" else "0")
    with pkg.Ensemble(2, 2304) as ens:
        _lattice(pkg, ens, tracked=True)
        pkg._lib.check(ens._L.pdmp_debug_set_proposal_dump(ens._h, C.c_int64(4)))  # (after set_state, which refuses the pair itself)
        _refused(pkg, ens, 0.3, "the proposal dump belongs to the one-event kernel")
        pkg._lib.check(ens._L.pdmp_debug_set_proposal_dump(ens._h, C.c_int64(0)))
        ens.run(0.3, pkg._lib.RUN_STOP_BEFORE)
        assert ens.kernel_name() == {"lines": "zz_local_trackl_kernel", "pairs": "zz_local_trackp_kernel", "groups": "zz_local_track_kernel"}[form]
        assert ens.last_run_ms() > 0.0


def test_refusal_exactp_by_name_in_the_default_library(gpu_pkg, monkeypatch):
    pkg = gpu_pkg
    monkeypatch.delenv("PDMP_KERNEL", raising=False)
    with pkg.Ensemble(2, 2304) as ens:
        ens.debug_set_kernel("exactp")
        _lattice(pkg, ens)
        _refused(pkg, ens, 0.3, "PDMP_DEBUG_KERNEL_EXACTP: zz_local_exactp_kernel is not part of this library: it lives in the parity build "
                                "(build.py --variant parity, -DPDMP_EXTRA_KERNELS)")


def test_refusal_exactp_by_name_off_the_lattice_in_the_parity_library(gpu_pkg_parity, monkeypatch):
    pkg = gpu_pkg_parity
    monkeypatch.delenv("PDMP_KERNEL", raising=False)
    G = pkg.problems.random_sparse_precision(2500, 6, seed=3)
    d = G.shape[0]
    with pkg.Ensemble(2, d) as ens:
        ens.debug_set_kernel("exactp")
        ens.set_flow(pkg.ZigZag(G, np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(G))
        _state(ens, pkg, d, 2, pkg.problems.column_norms(G), 2)
        _refused(pkg, ens, 0.3, "PDMP_DEBUG_KERNEL_EXACTP: spdmp on a plain lattice (16 <= n <= 128, d >= 2048) with the bounding matrix equal to the "
                                "target's, no adaptation, and a trace or no trace")


def test_refusal_logistic_tracking_off_the_lds_kernel(gpu_pkg, monkeypatch):
    pkg = gpu_pkg
    monkeypatch.delenv("PDMP_KERNEL", raising=False)
    with _make(pkg, dict(d=_logistic_d(), adapt=True, factor=5.0)) as ens:
        _logistic(pkg, ens, ksub=33, tracked=True)  # (k_sub <= 32 on the LDS-resident kernel)
        _refused(pkg, ens, 2.0, "gradient tracking with the logistic target runs on the LDS-resident kernel: d <= 512, k_sub <= 32, rows of <= 6 regressors")


@pytest.mark.parametrize("why", ["k_sub", "profile"])
def test_refusal_logistic_rows_that_do_not_fit(gpu_pkg_parity, monkeypatch, why):
    """Rows of 16 lanes hold k_sub + 2 <= 16 draws; and the rows kernel has no instantiation that takes a profile buffer, so with the phase
    profile on a width asked for by name is refused as well."""
    pkg = gpu_pkg_parity
    monkeypatch.delenv("PDMP_KERNEL", raising=False)
    monkeypatch.delenv("PDMP_LG_ROWS", raising=False)
    with _make(pkg, dict(d=_logistic_d(), adapt=True, factor=5.0), nch=4) as ens:
        ens.debug_set_logistic_rows(16)
        _logistic(pkg, ens, ksub=15 if why == "k_sub" else 10)
        if why == "profile":
            ens.debug_phase_profile(True)
        _refused(pkg, ens, 2.0, "pdmp_debug_set_logistic_rows: this ensemble does not fit rows of 16 lanes")
        if why == "profile":
            ens.debug_phase_profile(False)
            ens.run(2.0, pkg._lib.RUN_STOP_BEFORE)
            assert ens.kernel_name() == "zz_logistic_rows_kernel"
            assert ens.last_run_ms() > 0.0
            _refuses_profile(pkg, ens)
