"""The logistic kernel family of config C4 across d, k_sub and row lengths (-m gpu): every case of tests/logistic_cases.py (its docstring is the
covering table, case x what it reaches) in every form that serves it, against the oracle bit for bit -- events, num, acc, the adapted c, final
(t, x, θ), both stream positions -- with the kernel's name asserted in each form, so that no case runs on another kernel than the one it names:

    lds, lds_noI      zz_logistic_lds_kernel<.., WITH_I>           the default, with and without the engine's ∫x dt
    hbm               zz_general_run_kernel (debug_set_kernel "seq") the records in HBM
    trk, trk_noI      zz_logistic_lds_kernel<.., TRK>              set_gradient_tracking, against the oracle's tracked evaluation
    rows32, rows16    zz_logistic_rows_kernel<W> (parity library)  wherever dk <= 448 and k_sub + 2 <= W

The forms that move (lds, hbm, rows) agree on ∫x dt of every coordinate bit for bit; the tracked form agrees with them to rtol 1e-9 (the
tolerance of test_c4_tracked_bounds_equal_the_tracked_oracle: the same path, other roundings of the bounds).  The cases one size beyond a limit of
the LDS kernel (rows of 8 regressors, dk = 576, k_sub = 33) run on zz_general_run_kernel and refuse tracking with a status."""
import numpy as np
import pytest
import scipy.sparse as sp

import logistic_cases as LC

pytestmark = pytest.mark.gpu


def check_case(pkg, parity, name):
    P = LC.problem(name)
    mov, trk = LC.refs(name), LC.refs(name, tracked=True)
    LC.guard_case(P, mov)
    LC.guard_case(P, trk)
    forms = [("lds", pkg, dict(), LC.LDS_KERNEL, mov), ("lds_noI", pkg, dict(integrals=False), LC.LDS_KERNEL, mov),
             ("hbm", pkg, dict(kernel="seq"), LC.GENERAL_KERNEL, mov),
             ("trk", pkg, dict(tracked=True), LC.LDS_KERNEL, trk), ("trk_noI", pkg, dict(tracked=True, integrals=False), LC.LDS_KERNEL, trk)]
    forms += [("rows%d" % W, parity, dict(rows=W), LC.ROWS_KERNEL, mov) for W in (32, 16) if LC.rows_fit(P, W)]
    runs = {}
    for form, pk, kw, kernel, rs in forms:
        run = runs[form] = LC.device_run(pk, P, **kw)
        assert run["kernel"] == kernel, (name, form, run["kernel"])
        LC.compare_with_oracle((name, form), P, run, rs)
        if P["cuts"]:
            assert run["launches"] >= len(P["cuts"]) + 1 + 3, (name, form, run["launches"])  # (the trace buffer filled three times at least)
    if not P["tail"]:
        for form in runs:
            if form in ("hbm", "rows32", "rows16"):
                assert np.array_equal(runs[form]["pj"], runs["lds"]["pj"]), (name, form)
        assert np.all(np.isfinite(runs["lds"]["pj"])) and np.count_nonzero(runs["lds"]["pj"]) > P["p"] * LC.NCH // 2
        assert np.allclose(runs["trk"]["pj"], runs["lds"]["pj"], rtol=1e-9, atol=1e-9), name
    return runs


@pytest.mark.parametrize("name", LC.LDS_NAMES)
def test_lds_family_matches_the_oracle_in_every_form(gpu_pkg, gpu_pkg_parity, name):
    check_case(gpu_pkg, gpu_pkg_parity, name)


@pytest.mark.parametrize("name", LC.GENERAL_NAMES)
def test_one_size_beyond_the_lds_kernel_runs_on_the_general_kernel(gpu_pkg, name):
    """Rows of 8 regressors (the packed tables are not built: the general kernel's unpacked gradient), d = 512 and 513 (dk = 576), k_sub = 33:
    zz_general_run_kernel, the same chains as the oracle; with tracking switched on, select_family's refusal."""
    pkg = gpu_pkg
    P = LC.problem(name)
    mov = LC.refs(name)
    LC.guard_case(P, mov)
    assert not LC.lds_takes(P)
    pjs = []
    for kw in (dict(), dict(integrals=False), dict(kernel="seq")):
        run = LC.device_run(pkg, P, **kw)
        assert run["kernel"] == LC.GENERAL_KERNEL, (name, kw, run["kernel"])
        LC.compare_with_oracle((name, tuple(kw)), P, run, mov)
        pjs.append(run["pj"])
    if not P["tail"]:
        assert np.array_equal(pjs[0], pjs[2]) and np.all(np.isfinite(pjs[0]))
    with LC.open_ensemble(pkg, P, tracked=True) as ens:
        with pytest.raises(pkg._lib.PdmpError) as ei:
            ens.set_state(P["t0"], P["X0"], P["TH0"], P["c"], P["seeds"])
            ens.run(P["T"], pkg._lib.RUN_STOP_BEFORE)
        assert ei.value.code == pkg._lib.PDMP_ERR_UNSUPPORTED and "LDS-resident" in str(ei.value)


def test_a_column_without_observation_is_refused(gpu_pkg):
    """rand over an empty range in the reference: PDMP_ERR_UNSUPPORTED from set_target."""
    pkg = gpu_pkg
    P = dict(LC.problem("a"))
    A = P["A"].tocoo()
    keep = A.col != 5
    P["A"] = sp.csc_matrix((A.data[keep], (A.row[keep], A.col[keep])), shape=A.shape)
    assert np.diff(P["A"].indptr)[5] == 0
    with pytest.raises(pkg._lib.PdmpError) as ei:
        LC.open_ensemble(pkg, P).close()
    assert ei.value.code == pkg._lib.PDMP_ERR_UNSUPPORTED and "has no observation" in str(ei.value)


def test_rows_of_16_lanes_refuse_k_sub_15(gpu_pkg_parity):
    """k_sub + 2 <= W: 14 observations fit a row of 16 lanes (and run there), 15 do not -- asked for by name, never another kernel in its place."""
    pk = gpu_pkg_parity
    P = dict(LC.problem("c"), T=2.0)
    with LC.open_ensemble(pk, P, rows=16, ksub=14) as ens:
        ens.set_state(P["t0"], P["X0"], P["TH0"], P["c"], P["seeds"])
        ens.run(P["T"], pk._lib.RUN_STOP_BEFORE)
        assert ens.kernel_name() == LC.ROWS_KERNEL and np.all(ens.counters()["nacc"] > 10)
    with LC.open_ensemble(pk, P, rows=16, ksub=15) as ens:
        with pytest.raises(pk._lib.PdmpError) as ei:
            ens.set_state(P["t0"], P["X0"], P["TH0"], P["c"], P["seeds"])
            ens.run(P["T"], pk._lib.RUN_STOP_BEFORE)
        assert ei.value.code == pk._lib.PDMP_ERR_UNSUPPORTED and "does not fit rows" in str(ei.value)
