"""Every slot-count form of the Bouncy-Particle-family event loops on gfx950 (-m gpu) against the references the suite already holds them to, bit
for bit: the case table, its covering table (form x d) and the reasons for each width are in tests/bps_width_cases.py; the references alone
run in tests/test_bps_width_cases_ref.py.  Widths 65 ... 1023: NS = 2, 4, 8 and 16 slots per lane with full, partly full and wholly empty
trailing slots, and the FULL form at 128, 256 and 512."""
import numpy as np
import pytest

import bps_width_cases as BW
import test_gpu_modern_bps_parity as MP
import test_gpu_sticky_bps_parity as SP

pytestmark = pytest.mark.gpu


def same(a, b):
    return SP.same(a, b)  # on the bit patterns: −0 and +0 differ


def check_plain(pkg, name, d):
    """As test_gpu_bps_parity.check, through pdmp(...): events, counters, final state and c of every chain; any t0, target and flow."""
    P, refs = BW.plain_refs(pkg, name, d)
    BW.guard_plain(P, refs)
    c = pkg.LocalBound(np.array([P["c"]])) if P["local_bound"] else P["c"]
    tr, (t, x, th), (acc, num), cout = pkg.pdmp(P["target"], P["t0"], P["x0"], P["th0"], P["T"], c, P["F"], adapt=P["adapt"], seed=P["seed"],
                                                factor=2.0, subsample=P["subsample"])
    for k, r in enumerate(refs):
        what = (name, d, k)
        assert len(tr[k].t) == r["nevents"], (what, len(tr[k].t), r["nevents"])
        assert same(tr[k].t, r["t_ev"]) and same(tr[k].x, r["x_ev"]) and same(tr[k].θ, r["theta_ev"]), what
        assert (int(acc[k]), int(num[k])) == (r["nacc"], r["num"]), what
        assert same(t[k], r["t"]) and same(x[k], r["x"]) and same(th[k], r["theta"]) and same(cout[k], r["c"]), what


@pytest.mark.parametrize("d", BW.W)
def test_plain_loop(gpu_pkg, d):
    """bps_run_kernel: the dispatcher's branches that the table gives this width (the branches of one width share a test: creating the
    ensembles dominates, not the runs)."""
    names = [n for n, dd in BW.PLAIN_CASES if dd == d]
    assert "ident" in names
    for name in names:
        check_plain(gpu_pkg, name, d)


@pytest.mark.parametrize("flow,d", BW.STICKY_CASES)
def test_sticky_loop(gpu_pkg, flow, d):
    """bps_sticky_run_kernel: events (t, x, θ, f), every counter, the final state, final f and θf, with κ per coordinate and t0 ≠ 0 at every
    other width (the driver draws tref without t0, as the reference does)."""
    P, refs = BW.sticky_refs(gpu_pkg, flow, d)
    BW.guard_sticky(P, refs)
    tr, nfz = SP.check(gpu_pkg, P, P["T"], P["c"], P["kappa"], seed=P["seed"], strong=P["strong"], adapt=P["adapt"], t0=P["t0"],
                       state=(P["x0"], P["th0"]), refs=refs)
    assert nfz >= 20


@pytest.mark.parametrize("form,d", BW.MODERN_CASES)
def test_speed_recorded_loop(gpu_pkg, form, d):
    """bps_modern_run_kernel: 40 records of 3 chains, counters, status and the final (t, x, θ, c)."""
    P, refs = BW.modern_refs(form, d)
    BW.guard_modern(P, refs)
    MP.compare(MP.one_run(gpu_pkg, P, BW.MODERN_RECORDS, BW.MODERN_C), refs)
