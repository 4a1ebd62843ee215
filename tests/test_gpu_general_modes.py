"""Every mode of zz_general_run_kernel (csrc/pdmp_general.hip) against the oracle, ACROSS LAUNCHES (-m gpu): adaptscale, LocalBound, an explicit
neighbourhood G ⊋ G1 with columns beyond one wavefront, G = All(), sspdmp on wide graphs, FactBoomerang -- the cases and seeded stress draws of
tests/general_cases.py (tests/test_general_cases_ref.py shows on the CPU that none of them is vacuous).

Each mode keeps per-chain state in global memory between launches (the tuned σ, the `renew` flags, θ_f, the adapted c, the refresh clock's key
slot), so every case runs twice: (a) one launch sequence to T with a trace buffer that never fills; (b) cut at three fixed interior times with
RUN_STOP_BEFORE, a trace buffer of at most a quarter of the shortest chain, re-launched while a chain needs it.  Both are compared bit for bit
with the oracle's chains.  A case that passes (a) and fails (b) points at what a launch hands to the next one."""
import numpy as np
import pytest

import general_cases as GC

pytestmark = pytest.mark.gpu

ONE_LAUNCH_CAP = 8192  # more than any case's events per chain (asserted below)


def _check(pkg, P, rs, guard):
    guard(P, rs)
    L = pkg._lib
    if P["expect"] == "refuse":
        # what the device does not serve it refuses when the state is set, with a status -- never a different chain
        ens = GC.open_ensemble(pkg, P, 64)
        try:
            with pytest.raises(L.PdmpError) as ei:
                ens.set_state(P["t0"], P["X0"], P["TH0"], P["c"], P["seeds"])
            assert ei.value.code == L.PDMP_ERR_UNSUPPORTED, ei.value
        finally:
            ens.close()
        return
    assert max(len(r["events"]) for r in rs) < ONE_LAUNCH_CAP
    one = GC.device_run(pkg, P, ONE_LAUNCH_CAP, ())
    assert one["kernels"] == {P["kernel"]}, one["kernels"]
    assert one["launches"] == 1 and not one["full"].any()
    GC.compare_with_oracle("one launch", P, one, rs)
    cap = GC.slice_cap(rs)
    assert 4 * cap <= min(len(r["events"]) for r in rs)
    cut = GC.device_run(pkg, P, cap, P["cuts"])
    assert cut["kernels"] == {P["kernel"]}, cut["kernels"]
    assert np.all(cut["full"] >= 3), cut["full"]  # the run really was cut: every chain came back with a full trace three times at least
    assert cut["launches"] >= 4 + 3
    GC.compare_with_oracle("in slices, trace of %d" % cap, P, cut, rs)


@pytest.mark.parametrize("name", GC.NAMES)
def test_general_kernel_mode_across_launches(gpu_pkg, name):
    _check(gpu_pkg, GC.problem(name), GC.refs(name), GC.guard_case)


@pytest.mark.parametrize("case", range(GC.STRESS_N))
def test_general_kernel_stress_draw_across_launches(gpu_pkg, case):
    P, rs = GC.stress_problem(case)
    _check(gpu_pkg, P, rs, GC.guard_common)
