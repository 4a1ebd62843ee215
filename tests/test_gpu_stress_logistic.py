"""Randomised stress of the logistic kernel family of config C4 (-m gpu): 12 seeded draws of tests/logistic_cases.stress_problem -- p in 8..512,
the row-length set, intercept or not, k_sub in 1..32, tracked or not, the engine's path integrals or not, t0, a small trace buffer and random
slice boundaries -- bit for bit the oracle.  tests/test_logistic_cases_ref.py replays them on the oracle alone and records the slot counts and
k_sub they reach."""
import numpy as np
import pytest

import logistic_cases as LC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", range(LC.STRESS_N))
def test_random_logistic_shape(gpu_pkg, case):
    P = LC.stress_problem(case)
    refs = LC.stress_refs(case)
    what = {k: P[k] for k in ("name", "p", "n", "lens", "intercept", "ksub", "tracked", "integrals", "t0", "cap", "cuts")}
    assert all(r["status"] == 0 and len(r["events"]) >= 100 for r in refs), what
    run = LC.device_run(gpu_pkg, P, tracked=P["tracked"], integrals=P["integrals"])
    assert run["kernel"] == (LC.LDS_KERNEL if LC.lds_takes(P) else LC.GENERAL_KERNEL), (what, run["kernel"])
    LC.compare_with_oracle(what, P, run, refs)
    if run["pj"] is not None:
        assert np.all(np.isfinite(run["pj"]))
