"""Randomised stress of the bouncy particle kernels (-m gpu; pdmp_inner!, src/not_fact_samplers.jl:52-147): random dimensions across the register /
AGPR / scratch instantiations, Γ = I, diagonal or sparse with the reference's mass factor cholesky(Γ).L or the identity, a mean, refresh rates, ρ,
adapt, LocalBound, subsample -- bit for bit the oracle (events t, x, θ; counters; final state; c).  Round 6, seeds fixed.  The draws live in
tests/stress_cases.py; tests/test_stress_cases_ref.py shows on the CPU that every reference chain is healthy, so a draw is never skipped: whatever
check() raises is a failure.  Draws 16.. are appended ones (subsample with adapt on and off, LocalBound with a mean, d = 1 and 1025, 100 events per
chain); the first 16 stay as they were, thin ones included."""
import numpy as np
import pytest

import stress_cases as S
from test_gpu_bps_parity import check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", range(S.BPS_N))
def test_random_bps_options(gpu_pkg, case):
    P = S.bps_draw(case)
    assert all(r["status"] == 0 for r in S.bps_refs(case))
    check(gpu_pkg, P["G"], P["mu"], P["x0"], P["th0"], P["c"], P["T"], P["lam"], rho=P["rho"], adapt=P["adapt"], seed=P["seed"], L=P["L"],
          local_bound=P["local_bound"], subsample=P["subsample"])
