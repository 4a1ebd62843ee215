"""Randomised stress of the general kernel (-m gpu): FactBoomerang (mandatory refresh, rotation, ρ, means, speeds) on random graphs, and the ZigZag
on graphs whose neighbourhoods exceed one wavefront, with random slice boundaries and tiny trace buffers -- bit for bit the oracle.  Fixed seeds.  The draws and the oracle's chains live in
tests/stress_cases.py (tests/test_stress_cases_ref.py: every reference chain is healthy, so no draw is skipped here); FactBoomerang draws 14..
are appended ones whose horizon gives every chain 100 events.  tests/test_gpu_general_modes.py holds the kernel's other modes to the oracle."""
import numpy as np
import pytest

import stress_cases as S

pytestmark = pytest.mark.gpu


def _run_sliced(pkg, ens, nch, T, cuts, ok_violation=False):
    events = [[] for _ in range(nch)]
    for Tk, flag in [(float(v), pkg._lib.RUN_STOP_BEFORE) for v in cuts] + [(T, pkg._lib.RUN_REFERENCE_TAIL)]:
        while True:
            ens.run(Tk, flag)
            cnt = ens.counters()
            assert not np.any(cnt["status"] == pkg._lib.CHAIN_BOUND_VIOLATED)
            for k in range(nch):
                if cnt["ntrace"][k]:
                    events[k].append(ens.trace(k, counters=cnt))
            ens.trace_reset()
            if not pkg._lib.needs_rerun(cnt["status"]):
                break
    return [np.concatenate(e) if e else np.empty(0, dtype=pkg._lib.EVENT_DTYPE) for e in events], ens.final_state(), ens.counters()


def _compare(what, evs, fs, cnt, refs, adapt):
    for k, r in enumerate(refs):
        ev = evs[k]
        assert len(ev) == len(r["events"]), (what, k, len(ev), len(r["events"]))
        for f in ("i", "t", "x", "theta"):
            assert np.array_equal(ev[f], r["events"][f]), (what, k, f)
        assert int(cnt["num"][k]) == r["num"] and np.array_equal(fs["acc"][k], r["acc"]), what
        assert np.array_equal(fs["x"][k], r["x"]) and np.array_equal(fs["theta"][k], r["theta"]) and np.array_equal(fs["t"][k], r["t"]), what
        if adapt:
            assert np.array_equal(fs["c"][k], r["c"]), what


@pytest.mark.parametrize("case", range(S.FACTBOOMERANG_N))
def test_random_factboomerang(gpu_pkg, case):
    """src/fact_samplers.jl:37-39,58-65 (λ, ab), src/sfact.jl:29-36 (rotation), :103 (refresh draw) on random graphs, means, speeds, ρ and λref."""
    pkg = gpu_pkg
    P, refs = S.factboomerang_draw(case), S.factboomerang_refs(case)
    G, d, nch, mu, sig, lam, rho, x0, th0 = (P[k] for k in ("G", "d", "nch", "mu", "sig", "lam", "rho", "x0", "th0"))
    adapt, c, T, cap, seed, cuts = (P[k] for k in ("adapt", "c", "T", "cap", "seed", "cuts"))
    F = pkg.FactBoomerang(G, mu, lam, σ=sig, ρ=rho)
    assert all(r["status"] == 0 for r in refs)
    with pkg.Ensemble(nch, d, adapt=adapt, factor=1.7, trace_capacity=cap) as ens:
        ens.set_flow(F)
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_state(0.0, x0, th0, c, np.arange(nch, dtype=np.uint64) + seed)
        evs, fs, cnt = _run_sliced(pkg, ens, nch, T, cuts)
        kname = ens.kernel_name()
    what = dict(case=case, d=d, mu=bool(np.any(mu)), rho=rho, lam=lam, adapt=adapt, cap=cap, cuts=len(cuts), kernel=kname)
    assert kname == "zz_general_run_kernel", what
    assert sum(len(r["events"]) for r in refs) > 20, what
    _compare(what, evs, fs, cnt, refs, adapt)


@pytest.mark.parametrize("case", range(8))
def test_random_wide_neighbourhoods_zigzag(gpu_pkg, case):
    """The ZigZag where |S[i]| exceeds a wavefront (the general kernel's chunked re-bound), with its options drawn at random."""
    pkg = gpu_pkg
    P, refs = S.wide_zigzag_draw(case), S.wide_zigzag_refs(case)
    G, Gb, d, nch, mu_b, sig, lam, x0, th0 = (P[k] for k in ("G", "Gb", "d", "nch", "mu_b", "sig", "lam", "x0", "th0"))
    adapt, c, T, cap, seed, cuts = (P[k] for k in ("adapt", "c", "T", "cap", "seed", "cuts"))
    assert all(r["status"] == 0 for r in refs)
    with pkg.Ensemble(nch, d, adapt=adapt, factor=1.6, trace_capacity=cap) as ens:
        ens.set_flow(pkg.ZigZag(Gb, np.zeros(d) if mu_b is None else mu_b, sig, λref=lam))
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_state(0.0, x0, th0, c, np.arange(nch, dtype=np.uint64) + seed)
        evs, fs, cnt = _run_sliced(pkg, ens, nch, T, cuts)
        kname = ens.kernel_name()
    what = dict(case=case, d=d, own_bound=Gb is not G, mu_b=mu_b is not None, lam=lam, adapt=adapt, cap=cap, kernel=kname)
    assert kname == S.zigzag_kernel(G) == "zz_general_run_kernel", what
    _compare(what, evs, fs, cnt, refs, adapt)
