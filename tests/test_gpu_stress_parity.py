"""Randomised stress of the speculative kernels (-m gpu): random lattices / random sparse precisions, random slice boundaries,
tiny trace buffers (TRACE_FULL in the middle of a multi-event commit), adapt on/off -- every chain must equal the oracle bit
for bit.  Seeds are fixed: the cases are reproducible.  The draws and the oracle's chains live in tests/stress_cases.py;
tests/test_stress_cases_ref.py shows on the CPU that every reference chain is healthy, so no draw is skipped here."""
import numpy as np
import pytest

import stress_cases as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", range(12))
def test_random_slices_and_tiny_traces_zigzag(gpu_pkg, case):
    pkg = gpu_pkg
    P, refs = S.parity_slices_draw(case), S.parity_slices_refs(case)
    G, d, nch, x0, th0, adapt, c, T, cap, seed, cuts = (P[k] for k in ("G", "d", "nch", "x0", "th0", "adapt", "c", "T", "cap", "seed", "cuts"))
    assert all(r["status"] == 0 for r in refs)
    events = [[] for _ in range(nch)]
    with pkg.Ensemble(nch, d, adapt=adapt, trace_capacity=cap) as ens:
        ens.set_flow(pkg.ZigZag(G, np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_state(0.0, x0, th0, c, np.arange(nch, dtype=np.uint64) + seed)
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
        fs = ens.final_state()
        cnt = ens.counters()
        kname = ens.kernel_name()
    assert kname.startswith(S.zigzag_kernel(G)), (case, kname)
    for k, r in enumerate(refs):
        ev = np.concatenate(events[k]) if events[k] else np.empty(0, dtype=pkg._lib.EVENT_DTYPE)
        assert len(ev) == len(r["events"]), (case, k, len(ev), len(r["events"]))
        for f in ("i", "t", "x", "theta"):
            assert np.array_equal(ev[f], r["events"][f]), (case, k, f)
        assert int(cnt["num"][k]) == r["num"] and np.array_equal(fs["acc"][k], r["acc"])
        assert np.array_equal(fs["x"][k], r["x"]) and np.array_equal(fs["theta"][k], r["theta"]) and np.array_equal(fs["t"][k], r["t"])
        if adapt:
            assert np.array_equal(fs["c"][k], r["c"])


@pytest.mark.parametrize("kern", ["auto", "seq"])
@pytest.mark.parametrize("case", range(14))
def test_random_means_bounds_and_refresh_zigzag(gpu_pkg, monkeypatch, case, kern):
    """Round 6: the options the first stress test leaves at their defaults -- a flow mean and / or a target mean (equal or not), a bounding Γ of its own
    (0.9 Γ, test/maintest.jl:23), a refresh clock with speeds σ_i, a start time -- on the speculative kernels and on the one-event kernel."""
    pkg = gpu_pkg
    if kern == "seq":
        monkeypatch.setenv("PDMP_KERNEL", "seq")
    else:
        monkeypatch.delenv("PDMP_KERNEL", raising=False)
    P, refs = S.parity_options_draw(case), S.parity_options_refs(case)
    G, Gb, d, nch, mu_b, mu_t, sig, lam, t0 = (P[k] for k in ("G", "Gb", "d", "nch", "mu_b", "mu_t", "sig", "lam", "t0"))
    x0, th0, adapt, c, T, cap, seed = (P[k] for k in ("x0", "th0", "adapt", "c", "T", "cap", "seed"))
    assert all(r["status"] == 0 for r in refs)
    events = [[] for _ in range(nch)]
    with pkg.Ensemble(nch, d, adapt=adapt, factor=1.8, trace_capacity=cap) as ens:
        ens.set_flow(pkg.ZigZag(Gb, np.zeros(d) if mu_b is None else mu_b, sig, λref=lam))
        ens.set_target(pkg.GaussianTarget(G) if mu_t is None else pkg.GaussianTarget(G, mu_t))
        ens.set_state(t0, x0, th0, c, np.arange(nch, dtype=np.uint64) + seed)
        while True:
            ens.run(T, pkg._lib.RUN_REFERENCE_TAIL)
            cnt = ens.counters()
            assert not np.any(cnt["status"] == pkg._lib.CHAIN_BOUND_VIOLATED)
            for k in range(nch):
                if cnt["ntrace"][k]:
                    events[k].append(ens.trace(k, counters=cnt))
            ens.trace_reset()
            if not pkg._lib.needs_rerun(cnt["status"]):
                break
        fs = ens.final_state()
        cnt = ens.counters()
        kname = ens.kernel_name()
    what = dict(case=case, kern=kern, d=d, own_bound=Gb is not G, mu_b=mu_b is not None, mu_t=mu_t is not None, lam=lam, t0=t0, adapt=adapt, kernel=kname)
    assert kname.startswith(S.zigzag_kernel(G, kern)), what
    for k, r in enumerate(refs):
        ev = np.concatenate(events[k]) if events[k] else np.empty(0, dtype=pkg._lib.EVENT_DTYPE)
        assert len(ev) == len(r["events"]), (what, k, len(ev), len(r["events"]))
        for f in ("i", "t", "x", "theta"):
            assert np.array_equal(ev[f], r["events"][f]), (what, k, f)
        assert int(cnt["num"][k]) == r["num"] and np.array_equal(fs["acc"][k], r["acc"]), what
        assert np.array_equal(fs["x"][k], r["x"]) and np.array_equal(fs["theta"][k], r["theta"]) and np.array_equal(fs["t"][k], r["t"]), what
        if adapt:
            assert np.array_equal(fs["c"][k], r["c"]), what


@pytest.mark.parametrize("case", range(8))
def test_random_slices_and_tiny_traces_sticky(gpu_pkg, case):
    pkg = gpu_pkg
    P, refs = S.parity_sticky_draw(case), S.parity_sticky_refs(case)
    G, d, nch, x0, th0, c, kappa, reversible, strong = (P[k] for k in ("G", "d", "nch", "x0", "th0", "c", "kappa", "reversible", "strong"))
    T, cap, seed, cuts = (P[k] for k in ("T", "cap", "seed", "cuts"))
    assert all(r["status"] == 0 for r in refs)
    events = [[] for _ in range(nch)]
    with pkg.Ensemble(nch, d, sampler=pkg._lib.SAMPLER_STICKY_ZIGZAG, adapt=True, factor=1.5, trace_capacity=cap) as ens:
        ens.set_flow(pkg.ZigZag(G, np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_sticky(kappa, reversible, strong)
        ens.set_state(0.0, x0, th0, c, np.arange(nch, dtype=np.uint64) + seed)
        for Tk, flag in [(float(v), pkg._lib.RUN_STOP_BEFORE) for v in cuts] + [(T, pkg._lib.RUN_REFERENCE_TAIL)]:
            while True:
                ens.run(Tk, flag)
                cnt = ens.counters()
                for k in range(nch):
                    if cnt["ntrace"][k]:
                        events[k].append(ens.trace(k, counters=cnt))
                ens.trace_reset()
                if not pkg._lib.needs_rerun(cnt["status"]):
                    break
        fs = ens.final_state()
        cnt = ens.counters()
        kname = ens.kernel_name()
    assert kname == S.sticky_kernel(G), (case, kname)
    for k, r in enumerate(refs):
        ev = np.concatenate(events[k]) if events[k] else np.empty(0, dtype=pkg._lib.EVENT_DTYPE)
        assert len(ev) == len(r["events"]), (case, k, len(ev), len(r["events"]))
        for f in ("i", "t", "x", "theta"):
            assert np.array_equal(ev[f], r["events"][f]), (case, k, f)
        assert (int(cnt["nacc"][k]), int(cnt["num"][k])) == (r["nacc"], r["num"])
        assert np.array_equal(fs["x"][k], r["x"]) and np.array_equal(fs["theta"][k], r["theta"]) and np.array_equal(fs["t"][k], r["t"])
