"""Randomised stress of the sticky ZigZag kernels (-m gpu; sspdmp, src/ss_fact.jl:78-215): random lattices and banded / random sparse precisions, a
bounding Γ of its own or the target's, flow and target means, per-coordinate thaw rates, adapt, `reversible`, `strong_upperbounds`, speeds that are
not one -- on the speculative kernel and (PDMP_KERNEL=seq) the one-event kernel, bit for bit the oracle.  Round 6 (after the flow-mean finding on
the tracked ZigZag kernel: option combinations no hand-written test had).  Seeds are fixed.  The draws and the oracle's chains live in
tests/stress_cases.py (tests/test_stress_cases_ref.py: every reference chain is healthy, so no draw is skipped here)."""
import numpy as np
import pytest

import stress_cases as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kern", ["auto", "seq"])
@pytest.mark.parametrize("case", range(12))
def test_random_sticky_options(gpu_pkg, monkeypatch, case, kern):
    pkg = gpu_pkg
    if kern == "seq":
        monkeypatch.setenv("PDMP_KERNEL", "seq")
    else:
        monkeypatch.delenv("PDMP_KERNEL", raising=False)
    P, refs = S.sticky_options_draw(case), S.sticky_options_refs(case)
    kind, G, Gb, d, nch, mu_b, mu_t, x0, th0 = (P[k] for k in ("kind", "G", "Gb", "d", "nch", "mu_b", "mu_t", "x0", "th0"))
    adapt, c, kappa, rev, strong, T, seed = (P[k] for k in ("adapt", "c", "kappa", "rev", "strong", "T", "seed"))
    assert all(r["status"] == 0 for r in refs)
    L = pkg._lib
    events = [[] for _ in range(nch)]
    with pkg.Ensemble(nch, d, sampler=L.SAMPLER_STICKY_ZIGZAG, adapt=adapt, factor=1.5, trace_capacity=2048) as ens:  # (sspdmp's default factor)
        ens.set_flow(pkg.ZigZag(Gb, np.zeros(d) if mu_b is None else mu_b))
        ens.set_target(pkg.GaussianTarget(G) if mu_t is None else pkg.GaussianTarget(G, mu_t))
        ens.set_sticky(kappa, rev, strong)
        ens.set_state(0.0, x0, th0, c, np.arange(nch, dtype=np.uint64) + seed)
        while True:
            ens.run(T, L.RUN_REFERENCE_TAIL)
            cnt = ens.counters()
            assert not np.any(cnt["status"] == L.CHAIN_BOUND_VIOLATED)
            for k in range(nch):
                if cnt["ntrace"][k]:
                    events[k].append(ens.trace(k, counters=cnt))
            ens.trace_reset()
            if not L.needs_rerun(cnt["status"]):
                break
        fs = ens.final_state()
        kname = ens.kernel_name()
    assert kname == S.sticky_kernel(G, kern), (case, kern, kname)
    acc, num, t, x, th, cout = cnt["nacc"], cnt["num"], fs["t"], fs["x"], fs["theta"], fs["c"]
    what = dict(case=case, kern=kern, kind=kind, d=d, own_bound=Gb is not G, mu_b=mu_b is not None, mu_t=mu_t is not None, adapt=adapt, rev=rev, strong=strong)
    for k in range(nch):
        r = refs[k]
        ev, oe = (np.concatenate(events[k]) if events[k] else np.empty(0, dtype=L.EVENT_DTYPE)), r["events"]
        assert len(ev) == len(oe), (what, k, len(ev), len(oe))
        for f in ("i", "t", "x", "theta"):
            assert np.array_equal(ev[f], oe[f]), (what, k, f)
        assert (int(acc[k]), int(num[k])) == (r["nacc"], r["num"]), what
        assert np.array_equal(t[k], r["t"]) and np.array_equal(x[k], r["x"]) and np.array_equal(th[k], r["theta"]), what
        assert np.array_equal(cout[k], r["c"]), what
