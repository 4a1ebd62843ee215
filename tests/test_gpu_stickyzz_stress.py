"""Randomised and named-edge stress of the barrier ZigZag kernel (-m gpu; stickyzz, src/stickyzz.jl; zz_barrier_run_kernel, csrc/pdmp_barrier.hip):
random lattices and banded / random sparse precisions, a bounding Γ of its own, flow and target means apart and together, start times, adapt,
strong_upperbounds, every barrier shape and rule, starts on a barrier, tiny trace buffers and RUN_STOP_BEFORE cuts; then the edges of the
kernel's geometry -- a column of 63 members (candidate 63 of an iteration's 64 draws), d around multiples of the 64 keys of a block, exact
key ties between blocks, starts on a two-sided level, 130 chains -- bit for bit the restatement (tests/ref/stickyzz_ref.c).  Seeds are
fixed.  The draws and the restatement's chains live in tests/stickyzz_stress_cases.py; tests/test_stickyzz_stress_cases_ref.py asserts on the
CPU that every reference chain is healthy and what the draws reach, so no draw is skipped here."""
import numpy as np
import pytest

import stickyzz_cases as K
import stickyzz_ref_lib as R
import stickyzz_stress_cases as Z

pytestmark = pytest.mark.gpu


def run_device(pkg, P):
    """The draw on the device, driven through the ABI: the setup calls as samplers.stickyzz makes them, RUN_STOP_BEFORE to every cut, then
    RUN_REFERENCE_TAIL to T; the trace drained and reset while a chain needs a rerun."""
    L = pkg._lib
    nch, d = P["nch"], P["d"]
    events = [[] for _ in range(nch)]
    with pkg.Ensemble(nch, d, sampler=L.SAMPLER_BARRIER_ZIGZAG, adapt=P["adapt"], factor=Z.FACTOR, trace_capacity=P["cap"]) as ens:
        ens.set_flow(pkg.ZigZag(P["Gb"], np.zeros(d) if P["mu_b"] is None else P["mu_b"]))
        ens.set_target(pkg.GaussianTarget(P["G"], P["mu_t"]))
        ens.set_barriers(*R.barrier_table(P["bars"], d), P["strong"])
        ens.set_state(P["t0"], P["x0"], P["th0"], P["c"], np.arange(nch, dtype=np.uint64) + np.uint64(P["seed"]))
        for T, flags in [(float(t), L.RUN_STOP_BEFORE) for t in P["cuts"]] + [(P["T"], L.RUN_REFERENCE_TAIL)]:
            while True:
                ens.run(T, flags)
                cnt = ens.counters()
                assert not np.any(cnt["status"] == L.CHAIN_BOUND_VIOLATED), Z.what(P)
                for k in range(nch):
                    if cnt["ntrace"][k]:
                        events[k].append(ens.trace(k, counters=cnt))
                ens.trace_reset()
                if not L.needs_rerun(cnt["status"]):
                    break
        fs, fb, kname = ens.final_state(), ens.final_barrier(), ens.kernel_name()
    assert kname == "zz_barrier_run_kernel", (Z.what(P), kname)
    ev = [np.concatenate(e) if e else np.empty(0, dtype=L.EVENT_DTYPE) for e in events]
    return ev, cnt, fs, fb


def compare(pkg, P, refs):
    what = Z.what(P)
    assert all(r["status"] == R.REF_OK for r in refs), what
    ev, cnt, fs, fb = run_device(pkg, P)
    for k, r in enumerate(refs):
        assert cnt["status"][k] == pkg._lib.CHAIN_OK, (what, k)
        assert len(ev[k]) == r["nevents"] == len(r["t"]), (what, k, len(ev[k]), r["nevents"])
        for f in ("i", "t", "x", "theta"):
            assert np.array_equal(ev[k][f], r[f]), (what, k, f, int(np.argmax(ev[k][f] != r[f])))
        got = (int(cnt["nacc"][k]), int(cnt["num"][k]), int(cnt["nevents"][k]), int(cnt["ndraw_main"][k]))
        assert got == (r["nacc"], r["num"], r["nevents"], r["ndraw_main"]), (what, k, got)
        assert cnt["t_last"][k] == r["t_final"], (what, k)
        assert np.array_equal(fs["t"][k], r["t_state"]) and np.array_equal(fs["x"][k], r["x_final"]), (what, k)
        assert np.array_equal(fs["theta"][k], r["theta_final"]), (what, k)
        assert np.array_equal(fs["c"][k], r["c_final"]), (what, k)
        assert np.array_equal(fb["frozen"][k], r["frozen"]) and np.array_equal(fb["theta_saved"][k], r["theta_saved"]), (what, k)


@pytest.mark.parametrize("case", range(Z.OPTIONS_N))
def test_random_barrier_options(gpu_pkg, monkeypatch, case):
    """Family A.  One case in four also with PDMP_LAUNCH_COUNT_LIMIT set low: the launches pause and resume between the cuts as well."""
    P, refs = Z.options_draw(case), Z.options_refs(case)
    compare(gpu_pkg, P, refs)
    if case % 4 == 0:
        monkeypatch.setenv("PDMP_LAUNCH_COUNT_LIMIT", "300")
        compare(gpu_pkg, P, refs)


@pytest.mark.parametrize("name", Z.EDGE_NAMES)
def test_named_edges(gpu_pkg, name):
    """Family B (what each reference run shows is asserted in tests/test_stickyzz_stress_cases_ref.py)."""
    compare(gpu_pkg, Z.edge_draw(name), Z.edge_refs(name))


def test_a_column_of_64_members_is_refused(gpu_pkg):
    """The hub with 63 leaves: |G1[0]| = 64 inside a two-hop zone of 64 -- no general-kernel graph, so needs_general does not stop it first: the
    barrier sampler's own check does (the head draw and 64 re-bounds would need 65 candidates)."""
    pkg = gpu_pkg
    L = pkg._lib
    G = Z.refused_hub()
    d = G.shape[0]
    assert d == 64 and Z.sticky_kernel(G) != "zz_general_run_kernel"
    with pkg.Ensemble(1, d, sampler=L.SAMPLER_BARRIER_ZIGZAG, factor=Z.FACTOR, trace_capacity=64) as ens:
        ens.set_flow(pkg.ZigZag(G, np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(G, None))
        ens.set_barriers(*R.barrier_table(K.NO_BARRIER, d))
        with pytest.raises(L.PdmpError) as ei:
            ens.set_state(0.0, np.zeros((1, d)), np.ones((1, d)), np.ones(d), np.array([3], dtype=np.uint64))
    assert ei.value.code == L.PDMP_ERR_UNSUPPORTED and "|G1[0]| = 64 > 63" in str(ei.value), str(ei.value)
