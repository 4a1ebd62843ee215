"""tests/general_cases.py on the CPU (no device; not marked gpu): every case of the general kernel's mode table and every stress draw passes its
guard on the oracle alone, and the table as a whole reaches what its docstring names.  tests/test_gpu_general_modes.py compares the device with
the same chains; this file is what shows that none of those comparisons is vacuous."""
import numpy as np
import pytest
import scipy.sparse as sp

import general_cases as GC
import oracle_lib as O


@pytest.mark.parametrize("name", GC.NAMES)
def test_every_case_passes_its_guard(name):
    GC.guard_case(GC.problem(name), GC.refs(name))


@pytest.mark.parametrize("case", range(GC.STRESS_N))
def test_every_stress_draw_passes_its_guard(case):
    P, rs = GC.stress_problem(case)
    GC.guard_common(P, rs)


def test_the_table_reaches_what_it_names():
    Ps = [GC.problem(n) for n in GC.NAMES]
    clock = [P for P in Ps if P["lam"] > 0 or P["boom"]]
    # the refresh clock's slot d inside a key block that holds coordinates, and alone in a block of its own; several key blocks
    assert any(GC.clock_shares_block(P["d"]) and P["d"] > 64 for P in clock) and any(not GC.clock_shares_block(P["d"]) for P in clock)
    assert {P["d"] for P in Ps if P["adaptscale"] and not P["nbr"]} == {64, 81, 144}
    # |G1| > 64 (chunks of the re-bound), and |G| > 64 with members that are moved but not re-bounded
    assert any(GC.col_sizes(P["Gb"]).max() > 64 for P in Ps if P["local"]) and any(GC.col_sizes(P["Gb"]).max() > 64 for P in Ps if P["sticky"] is not None)
    masked = [P for P in Ps if P["nbr"]]
    for P in masked:
        extra = GC.col_sizes(P["G"]) - GC.col_sizes(P["Gb"])
        assert (GC.col_sizes(P["G"]) > 64).sum() >= 100 and extra.max() >= 50, P["name"]
    wide = GC.problem("g_adapt")
    assert int((GC.col_sizes(wide["G"]) > 64).sum()) == 103 and int(GC.col_sizes(wide["G"]).max()) == 112 and int(GC.col_sizes(wide["Gb"]).max()) == 62
    assert any(GC.col_sizes(P["Gb"]).max() > 64 for P in masked)  # ... and one whose G1 itself has columns above 64
    # each of the five modes with adapt on and off; FactBoomerang; t0 > 0; both ends of a run
    for mode in ("adaptscale", "local", "masked", "all", "sticky"):
        assert {P["adapt"] for P in Ps if P["mode"] == mode} == {True, False}, mode
        assert any(P["t0"] > 0 for P in Ps if P["mode"] == mode) or mode in ("all", "sticky"), mode
    assert sum(P["boom"] for P in Ps) >= 4 and any(P["boom"] and P["nbr"] for P in Ps) and any(P["boom"] and P["move_all"] for P in Ps)
    assert sum(P["tail"] for P in Ps) * 2 >= len(Ps) and sum(not P["tail"] for P in Ps) >= 6
    assert {P["sticky"] for P in Ps if P["sticky"] is not None} == {(False, False), (True, False), (False, True)}
    assert any(P["local"] and P["Gb"] is not P["G"] and P["mu_b"] is not None for P in Ps)
    assert all(P["kernel"] == GC.GENERAL_KERNEL for P in Ps)
    # the combinations with an explicit G: sspdmp, a clock, adaptscale, FactBoomerang run; LocalBound is refused
    assert {P["name"] for P in Ps if P["expect"] == "refuse"} == {"g_local"}


def test_the_stress_draws_reach_a_stated_set():
    Ps = [GC.stress_problem(c)[0] for c in range(GC.STRESS_N)]
    assert {P["stress_mode"] for P in Ps} == set(GC._STRESS_MODES)
    assert {True, False} == {P["adapt"] for P in Ps} == {P["tail"] for P in Ps}
    assert any(P["t0"] > 0 for P in Ps) and any(P["mu_t"] is not None for P in Ps) and any(P["Gb"] is not P["G"] and not P["nbr"] for P in Ps)
    assert sum(P["d"] > 128 for P in Ps) >= 4 and any(P["d"] <= 64 for P in Ps) and any(P["d"] % 64 == 0 for P in Ps) and any(P["d"] % 64 for P in Ps)
    assert all(P["kernel"] == GC.GENERAL_KERNEL for P in Ps)


def test_local_bound_takes_the_argument_G_as_its_one_graph():
    """src/local.jl:95-149 has no G1: spdmp(∇ϕ, t0, x0, θ0, T, C::LocalBound, G, F) moves G[i] (:43), re-bounds every member of G[i] with a draw of
    its own (:61-67) and takes G2 from G's two-hop sets (:108); without the argument G is the pattern of F.Γ (:148).  So a run with an explicit
    G ⊋ pattern(F.Γ) equals the run whose F.Γ carries G's pattern (explicit zeros), bit for bit, and differs from the run without G.  (The oracle
    used to re-bound pattern(F.Γ) only, as src/sfact.jl does for its c::Vector signature.)"""
    P = GC.problem("g_local")
    G, Gb = P["G"], P["Gb"]
    k = 0
    kw = dict(t0=P["t0"], target_mu=P["mu_t"], seed=int(P["seeds"][k]), local_bound=True)
    a = O.spdmp_zigzag(Gb, None, G, P["X0"][k], P["TH0"][k], P["c"], P["T"], G=G, **kw)
    cols = np.repeat(np.arange(P["d"]), np.diff(G.indptr))
    Gb_on_G = sp.csc_matrix((np.asarray(sp.csr_matrix(Gb)[G.indices, cols]).ravel(), G.indices.copy(), G.indptr.copy()), shape=G.shape)  # explicit zeros
    assert np.array_equal(np.diff(Gb_on_G.indptr), np.diff(G.indptr))
    b = O.spdmp_zigzag(Gb_on_G, None, G, P["X0"][k], P["TH0"][k], P["c"], P["T"], **kw)
    c = O.spdmp_zigzag(Gb, None, G, P["X0"][k], P["TH0"][k], P["c"], P["T"], **kw)
    assert a["status"] == b["status"] == 0 and len(a["events"]) >= 150
    assert np.array_equal(a["events"], b["events"]) and a["ndraw_main"] == b["ndraw_main"] and np.array_equal(a["x"], b["x"])
    assert not np.array_equal(a["t"], c["t"])
    # G = All() under LocalBound (src/local.jl:103-105) is not restated by the oracle: refused, not run as something else
    assert O.spdmp_zigzag(G, None, G, P["X0"][k], P["TH0"][k], P["c"], 0.1, local_bound=True, move_all=True)["status"] == 4
