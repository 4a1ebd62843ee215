"""The census of the barrier ZigZag's randomised and named-edge draws, on the CPU (no device; not marked gpu): tests/stickyzz_stress_cases.py
holds the draws, this file runs every draw through the restatement (tests/ref/stickyzz_ref.c) and pins what came out.

  * a fingerprint per draw (a hash over the drawn arrays) and its event counts: a refactor that shifts one rng call fails HERE;
  * every reference chain has status REF_OK -- so tests/test_gpu_stickyzz_stress.py asserts it and never skips a draw;
  * what family A reaches, asserted over the whole family and printed under -s; what every named edge must show;
  * the restatement under a flow mean and a start time, which it is the authority for on the device side: a time shift and a translation
    of the whole problem, two identities of the process that its arithmetic knows nothing of."""
import numpy as np
import pytest
import scipy.sparse as sp

import stickyzz_cases as K
import stickyzz_ref_lib as R
import stickyzz_stress_cases as Z

INF = float("inf")

OPTIONS = [  # (fingerprint, d, events per chain) of options_draw(case), in case order
    ("5a51a1eb310d", 79, (247, 252)), ("4207d46b7fd8", 184, (300, 290, 294)), ("faf0456ae325", 70, (280, 250, 277)), ("cd1a5e4c9188", 94, (242, 274)),
    ("46e7b083b31b", 111, (256, 216)), ("c56f0fb0e279", 144, (285, 279, 285)), ("1d21f45feb8f", 8, (213, 261)), ("7d2832a39771", 9, (359, 385)),
    ("8a16eef89fbb", 191, (262, 289, 269)), ("d4db89950b3c", 29, (218, 296, 225)), ("70a1f19b8c6a", 82, (231, 264)), ("b736c7ef67dc", 10, (457, 377, 358)),
    ("d5a70cce1dd7", 107, (243, 272)), ("0b9ba18981e6", 100, (265, 282, 292)), ("44c4999b01e4", 25, (303, 354, 334)), ("538700d88431", 47, (305, 320)),
]
EDGES = {  # fingerprint and the events of the first two chains of edge_draw(name)
    "hub63_free": ("d360bee621b1", (1182, 1184)), "hub63_reversible": ("0f7b6ee66bc4", (1190, 1251)), "hub63_mixed": ("d30c48e80e0d", (982, 1075)),
    "hub63_mixed_strong": ("4cb49245dd0c", (1022, 1045)), "blocks_63": ("fbf6f6a6d1cc", (842, 869)), "blocks_64": ("d7831c81c213", (992, 1003)),
    "blocks_65": ("c68e7dd49f6b", (948, 947)), "blocks_128": ("44ca048802c7", (1906, 1780)), "blocks_129": ("a8e9dcb1f0b0", (1911, 1920)),
    "ties_0": ("3f2cd8f92b6b", (509,)), "ties_1": ("ed5e174ae778", (559,)), "ties_2": ("81d7fd793201", (402,)),
    "level_start_8": ("987ff2cbcd31", (184, 196)), "level_start_144": ("5912a243d8de", (2111, 2185)), "many_chains": ("c557cc3fcfd9", (175, 286)),
}


def _healthy(P, rs):
    assert all(r["status"] == R.REF_OK for r in rs), (P["case"], [r["status"] for r in rs])
    assert all(r["nevents"] == len(r["t"]) for r in rs), P["case"]  # (no chain outgrew the restatement's event buffer)
    assert all(np.all(np.diff(r["t"]) >= 0) and r["t"][0] >= P["t0"] for r in rs), P["case"]
    assert Z.sticky_kernel(P["G"]) != "zz_general_run_kernel" and Z.col_max(P["G"]) <= 63, P["case"]  # a graph the barrier kernel takes
    assert np.all((P["cuts"] > P["t0"]) & (P["cuts"] < P["T"])) and np.any(np.diff(P["cuts"]) == 0), P["case"]


def test_the_draws_have_not_moved_and_every_reference_chain_is_healthy():
    assert len(OPTIONS) == Z.OPTIONS_N and list(EDGES) == Z.EDGE_NAMES
    for case, (fp, d, nev) in enumerate(OPTIONS):
        P, rs = Z.options_draw(case), Z.options_refs(case)
        assert (Z.fingerprint(P), P["d"], tuple(r["nevents"] for r in rs)) == (fp, d, nev), (case, Z.fingerprint(P), P["d"], [r["nevents"] for r in rs])
        _healthy(P, rs)
        assert min(nev) >= Z.MIN_EVENTS and max(nev) <= Z.MAX_EVENTS  # (the doubling ended on the first condition in every draw)
    for name, (fp, nev) in EDGES.items():
        P, rs = Z.edge_draw(name), Z.edge_refs(name)
        assert (Z.fingerprint(P), tuple(r["nevents"] for r in rs[:2])) == (fp, nev), (name, Z.fingerprint(P), [r["nevents"] for r in rs[:2]])
        _healthy(P, rs)
        assert name.startswith("ties") == (P["mu_b"] is None)  # the flow mean is non-zero everywhere but where coordinates must stay identical


def test_census_of_the_random_options():
    """What the 16 draws reach together (printed under -s)."""
    draws = [Z.options_draw(c) for c in range(Z.OPTIONS_N)]
    met, thawed0, adapted = set(), 0, 0
    for P in draws:
        fro = Z.starts_frozen(P)
        rs = Z.options_refs(P["case"])
        for k, r in enumerate(rs):
            m, th = Z.thaw_census(r, P["th0"][k], P["bars"], fro[k])
            met |= m
            thawed0 += len(th)
        adapted += any(r["nadapt"] >= 1 for r in rs)
        print(Z.what(P), "start-frozen", int(fro.sum()), "events", [r["nevents"] for r in rs], "hit/thaw/refl",
              [(r["nhit"], r["nthaw"], r["nrefl"]) for r in rs], "nadapt", [r["nadapt"] for r in rs])
    means = {(P["mu_b"] is not None, P["mu_t"] is not None) for P in draws}
    print("thaws met (side, rule, wall):", sorted(met), "start-frozen thawed:", thawed0, "cases that adapt:", adapted, "means:", sorted(means))
    assert {(s, r) for s, r, _ in met} == {(s, r) for s in (0, 1) for r in Z.RULE_NAMES}  # every rule on every side met by a thaw
    assert {w for _, _, w in met} == {False, True}  # a wall and a finite κ
    assert thawed0 >= 1 and adapted >= 3
    assert means == {(False, False), (True, False), (False, True), (True, True)}
    assert any(P["mu_t"] is not None and P["mu_t"] is P["mu_b"] for P in draws)  # (and, among "both", the target's mean being the flow's)
    assert any(P["t0"] != 0 for P in draws) and any(P["t0"] == 0 for P in draws)
    assert any(P["strong"] for P in draws) and not all(P["strong"] for P in draws)
    assert any(P["Gb"] is not P["G"] for P in draws) and any(P["Gb"] is P["G"] for P in draws)
    assert {P["kind"] for P in draws} == set(Z.GRAPH_KINDS)
    assert {P["nch"] for P in draws} == {2, 3} and all(16 <= P["cap"] <= 128 and 2 <= len(P["cuts"]) <= 5 for P in draws)
    assert any(P["d"] > 128 for P in draws) and any(P["d"] < 64 for P in draws)  # one key block, and three


def _events_of(r, i):
    return np.nonzero(r["i"] == i)[0]


@pytest.mark.parametrize("name", ["hub63_free", "hub63_reversible", "hub63_mixed", "hub63_mixed_strong"])
def test_hub_edges(name):
    """|G1[0]| = 63, |G1 ∪ G2| = 64 for the hub and for leaf 1: the widest column the barrier sampler takes, whose events use candidate 63."""
    P, rs = Z.edge_draw(name), Z.edge_refs(name)
    G = P["G"]
    assert P["d"] == 64 and G.indptr[1] - G.indptr[0] == 63 and Z.col_max(G) == 63 and Z.two_hop_max(G) == 64
    A = sp.csc_matrix((np.ones(G.nnz), G.indices, G.indptr), shape=G.shape)
    assert np.diff(sp.csc_matrix(A @ A).indptr)[:2].tolist() == [64, 64]
    for k, r in enumerate(rs):
        hub = _events_of(r, 0)
        if name == "hub63_free":  # nobody is ever frozen: an accepted reflection of the hub re-bounds 63 members behind its coin
            assert P["t0"] == 1.5 and r["nhit"] == 0 and not Z.starts_frozen(P).any()
            assert np.sum(r["kind"][hub] == R.EV_REFLECTION) >= 20, (name, k, len(hub))
        elif name == "hub63_reversible":  # only the hub has barriers: at its thaw all 63 members are free, the sign coin makes 64 draws
            assert all(b == K.NO_BARRIER for b in P["bars"][1:]) and P["bars"][0][1] == ("reversible", "reversible") and max(P["bars"][0][2]) < INF
            assert np.sum(r["kind"][hub] == R.EV_THAW) >= 10, (name, k)
        else:
            assert P["adapt"] and P["strong"] == (name == "hub63_mixed_strong")
            assert min(r["nhit"], r["nthaw"], r["nrefl"]) > 100 and len(hub) >= 15, (name, k, r["nhit"], r["nthaw"], r["nrefl"], len(hub))


@pytest.mark.parametrize("d", Z.BLOCKS_D)
def test_block_edges(d):
    """d at, just below and just above a multiple of the 64 keys of a block: events in every key block, a hit and a thaw of the last coordinate."""
    P, rs = Z.edge_draw("blocks_%d" % d), Z.edge_refs("blocks_%d" % d)
    assert P["d"] == d and (P["t0"] == 0.75) == (d in (65, 129)) and Z.col_max(P["G"]) == 5
    for r in rs:
        assert set(r["i"] // 64) == set(range((d + 63) // 64))
        last = r["kind"][_events_of(r, d - 1)]
        assert np.any(last == R.EV_HIT) and np.any(last == R.EV_THAW), (d, last)


@pytest.mark.parametrize("k", range(len(Z.TIES_RULES)))
def test_ties_edges(k):
    """Identical coordinates under Γ = I and walls give bit-equal keys; the queue's "lowest coordinate wins" is then decided between key blocks."""
    P, (r,) = Z.edge_draw("ties_%d" % k), Z.edge_refs("ties_%d" % k)
    assert P["d"] == 130 and P["seed"] == 9 and P["T"] == 3.0 and np.all(P["c"] == 0.01) and P["mu_b"] is None and P["mu_t"] is None
    same_t = r["t"][1:] == r["t"][:-1]
    cross = same_t & (r["i"][1:] // 64 != r["i"][:-1] // 64)
    hit_hit = same_t & (r["kind"][1:] == R.EV_HIT) & (r["kind"][:-1] == R.EV_HIT)
    print("ties", k, "cross-block tie pairs", int(cross.sum()), "hit-hit pairs at equal t", int(hit_hit.sum()))
    assert cross.sum() >= 2
    assert np.all(r["i"][1:][same_t & (r["kind"][1:] == r["kind"][:-1])] > r["i"][:-1][same_t & (r["kind"][1:] == r["kind"][:-1])])  # lowest first
    if k != 1:
        assert hit_hit.sum() >= 50


@pytest.mark.parametrize("d", [8, 144])
def test_level_start_edges(d):
    """lo == hi = 0.3 on every coordinate, x0 exactly 0.3 on a third of them, two neighbours among them (at d = 144: 63 and 64, either side of a
    key-block boundary), both signs of θ0: each starts frozen, and its first event is its thaw, later than t0."""
    P, rs = Z.edge_draw("level_start_%d" % d), Z.edge_refs("level_start_%d" % d)
    on = P["on_level"]
    G = P["G"]
    assert P["t0"] == 2.5 and all(b[0] == (0.3, 0.3) for b in P["bars"]) and {b[1][0] for b in P["bars"]} == set(Z.RULE_NAMES)
    assert d // 3 <= len(on) <= d // 3 + 2 and np.all(P["x0"][:, on] == 0.3)
    assert any(j in G.indices[G.indptr[i]:G.indptr[i + 1]] for i in on for j in on if i != j)
    if d == 144:
        assert 63 in on and 64 in on and 63 in G.indices[G.indptr[64]:G.indptr[65]]
    for k, r in enumerate(rs):
        assert {-1.0, 1.0} <= set(P["th0"][k, on])
        assert np.array_equal(Z.starts_frozen(P)[k], np.isin(np.arange(d), on))
        for i in on:
            first = _events_of(r, i)[0]
            assert r["kind"][first] == R.EV_THAW and r["t"][first] > P["t0"] and r["x"][first] == 0.3, (d, k, i)


def test_many_chains_edge():
    P, rs = Z.edge_draw("many_chains"), Z.edge_refs("many_chains")
    assert P["nch"] == 130 and P["d"] == 8 and P["T"] == 20.0 and len(rs) == 130 and all(r["status"] == R.REF_OK for r in rs)


def test_the_refused_hub_is_not_a_general_kernel_graph():
    G = Z.refused_hub()
    assert G.indptr[1] - G.indptr[0] == 64 and Z.col_max(G) == 64 and Z.two_hop_max(G) == 64 and Z.sticky_kernel(G) == "zz_sticky_run_kernel"


# ------------------------------------------------------------------------------------------------- the restatement under μ and t0, pinned

def _identity_cases():
    P8, PH = Z.edge_draw("many_chains"), Z.edge_draw("hub63_mixed")
    return {"d8_mixed": (P8, 3), "hub63_mixed": (PH, 2)}


def _generic_start(P, k):
    """x0 of chain k drawn uniformly inside the middle 80 % of its barriers.  The cases' own starts are clipped to 0.05 from a barrier
    (fit_state), so a dozen coordinates of speed ±1 hit at t0 + 0.05 up to the last bit, and the order of hits that tie up to rounding is
    arithmetic, not process: under a shift it changes, and with it the order of the draws.  Everything else is the case's."""
    rng = np.random.default_rng(900 + k)
    lo, hi = np.array([b[0][0] for b in P["bars"]]), np.array([b[0][1] for b in P["bars"]])
    a = np.where(np.isfinite(lo), lo, np.where(np.isfinite(hi), hi - 2.0, -1.0))
    b = np.where(np.isfinite(hi), hi, a + 2.0)
    return a + (b - a) * rng.uniform(0.1, 0.9, P["d"])


def _run(P, k, *, t0, T, x0=None, bars=None, mu=None, mu_t=None):
    r = R.stickyzz(t0, _generic_start(P, k) if x0 is None else x0, P["th0"][k], T, P["c"], P["bars"] if bars is None else bars, gamma=P["Gb"], mu=mu,
                   target_gamma=P["G"], target_mu=mu_t, strong_upperbounds=P["strong"], adapt=P["adapt"], factor=Z.FACTOR, seed=P["seed"] + k)
    assert r["status"] == R.REF_OK and r["nevents"] > 100 and min(r["nhit"], r["nthaw"], r["nrefl"]) > 20
    return r


@pytest.mark.parametrize("name", ["d8_mixed", "hub63_mixed"])
def test_restatement_time_shift(name):
    """The run from t0 = 0 to 20 and the run from t0 = 4 to 24 (the case's own means) are one path: the same i, kind and θ sequences, x and
    t − t0 within 1e-9.  An identity of the process, not of the arithmetic (x[j] + θ (t′ − t[j]) rounds differently at other times), so 1e-9
    is a rounding allowance -- eight digits above the unit roundoff at these magnitudes -- and not a measured tolerance.  No thinning coin
    flips under the changed rounding at the cases' own seeds."""
    P, nch = _identity_cases()[name]
    for k in range(nch):
        a = _run(P, k, t0=0.0, T=20.0, mu=P["mu_b"], mu_t=P["mu_t"])
        b = _run(P, k, t0=4.0, T=24.0, mu=P["mu_b"], mu_t=P["mu_t"])
        for f in ("i", "kind", "theta"):
            assert np.array_equal(a[f], b[f]), (name, k, f)
        assert np.max(np.abs(a["x"] - b["x"])) <= 1e-9 and np.max(np.abs(a["t"] - (b["t"] - 4.0))) <= 1e-9
        assert np.all(b["t"] > 4.0) and (a["nacc"], a["num"], a["ndraw_main"]) == (b["nacc"], b["num"], b["ndraw_main"])


@pytest.mark.parametrize("name", ["d8_mixed", "hub63_mixed"])
def test_restatement_translation(name):
    """One vector s added to x0, to both barrier levels and to both means: the run is the zero-mean run moved by s -- the same i, kind and θ,
    x − s[i] and t within 1e-9 (a rounding allowance, as above).  This is what holds the restatement's flow mean (gmu of ab) and target mean
    to the process: with either ignored the bound or the gradient sees x instead of x − s and the chains part within a few events."""
    P, nch = _identity_cases()[name]
    d = P["d"]
    s = 0.7 * np.random.default_rng(77).standard_normal(d)
    moved = [((b[0][0] + s[i], b[0][1] + s[i]), b[1], b[2]) for i, b in enumerate(P["bars"])]
    for k in range(nch):
        a = _run(P, k, t0=0.0, T=20.0)
        b = _run(P, k, t0=0.0, T=20.0, x0=_generic_start(P, k) + s, bars=moved, mu=s, mu_t=s)
        for f in ("i", "kind", "theta"):
            assert np.array_equal(a[f], b[f]), (name, k, f)
        assert np.max(np.abs(a["x"] - (b["x"] - s[b["i"]]))) <= 1e-9 and np.max(np.abs(a["t"] - b["t"])) <= 1e-9
        assert np.max(np.abs(a["x_final"] - (b["x_final"] - s))) <= 1e-9
