"""The census of the four oldest randomised suites, on the CPU (no device; not marked gpu): tests/stress_cases.py holds their draws, this file
runs every draw through the oracle and pins what came out.

  * every reference chain of every draw has status 0 -- so the device tests assert it and never skip a draw;
  * the event count of every chain: a fingerprint of the draw.  A refactor that shifts one rng call changes the problems and fails HERE;
  * what the draws reach: options on / off, d against 64, 1024 and the key-block size, refresh clocks, start times, bounds and means -- and
    what the old draws did NOT reach, which the appended draws (bps 16.., factboomerang 14..) are there for."""
import numpy as np
import pytest

import stress_cases as S

# events per chain of every draw, in case order (ZigZag families: trace events; bps: trace records)
EVENTS = {
    "parity_slices": [(140, 125, 137), (219, 188, 223), (406, 490, 469), (60, 65, 69), (28, 34, 30), (187, 187, 194), (291, 288, 315), (63, 55, 50),
                      (270, 283, 257), (54, 68, 51), (97, 105, 95), (91, 94, 101)],
    "parity_options": [(127, 135), (372, 355), (106, 112), (99, 106), (313, 318), (125, 128), (45, 51), (201, 193), (318, 333), (446, 437), (98, 81),
                       (308, 311), (185, 179), (86, 90)],
    "parity_sticky": [(229, 242), (291, 300), (521, 549), (304, 294), (517, 510), (422, 453), (431, 425), (438, 436)],
    "factboomerang": [(120, 101), (377, 517), (58, 43), (332, 348), (24, 45), (305, 353), (13, 30), (76, 112), (57, 118), (308, 338), (242, 234),
                      (131, 115), (131, 145), (112, 113),
                      (349, 345), (144, 115), (393, 391), (139, 158), (164, 156), (116, 112)],
    "wide_zigzag": [(373, 357), (440, 463), (630, 606), (193, 189), (292, 311), (528, 562), (405, 405), (312, 294)],
    "sticky_options": [(258, 251), (504, 461), (1358, 1417), (915, 930), (1232, 1310), (1128, 1162), (724, 809), (427, 485), (798, 809), (769, 795),
                       (1284, 1365), (1397, 1453)],
    "bps": [(33, 37), (36, 36), (102, 89), (62, 64), (12, 17), (52, 46), (41, 34), (64, 65), (17, 20), (49, 42), (75, 83), (8, 8), (97, 109), (151, 160),
            (123, 182), (41, 25),
            (152, 178), (180, 178), (139, 138), (216, 189), (142, 123), (138, 137), (100, 104), (127, 126)],
}
D = {
    "parity_slices": [64, 76, 79, 25, 8, 21, 70, 9, 37, 14, 18, 36],
    "parity_options": [56, 169, 33, 14, 144, 23, 9, 57, 101, 144, 21, 102, 41, 15],
    "parity_sticky": [81, 49, 107, 40, 79, 100, 144, 153],
    "factboomerang": [25, 64, 9, 81, 15, 37, 9, 14, 13, 76, 36, 89, 9, 51, 121, 6, 121, 28, 11, 19],
    "wide_zigzag": [117, 134, 146, 112, 126, 170, 128, 143],
    "sticky_options": [208, 99, 115, 324, 529, 182, 201, 81, 841, 256, 90, 283],
    "bps": [200, 49, 64, 4, 14, 9, 65, 1024, 27, 81, 36, 3, 20, 81, 121, 100, 1, 1025, 81, 21, 21, 36, 1025, 1],
}
N = dict(parity_slices=S.PARITY_SLICES_N, parity_options=S.PARITY_OPTIONS_N, parity_sticky=S.PARITY_STICKY_N, factboomerang=S.FACTBOOMERANG_N,
         wide_zigzag=S.WIDE_ZIGZAG_N, sticky_options=S.STICKY_OPTIONS_N, bps=S.BPS_N)
OLD = dict(N, factboomerang=S.FACTBOOMERANG_OLD_N, bps=S.BPS_OLD_N)


def _draw(fam, case):
    return getattr(S, fam + "_draw")(case)


def _refs(fam, case):
    return getattr(S, fam + "_refs")(case)


def _events(fam, r):
    return int(r["nevents"]) if fam == "bps" else len(r["events"])


def test_the_old_files_hold_84_draws():
    assert sum(OLD.values()) == 84 and all(len(EVENTS[f]) == N[f] == len(D[f]) for f in N)


@pytest.mark.parametrize("fam", list(N))
def test_every_reference_chain_is_healthy_and_the_draws_have_not_moved(fam):
    for case in range(N[fam]):
        P, rs = _draw(fam, case), _refs(fam, case)
        assert P["d"] == D[fam][case], (fam, case, P["d"])
        assert all(r["status"] == 0 for r in rs), (fam, case, [r["status"] for r in rs])
        assert tuple(_events(fam, r) for r in rs) == EVENTS[fam][case], (fam, case, [_events(fam, r) for r in rs])


def test_the_appended_draws_are_not_thin():
    for fam in ("bps", "factboomerang"):
        for case in range(OLD[fam], N[fam]):
            assert min(_events(fam, r) for r in _refs(fam, case)) >= S.MIN_EVENTS_NEW, (fam, case)


def test_what_the_bps_draws_reach():
    old = [S.bps_draw(c) for c in range(S.BPS_OLD_N)]
    new = [S.bps_draw(c) for c in range(S.BPS_OLD_N, S.BPS_N)]
    # the old draws: thin chains, one subsample, never d = 1 or 1025 (a statement of the gap the appended draws close; the draws stay)
    assert sorted(min(EVENTS["bps"][c]) for c in range(S.BPS_OLD_N))[:3] == [8, 12, 17]
    assert [P["case"] for P in old if P["subsample"]] == [15] and not any(P["d"] in (1, 1025) for P in old)
    assert sum(P["adapt"] for P in old) == 8 and sum(P["local_bound"] for P in old) == 4 and sum(P["mu"] is not None for P in old) == 12
    assert sum(P["rho"] > 0 for P in old) == 4 and sum(isinstance(P["L"], str) for P in old) == 7
    assert {P["lam"] for P in old} == {0.3, 1.0, 2.5}
    # d against one wavefront (64 lanes: one slot per lane up to 64) and the 1024 of config C2
    assert sum(P["d"] < 64 for P in old) == 8 and [P["d"] for P in old if P["d"] in (64, 65)] == [64, 65] and sum(P["d"] == 1024 for P in old) == 1
    # the appended ones
    assert {(P["subsample"], P["adapt"]) for P in new if P["subsample"]} == {(True, True), (True, False)}
    assert any(P["local_bound"] and P["mu"] is not None for P in new)
    assert {1, 1025} <= {P["d"] for P in new}
    assert any(P["d"] == 1025 and P["subsample"] for P in new) and any(P["d"] == 1 and P["subsample"] for P in new)


def test_what_the_zigzag_draws_reach():
    ps = [S.parity_slices_draw(c) for c in range(S.PARITY_SLICES_N)]
    assert sum(P["adapt"] for P in ps) == sum(bool(P["adapt"]) for P in ps) and 0 < sum(P["adapt"] for P in ps) < len(ps)
    assert all(S.zigzag_kernel(P["G"]) == "zz_local_spec" for P in ps)
    assert sum(P["d"] < 64 for P in ps) == 8 and sum(P["d"] == 64 for P in ps) == 1 and sum(P["d"] > 64 for P in ps) == 3  # (d = 64: the clock's slot alone in block 1)
    po = [S.parity_options_draw(c) for c in range(S.PARITY_OPTIONS_N)]
    assert all(S.zigzag_kernel(P["G"]) == "zz_local_spec" and S.zigzag_kernel(P["G"], "seq") == "zz_local_run_kernel" for P in po)
    reach = dict(lam=[c for c, P in enumerate(po) if P["lam"] > 0], t0=[c for c, P in enumerate(po) if P["t0"] > 0],
                 own=[c for c, P in enumerate(po) if P["Gb"] is not P["G"]], mu_b=[c for c, P in enumerate(po) if P["mu_b"] is not None],
                 mu_t=[c for c, P in enumerate(po) if P["mu_t"] is not None], adapt=[c for c, P in enumerate(po) if P["adapt"]])
    for k, v in reach.items():  # every option occurs on and off
        assert 0 < len(v) < len(po), (k, v)
    assert any(P["lam"] > 0 and P["d"] > 64 and P["d"] % 64 for P in po)  # a refresh clock in a key block it shares with coordinates, beyond block 0
    wz = [S.wide_zigzag_draw(c) for c in range(S.WIDE_ZIGZAG_N)]
    assert all(S.zigzag_kernel(P["G"]) == "zz_general_run_kernel" and S.two_hop_max(P["G"]) > 64 for P in wz)
    for k in ("lam", "adapt"):
        assert 0 < sum(bool(P[k]) for P in wz) < len(wz), k
    assert 0 < sum(P["Gb"] is not P["G"] for P in wz) < len(wz) and 0 < sum(P["mu_b"] is not None for P in wz) < len(wz)
    fb = [S.factboomerang_draw(c) for c in range(S.FACTBOOMERANG_N)]
    assert sorted(EVENTS["factboomerang"][6]) == [13, 30]  # the thin old draw the issue names; the appended ones have 100 events per chain
    for k in ("rho", "adapt"):
        assert 0 < sum(bool(P[k]) for P in fb) < len(fb), k
    assert 0 < sum(bool(np.any(P["mu"])) for P in fb) < len(fb) and any(P["d"] > 64 for P in fb) and any(P["d"] == 64 for P in fb)


def test_what_the_sticky_draws_reach():
    st = [S.sticky_options_draw(c) for c in range(S.STICKY_OPTIONS_N)]
    for k in ("adapt", "rev", "strong"):
        assert 0 < sum(bool(P[k]) for P in st) < len(st), k
    assert 0 < sum(P["Gb"] is not P["G"] for P in st) < len(st)
    assert 0 < sum(P["mu_b"] is not None for P in st) < len(st) and 0 < sum(P["mu_t"] is not None for P in st) < len(st)
    kern = [S.sticky_kernel(P["G"]) for P in st]
    assert set(kern) == {"zz_sticky_spec_kernel", "zz_sticky_run_kernel"} and kern.count("zz_sticky_run_kernel") == 2
    ps = [S.parity_sticky_draw(c) for c in range(S.PARITY_STICKY_N)]
    assert [S.sticky_kernel(P["G"]) for P in ps].count("zz_sticky_run_kernel") == 3
    assert 0 < sum(P["reversible"] for P in ps) < len(ps) and 0 < sum(P["strong"] for P in ps) < len(ps)
