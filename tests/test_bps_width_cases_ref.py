"""Every case of tests/bps_width_cases.py on its reference alone (no device): the case is not vacuous -- status OK, enough accepted reflections
and refreshments, rejected proposals somewhere in each family; the sticky cases freeze and thaw, freeze their last coordinate and freeze in more
than one slot; the speed-recorded cases hold their 40 records.  tests/test_gpu_bps_widths.py asserts the same guards again before it compares."""
import numpy as np
import pytest

import bps_width_cases as BW


def test_the_table_covers_every_form_at_every_slot_count():
    """What the module's docstring promises, from the table itself: every case name at an NS = 4 width, at 257 and at 513, one of the NS = 4
    widths with an empty trailing slot; the FULL widths; Γ couples slots and lanes."""
    for names, cases in ((BW.PLAIN_NAMES, BW.PLAIN_CASES), (["bps", "boom"], BW.STICKY_CASES), (BW.MODERN_FORMS, BW.MODERN_CASES)):
        for name in names:
            at = {d for n, d in cases if n == name}
            assert 129 in at and 257 in at and 513 in at, (name, sorted(at))
            assert at <= set(BW.W)
    assert {d for n, d in BW.PLAIN_CASES if n == "ident"} >= {128, 256, 512}
    assert [BW.slots(d) for d in BW.W] == [2, 2, 3, 4, 4, 5, 8, 9, 16]
    for d in BW.W:
        G = BW.coupling_gamma(d).tocoo()
        off = G.row != G.col
        assert np.any((G.row[off] // 64 != G.col[off] // 64) & (G.row[off] % 64 != G.col[off] % 64))
        A = abs(BW.coupling_gamma(d)).toarray()
        assert np.all(2 * A.diagonal() > A.sum(0))  # strictly diagonally dominant
        mu = BW.coupling_mean(d)
        assert (mu == 0).sum() >= d // 3 and (mu != 0).sum() >= d // 2
        Ls = BW.slot_crossing_factor(d).tocoo()
        assert np.all(Ls.row >= Ls.col) and np.any(Ls.row // 64 != Ls.col // 64)


@pytest.mark.parametrize("d", BW.W)
def test_plain_cases_are_not_vacuous(pkg, d):
    rejected = 0
    for name in [n for n, dd in BW.PLAIN_CASES if dd == d]:
        P, refs = BW.plain_refs(pkg, name, d)
        BW.guard_plain(P, refs)
        assert all(r["t"] >= P["T"] for r in refs)
        rejected += sum(r["num"] - r["nacc"] for r in refs)
    assert rejected > 0 or d == 128  # (128 runs Γ = I alone: the bound is exact)


@pytest.mark.parametrize("d", BW.W)
def test_sticky_cases_are_not_vacuous(pkg, d):
    rejected = 0
    for flow in ("bps", "boom"):
        P, refs = BW.sticky_refs(pkg, flow, d)
        BW.guard_sticky(P, refs)
        assert all(r["t"][0] == P["t0"] and r["t_final"] >= P["T"] for r in refs)
        assert np.unique(P["kappa"]).size == d
        rejected += sum(r["num"] - r["nacc"] for r in refs)
    assert rejected > 0


@pytest.mark.parametrize("d", BW.W)
def test_speed_recorded_cases_are_not_vacuous(d):
    rejected = 0
    for form in [f for f, dd in BW.MODERN_CASES if dd == d]:
        P, refs = BW.modern_refs(form, d)
        BW.guard_modern(P, refs)
        assert all(r["t"][0] > P["t0"] for r in refs)
        rejected += sum(r["num"] - r["nacc"] for r in refs)
    assert rejected > 0
