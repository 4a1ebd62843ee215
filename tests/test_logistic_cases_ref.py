"""Every case of tests/logistic_cases.py on the oracle alone (no device): the case is not vacuous -- healthy chains, at least 150 events and 64
proposals each, the row lengths its line names in at least 5 % of its rows -- and the table as a whole reaches what its docstring says: every
row length 1..6, every remainder |G1[i]| & 7 among the accepted coordinates, accepted coordinates with |G1[i]| > 64 under tracking and at odd d,
an accepted event on the column with a single observation; the violation cases' c; the stress draws' slot counts and k_sub.
tests/test_gpu_logistic_shapes.py asserts the per-case guards again before it compares."""
import numpy as np
import pytest

import logistic_cases as LC
import oracle_lib as O


def _k(P):
    return np.diff(P["Gdrop"].indptr)  # |G1[i]|


def test_the_table_is_what_its_docstring_says():
    P = {n: LC.problem(n) for n in LC.NAMES}
    assert {n: (P[n]["p"], P[n]["ksub"]) for n in LC.NAMES} == {
        "a": (12, 1), "b": (60, 7), "c": (72, 32), "d": (65, 31), "e": (129, 3), "f": (511, 13), "g": (512, 32), "g511": (511, 32), "h": (70, 9),
        "i": (129, 20), "j63": (63, 2), "j64": (64, 10), "j128": (128, 2), "k": (38, 5), "l": (513, 10), "m": (72, 33)}
    # which kernel takes which case follows from the shapes alone (zz_logistic_lds_supported): the key array holds d coordinates and the refresh
    # clock in blocks of 64, and the LDS kernel owns eight blocks -- d = 511 is the largest it takes, 512 the first it does not
    assert [LC.dk_of(d) for d in (63, 64, 447, 448, 511, 512)] == [64, 128, 448, 512, 512, 576]
    for n in LC.NAMES:
        assert LC.lds_takes(P[n]) == (P[n]["kernel"] == "lds"), n
    assert int(LC.row_lengths(P["k"]["A"]).max()) == 8 and LC.lds_takes(dict(P["m"], ksub=32)) and LC.lds_takes(dict(P["g"], p=511))
    assert sum(P[n]["t0"] == 2.5 for n in LC.NAMES) == 2
    sliced = [n for n in LC.NAMES if P[n]["cuts"]]
    assert len(sliced) == 2 and any(P[n]["p"] % 2 for n in sliced) and all(P[n]["kernel"] == "lds" for n in sliced)
    assert [n for n in LC.NAMES if P[n]["cap"] == 0] == ["j64"]
    # the rows kernel (dk <= 448, k_sub + 2 <= W) serves these
    assert [n for n in LC.NAMES if LC.rows_fit(P[n], 32)] == ["a", "b", "e", "h", "i", "j63", "j64", "j128"]
    assert [n for n in LC.NAMES if LC.rows_fit(P[n], 16)] == ["a", "b", "e", "h", "j63", "j64", "j128"]
    # design properties the lines name
    assert np.diff(P["h"]["A"].indptr).min() == 1 == np.diff(P["h"]["A"].indptr)[LC.SINGLE]
    for n in ("d", "f", "j64"):  # an intercept: a column in every row, a G1 set that holds (nearly) every coordinate
        assert np.diff(P[n]["A"].indptr)[0] == P[n]["n"] and _k(P[n])[0] >= P[n]["p"] - 1
    assert _k(P["d"]).max() == 65 and (_k(P["e"]) > 64).sum() > 40 and _k(P["f"])[0] > 448


@pytest.mark.parametrize("name", LC.NAMES)
def test_case_is_not_vacuous(name):
    P = LC.problem(name)
    ne = LC.row_lengths(P["A"])
    for v in P["lens"]:
        assert (ne == v).sum() >= 0.05 * P["n"], (name, v, int((ne == v).sum()), P["n"])
    for tracked in (False, True):
        rs = LC.refs(name, tracked)
        LC.guard_case(P, rs)
        for r in rs:
            assert r["t"].max() <= P["T"] or P["tail"]
            assert r["num"] > r["nacc"]  # (rejections happen)
    # the tracked evaluation is the same process: the same accepted coordinates
    for a, b in zip(LC.refs(name), LC.refs(name, True)):
        assert np.array_equal(a["events"]["i"], b["events"]["i"]) and np.allclose(a["events"]["t"], b["events"]["t"], rtol=1e-9, atol=0)


def test_the_table_reaches_what_it_names():
    lens, rem, wide_tracked, wide_odd = set(), set(), 0, 0
    for name in LC.LDS_NAMES:
        P = LC.problem(name)
        lens |= set(np.unique(LC.row_lengths(P["A"])).tolist())
        for tracked in (False, True):
            for r in LC.refs(name, tracked):
                k = _k(P)[r["events"]["i"]]
                rem |= set((k & 7).tolist())
                wide_tracked += int((k > 64).sum()) if tracked else 0
                wide_odd += int((k > 64).sum()) if P["p"] % 2 else 0
    assert lens >= {0, 1, 2, 3, 4, 5, 6} and rem == set(range(8)) and wide_tracked > 100 and wide_odd > 100
    # odd k_sub (the `two` tail of the staging loop), k_sub = 1 (no pair), 32 (both buffers full), 20 (the partner lanes straddle lane 63 / 0)
    ks = {LC.problem(n)["ksub"] for n in LC.LDS_NAMES}
    assert ks >= {1, 20, 32} and sum(k % 2 for k in ks) >= 5
    # the 65-entry column of case d and the one-observation column of case h are accepted somewhere (an accepted event is a proposal)
    d = LC.problem("d")
    assert sum(int(r["acc"][0]) for r in LC.refs("d")) >= 3 and _k(d)[0] == 65
    assert sum(int(r["acc"][LC.SINGLE]) for r in LC.refs("h")) >= 1 and sum(int(r["acc"][LC.SINGLE]) for r in LC.refs("h", True)) >= 1


@pytest.mark.parametrize("name", sorted(LC.VIOLATION_C))
def test_violation_c_stops_chains_late(name):
    """adapt = false: with c = 0.01 every chain is violated within its first proposals; at the chosen uniform c at least two of six stop after
    at least 20 events."""
    rs = LC.violation_refs(name)
    LC.guard_violation(rs)
    early = [LC.oracle_run(dict(LC.violation_problem(name), c=np.full(LC.problem(name)["p"], 0.01)), k, adapt=False) for k in range(LC.VIOLATION_NCH)]
    assert all(r["status"] == O.ORC_BOUND_VIOLATED and len(r["events"]) < 20 for r in early)


def test_stress_draws_reach_these_slot_counts_and_k_sub():
    slots, ks, odd_d, tracked, t0s = set(), set(), 0, 0, set()
    for case in range(LC.STRESS_N):
        P = LC.stress_problem(case)
        rs = LC.stress_refs(case)
        assert all(r["status"] == 0 and len(r["events"]) >= 100 for r in rs), (case, [(r["status"], len(r["events"])) for r in rs])
        assert 8 <= P["p"] <= 512 and 1 <= P["ksub"] <= 32
        slots.add((P["p"] + 63) // 64)
        ks.add(P["ksub"])
        odd_d += P["p"] % 2
        tracked += P["tracked"]
        t0s.add(P["t0"] > 0)
    assert slots == {1, 2, 3, 4, 6, 7, 8}, sorted(slots)
    assert ks == {7, 9, 15, 16, 19, 21, 23, 24, 26, 27}, sorted(ks)
    assert odd_d >= 3 and 3 <= tracked <= 9 and t0s == {False, True}
