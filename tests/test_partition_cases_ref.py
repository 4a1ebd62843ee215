"""The census of tests/partition_cases.py on the oracle alone (no device): every row reaches what it claims.  These are conditions on the INPUTS of
tests/test_gpu_partition_cases.py, not measurements of the kernel; run with -s for the per-case figures (events, rounds, waits)."""
import numpy as np
import pytest

import oracle_lib as O
import partition_cases as PC

MIN_BEFORE = 99  # a violation case has at least 100 events, the 100th before the stopping proposal


@pytest.mark.parametrize("name", PC.NAMES)
def test_case_reaches_what_its_row_claims(name):
    c = PC.case(name)
    o = c.opt
    assert c.d % c.K == 0 and c.d <= 8320
    assert c.kG == o["kG"] and c.g2 == o["g2"]  # max |G[i]|, max |G2[i]|
    assert c.kG <= 64
    has_links = not c.inner.all()
    assert has_links == c.links
    for chain in range(c.nchains):
        r = PC.reference(name, chain)
        ev = r["events"]
        print("%-15s chain %d: d = %d, K = %d, k = %d, events %d, proposals %d, rounds %d, waits %d" %
              (name, chain, c.d, c.K, c.k, len(ev), r["num"], r["rounds"], PC.waits(r, c.K)))
        assert r["status"] == PC.expected_status(c)
        assert PC.MIN_EVENTS <= len(ev) <= 3000 and r["nacc"] == len(ev)
        if c.K > 1 and has_links:
            assert PC.waits(r, c.K) > 0  # some chunk waited for a neighbouring chunk
        else:
            assert PC.waits(r, c.K) == 0
        if c.expect == PC.TRACE_FULL:
            assert len(ev) > c.trace_capacity > 0
        elif c.trace_capacity:
            assert len(ev) <= c.trace_capacity


def test_chunk_shapes():
    """nbc = ceil(k / 64): beyond one pass of peek's 64 lanes, a partial last block behind a full one, one key per chunk; K odd, 1 and 16."""
    nbc = {n: -(-PC.case(n).k // 64) for n in PC.NAMES}
    assert nbc["tri_K1"] == 65 and PC.case("tri_K1").K == 1 and PC.case("tri_K1").inner.all()
    assert nbc["tri_K2_long"] == 65 and PC.case("tri_K2_long").K == 2
    assert nbc["tri_K7"] == 2 and PC.case("tri_K7").k % 64 != 0 and PC.case("tri_K7").K == 7
    assert PC.case("tri_k1").k == 1 and not PC.case("tri_k1").inner.any()
    assert PC.case("band31_K3").inner.sum() < PC.case("band31_K3").d / 2  # most coordinates on the border
    assert PC.case("dense64_K4").inner.all()
    assert {PC.case(n).K for n in PC.NAMES} >= {1, 2, 3, 4, 7, 16}
    assert max(PC.case(n).g2 for n in PC.NAMES) > 64


def test_horizon_cases():
    """Δ = 50: the run is over before the first horizon, so a worker never parks because of it, and the workers do propose (more looks at
    their queues than wakes).  Δ = 1e-4: the coordinator proposes what a worker parked on, and the woken worker's new head lies beyond its
    horizon again, so it parks on its first look: num (the workers' looks) = spawns (their wakes), no proposal is a worker's."""
    big, tiny = PC.case("tri_k3_bigΔ"), PC.case("tri_k3_tinyΔ")
    rb, rt = PC.reference("tri_k3_bigΔ"), PC.reference("tri_k3_tinyΔ")
    assert big.t0 + big.delta > 2 * big.T and rb["events"]["t"].max() < big.t0 + big.delta
    assert rb["num"] > rb["spawns"]
    assert rt["num"] == rt["spawns"] and tiny.inner[rt["events"]["i"]].sum() > 0  # (inner coordinates have events all the same: the coordinator's)


def test_weak_adapt_adapts_in_workers_and_in_the_coordinator():
    c, r = PC.case("weak_adapt"), PC.reference("weak_adapt")
    grew = r["c"] > c.c
    assert grew[c.inner].any() and grew[~c.inner].any()
    assert np.array_equal(r["c"][~grew], c.c[~grew])
    # the control: with the chunk-diagonal of the target itself as the bound no INNER coordinate is ever adapted (the module's docstring)
    cc = PC.Case("weak_adapt", bscale=1.0)
    rc = cc.oracle()
    assert np.array_equal(rc["c"][cc.inner], cc.c[cc.inner]) and (rc["c"][~cc.inner] > cc.c[~cc.inner]).any()


def test_weak_violate_stops_on_a_worker():
    """The oracle's result does not name the coordinate that stopped the run.  With Δ beyond T the coordinator proposes border coordinates only
    (the module's docstring), and the same inputs with adapt=True -- the same run up to the first violation, which is then an adaptation --
    adapt inner coordinates ONLY, over the whole of [t0, T]: so the first violation, like every later one, is an inner coordinate's, raised
    by the worker of its chunk."""
    c, r = PC.case("weak_violate"), PC.reference("weak_violate")
    assert r["status"] == O.ORC_BOUND_VIOLATED and len(r["events"]) > 100
    assert c.t0 + c.delta > c.T
    ra = c.oracle(adapt=True)
    assert ra["status"] == O.ORC_OK
    grew = ra["c"] > c.c
    assert grew[c.inner].any() and not grew[~c.inner].any()
    # the workers of the stopped run did what those of the adapting run did, up to the stop: its inner events are among the adapting run's
    inner_ev = r["events"][c.inner[r["events"]["i"]]]
    assert len(inner_ev) > 100 and set(map(tuple, inner_ev.tolist())) <= set(map(tuple, ra["events"].tolist()))
    # and the proposal that stopped it, told from the two runs: an inner coordinate's, moved to its time and not recorded
    stop = PC.stopping_proposal(c, r, ra)
    assert stop is not None and c.inner[stop[0]] and stop[1] > r["events"]["t"][MIN_BEFORE]
    # the coordinator's draws decide accepts here (the module's docstring: why these inputs): it has accepted border proposals
    assert (~c.inner[r["events"]["i"]]).sum() > 0


def test_border_violate_stops_on_the_coordinator():
    """Bound = the chunk-diagonal of the target: an inner coordinate's bound is exact, so only a border coordinate -- the coordinator's -- violates."""
    c, r = PC.case("border_violate"), PC.reference("border_violate")
    assert r["status"] == O.ORC_BOUND_VIOLATED and len(r["events"]) > 100
    ra = c.oracle(adapt=True)
    grew = ra["c"] > c.c
    assert grew[~c.inner].any() and not grew[c.inner].any()


def test_mu_case_differs_from_the_run_without_means():
    c, r = PC.case("rand12_K3_mu"), PC.reference("rand12_K3_mu")
    assert c.mu_t is not None and c.mu_b is not None and np.all(c.mu_t != 0) and np.all(c.mu_b != c.mu_t)
    for over in (dict(target_mu=None), dict(bound_mu=None), dict(target_mu=None, bound_mu=None)):
        r0 = c.oracle(**over)
        assert not np.array_equal(r0["x"], r["x"])
        assert len(r0["events"]) != len(r["events"]) or not np.array_equal(r0["events"]["t"], r["events"]["t"])


def test_t0_cases_start_at_the_references_unoffset_times():
    """src/parallel.jl:132-136 enqueues the first times without t0: with t0 = 0.75 the first events lie BEFORE t0 (below t0 + Δ, the first
    segment negative), with t0 = −2.5 they lie at 0+, beyond the first horizon t0 + Δ (every worker parks on its first look)."""
    pos, neg = PC.case("tri_K7_t0pos"), PC.case("tri_K7_t0neg")
    tp, tn = PC.reference("tri_K7_t0pos")["events"]["t"], PC.reference("tri_K7_t0neg")["events"]["t"]
    assert 0 < tp[0] < pos.t0 < pos.t0 + pos.delta and (tp < pos.t0).sum() > 100
    assert neg.t0 + neg.delta < 0 < tn[0] < 0.05


def test_wide_G_has_masked_members_and_no_G2():
    c = PC.case("wide_G")
    full, own = c.Gfull, PC.pattern(c.Gb)
    assert c.g2 == 0 and full.nnz > (own + PC.pattern(c.Gt)).nnz  # members of G that neither matrix has: zeros of both
    masked = np.diff(full.indptr) - np.diff(own.indptr)
    assert masked.min() >= 0 and masked.max() >= 4 and (masked[c.inner] > 0).any()


@pytest.mark.parametrize("name", PC.NAMES)
def test_the_oracles_own_trace_is_on_its_path(name):
    """check_path on the reference alone: the derived bound 2u·X_i·m holds for the oracle's trace and final state."""
    c = PC.case(name)
    for chain in range(min(c.nchains, 2)):
        r = PC.reference(name, chain)
        worst = PC.check_path(c.t0, c.x0[chain], c.th0[chain], r["events"], r["t"], r["x"], r["theta"], r["num"] + len(r["events"]) + 1)
        print("%-15s chain %d: largest error / bound = %.2e" % (name, chain, worst))
