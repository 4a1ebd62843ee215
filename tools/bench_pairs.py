"""The pair integrals on the device (pdmp_ensemble_[bps_]consume_pairs) beside the sampler and the plain consumer, on the same slices.

    python tools/bench_pairs.py [--case c3_diag|c3_gamma|c2_diag|c2_block|all] [--slices 4] [--chains 4096]

Cases (DESIGN.md "Pair integrals" records the figures):
    c3_diag    C3's geometry: 128 x 128 lattice GMRF, d = 16384, tracked sampler, steps of dT = 1; pairs = the diagonal (16 384)
    c3_gamma   the same, pairs = the lower triangle of Γ with the diagonal (48 896): every event closes its own square and four neighbours
    c2_diag    C2's geometry: BouncyParticle, d = 1024, Γ = I, steps of dT = 30; pairs = the diagonal
    c2_block   the same, pairs = a dense 64 x 64 block (2080)
Two ensembles with the same seeds run the same slices, one without and one with pairs.  Per slice: the sampler's ms from the device events of
the run (pdmp_ensemble_last_run_ms); consume() of either ensemble -- the Bouncy Particle family's from the device events around its kernels
(pdmp_ensemble_last_consume_ms), the factorised family's synchronous consume() on the host clock with the device idle before it (it keeps no
device timing) --; the pair consumer's ms is their difference.  The trace buffer is recycled after every slice.  Prints ONE JSON line per case
with the medians over the slices and the walker's events per second (events of the slice over the pair consumer's time).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402


def timed_slices(pkg, ens, T_step, slices, consume, device_ms):
    """run -> consume (timed) -> trace_reset until `slices` slices are done; a slice whose buffer filled is consumed in several calls"""
    L = pkg._lib
    run_ms, ms, nev = [], [], []
    for s in range(-1, slices):  # slice −1: warm-up
        tot, run, ev0 = 0.0, 0.0, int(ens.counters()["nevents"].sum())
        while True:
            ens.run(T_step * (s + 2), L.RUN_STOP_BEFORE)
            cnt = ens.counters()
            ens.sync()
            run += ens.last_run_ms()
            t = time.perf_counter()
            consume()
            tot += ens.last_consume_ms() if device_ms else 1e3 * (time.perf_counter() - t)
            ens.trace_reset()
            if not L.needs_rerun(cnt["status"]):
                break
        assert np.all(cnt["status"] == L.CHAIN_OK), np.unique(cnt["status"])
        if s >= 0:
            run_ms.append(run)
            ms.append(tot)
            nev.append(int(cnt["nevents"].sum()) - ev0)
    return float(np.median(run_ms)), float(np.median(ms)), int(np.median(nev))


def report(case, d, chains, npairs, out, clock):
    (run0, plain, _), (run1, both, nev) = out[False], out[True]
    pair_ms = both - plain
    return dict(case=case, d=d, chains=chains, npairs=npairs, events_per_slice=nev, sampler_ms=run1, consume_ms_plain=plain, consume_ms_with_pairs=both,
                pairs_ms=pair_ms, walker_events_per_s=nev / (1e-3 * pair_ms) if pair_ms > 0 else None, consume_clock=clock)


def lattice(pkg, kind, chains, slices):
    m = 128
    d = m * m
    G = pkg.problems.gmrf_precision(m)
    c = pkg.problems.column_norms(G)
    rng = np.random.default_rng(1)
    x0, th0 = pkg.problems.gmrf_stationary_sample(m, chains, rng), rng.choice([-1.0, 1.0], (chains, d))
    pi = pj = np.arange(d, dtype=np.int64)
    if kind == "c3_gamma":
        A = sp.coo_matrix(sp.tril(G, -1))
        pi, pj = np.concatenate([pi, A.row.astype(np.int64)]), np.concatenate([pj, A.col.astype(np.int64)])
    out = {}
    for pairs in (False, True):
        with pkg.Ensemble(chains, d, trace_capacity=20480) as e:  # a step of dT = 1 is ~13 000 events per chain
            e.set_flow(pkg.ZigZag(G, np.zeros(d)))
            e.set_target(pkg.GaussianTarget(G))
            e.set_gradient_tracking(True)
            e.set_state(0.0, x0, th0, c, np.uint64(7) + np.arange(chains, dtype=np.uint64))
            e.consume_begin()
            if pairs:
                e.consume_pairs(pi, pj)
            out[pairs] = timed_slices(pkg, e, 1.0, slices, e.consume, False)
    return report(kind, d, chains, len(pi), out, "host")


def bps(pkg, kind, chains, slices):
    d = 1024
    I = sp.identity(d, format="csc")
    rng = np.random.default_rng(2)
    x0, th0 = rng.standard_normal((chains, d)), rng.standard_normal((chains, d))
    if kind == "c2_diag":
        pi = pj = np.arange(d, dtype=np.int64)
    else:
        a, b = np.tril_indices(64)
        pi, pj = a.astype(np.int64) + 480, b.astype(np.int64) + 480
    out = {}
    for pairs in (False, True):
        with pkg.Ensemble(chains, d, sampler=pkg._lib.SAMPLER_BPS, factor=2.0, trace_capacity=512) as e:  # a step of dT = 30 is ~410 events
            e.set_flow_bps(pkg.BouncyParticle(I, np.zeros(d), 1.0))
            e.set_state_bps(0.0, x0, th0, 1e-3, np.uint64(7) + np.arange(chains, dtype=np.uint64))
            e.bps_consume_begin()
            if pairs:
                e.bps_consume_pairs(pi, pj)
            out[pairs] = timed_slices(pkg, e, 30.0, slices, e.bps_consume, True)
    return report(kind, d, chains, len(pi), out, "device events")


def main():
    cases = ["c3_diag", "c3_gamma", "c2_diag", "c2_block"]
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=cases + ["all"])
    ap.add_argument("--slices", type=int, default=4)
    ap.add_argument("--chains", type=int, default=4096, help="the benchmark's chain count")
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    for case in (cases if a.case == "all" else [a.case]):
        r = lattice(pkg, case, a.chains, a.slices) if case.startswith("c3") else bps(pkg, case, a.chains, a.slices)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
