"""The pair integrals of arcs on the device (pdmp_ensemble_bps_consume_arc_pairs) beside the sampler and the plain consumer, on the same slices:
tools/bench_pairs.py's c2 cases on a Boomerang.

    python tools/bench_arc_pairs.py [--case c2_diag|c2_block|all] [--slices 4] [--chains 4096]

Cases (DESIGN.md "Pair integrals of arcs" records the figures, beside bench_pairs.py's c2_diag / c2_block of the same session):
    c2_diag    C2's geometry on a Boomerang: d = 1024, Γ = I, μ = 0, λref = 1, target 1.2 I, steps of dT = 30; pairs = the diagonal
    c2_block   the same, pairs = a dense 64 x 64 block (2080)
Two ensembles with the same seeds run the same slices, one without and one with the pair list.  Per slice: the sampler's ms from the device
events of the run (pdmp_ensemble_last_run_ms) and bps_consume()'s from the device events around its kernels (pdmp_ensemble_last_consume_ms); the
arc walker's ms is the difference of the two ensembles' consume().  The trace buffer is recycled after every slice.  Prints ONE JSON line per
case with the medians over the slices, the smallest and largest plain consume() of the slices (its slice-to-slice spread) and the walker's
events per second (events of the slice over the walker's time).
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402


def timed_slices(pkg, ens, T_step, slices):
    """run -> bps_consume (timed) -> trace_reset until `slices` slices are done; a slice whose buffer filled is consumed in several calls"""
    L = pkg._lib
    run_ms, ms, nev = [], [], []
    for s in range(-1, slices):  # slice −1: warm-up
        tot, run, ev0 = 0.0, 0.0, int(ens.counters()["nevents"].sum())
        while True:
            ens.run(T_step * (s + 2), L.RUN_STOP_BEFORE)
            cnt = ens.counters()
            ens.sync()
            run += ens.last_run_ms()
            ens.bps_consume()
            tot += ens.last_consume_ms()
            ens.trace_reset()
            if not L.needs_rerun(cnt["status"]):
                break
        assert np.all(cnt["status"] == L.CHAIN_OK), np.unique(cnt["status"])
        if s >= 0:
            run_ms.append(run)
            ms.append(tot)
            nev.append(int(cnt["nevents"].sum()) - ev0)
    return float(np.median(run_ms)), ms, int(np.median(nev))


def boomerang(pkg, kind, chains, slices):
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
        with pkg.Ensemble(chains, d, sampler=pkg._lib.SAMPLER_BPS, adapt=True, factor=2.0, trace_capacity=512) as e:
            e.set_flow_boomerang(pkg.GaussianTarget(sp.csc_matrix(1.2 * I), np.zeros(d)), pkg.Boomerang(I, np.zeros(d), 1.0))
            e.set_state_bps(0.0, x0, th0, 3.0, np.uint64(7) + np.arange(chains, dtype=np.uint64))
            e.bps_consume_begin()
            if pairs:
                e.bps_consume_arc_pairs(pi, pj)
            out[pairs] = timed_slices(pkg, e, 30.0, slices)
    (_, plain, _), (run1, both, nev) = out[False], out[True]
    arc_ms = float(np.median(both)) - float(np.median(plain))
    return dict(case=kind, flow="Boomerang", d=d, chains=chains, npairs=len(pi), events_per_slice=nev, sampler_ms=run1,
                consume_ms_plain=float(np.median(plain)), consume_ms_plain_min=float(min(plain)), consume_ms_plain_max=float(max(plain)),
                consume_ms_with_pairs=float(np.median(both)), arc_pairs_ms=arc_ms, walker_events_per_s=nev / (1e-3 * arc_ms) if arc_ms > 0 else None,
                consume_clock="device events")


def main():
    cases = ["c2_diag", "c2_block"]
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=cases + ["all"])
    ap.add_argument("--slices", type=int, default=4)
    ap.add_argument("--chains", type=int, default=4096, help="the benchmark's chain count")
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    for case in (cases if a.case == "all" else [a.case]):
        print(json.dumps(boomerang(pkg, case, a.chains, a.slices)), flush=True)


if __name__ == "__main__":
    main()
