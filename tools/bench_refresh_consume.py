"""The unordered device consumers (pdmp_ensemble_refresh_consume_begin) beside the sampler, and the sorted consumer on the same geometry.

    python tools/bench_refresh_consume.py [--case refresh|plain|all] [--slices 4] [--chains 4096] [--lambda-ref 1.0] [--grid-dt 0.5]

Cases (DESIGN.md §20 records the figures):
    refresh   C3R's configuration: 128 x 128 lattice GMRF, d = 16384, ZigZag(Γ, 0, σ = 1; λref), the reference's own arithmetic (the tracked
              evaluation has no refresh clock), steps of dT = 1; consume() after refresh_consume_begin
    plain     the same geometry and sampler arithmetic without the refresh clock; consume() after consume_begin (the sorted walk)
Each case runs twice with the same seeds, without a grid and with a grid of step --grid-dt.  Per slice: the sampler's ms from the device events of
the run (pdmp_ensemble_last_run_ms) and the synchronous consume() on the host clock with the device idle before it (the factorised consumers
keep no device timing).  The trace buffer is recycled after every slice.  Prints ONE JSON line per case with the medians over the slices.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402


def timed_slices(pkg, ens, T_step, slices):
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
            ens.consume()
            tot += 1e3 * (time.perf_counter() - t)
            ens.trace_reset()
            if not L.needs_rerun(cnt["status"]):
                break
        assert np.all(cnt["status"] == L.CHAIN_OK), np.unique(cnt["status"])
        if s >= 0:
            run_ms.append(run)
            ms.append(tot)
            nev.append(int(cnt["nevents"].sum()) - ev0)
    return float(np.median(run_ms)), float(np.median(ms)), int(np.median(nev))


def lattice(pkg, case, chains, slices, lambda_ref, grid_dt):
    m_side = 128
    d = m_side * m_side
    G = pkg.problems.gmrf_precision(m_side)
    c = pkg.problems.column_norms(G)
    rng = np.random.default_rng(1)
    x0, th0 = pkg.problems.gmrf_stationary_sample(m_side, chains, rng), rng.choice([-1.0, 1.0], (chains, d))
    K = int((slices + 2) / grid_dt) + 8

    def run(grid):
        with pkg.Ensemble(chains, d, trace_capacity=int(2.0 * d) + 1024) as e:  # bench.py's capacity for a step of dT = 1
            e.set_flow(pkg.ZigZag(G, np.zeros(d), np.ones(d), λref=lambda_ref) if case == "refresh" else pkg.ZigZag(G, np.zeros(d)))
            e.set_target(pkg.GaussianTarget(G))
            e.set_state(0.0, x0, th0, c, np.uint64(7) + np.arange(chains, dtype=np.uint64))
            (e.refresh_consume_begin if case == "refresh" else e.consume_begin)(*((grid_dt, K) if grid else ()))
            out = timed_slices(pkg, e, 1.0, slices)
            return out + (e.kernel_name(),)

    plain, grid = run(False), run(True)
    return dict(case=case, d=d, chains=chains, lambda_ref=lambda_ref if case == "refresh" else 0.0, kernel=plain[3], events_per_slice=plain[2],
                sampler_ms=plain[0], consume_ms=plain[1], consume_ms_with_grid=grid[1], grid_dt=grid_dt,
                ns_per_event=1e6 * plain[1] / max(plain[2], 1), consume_clock="host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["refresh", "plain", "all"])
    ap.add_argument("--slices", type=int, default=4)
    ap.add_argument("--chains", type=int, default=4096, help="the benchmark's chain count")
    ap.add_argument("--lambda-ref", type=float, default=1.0, help="C3R's refresh rate")
    ap.add_argument("--grid-dt", type=float, default=0.5)
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    for case in (["refresh", "plain"] if a.case == "all" else [a.case]):
        print(json.dumps(lattice(pkg, case, a.chains, a.slices, a.lambda_ref, a.grid_dt)), flush=True)


if __name__ == "__main__":
    main()
