"""zz_barrier_run_kernel (stickyzz, csrc/pdmp_barrier.hip) beside zz_sticky_run_kernel (sspdmp with the one-event kernel) in one process.

    python tools/stickyzz_rate.py [--n 128] [--chains 1024] [--T 5] [--reps 3]

Problem for both: Γ = problems.gmrf_precision(n) (d = n²), flow and target the same Γ, c = column norms, κ = 1, x0 ~ N(0, 1), θ0 = ±1, no trace.
    s  sspdmp, kernel forced to the sequential one (PDMP_DEBUG_KERNEL_SEQ)
    b  stickyzz with barriers (0, 0), :sticky, κ = 1 on every coordinate (sspdmp2's barriers)
The two sample different arithmetic (stickyzz draws its proposals with the 0.01 floor), so ms per event is printed beside ms per run.  A warm-up
run of each, then `reps` runs of each in turn (a fresh state every run).  Prints one JSON line per run.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--T", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    L = pkg._lib
    G = pkg.problems.gmrf_precision(a.n)
    d = G.shape[0]
    rng = np.random.default_rng(1)
    x0 = rng.standard_normal((a.chains, d))
    th0 = rng.choice([-1.0, 1.0], size=(a.chains, d))
    c = pkg.problems.column_norms(G)
    seeds = np.uint64(100) + np.arange(a.chains, dtype=np.uint64)
    Z, tgt = pkg.ZigZag(G, np.zeros(d)), pkg.GaussianTarget(G, None)
    kap = np.ones(d)

    def make(mode):
        e = pkg.Ensemble(a.chains, d, sampler=L.SAMPLER_STICKY_ZIGZAG if mode == "s" else L.SAMPLER_BARRIER_ZIGZAG, factor=1.5, trace_capacity=0)
        if mode == "s":
            e.debug_set_kernel("seq")
        e.set_flow(Z)
        e.set_target(tgt)
        if mode == "s":
            e.set_sticky(kap)
        else:
            e.set_barriers(np.zeros(d), np.zeros(d), np.zeros(d, np.int32), np.zeros(d, np.int32), kap, kap)
        return e

    ens = {m: make(m) for m in "sb"}
    try:
        for rep in range(-1, a.reps):  # rep -1: warm-up
            for m in "sb":
                e = ens[m]
                e.set_state(0.0, x0, th0, c, seeds)
                ms = 0.0
                while True:
                    e.run(a.T)
                    ms += e.last_run_ms()
                    cnt = e.counters()
                    if not L.needs_rerun(cnt["status"]):
                        break
                assert np.all(cnt["status"] == L.CHAIN_OK), np.unique(cnt["status"])
                nev, num = int(cnt["nevents"].sum()), int(cnt["num"].sum())
                print(json.dumps(dict(mode=m, kernel=e.kernel_name(), rep=rep, d=d, chains=a.chains, T=a.T, ms_per_run=ms, events=nev, proposals=num,
                                      us_per_event_per_chain=1e3 * ms * a.chains / nev, ms_per_million_events=1e6 * ms / nev)), flush=True)
    finally:
        for e in ens.values():
            e.close()


if __name__ == "__main__":
    main()
