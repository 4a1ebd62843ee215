"""zz_bridge_run_kernel (the diffusion bridge, csrc/pdmp_bridge.inc) at a named ensemble width and T′, beside its sequential restatement
(tests/ref/bridge_ref.c) on one host thread.

    python tools/bench_bridge.py [--L 7] [--chains 256] [--T 20] [--reps 3] [--host-T 20]

The script's problem (research/diffusion_bridge/diffbridge.jl): T = 2, u = 1.5, v = −0.5, α = 1.5, β = 0.1, ω = 2π, adapt from c = 1, no trace.
A warm-up run, then `reps` timed runs from a fresh state; the fastest is reported.  The host figure is one chain of the restatement run to
--host-T.  Prints ONE JSON line: events/s, proposals/s and ms per unit of PDMP time, for the device (all chains together) and for the host.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__  # noqa: E402
import bridge_ref_lib as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=7)
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--T", type=float, default=20.0, help="T′, the PDMP clock every chain runs to")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-T", type=float, default=20.0)
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    Lb = pkg._lib
    Tb, drift = 2.0, dict(alpha=1.5, beta=0.1, omega=2 * np.pi)
    d = (2 << a.L) + 1
    x0, th0, c = pkg.problems.diffusion_bridge_problem(a.L, Tb, 1.5, -0.5, nchains=a.chains, rng=np.random.default_rng(1))
    seeds = np.uint64(100) + np.arange(a.chains, dtype=np.uint64)
    best = None
    with pkg.Ensemble(a.chains, d, adapt=True, trace_capacity=0) as e:
        e.set_flow(pkg.ZigZag(sp.identity(d, format="csc"), np.zeros(d)))
        e.set_target(pkg.DiffusionBridgeTarget(a.L, Tb, drift["alpha"], drift["beta"], drift["omega"]))
        for rep in range(-1, a.reps):  # rep -1: warm-up
            e.set_state(0.0, x0, th0, c, seeds)
            ms = 0.0
            while True:
                e.run(a.T)
                ms += e.last_run_ms()
                cnt = e.counters()
                if not Lb.needs_rerun(cnt["status"]):
                    break
            assert np.all(cnt["status"] == Lb.CHAIN_OK), np.unique(cnt["status"])
            if rep >= 0 and (best is None or ms < best[0]):
                best = (ms, int(cnt["nevents"].sum()), int(cnt["num"].sum()))
        kernel = e.kernel_name()
    ms, nev, num = best
    R.load()  # (compiled before the clock starts)
    t = time.perf_counter()
    r = R.bridge(x0[0], th0[0], a.host_T, c, L=a.L, T=Tb, adapt=True, seed=int(seeds[0]), ev_cap=1 << 22, **drift)
    hs = time.perf_counter() - t
    print(json.dumps(dict(kernel=kernel, L=a.L, d=d, chains=a.chains, T_prime=a.T, ms_per_run=ms, events=nev, proposals=num,
                          events_per_s=nev / (ms * 1e-3), proposals_per_s=num / (ms * 1e-3), ms_per_unit_time=ms / a.T,
                          ms_per_unit_time_per_chain=ms / a.T / a.chains,
                          host=dict(chains=1, T_prime=a.host_T, events=r["nevents"], proposals=r["num"], events_per_s=r["nevents"] / hs,
                                    proposals_per_s=r["num"] / hs, ms_per_unit_time=1e3 * hs / a.host_T))), flush=True)


if __name__ == "__main__":
    main()
