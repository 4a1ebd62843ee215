"""zz_precision_run_kernel (the Cholesky factor of a precision matrix under the sticky ZigZag, csrc/pdmp_precision.inc) at a named ensemble
width and T, beside its sequential restatement (tests/ref/precision_ref.c) on one host thread.

    python tools/bench_precision.py [--n 60] [--N 1000] [--chains 1024] [--T 2] [--reps 3] [--host-T 2]

The case study's problem (casestudies/precision/precision.jl: Γtrue = SymTridiagonal(1, −0.3), c = 10, κ = 0.01, adapt) with the flow of
problems.precision_cholesky_problem, no trace.  A warm-up run, then `reps` timed runs from a fresh state; the fastest is reported.  The host
figure is one chain of the restatement run to --host-T.  Prints ONE JSON line: events/s, draws/s and ms per unit of PDMP time, for the
device (all chains together) and for the host.  (acc and num restart at every adaptation of c, as in the reference: the proposals counted are
those since the last one: the draws of PDMP_STREAM_MAIN past the setup, two per proposal and one per freeze or thaw, are counted instead.)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__  # noqa: E402
import precision_ref_lib as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60)
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--T", type=float, default=2.0, help="the PDMP clock every chain runs to")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-T", type=float, default=2.0)
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    Lb = pkg._lib
    P = pkg.problems.precision_cholesky_problem(a.n, a.N, 5, nchains=a.chains)
    d = P["d"]
    seeds = np.uint64(100) + np.arange(a.chains, dtype=np.uint64)
    best = None
    with pkg.Ensemble(a.chains, d, sampler=Lb.SAMPLER_STICKY_ZIGZAG, adapt=True, factor=1.5, trace_capacity=0) as e:
        e.set_flow(pkg.ZigZag(P["Γ̂"], P["μ̂"]))
        e.set_target(pkg.PrecisionCholeskyTarget(P["YY"], P["N"], P["γ0"]))
        e.set_sticky(P["κ"])
        for rep in range(-1, a.reps):  # rep -1: warm-up
            e.set_state(0.0, P["x0"], P["θ0"], P["c"], seeds)
            ms = 0.0
            while True:
                e.run(a.T)
                ms += e.last_run_ms()
                cnt = e.counters()
                if not Lb.needs_rerun(cnt["status"]):
                    break
            assert np.all(cnt["status"] == Lb.CHAIN_OK), np.unique(cnt["status"])
            if rep >= 0 and (best is None or ms < best[0]):
                best = (ms, int(cnt["nevents"].sum()), int((cnt["ndraw_main"] - d).sum()))
        kernel = e.kernel_name()
    ms, nev, ndraw = best
    R.load()  # (compiled before the clock starts)
    t = time.perf_counter()
    r = R.precision(P["YY"], P["N"], P["x0"][0], P["θ0"][0], a.host_T, P["c"], P["γ̂"], P["μ̂"], P["κ"], gamma0=P["γ0"], adapt=True, factor=1.5,
                    seed=int(seeds[0]), ev_cap=1 << 22)
    hs = time.perf_counter() - t
    print(json.dumps(dict(kernel=kernel, n=a.n, d=d, N=a.N, chains=a.chains, T=a.T, ms_per_run=ms, events=nev, draws=ndraw,
                          events_per_s=nev / (ms * 1e-3), draws_per_s=ndraw / (ms * 1e-3), ms_per_unit_time=ms / a.T,
                          ms_per_unit_time_per_chain=ms / a.T / a.chains,
                          host=dict(chains=1, T=a.host_T, events=r["nevents"], draws=r["ndraw_main"] - d, events_per_s=r["nevents"] / hs,
                                    draws_per_s=(r["ndraw_main"] - d) / hs, ms_per_unit_time=1e3 * hs / a.host_T))), flush=True)


if __name__ == "__main__":
    main()
