"""The device consumers of a barrier ensemble (pdmp_ensemble_barrier_consume_begin) beside the barrier sampler, on the same slices.

    python tools/bench_barrier_consume.py [--n 128] [--chains 1024] [--slices 4] [--dT 1.0] [--sampler-only]

Problem (that of tools/stickyzz_rate.py): Γ = problems.gmrf_precision(n) (d = n², 16384 by default), flow and target the same Γ, c = column
norms, barriers (0, 0), :sticky, κ = 1 on every coordinate (sspdmp2's), x0 ~ N(0, 1), θ0 = ±1, 1024 chains, the trace written to a buffer of
32768 events per chain (1 GiB) that is recycled after every slice of dT units of process time.
Two ensembles with the same seeds run the same slices in turn: one only recycles the buffer (run -> trace_reset), the other consumes it first
(run -> consume -> trace_reset; mean, a grid of 8 rows and the barrier occupation).  Every slice is timed on the host clock from the launch to
the end of trace_reset with the device idle before it; the sampler's own kernel time (pdmp_ensemble_last_run_ms) is printed beside it.  A warm-up
slice, then `slices` timed ones.  Prints ONE JSON line: the median ms per slice of either ensemble, `ratio` = without / with (the share of
the sampler's rate that is left with the consumers on; DESIGN.md "Barrier occupation" records it), the spread of the slices and the events
per slice.  --sampler-only: the first ensemble alone, through calls that older builds of the library have too -- for an interleaved comparison
of the sampler between two builds (PDMP_MI355_LIB, tools/ab.sh).
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


def timed_slices(pkg, ens, dT, slices, consume):
    L = pkg._lib
    ms, kern, nev = [], [], []
    for s in range(-1, slices):  # slice −1: warm-up
        ev0 = int(ens.counters()["nevents"].sum())
        ens.sync()
        t = time.perf_counter()
        k = 0.0
        while True:
            ens.run(dT * (s + 2), L.RUN_STOP_BEFORE)
            k += ens.last_run_ms()
            cnt = ens.counters()
            if consume:
                ens.consume()
            ens.trace_reset()
            if not L.needs_rerun(cnt["status"]):
                break
        tot = 1e3 * (time.perf_counter() - t)
        assert np.all(cnt["status"] == L.CHAIN_OK), np.unique(cnt["status"])
        if s >= 0:
            ms.append(tot)
            kern.append(k)
            nev.append(int(cnt["nevents"].sum()) - ev0)
    return ms, kern, nev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--slices", type=int, default=4)
    ap.add_argument("--dT", type=float, default=1.0)
    ap.add_argument("--sampler-only", action="store_true")
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
    kap = np.ones(d)
    out = {}
    for consume in ((False,) if a.sampler_only else (False, True)):
        with pkg.Ensemble(a.chains, d, sampler=L.SAMPLER_BARRIER_ZIGZAG, factor=1.5, trace_capacity=32768) as e:
            e.set_flow(pkg.ZigZag(G, np.zeros(d)))
            e.set_target(pkg.GaussianTarget(G, None))
            e.set_barriers(np.zeros(d), np.zeros(d), np.zeros(d, np.int32), np.zeros(d, np.int32), kap, kap)
            e.set_state(0.0, x0, th0, c, seeds)
            if consume:
                e.barrier_consume_begin(a.dT, 8)
            out[consume] = timed_slices(pkg, e, a.dT, a.slices, consume)
            kernel = e.kernel_name()
            if consume:
                zl, zh, nl, nh, T = e.barrier_consume_occupation()
                frozen = float(((zl + zh) / T[:, None]).mean())
    r = dict(kernel=kernel, d=d, chains=a.chains, dT=a.dT, slices=a.slices, events_per_slice=int(np.median(out[False][2])),
             ms_without=float(np.median(out[False][0])), ms_without_all=out[False][0], sampler_kernel_ms=float(np.median(out[False][1])))
    if not a.sampler_only:
        r.update(ms_with=float(np.median(out[True][0])), ms_with_all=out[True][0], ratio=float(np.median(out[False][0]) / np.median(out[True][0])),
                 sampler_kernel_ms_with=float(np.median(out[True][1])), mean_fraction_frozen=frozen)
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
