"""The marginal histograms of arcs on the device (pdmp_ensemble_bps_consume_arc_hist) beside the sampler and the plain consumer, on the same
slices: tools/bench_hist.py's c2 shapes on a Boomerang.

    python tools/bench_arc_hist.py [--slices 4] [--chains 4096] [--shapes 64x64,1024x64,1024x256] [--no-hist]

C2's geometry on a Boomerang, as tools/bench_arc_pairs.py sets it up: d = 1024, Γ = I, μ = 0, λref = 1, target 1.2 I, steps of dT = 30; the first
m coordinates, B bins on [−4, 4] (DESIGN.md "Marginal histograms of arcs" records the figures, beside bench_hist.py's c2 rows of the same
session).  For every shape (m, B) two ensembles with the same seeds run the same slices, one without and one with the list.  Per slice: the
sampler's ms from the device events of the run (pdmp_ensemble_last_run_ms) and bps_consume()'s from the device events around its kernels
(pdmp_ensemble_last_consume_ms); the arc walker's ms is the difference of the two ensembles' consume(), `ratio` the consumer with the list over
the consumer without.  The trace buffer is recycled after every slice.  Prints ONE JSON line per shape with the medians over the slices after
a warm-up slice, and the library it ran (PDMP_MI355_LIB selects an experimental build, as tools/ab.sh does).  --no-hist measures the plain
consumer alone.
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
    return float(np.median(run_ms)), float(np.median(ms)), int(np.median(nev)), float(min(ms)), float(max(ms))


def boomerang(pkg, chains, slices, shapes):
    d = 1024
    I = sp.identity(d, format="csc")
    rng = np.random.default_rng(2)
    x0, th0 = rng.standard_normal((chains, d)), rng.standard_normal((chains, d))
    lib = os.path.basename(pkg._lib.loaded_path())

    def run(shape):
        with pkg.Ensemble(chains, d, sampler=pkg._lib.SAMPLER_BPS, adapt=True, factor=2.0, trace_capacity=512) as e:
            e.set_flow_boomerang(pkg.GaussianTarget(sp.csc_matrix(1.2 * I), np.zeros(d)), pkg.Boomerang(I, np.zeros(d), 1.0))
            e.set_state_bps(0.0, x0, th0, 3.0, np.uint64(7) + np.arange(chains, dtype=np.uint64))
            e.bps_consume_begin()
            if shape is not None:
                e.bps_consume_arc_hist(np.arange(shape[0], dtype=np.int64), -4.0, 4.0, shape[1])
            return timed_slices(pkg, e, 30.0, slices)

    plain = run(None)
    base = dict(case="c2", flow="Boomerang", d=d, chains=chains, events_per_slice=plain[2], sampler_ms=plain[0], consume_ms_plain=plain[1],
                consume_ms_plain_min=plain[3], consume_ms_plain_max=plain[4], consume_clock="device events", lib=lib)
    if shapes is None:
        return [base]
    out = []
    for m, bins in shapes:
        if m > d:
            continue
        both = run((m, bins))
        hist_ms = both[1] - plain[1]
        out.append(dict(base, m=m, bins=bins, consume_ms_with_hist=both[1], arc_hist_ms=hist_ms, ratio=both[1] / plain[1],
                        ns_per_piece=1e6 * hist_ms / (both[2] * m) if hist_ms > 0 else None,
                        accumulator_MiB=chains * m * (bins + 2) * 8 / 2.0**20))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=4)
    ap.add_argument("--chains", type=int, default=4096, help="the benchmark's chain count")
    ap.add_argument("--shapes", default="64x64,1024x64,1024x256", help="m x bins, comma-separated")
    ap.add_argument("--no-hist", action="store_true", help="the plain consumer alone")
    a = ap.parse_args()
    shapes = None if a.no_hist else [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    pkg = __graft_entry__.load_package()
    pkg._lib.load()
    for r in boomerang(pkg, a.chains, a.slices, shapes):
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
