"""The marginal histograms on the device (pdmp_ensemble_[bps_]consume_hist) beside the sampler and the plain consumer, on the same slices.

    python tools/bench_hist.py [--case c3|c2|all] [--slices 4] [--chains 4096] [--shapes 64x64,1024x64,1024x256] [--no-hist]

Cases (DESIGN.md "Marginal histograms" records the figures):
    c3    C3's geometry: 128 x 128 lattice GMRF, d = 16384, tracked sampler, steps of dT = 1; m coordinates spread evenly over the lattice,
          B bins on [−4 sd, 4 sd] of the stationary marginal
    c2    C2's geometry: BouncyParticle, d = 1024, Γ = I, steps of dT = 30; the first m coordinates, B bins on [−4, 4]
For every shape (m, B) two ensembles with the same seeds run the same slices, one without and one with hist.  Per slice: the sampler's ms from
the device events of the run (pdmp_ensemble_last_run_ms); consume() of either ensemble -- the Bouncy Particle family's from the device events
around its kernels (pdmp_ensemble_last_consume_ms), the factorised family's synchronous consume() on the host clock with the device idle
before it (it keeps no device timing) --; the histogram consumer's ms is their difference, `ratio` the consumer with hist over the consumer
without.  The trace buffer is recycled after every slice.  Prints ONE JSON line per case and shape with the medians over the slices.
--no-hist measures the plain consumer alone (one line per case): what a commit without the histogram consumer can run, for the same figure there.
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


def report(case, d, chains, shape, plain, both, clock):
    out = dict(case=case, d=d, chains=chains, events_per_slice=plain[2], sampler_ms=plain[0], consume_ms_plain=plain[1], consume_clock=clock)
    if both is not None:
        hist_ms = both[1] - plain[1]
        out.update(m=shape[0], bins=shape[1], consume_ms_with_hist=both[1], hist_ms=hist_ms, ratio=both[1] / plain[1],
                   accumulator_MiB=chains * shape[0] * (shape[1] + 2) * 8 / 2.0**20)
    return out


def lattice(pkg, chains, slices, shapes):
    m_side = 128
    d = m_side * m_side
    G = pkg.problems.gmrf_precision(m_side)
    c = pkg.problems.column_norms(G)
    rng = np.random.default_rng(1)
    x0, th0 = pkg.problems.gmrf_stationary_sample(m_side, chains, rng), rng.choice([-1.0, 1.0], (chains, d))
    sd = float(np.std(x0))

    def run(shape):
        with pkg.Ensemble(chains, d, trace_capacity=20480) as e:  # a step of dT = 1 is ~13 000 events per chain
            e.set_flow(pkg.ZigZag(G, np.zeros(d)))
            e.set_target(pkg.GaussianTarget(G))
            e.set_gradient_tracking(True)
            e.set_state(0.0, x0, th0, c, np.uint64(7) + np.arange(chains, dtype=np.uint64))
            e.consume_begin()
            if shape is not None:
                e.consume_hist(np.arange(shape[0], dtype=np.int64) * (d // shape[0]), -4.0 * sd, 4.0 * sd, shape[1])
            return timed_slices(pkg, e, 1.0, slices, e.consume, False)

    plain = run(None)
    if shapes is None:
        return [report("c3", d, chains, None, plain, None, "host")]
    return [report("c3", d, chains, s, plain, run(s), "host") for s in shapes]


def bps(pkg, chains, slices, shapes):
    d = 1024
    I = sp.identity(d, format="csc")
    rng = np.random.default_rng(2)
    x0, th0 = rng.standard_normal((chains, d)), rng.standard_normal((chains, d))

    def run(shape):
        with pkg.Ensemble(chains, d, sampler=pkg._lib.SAMPLER_BPS, factor=2.0, trace_capacity=512) as e:  # a step of dT = 30 is ~410 events
            e.set_flow_bps(pkg.BouncyParticle(I, np.zeros(d), 1.0))
            e.set_state_bps(0.0, x0, th0, 1e-3, np.uint64(7) + np.arange(chains, dtype=np.uint64))
            e.bps_consume_begin()
            if shape is not None:
                e.bps_consume_hist(np.arange(shape[0], dtype=np.int64), -4.0, 4.0, shape[1])
            return timed_slices(pkg, e, 30.0, slices, e.bps_consume, True)

    plain = run(None)
    if shapes is None:
        return [report("c2", d, chains, None, plain, None, "device events")]
    return [report("c2", d, chains, s, plain, run(s), "device events") for s in shapes if s[0] <= d]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["c3", "c2", "all"])
    ap.add_argument("--slices", type=int, default=4)
    ap.add_argument("--chains", type=int, default=4096, help="the benchmark's chain count")
    ap.add_argument("--shapes", default="64x64,1024x64,1024x256", help="m x bins, comma-separated")
    ap.add_argument("--no-hist", action="store_true", help="the plain consumer alone")
    a = ap.parse_args()
    shapes = None if a.no_hist else [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    pkg = __graft_entry__.load_package()
    for case in (["c3", "c2"] if a.case == "all" else [a.case]):
        for r in (lattice if case == "c3" else bps)(pkg, a.chains, a.slices, shapes):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
