"""The conditional trace on the device (pdmp_ensemble_[bps_]consume_condition) beside the plain consumer, on the same slices.

    python tools/bench_condition.py [--case pair|block|bps|all] [--slices 6] [--chains N]

Cases (DESIGN.md "Conditional trace" records the figures):
    pair    128 x 128 lattice GMRF, d = 16384, 512 chains, n = e_i − e_j (two neighbouring sites)
    block   the same lattice, a 64-entry block of n (a contrast over an 8 x 8 patch)
    bps     BouncyParticle, d = 1024, Γ = I, 1024 chains, dense n
Two ensembles with the same seeds run the same slices; after every slice consume() is timed on the host clock (the call is synchronous: launch,
kernels, wait) with the device idle before it, once without and once with a condition; the trace buffer is recycled after every slice.  max_hits
is sized so that the rows stay under 4 GiB.  Prints ONE JSON line per case: the median ms per consume() of either ensemble, their ratio, the
events per slice and the hits found.
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


def timed_slices(pkg, ens, T_step, slices, consume):
    """run -> consume (timed) -> trace_reset until `slices` slices are done; a slice whose buffer filled is consumed in several calls"""
    L = pkg._lib
    ms, nev = [], []
    for s in range(-1, slices):  # slice −1: warm-up
        tot, ev0 = 0.0, int(ens.counters()["nevents"].sum())
        while True:
            ens.run(T_step * (s + 2), L.RUN_STOP_BEFORE)
            cnt = ens.counters()
            ens.sync()
            t = time.perf_counter()
            consume()
            tot += 1e3 * (time.perf_counter() - t)
            ens.trace_reset()
            if not L.needs_rerun(cnt["status"]):
                break
        assert np.all(cnt["status"] == L.CHAIN_OK), np.unique(cnt["status"])
        if s >= 0:
            ms.append(tot)
            nev.append(int(cnt["nevents"].sum()) - ev0)
    return float(np.median(ms)), int(np.median(nev))


def lattice(pkg, kind, chains, slices):
    m = 128
    d = m * m
    G = pkg.problems.gmrf_precision(m)
    c = pkg.problems.column_norms(G)
    rng = np.random.default_rng(1)
    x0, th0 = pkg.problems.gmrf_stationary_sample(m, chains, rng), rng.choice([-1.0, 1.0], (chains, d))
    p, n = np.zeros(d), np.zeros(d)
    i = 64 * m + 64
    if kind == "pair":
        n[i], n[i + 1] = 1.0, -1.0
    else:  # an 8 x 8 patch against its mean level: Σ w_k x_k = 0 with weights of both signs
        idx = (i + np.arange(8)[:, None] + m * np.arange(8)[None, :]).ravel()
        n[idx] = np.where(np.arange(64) % 2 == 0, 1.0, -1.0)
    max_hits = 32  # 512 x 32 x 16384 doubles = 2 GiB of rows
    out = {}
    for cond in (False, True):
        with pkg.Ensemble(chains, d, trace_capacity=65536) as e:  # 1 GiB of trace: a slice of ~40000 events per chain
            e.set_flow(pkg.ZigZag(G, np.zeros(d)))
            e.set_target(pkg.GaussianTarget(G))
            e.set_state(0.0, x0, th0, c, np.uint64(7) + np.arange(chains, dtype=np.uint64))
            e.consume_begin()
            if cond:
                e.consume_condition(p, n, max_hits)
            out[cond] = timed_slices(pkg, e, 3.0, slices, e.consume)
            nh = [e.consume_conditioned(k, count=0)[2] for k in range(chains)] if cond else None
    return dict(case=kind, d=d, chains=chains, support=int(np.count_nonzero(n)), max_hits=max_hits, events_per_slice=out[True][1],
                ms_plain=out[False][0], ms_condition=out[True][0], ratio=out[True][0] / out[False][0], hits_per_chain=float(np.mean(nh)))


def bps(pkg, chains, slices):
    d = 1024
    I = sp.identity(d, format="csc")
    rng = np.random.default_rng(2)
    x0, th0 = rng.standard_normal((chains, d)), rng.standard_normal((chains, d))
    p, n = np.zeros(d), rng.standard_normal(d)
    max_hits = 128  # 1024 x 128 x 1024 doubles = 1 GiB of rows
    out = {}
    for cond in (False, True):
        with pkg.Ensemble(chains, d, sampler=pkg._lib.SAMPLER_BPS, factor=2.0, trace_capacity=256) as e:  # 4 GiB of trace
            e.set_flow_bps(pkg.BouncyParticle(I, np.zeros(d), 1.0))
            e.set_state_bps(0.0, x0, th0, 1e-3, np.uint64(7) + np.arange(chains, dtype=np.uint64))
            e.bps_consume_begin()
            if cond:
                e.bps_consume_condition(p, n, max_hits)
            out[cond] = timed_slices(pkg, e, 16.0, slices, e.bps_consume)
            nh = [e.bps_consume_conditioned(k, count=0)[2] for k in range(chains)] if cond else None
    return dict(case="bps", d=d, chains=chains, support=d, max_hits=max_hits, events_per_slice=out[True][1], ms_plain=out[False][0],
                ms_condition=out[True][0], ratio=out[True][0] / out[False][0], hits_per_chain=float(np.mean(nh)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["pair", "block", "bps", "all"])
    ap.add_argument("--slices", type=int, default=6)
    ap.add_argument("--chains", type=int, default=0, help="0: 512 on the lattice, 1024 for the Bouncy Particle")
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    for case in (("pair", "block", "bps") if a.case == "all" else (a.case,)):
        r = bps(pkg, a.chains or 1024, a.slices) if case == "bps" else lattice(pkg, case, a.chains or 512, a.slices)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
