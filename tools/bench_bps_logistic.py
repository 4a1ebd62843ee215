"""The speed-recorded Bouncy Particle on the logistic-regression target (csrc/pdmp_bps_logit.inc): one ensemble of 4096 chains on two problems,
beside the C restatement (tests/ref/bps_logistic_ref.c) on 16 host threads.  Reported, not a gate: bench.py has no such configuration.

    python tools/bench_bps_logistic.py [--steps 5] [--warmup 2] [--chains 4096] [--problems ds] [--cpu-chains 16]

Problems:
    d  dense, n = 1000, d = 25 (the shape of turing/lr.jl): A ~ N(0, 1), y ~ Bernoulli(sigmoid(A β)), γ0 = 1, steps of dT = 50
    s  sparse, n = 8840, d = 442: the design of config C4 (problems.logistic_problem), γ0 = 0.01, x0 at the mode, steps of dT = 10
λref = 1, ρ = 0.9, L = I, LocalBound(c) with adapt (factor 2) from c = 10, θ0 ~ N(0, I), trace capacity 64 records per chain and launch, run
PDMP_RUN_STOP_BEFORE to (k+1)·dT, drained and re-run while a chain asks for it.  Timing: warm-up steps first, then every step timed by the
ensemble's device events (last_run_ms summed over the step's launches); the median step gives the figures.
Prints one JSON line per problem for the device -- records/s, proposals/s, kernel ms per unit of process time (the whole ensemble) -- and one
for the build's CPU restatement: --cpu-chains chains of the same problem over the same span on 16 threads, wall clock.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__  # noqa: E402

CPU_THREADS = 16


def make_problem(pkg, which, nch):
    rng = np.random.default_rng(4242)
    if which == "d":
        n, d = 1000, 25
        A = rng.standard_normal((n, d))
        beta = rng.standard_normal(d)
        y = (rng.random(n) < 1.0 / (1.0 + np.exp(-A @ beta))).astype(np.float64)
        return dict(name="dense n=1000 d=25", A=A, y=y, gamma0=1.0, dT=50.0, x0=np.zeros((nch, d)), th0=rng.standard_normal((nch, d)))
    P = pkg.problems.logistic_problem()
    d = P["p"]
    return dict(name="sparse n=%d d=%d (C4)" % (P["n"], d), A=P["A"], y=P["y"], gamma0=P["gamma0"], dT=10.0, x0=np.tile(P["x0"], (nch, 1)),
                th0=rng.standard_normal((nch, d)))


def run_device(pkg, P, args):
    L = pkg._lib
    nch, d = P["x0"].shape
    seeds = np.arange(nch, dtype=np.uint64) + np.uint64(0x5EED0000)
    with pkg.Ensemble(nch, d, sampler=L.SAMPLER_BPS, adapt=True, factor=2.0, trace_capacity=64) as ens:
        ens.set_flow_bps_modern(1.0, 0.9, None, False)
        ens.set_target(pkg.LogisticRegressionTarget(P["A"], P["y"], None, P["gamma0"]))
        ens.set_state_bps(0.0, P["x0"], P["th0"], 10.0, seeds)
        ms, recs, props, launches = [], [], [], 0
        prev = ens.counters()
        for k in range(args.warmup + args.steps):
            m = 0.0
            while True:
                ens.run((k + 1) * P["dT"], L.RUN_STOP_BEFORE)
                m += ens.last_run_ms()
                launches += 1
                st = ens.counters()["status"]
                if np.any(st == L.CHAIN_BOUND_VIOLATED) or np.any(st == L.CHAIN_STALLED):
                    raise RuntimeError("a chain ended as BOUND_VIOLATED or STALLED")
                ens.trace_reset()
                if not L.needs_rerun(st):
                    break
            cur = ens.counters()
            ms.append(m)
            recs.append(int(cur["nevents"].sum()) - int(prev["nevents"].sum()))
            props.append(int(cur["num"].sum()) - int(prev["num"].sum()))
            prev = cur
        w = args.warmup
        k = w + int(np.argsort(ms[w:])[len(ms[w:]) // 2])  # the median step
        secs = ms[k] * 1e-3
        return dict(what="device", problem=P["name"], chains=nch, kernel=ens.kernel_name(), dT=P["dT"], steps=args.steps, warmup=w, launches=launches,
                    records_per_s=recs[k] / secs, proposals_per_s=props[k] / secs, ms_per_unit_time=ms[k] / P["dT"],
                    proposals_per_chain_per_unit_time=props[k] / nch / P["dT"], c_max=float(ens.bps_final_state()["c"].max()),
                    step_ms=[round(v, 3) for v in ms[w:]])


def run_cpu(P, args):
    import bps_logistic_ref_lib as B
    B.load()
    nch = args.cpu_chains
    span = (args.warmup + args.steps) * P["dT"]

    def one(k):
        return B.pdmp(0.0, P["x0"][k], P["th0"][k], float(span), 10.0, A=P["A"], y=P["y"], gamma0=P["gamma0"], lambda_ref=1.0, rho=0.9, adapt=True,
                      factor=2.0, seed=0x5EED0000 + k, ev_cap=1)

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=CPU_THREADS) as pool:
        res = list(pool.map(one, range(nch)))
    secs = time.perf_counter() - t0
    nrec, nprop = sum(r["nevents"] for r in res), sum(r["num"] for r in res)
    return dict(what="the build's CPU restatement, %d threads" % CPU_THREADS, problem=P["name"], chains=nch, span=span, records_per_s=nrec / secs,
                proposals_per_s=nprop / secs, ms_per_unit_time=1e3 * secs / span, proposals_per_chain_per_unit_time=nprop / nch / span)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--cpu-chains", type=int, default=16)
    ap.add_argument("--problems", default="ds")
    ap.add_argument("--no-device", action="store_true", help="the CPU restatement's figures only")
    args = ap.parse_args()
    if args.warmup < 1 or args.steps < 1:
        ap.error("need --warmup >= 1 and --steps >= 1")
    pkg = __graft_entry__.load_package()  # (the library built beforehand: __graft_entry__.build())
    for which in args.problems:
        P = make_problem(pkg, which, max(args.chains, args.cpu_chains))
        if not args.no_device:
            pkg._lib.load()
            Pd = dict(P, x0=P["x0"][:args.chains], th0=P["th0"][:args.chains])
            print(json.dumps(run_device(pkg, Pd, args)), flush=True)
        print(json.dumps(run_cpu(P, args)), flush=True)


if __name__ == "__main__":
    main()
