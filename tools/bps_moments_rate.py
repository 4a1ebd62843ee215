"""Config C2 with and without event records, with and without the device path moments (pdmp_ensemble_set_bps_moments).

    python tools/bps_moments_rate.py [--steps 10] [--warmup 3] [--modes abcde]

One process, the C2 shape of bench.py --config C2: 4096 chains, d = 1024, BouncyParticle(I, 0, 1), c = 1e-3, steps of dT = 30
(run PDMP_RUN_STOP_BEFORE to (k+1)·30, re-run on TRACE_FULL).  Modes:
    a  events as bench.py writes them (trace capacity 512), no moments
    b  no events (capacity 0), no moments      -- the event loop without its writes
    c  no events, order 1 (∫x dt)
    d  no events, order 2 (∫x dt, ∫x² dt)
    e  events (capacity 512) and order 2
Prints one JSON line per mode: kernel ms per step (sum of last_run_ms over the step's launches), events/s, and for order >= 1 the ESS of the
coordinates' time averages from pdmp_ensemble_ess_* (batches of one step after the warm-up, Var_π = 1): per chain and second of kernel time
(median and minimum over coordinates) and per chain and unit of process time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402

MODES = {"a": (512, 0), "b": (0, 0), "c": (0, 1), "d": (0, 2), "e": (512, 2)}


def run_mode(pkg, mode, args):
    L = pkg._lib
    cap, order = MODES[mode]
    nch, d, dt = args.chains, 1024, 30.0
    rng = np.random.default_rng(1000)
    t_setup = time.time()
    ens = pkg.Ensemble(nch, d, sampler=L.SAMPLER_BPS, factor=2.0, trace_capacity=cap)
    try:
        ens.set_flow_bps(pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0))
        if order:
            ens.set_bps_moments(order)
        ens.set_state_bps(0.0, rng.standard_normal((nch, d)), rng.standard_normal((nch, d)), 1e-3,
                          np.arange(nch, dtype=np.uint64) + np.uint64(0x5EED0000))
        t_setup = time.time() - t_setup
        ms, launches = [], 0
        c0 = None
        for k in range(args.warmup + args.steps):
            T = (k + 1) * dt
            m = 0.0
            while True:
                ens.run(T, L.RUN_STOP_BEFORE)
                m += ens.last_run_ms()
                launches += 1
                st = ens.counters()["status"]
                if cap:
                    ens.trace_reset()
                if not L.needs_rerun(st):
                    break
            ms.append(m)
            if order and k == args.warmup - 1:
                ens.ess_begin(T)  # burn-in: the warm-up steps
                c0 = ens.counters()
            elif order and k >= args.warmup:
                ens.ess_batch(T)
            if not order and k == args.warmup - 1:
                c0 = ens.counters()
        c1 = ens.counters()
        out = dict(mode=mode, trace_capacity=cap, order=order, chains=nch, d=d, dT=dt, steps=args.steps, warmup=args.warmup,
                   kernel=ens.kernel_name(), setup_s=round(t_setup, 2))
        secs = float(np.sum(ms[args.warmup:])) * 1e-3
        nev = int(c1["nevents"].sum()) - int(c0["nevents"].sum())
        out.update(ms_per_step=1e3 * secs / args.steps, launches=launches, events_per_s=nev / secs,
                   events_per_chain_per_step=nev / nch / args.steps)
        if order:
            sy, sy2, sm, sm2, nb, T0, T1 = ens.ess_end()
            r = pkg.ess.batch_means_ess(sy, sy2, sm, sm2, nch, nb, dt, np.ones(d))
            ess_chain = r["ess"] / nch  # effective samples per chain over the timed run
            out.update(ess_per_chain_per_s_median=float(np.median(ess_chain) / secs), ess_per_chain_per_s_min=float(ess_chain.min() / secs),
                       ess_per_chain_per_time_median=float(np.median(r["ess_per_time"])), batches=int(nb), T0=T0, T1=T1,
                       mean_abs_max=float(np.abs(r["mean"]).max()))
        return out
    finally:
        ens.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--modes", default="abcde")
    args = ap.parse_args()
    if args.warmup < 1 or args.steps < 2:
        ap.error("need --warmup >= 1 (the ESS burn-in) and --steps >= 2 (batches)")
    pkg = __graft_entry__.load_package()  # (the library built beforehand: __graft_entry__.build())
    pkg._lib.load()
    for mode in args.modes:
        print(json.dumps(run_mode(pkg, mode, args)), flush=True)


if __name__ == "__main__":
    main()
