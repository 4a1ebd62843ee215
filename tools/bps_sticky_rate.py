"""The sticky Bouncy Particle (csrc/pdmp_bps_sticky.inc) on the shape of config C2, beside the plain Bouncy Particle of bench.py --config C2.

    python tools/bps_sticky_rate.py [--steps 10] [--warmup 4] [--modes ps]

One process, 4096 chains, d = 1024, BouncyParticle(I, 0, 1), c = 1e-3, x0, θ0 ~ N(0, I), trace capacity 512 events per chain and launch
(run PDMP_RUN_STOP_BEFORE to (k+1)·dT, drained and re-run on TRACE_FULL).  Modes:
    p  plain pdmp, steps of dT = 30 (about 410 events per chain and step: bench.py's C2)
    s  sspdmp with κ = 1.5 on every coordinate, steps of dT = 0.5: a coordinate freezes and thaws about once in four units of process time,
       so a chain writes some 35 times as many events per unit of process time as the plain sampler, and a step of 0.5 fills about half of a
       segment
Prints one JSON line per mode: kernel ms per step (sum of last_run_ms over the step's launches), ms per unit of process time, events per
second and per chain and unit of process time, bytes written per second (8(2d+1) per event, + 128 for the sticky mask), and for s the
fraction of free coordinates at the end (κ√(2π)/(1 + κ√(2π)) = 0.790 in equilibrium).
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402

MODES = {"p": (None, 30.0), "s": (1.5, 0.5)}


def run_mode(pkg, mode, args):
    L = pkg._lib
    kappa, dt = MODES[mode]
    nch, d, cap = args.chains, 1024, 512
    rng = np.random.default_rng(1000)
    ens = pkg.Ensemble(nch, d, sampler=L.SAMPLER_BPS, factor=2.0, trace_capacity=cap)
    try:
        ens.set_flow_bps(pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0))
        if kappa is not None:
            ens.set_bps_sticky(kappa)
        ens.set_state_bps(0.0, rng.standard_normal((nch, d)), rng.standard_normal((nch, d)), 1e-3,
                          np.arange(nch, dtype=np.uint64) + np.uint64(0x5EED0000))
        ms, launches, c0 = [], 0, None
        for k in range(args.warmup + args.steps):
            m = 0.0
            while True:
                ens.run((k + 1) * dt, L.RUN_STOP_BEFORE)
                m += ens.last_run_ms()
                launches += 1
                st = ens.counters()["status"]
                if np.any(st == L.CHAIN_BOUND_VIOLATED):
                    raise RuntimeError("a chain ended as PDMP_CHAIN_BOUND_VIOLATED")
                ens.trace_reset()
                if not L.needs_rerun(st):
                    break
            ms.append(m)
            if k == args.warmup - 1:
                c0 = ens.counters()
        c1 = ens.counters()
        secs = float(np.sum(ms[args.warmup:])) * 1e-3
        nev = int(c1["nevents"].sum()) - int(c0["nevents"].sum())
        ev_bytes = 8 * (2 * d + 1) + (128 if kappa is not None else 0)
        out = dict(mode=mode, kappa=kappa, chains=nch, d=d, dT=dt, steps=args.steps, warmup=args.warmup, kernel=ens.kernel_name(),
                   ms_per_step=1e3 * secs / args.steps, ms_per_unit_time=1e3 * secs / (args.steps * dt), launches=launches,
                   events_per_s=nev / secs, events_per_chain_per_unit_time=nev / nch / (args.steps * dt),
                   written_GB_per_s=ev_bytes * nev / secs / 1e9, step_ms=[round(v, 3) for v in ms[args.warmup:]])
        if kappa is not None:
            out["free_fraction_at_end"] = float(ens.bps_final_sticky()["f"].mean())
        return out
    finally:
        ens.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--modes", default="ps")
    args = ap.parse_args()
    if args.warmup < 1 or args.steps < 1:
        ap.error("need --warmup >= 1 and --steps >= 1")
    pkg = __graft_entry__.load_package()  # (the library built beforehand: __graft_entry__.build())
    pkg._lib.load()
    for mode in args.modes:
        print(json.dumps(run_mode(pkg, mode, args)), flush=True)


if __name__ == "__main__":
    main()
