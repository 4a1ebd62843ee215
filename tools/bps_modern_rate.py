"""The speed-recorded Bouncy Particle (csrc/pdmp_bps_modern.inc) on the shape of config C2, beside the plain Bouncy Particle of
bench.py --config C2, in one process.

    python tools/bps_modern_rate.py [--steps 10] [--warmup 4] [--modes pm]

4096 chains, d = 1024, identity target, λref = 1, x0, θ0 ~ N(0, I), trace capacity 512 records per chain and launch (run
PDMP_RUN_STOP_BEFORE to (k+1)·dT, drained and re-run on TRACE_FULL), steps of dT = 30.  Modes:
    p  plain pdmp, BouncyParticle(I, 0, 1), GlobalBound(1e-3): one record per event (about 410 per chain and step: bench.py's C2)
    m  the speed-recorded pdmp, BouncyParticle(missing, missing, 1, 0.9, missing, I), LocalBound(c): one record per unit of time (V ≡ 1)
c is chosen on the CPU with the restatement (tests/ref/modern_bps_ref.c): the smallest of 1e-3, 1e-2, 1e-1, 1 for which four chains run
the whole span without a violated bound.
Prints one JSON line per mode: kernel ms per step (sum of last_run_ms over the step's launches), records, proposals and bytes written per
second (8(2d+1) per record), and per chain and unit of process time.
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__  # noqa: E402

DT = 30.0


def choose_c(d, x0, th0, seeds, T):
    import modern_bps_ref_lib as M
    I = sp.identity(d, format="csc")
    for c in (1e-3, 1e-2, 1e-1, 1.0):
        ok = True
        for k in range(4):
            r = M.pdmp(0.0, x0[k], th0[k], float(T), c, gamma=I, lambda_ref=1.0, rho=0.9, seed=int(seeds[k]), adapt=True, ev_cap=1)
            ok = ok and r["status"] == M.REF_OK and r["nviol"] == 0
        if ok:
            return c
    raise RuntimeError("no c without a violated bound")


def run_mode(pkg, mode, args):
    L = pkg._lib
    nch, d, cap = args.chains, 1024, 512
    rng = np.random.default_rng(1000)
    x0, th0 = rng.standard_normal((nch, d)), rng.standard_normal((nch, d))
    seeds = np.arange(nch, dtype=np.uint64) + np.uint64(0x5EED0000)
    ens = pkg.Ensemble(nch, d, sampler=L.SAMPLER_BPS, factor=2.0, trace_capacity=cap)
    try:
        if mode == "p":
            c = 1e-3
            ens.set_flow_bps(pkg.BouncyParticle(sp.identity(d, format="csc"), np.zeros(d), 1.0))
        else:
            c = choose_c(d, x0, th0, seeds, min((args.warmup + args.steps) * DT, 120.0))
            ens.set_flow_bps_modern(1.0, 0.9, None, False)
            ens.set_target(pkg.GaussianTarget(sp.identity(d, format="csc")))
        ens.set_state_bps(0.0, x0, th0, c, seeds)
        ms, launches, c0 = [], 0, None
        for k in range(args.warmup + args.steps):
            m = 0.0
            while True:
                ens.run((k + 1) * DT, L.RUN_STOP_BEFORE)
                m += ens.last_run_ms()
                launches += 1
                st = ens.counters()["status"]
                if np.any(st == L.CHAIN_BOUND_VIOLATED) or np.any(st == L.CHAIN_STALLED):
                    raise RuntimeError("a chain ended as BOUND_VIOLATED or STALLED")
                ens.trace_reset()
                if not L.needs_rerun(st):
                    break
            ms.append(m)
            if k == args.warmup - 1:
                c0 = ens.counters()
        c1 = ens.counters()
        secs = float(np.sum(ms[args.warmup:])) * 1e-3
        nrec = int(c1["nevents"].sum()) - int(c0["nevents"].sum())
        nprop = int(c1["num"].sum()) - int(c0["num"].sum())
        nacc = int(c1["nacc"].sum()) - int(c0["nacc"].sum())
        span = args.steps * DT
        return dict(mode=mode, c=c, chains=nch, d=d, dT=DT, steps=args.steps, warmup=args.warmup, kernel=ens.kernel_name(),
                    ms_per_step=1e3 * secs / args.steps, ms_per_unit_time=1e3 * secs / span, launches=launches,
                    records_per_s=nrec / secs, proposals_per_s=nprop / secs, written_GB_per_s=8 * (2 * d + 1) * nrec / secs / 1e9,
                    records_per_chain_per_unit_time=nrec / nch / span, proposals_per_chain_per_unit_time=nprop / nch / span,
                    accepted_fraction=nacc / max(nprop, 1), step_ms=[round(v, 3) for v in ms[args.warmup:]])
    finally:
        ens.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--modes", default="pm")
    args = ap.parse_args()
    if args.warmup < 1 or args.steps < 1:
        ap.error("need --warmup >= 1 and --steps >= 1")
    pkg = __graft_entry__.load_package()  # (the library built beforehand: __graft_entry__.build())
    pkg._lib.load()
    for mode in args.modes:
        print(json.dumps(run_mode(pkg, mode, args)), flush=True)


if __name__ == "__main__":
    main()
