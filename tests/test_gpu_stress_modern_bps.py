"""Randomised stress of the speed-recorded Bouncy Particle loop (-m gpu; pdmp(dϕ, ∇ϕ!, ..., c::LocalBound, flow::BouncyParticle; oscn),
src/not_fact_samplers.jl:151-384; csrc/pdmp_bps_modern.inc): random dimensions across every slot count (empty trailing slots included), a
target Γ = I, banded or random sparse with a mean, the forms I / U / L / oscn, refresh rates, ρ, t0 ≠ 0, 1 / 2 / 5 chains, adapt and its factor, a
c far too small now and then, T as a record count, an end time or both, the record limit raised in steps, and a trace buffer so small that
most cases resume after PDMP_CHAIN_TRACE_FULL -- records (t, x, θ), every counter, status and the final (t, x, θ, c) bit for bit the
restatement's (tests/ref/modern_bps_ref.c).  No case skips: where the restatement ends as bound-violated (no adapt), the device ends with the
same status, counters and state.  Seeds are fixed; draw_case(case) is the whole draw and needs no device."""
import numpy as np
import pytest

import bps_width_cases as BW
import modern_bps_ref_lib as M
import test_gpu_modern_bps_parity as MP

pytestmark = pytest.mark.gpu

BASE_SEED = 9900
NCASES = 12
DIMS = [1, 3, 17, 64, 65, 129, 200, 257, 300, 513, 1024]


def draw_case(case):
    rng = np.random.default_rng(BASE_SEED + case)
    d = int(rng.choice(DIMS))
    kind = ["I", "banded", "sparse"][int(rng.integers(0, 3))]
    form = ["I", "U", "L", "oscn"][int(rng.integers(0, 4))]
    G = BW.drawn_gamma(rng, d, kind)
    nch = int(rng.choice([1, 2, 5]))
    lam = float(rng.choice([0.3, 1.0, 2.5]))
    D = dict(case=case, d=d, gamma=kind, form=form, lam=lam, rho=float(rng.choice([0.0, 0.4, 0.95])), t0=float(rng.choice([0.0, -1.5, 2.5])),
             nch=nch, adapt=bool(rng.integers(0, 2)), factor=float(rng.choice([1.5, 2.0, 3.0])), cap=int(rng.choice([2, 4, 16])),
             c=float(rng.choice([1e-18, 5.0, 5.0, 20.0, 20.0, 60.0])), mode=["count", "time", "both"][int(rng.integers(0, 3))],
             steps=bool(rng.integers(0, 3) == 0))
    n = int(rng.integers(10, 41))
    T_end = D["t0"] + float(rng.uniform(8.0, 25.0)) / lam  # (one record per 1/λref of speed-time)
    D["n"] = n if D["mode"] != "time" else 0
    D["T_end"] = T_end if D["mode"] != "count" else float("inf")
    D["T"] = {"count": n, "time": T_end, "both": (T_end, n)}[D["mode"]]
    if D["mode"] == "time":
        D["steps"] = False  # (no record limit to raise)
    D["P"] = dict(d=d, G=G, mu=BW.drawn_mean(rng, d), form=form, L=BW.slot_crossing_factor(d, seed=case) if form == "L" else None,
                  u=(0.5 + rng.random(d) * 1.5) if form == "U" else None, oscn=form == "oscn", rho=D["rho"], lam=lam, t0=D["t0"],
                  x0=rng.standard_normal((nch, d)), th0=rng.standard_normal((nch, d)),
                  seeds=np.uint64(9950 + 10 * case) + np.arange(nch, dtype=np.uint64))
    return D


def references(D):
    refs = MP.ref_runs(D["P"], D["T"], D["c"], adapt=D["adapt"], factor=D["factor"])
    assert all(r["nevents"] == len(r["t"]) for r in refs)  # (the record buffer held them all)
    return refs


def describe(D, refs=None):
    s = "case %2d: d %4d (%2d slots) Γ %-6s form %-4s λ %.1f ρ %.2f t0 %+.1f chains %d adapt %d factor %.1f c %-5g cap %2d T %-5s n %2d steps %d" % (
        D["case"], D["d"], BW.slots(D["d"]), D["gamma"], D["form"], D["lam"], D["rho"], D["t0"], D["nch"], D["adapt"], D["factor"], D["c"], D["cap"],
        D["mode"], D["n"], D["steps"])
    if refs is not None:
        s += " | " + " ".join("st %d rec %d acc %d rf %d" % (r["status"], r["nevents"], r["nacc"], r["nrefresh"]) for r in refs)
    return s


@pytest.mark.parametrize("case", range(NCASES))
def test_random_speed_recorded_options(gpu_pkg, case):
    pkg = gpu_pkg
    L = pkg._lib
    D = draw_case(case)
    refs = references(D)
    what = describe(D, refs)
    print(what)
    assert all(r["status"] in (M.REF_OK, M.REF_BOUND_VIOLATED) for r in refs), what
    with MP.open_ensemble(pkg, D["P"], D["c"], cap=D["cap"], adapt=D["adapt"], factor=D["factor"]) as ens:
        col = MP.Collector(pkg, ens)
        limits = [D["n"] // 3, 2 * D["n"] // 3, D["n"]] if D["steps"] else [D["n"]]
        for lim in limits:
            ens.set_bps_record_limit(lim)
            col.drive(D["T_end"], L.RUN_REFERENCE_TAIL)
        assert ens.kernel_name() == "bps_modern_run_kernel"
        res = col.result()
    MP.compare(res, refs)
    # a chain that gains more records than the buffer holds between two drains has to resume after PDMP_CHAIN_TRACE_FULL
    bounds = [0] + [lim if lim else 1 << 30 for lim in limits]
    gained = max(min(hi, r["nevents"]) - min(lo, r["nevents"]) for r in refs for lo, hi in zip(bounds, bounds[1:]))
    if gained > D["cap"]:
        assert col.launches > len(limits) and L.CHAIN_TRACE_FULL in col.statuses, what
