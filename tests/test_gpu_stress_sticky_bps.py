"""Randomised stress of the sticky Bouncy Particle / Boomerang loop (-m gpu; sspdmp, src/ss_not_fact.jl:104-201; csrc/pdmp_bps_sticky.inc): random
dimensions across every slot count (empty trailing slots included), Γ = I, banded or random sparse, flow and target means with exact zeros, a
target of its own, refresh rates, ρ, t0 ≠ 0, 1 / 2 / 5 chains, adapt and its factor, strong_upperbounds, thaw rates per coordinate with one at
1000 and one at 0.05, and a trace buffer so small that most cases resume after PDMP_CHAIN_TRACE_FULL many times -- events (t, x, θ, f), every
counter, status, final state, final f and θf bit for bit the restatement's (tests/ref/sticky_notfact_ref.c).  No case skips: where the
restatement ends as bound-violated (no adapt), the device ends with the same status, counters and state.  Seeds are fixed; draw_case(case) is
the whole draw and needs no device."""
import numpy as np
import pytest
import scipy.sparse as sp

import bps_width_cases as BW
import sticky_ref_lib as R
import test_gpu_sticky_bps_parity as SP

pytestmark = pytest.mark.gpu

BASE_SEED = 9700
NCASES = 12
DIMS = [1, 3, 17, 64, 65, 129, 200, 257, 300, 513, 1024]


def draw_case(pkg, case):
    rng = np.random.default_rng(BASE_SEED + case)
    d = int(rng.choice(DIMS))
    kind = ["I", "banded", "sparse"][int(rng.integers(0, 3))]
    flow = "boom" if rng.integers(0, 2) else "bps"
    G = BW.drawn_gamma(rng, d, kind)
    lam = float(rng.choice([0.3, 1.0, 2.5]))
    rho = float(rng.choice([0.0, 0.4, 0.95]))
    mu, mu2 = BW.drawn_mean(rng, d), BW.drawn_mean(rng, d)
    z = np.zeros(d)
    D = dict(case=case, d=d, gamma=kind, flow=flow, lam=lam, rho=rho, t0=float(rng.choice([0.0, -1.5, 2.5])), nch=int(rng.choice([1, 2, 5])),
             adapt=bool(rng.integers(0, 2)), factor=float(rng.choice([1.5, 2.0, 3.0])), strong=bool(rng.integers(0, 2)),
             cap=int(rng.choice([4, 16, 64])), own_target=False)
    P = dict(flow=flow, d=d, lam=lam, rho=rho, target=None)
    if flow == "bps":
        own = bool(rng.integers(0, 3) == 0)
        D["own_target"] = own
        Gf = sp.csc_matrix(1.4 * G) if own else G  # (a flow Γ that dominates the target's: the bound stays one)
        P.update(G=Gf, mu=z if mu is None else mu, F=pkg.BouncyParticle(Gf, z if mu is None else mu, lam, rho))
        if own:
            P["target"] = (G, mu2)
    else:
        P.update(G=G, mu=z if mu2 is None else mu2, mu_flow=z if mu is None else mu,
                 F=pkg.Boomerang(sp.identity(d, format="csc"), z if mu is None else mu, lam, rho))
    kappa = rng.uniform(0.3, 3.0, d)
    hi = int(rng.integers(0, d))
    kappa[hi] = 1000.0  # (thaws at once)
    if d > 1:
        kappa[(hi + 1 + int(rng.integers(0, d - 1))) % d] = 0.05  # (stays frozen)
    # without adapt c has to be large: the Boomerang's bound is a constant, and the Bouncy Particle's is computed from a θ whose frozen entries are 0
    c = float(rng.uniform(0.3, 1.5)) if D["adapt"] else float(rng.uniform(3.0, 6.0)) * float(np.sqrt(d))
    D.update(P=P, kappa=kappa, c=c, T=D["t0"] + float(rng.uniform(3.0, 10.0)) * min(1.0, 100.0 / d),
             x0=rng.standard_normal((D["nch"], d)), th0=rng.standard_normal((D["nch"], d)),
             seeds=np.uint64(9800 + 10 * case) + np.arange(D["nch"], dtype=np.uint64))
    return D


def reference(D, k):
    P = D["P"]
    kw = dict(flow_kind=0 if P["flow"] == "bps" else 1, gamma=P["G"], mu=P["mu"], lambda_ref=P["lam"], rho=P["rho"], strong_upperbounds=D["strong"],
              adapt=D["adapt"], factor=D["factor"], seed=int(D["seeds"][k]), ev_cap=32768)
    if P["flow"] == "bps":
        kw["target"] = P["target"]
    else:
        kw["mu_flow"] = P["mu_flow"]
    r = R.sspdmp_notfact(D["t0"], D["x0"][k], D["th0"][k], D["T"], D["c"], D["kappa"], **kw)
    assert r["nevents"] == len(r["t"])  # (the event buffer held them all)
    return r


def describe(D, refs=None):
    s = "case %2d: d %4d (%2d slots) Γ %-6s %-4s own_target %d λ %.1f ρ %.2f t0 %+.1f chains %d adapt %d factor %.1f strong %d cap %2d" % (
        D["case"], D["d"], BW.slots(D["d"]), D["gamma"], D["flow"], D["own_target"], D["lam"], D["rho"], D["t0"], D["nch"], D["adapt"], D["factor"],
        D["strong"], D["cap"])
    if refs is not None:
        s += " | " + " ".join("st %d ev %d acc %d rf %d" % (r["status"], r["nevents"], r["nacc"], r["nrefresh"]) for r in refs)
    return s


@pytest.mark.parametrize("case", range(NCASES))
def test_random_sticky_bps_options(gpu_pkg, case):
    pkg = gpu_pkg
    L = pkg._lib
    D = draw_case(pkg, case)
    P, nch, d = D["P"], D["nch"], D["d"]
    refs = [reference(D, k) for k in range(nch)]
    what = describe(D, refs)
    print(what)
    assert all(r["status"] in (R.REF_OK, R.REF_BOUND_VIOLATED) for r in refs), what
    ev = [[] for _ in range(nch)]
    launches = 0
    with SP.raw_ensemble(pkg, P, nch, D["cap"], adapt=D["adapt"], factor=D["factor"]) as ens:
        ens.set_bps_sticky(D["kappa"], D["strong"])
        ens.set_state_bps(D["t0"], D["x0"], D["th0"], D["c"], D["seeds"])
        for _ in range(100000):
            ens.run(D["T"], L.RUN_REFERENCE_TAIL)
            launches += 1
            cnt = ens.counters()
            for k in range(nch):
                if cnt["ntrace"][k]:
                    SP.drain(pkg, ens, k, ev[k])
            ens.trace_reset()
            if not L.needs_rerun(cnt["status"]):
                break
        else:
            raise AssertionError("the run does not end: " + what)
        cnt = ens.counters()
        fs = ens.bps_final_state()
        f_fin, thf_fin = SP.raw_final(pkg, ens)
    for k, r in enumerate(refs):
        assert int(cnt["status"][k]) == (L.CHAIN_OK if r["status"] == R.REF_OK else L.CHAIN_BOUND_VIOLATED), (what, k)
        for name in ("num", "nacc", "nrefresh", "ndraw_main", "nevents"):
            assert int(cnt[name][k]) == r[name], (what, k, name, int(cnt[name][k]), r[name])
        t, x, th, f = (np.concatenate([p[j] for p in ev[k]]) for j in range(4))
        assert len(t) == r["nevents"], (what, k, len(t), r["nevents"])
        assert SP.same(t, r["t"]) and SP.same(x, r["x"]) and SP.same(th, r["theta"]) and np.array_equal(f, r["f"]), (what, k)
        assert SP.same(fs["t"][k], r["t_final"]) and SP.same(fs["c"][k], r["c_final"]), (what, k)
        assert SP.same(fs["x"][k], r["x_final"]) and SP.same(fs["theta"][k], r["theta_final"]), (what, k)
        assert np.array_equal(f_fin[k], r["f_final"]) and SP.same(thf_fin[k], r["theta_f"]), (what, k)
    if max(r["nevents"] for r in refs) > D["cap"]:
        assert launches > 1, what  # resumed after PDMP_CHAIN_TRACE_FULL
