"""What the statistical checks of the sticky Bouncy Particle / Boomerang share between the host tests (the C restatement alone) and the
device tests (the same figures from the device's traces).  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import scipy.sparse as sp

import sticky_ref_lib as R


def p_free_exact(kappa):
    """Γ = I, μ = 0, κ_i = κ: the sticky target is ∏ (N(0,1)(dx_i) + δ0(dx_i)/κ) up to a constant, so P(x_i ≠ 0) = κ√(2π)/(1 + κ√(2π)) --
    the d-dimensional product version of w in test/sticky.jl:30 (σ = 1, μ = 0)."""
    return kappa * np.sqrt(2 * np.pi) / (1 + kappa * np.sqrt(2 * np.pi))


def free_fraction(t, f, burn):
    """Fraction of [burn, t[-1]] every coordinate is free, from the events' times [n] and masks [n x d] (f[k] holds on [t[k], t[k+1]))."""
    te = np.clip(np.asarray(t, dtype=np.float64), burn, None)
    return (np.asarray(f, dtype=np.float64)[:-1] * np.diff(te)[:, None]).sum(0) / (te[-1] - burn)


def closed_form_state(nch, d, seed0=1000):
    x0 = np.stack([np.random.default_rng(seed0 + k).standard_normal(d) for k in range(nch)])
    th0 = np.stack([np.random.default_rng(seed0 + 500000 + k).standard_normal(d) for k in range(nch)])
    return x0, th0


# flow -> (flow_kind, c): Γ = I makes the BouncyParticle's bound exact (any c > 0 does); the Boomerang's rate is 0 on its own target
CLOSED_FORM = {"bps": (0, 0.01), "boomerang": (1, 0.1)}
KAPPA, LAMBDA_REF, SEED = 1.5, 1.0, 77


def closed_form_ref(flow, nch, d, T, burn):
    """The restatement's per-chain free fractions (mean over coordinates) on the closed-form problem: [nch]."""
    kind, c = CLOSED_FORM[flow]
    x0, th0 = closed_form_state(nch, d)
    out = []
    for k in range(nch):
        r = R.sspdmp_notfact(0.0, x0[k], th0[k], T, c, KAPPA, flow_kind=kind, gamma=sp.identity(d, format="csc"), mu=np.zeros(d),
                             lambda_ref=LAMBDA_REF, mu_flow=np.zeros(d), seed=SEED + k, ev_cap=int(80 * d * T + 4096))
        assert r["status"] == R.REF_OK and r["nevents"] == len(r["t"])
        out.append(free_fraction(r["t"], r["f"], burn).mean())
    return np.array(out)


def z_score(fr, kappa=KAPPA):
    se = fr.std(ddof=1) / np.sqrt(len(fr))
    return (fr.mean() - p_free_exact(kappa)) / se, fr.mean(), se
