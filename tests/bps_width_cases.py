"""The slot-count matrix of the Bouncy-Particle-family event loops: one case table for tests/test_bps_width_cases_ref.py (the references alone,
no device) and tests/test_gpu_bps_widths.py (the device against them, bit for bit).  TEST INFRASTRUCTURE ONLY.

The loops keep x, θ, ∇ϕ in registers, element e = slot*64 + lane, and are compiled once per slot count NS in {1, 2, 4, 8, 16}; a dimension d is
served by the smallest NS >= ceil(d/64).  What differs per instantiation -- the guards of empty slots, the per-slot bit masks, the unrolled forms
themselves -- shows only where that instantiation runs, so W holds the smallest d that reach each one:

      d   NS  occupied slots   what it exercises
     65    2   2               one element in the last slot
    128    2   2               FULL of NS 2
    129    4   3               one element in slot 2, slot 3 wholly empty
    193    4   4               one element in the last slot
    256    4   4               FULL of NS 4
    257    8   5               three wholly empty slots
    512    8   8               FULL of NS 8
    513   16   9               seven wholly empty slots
   1023   16  16               the last lane missing

Γ (coupling_gamma) is symmetric and strictly diagonally dominant: a near band (±1), a far band at offset 64 + 3 -- element e gathers from another
slot AND another lane --, a few seeded random symmetric entries; sorted indices, at most 8 entries per column.  The mean (coupling_mean) is
non-zero with exact zeros (every third coordinate): the Boomerang's μ_flow == 0 branch of the freezing time is a code path of its own.  The
Cholesky cases take a pentadiagonal Γ (banded_gamma), whose factor stays banded.

The covering table, form x d (x = the case runs there).  Plain loop, bps_run_kernel<NS, DIAG, BOOM, IDENT, FULL, EXT>, against
oracle_lib.pdmp_bps:

    case           template form         65  128  129  193  256  257  512  513  1023
    ident          DIAG IDENT [FULL]      x   F    x    x   F    x    F    x    x       (F: the FULL form, d == NS*64)
    diag           DIAG                   .   .    x    .   .    x    .    x    x
    csc            (general gather)       x   .    x    x   .    x    x    x    x
    ext_chol       EXT, mass factor       .   .    x    .   .    x    .    x    x
    ext_local      EXT, local_bound       .   .    x    x   .    x    .    x    .
    ext_subsample  EXT, subsample         .   .    x    .   x    x    .    x    .
    ext_target     EXT, own target        .   .    x    x   .    x    x    x    .
    boom_diag      BOOM DIAG              .   .    x    .   x    x    .    x    x
    boom_csc       BOOM                   x   .    x    x   .    x    .    x    .
    boom_mass      BOOM EXT               .   .    x    x   .    x    .    x    .

Path moments (MOM = 2 against MOM = 0 and against trace.path_moments): tests/test_gpu_bps_moments.py, cases iso / csc / mass / boom_csc at
d = 129, 256, 257, 513 on this module's Γ.

Sticky loop, bps_sticky_run_kernel<NS, BOOM>, against sticky_ref_lib.sspdmp_notfact -- both flows at EVERY width of W; κ per coordinate in
[0.3, 3], adapt, strong_upperbounds at half the widths (128, 129, 257, 512), t0 = 2.5 at the odd-indexed widths (128, 193, 257, 513), x0[d−1] = 0.05 and
θ0[d−1] = −1 so that the last coordinate of the last occupied slot freezes at once.

Speed-recorded loop, bps_modern_run_kernel<NS, UDIAG, OSCN>, against modern_bps_ref_lib.pdmp, 40 records of 3 chains, t0 as above:

    case   template form          65  128  129  193  256  257  512  513  1023
    I      plain, L = I            x   x    x    .   x    x    x    x    .
    U      UDIAG                   .   .    x    x   x    x    .    x    x
    oscn   OSCN (ρ = 0.9)          .   .    x    x   .    x    x    x    x
    L      plain, sparse factor    x   .    x    x   .    x    .    x    x       (sub-diagonals at offsets 1 and 70: the solve crosses slots)

So every (loop, form) runs at NS = 4 (d = 129: an empty trailing slot), at NS = 8 (d = 257: three) and at NS = 16 (d = 513: seven), and FULL
runs at 128, 256 and 512.

Horizons: about as many events per case at every width.  The plain loop runs T − t0 = 4·min(1, 200/d) (a Boomerang three times that: it
reflects rarely) with λref raised to 8/(T − t0) where that is larger, so that every case refreshes.  The sticky Bouncy Particle runs
8·min(1, 100/d) at c = 20; the sticky Boomerang max(12·min(1, 300/d), 5) with its target's mean 3 away from the flow's in every coordinate -- it
starts downhill and cannot reflect before it has passed the target, a quarter period.  Where t0 ≠ 0 the sticky driver draws tref without t0 and so
refreshes at once, at tref < t0, moving the state BACK by t0 − tref (the plain driver does the same): x0[d−1] is 0.05 − (t0 − tref) there, so that
the coordinate stands at 0.05 after that move, and ρ = 0.95 keeps θ[d−1] < 0 through the refreshment.  The speed-recorded loop holds 40 records.
guard_* say what "not vacuous" means; both test files assert them on the reference before anything is compared with it."""
import functools

import numpy as np
import scipy.sparse as sp

import modern_bps_ref_lib as M
import oracle_lib as O
import sticky_ref_lib as R

W = [65, 128, 129, 193, 256, 257, 512, 513, 1023]
FAR = 64 + 3


def t0_of(d):
    return 2.5 if W.index(d) % 2 else 0.0


def slots(d):
    return (d + 63) // 64


@functools.lru_cache(maxsize=None)
def coupling_gamma(d, seed=0):
    """See the module's docstring.  Also defined for d not in W (the moments cases and the stress files use it): the far band needs d > 67."""
    rng = np.random.default_rng(7000 + 13 * d + seed)
    A = sp.lil_matrix((d, d))
    for i in range(d - 1):
        A[i, i + 1] = A[i + 1, i] = -0.3 - 0.2 * rng.random()
    for i in range(max(d - FAR, 0)):
        A[i, i + FAR] = A[i + FAR, i] = 0.25 + 0.2 * rng.random()
    cnt = np.asarray((A != 0).sum(axis=0)).ravel() + 1  # (+ the diagonal)
    want = max(d // 16, 2) if d > 3 else 0
    for _ in range(20 * want):
        if want == 0:
            break
        i, j = (int(v) for v in rng.integers(0, d, 2))
        if i == j or A[i, j] != 0 or cnt[i] >= 8 or cnt[j] >= 8:
            continue
        A[i, j] = A[j, i] = 0.3 * rng.standard_normal()
        cnt[i] += 1
        cnt[j] += 1
        want -= 1
    A = sp.csc_matrix(A)
    G = sp.csc_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=0)).ravel() + 1.0 + 0.5 * rng.random(d)))
    G.sort_indices()
    assert np.diff(G.indptr).max() <= 8 and abs(G - G.T).nnz == 0
    return G


def coupling_mean(d, seed=0):
    rng = np.random.default_rng(7100 + 13 * d + seed)
    return np.where(np.arange(d) % 3 == 0, 0.0, 0.3 * rng.standard_normal(d))


@functools.lru_cache(maxsize=None)
def banded_gamma(d):
    k = np.arange(d)
    G = sp.diags([np.full(d - 2, 0.15), np.full(d - 1, -0.4), 1.6 + 0.4 * np.cos(k), np.full(d - 1, -0.4), np.full(d - 2, 0.15)],
                 [-2, -1, 0, 1, 2], format="csc")
    G.sort_indices()
    return sp.csc_matrix(G)


def drawn_gamma(rng, d, kind):
    """The stress files' precisions: "I", "banded" (one or two bands a side) or "sparse" (random symmetric entries, about three per column);
    strictly diagonally dominant, sorted indices."""
    if kind == "I" or d == 1:
        return sp.identity(d, format="csc") * (1.0 if kind == "I" else 1.7)
    if kind == "banded":
        w = min(int(rng.integers(1, 3)), d - 1)
        bands = [np.full(d - o, -rng.uniform(0.2, 1.0)) for o in range(1, w + 1)]
        G = sp.diags([np.full(d, 2.0 * w + 1.0 + rng.random())] + bands + bands, [0] + list(range(1, w + 1)) + [-o for o in range(1, w + 1)], format="csc")
    else:
        Rm = sp.random(d, d, density=min(1.5 / d, 0.5), random_state=rng, data_rvs=rng.standard_normal, format="csc")
        A = sp.csc_matrix(Rm + Rm.T)
        G = sp.csc_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=0)).ravel() + 1.0))
    G = sp.csc_matrix(G)
    G.sort_indices()
    return G


def drawn_mean(rng, d):
    """None, or a mean with exact zeros in it."""
    kind = int(rng.integers(0, 3))
    if kind == 0:
        return None
    m = 0.4 * rng.standard_normal(d)
    return m if kind == 1 else np.where(rng.random(d) < 0.4, 0.0, m)


# ---------------------------------------------------------------------------------------------------------------------------- plain loop

PLAIN_NAMES = ["ident", "diag", "csc", "ext_chol", "ext_local", "ext_subsample", "ext_target", "boom_diag", "boom_csc", "boom_mass"]
_PLAIN_AT = {
    "ident": W,
    "diag": [129, 257, 513, 1023],
    "csc": [65, 129, 193, 257, 512, 513, 1023],
    "ext_chol": [129, 257, 513, 1023],
    "ext_local": [129, 193, 257, 513],
    "ext_subsample": [129, 256, 257, 513],
    "ext_target": [129, 193, 257, 512, 513],
    "boom_diag": [129, 256, 257, 513, 1023],
    "boom_csc": [65, 129, 193, 257, 513],
    "boom_mass": [129, 193, 257, 513],
}
PLAIN_CASES = [(name, d) for d in W for name in PLAIN_NAMES if d in _PLAIN_AT[name]]
PLAIN_NCH = 2


def plain_problem(pkg, name, d):
    """One dispatcher branch of launch_ns (csrc/pdmp_bps.hip) at width d: the flow F, the device's target (None: the flow's own Γ(x − μ)), the
    oracle's arguments, and the run's (t0, T, c, ...).  adapt wherever a constant Boomerang bound or a target of its own can be violated."""
    rng = np.random.default_rng(7200 + 31 * d + PLAIN_NAMES.index(name))
    I = sp.identity(d, format="csc")
    z = np.zeros(d)
    G, mu = coupling_gamma(d), coupling_mean(d)
    t0 = t0_of(d)
    boom = name.startswith("boom")
    h = (12.0 if boom else 4.0) * min(1.0, 200.0 / d)  # (the Boomerang reflects rarely)
    lam = max(0.5 if boom else 0.7, 8.0 / h)  # about 8 refreshments at least, whatever the horizon
    P = dict(name=name, d=d, t0=t0, T=t0 + h, lam=lam, rho=0.0, adapt=False, local_bound=False, subsample=False,
             target=None, okw={}, boom=boom, seed=7300 + d,
             x0=rng.standard_normal((PLAIN_NCH, d)), th0=rng.standard_normal((PLAIN_NCH, d)))
    if name == "ident":  # Γ = I, μ = 0: IDENT, FULL where d == NS*64
        P.update(F=pkg.BouncyParticle(I, z, lam), og=I, omu=None, c=1e-3)
    elif name == "diag":  # Γ = I, μ ≠ 0
        P.update(F=pkg.BouncyParticle(I, mu, lam, 0.4), og=I, omu=mu, c=1e-3, rho=0.4)
    elif name == "csc":  # the gather through LDS across slots, identity mass
        P.update(F=pkg.BouncyParticle(G, mu, lam, L=I), og=G, omu=mu, c=1.0)
    elif name == "ext_chol":
        Gb = banded_gamma(d)
        P.update(F=pkg.BouncyParticle(Gb, mu, lam, 0.2), og=Gb, omu=mu, c=1.0, rho=0.2)
    elif name == "ext_local":
        P.update(F=pkg.BouncyParticle(G, mu, lam, L=I), og=G, omu=mu, c=1.0, local_bound=True)
    elif name == "ext_subsample":
        P.update(F=pkg.BouncyParticle(G, mu, lam, L=I), og=G, omu=mu, c=1.0, subsample=True)
    elif name == "ext_target":  # ∇ϕ from a target of its own, the bound from the flow's 1.4 Γt
        Gf = sp.csc_matrix(1.4 * G)
        mut = mu + 0.05 * rng.standard_normal(d)
        P.update(F=pkg.BouncyParticle(Gf, mu, lam, 0.2, L=I), og=Gf, omu=mu, c=2.5, rho=0.2, adapt=True,
                 target=pkg.GaussianTarget(G, mut), okw=dict(target=(G, mut)))
    elif name == "boom_diag":  # a diagonal target other than the flow's I: grad_correct! leaves a gradient, reflections happen
        Gd = sp.diags(rng.uniform(1.3, 2.0, d), format="csc")
        mut = mu + 0.5 * rng.standard_normal(d)
        P.update(F=pkg.Boomerang(I, mu, lam, 0.4), og=Gd, omu=mut, c=3.0, rho=0.4, adapt=True, target=pkg.GaussianTarget(Gd, mut),
                 okw=dict(boomerang_mu=mu))
    elif name == "boom_csc":
        mut = mu + 0.5 * rng.standard_normal(d)
        P.update(F=pkg.Boomerang(I, mu, lam), og=G, omu=mut, c=8.0, adapt=True, target=pkg.GaussianTarget(G, mut),
                 okw=dict(boomerang_mu=mu))
    elif name == "boom_mass":
        Gb = banded_gamma(d)
        mut = mu + 0.5 * rng.standard_normal(d)
        P.update(F=pkg.Boomerang(Gb, mu, lam, 0.3), og=Gb, omu=mut, c=8.0, rho=0.3, adapt=True, target=pkg.GaussianTarget(Gb, mut),
                 okw=dict(boomerang_mu=mu))
    else:
        raise ValueError(name)
    return P


_plain_cache = {}


def plain_refs(pkg, name, d):
    """(P, [oracle result per chain]), computed once per session."""
    if (name, d) not in _plain_cache:
        P = plain_problem(pkg, name, d)
        refs = [O.pdmp_bps(P["og"], P["omu"], P["x0"][k], P["th0"][k], P["c"], P["T"], t0=P["t0"], lambda_ref=P["lam"], rho=P["rho"],
                           adapt=P["adapt"], factor=2.0, seed=P["seed"] + k, ev_cap=20000, mass_L=P["F"].L, local_bound=P["local_bound"],
                           subsample=P["subsample"], **P["okw"]) for k in range(PLAIN_NCH)]
        _plain_cache[(name, d)] = (P, refs)
    return _plain_cache[(name, d)]


def guard_plain(P, refs):
    for r in refs:
        assert r["status"] == 0 and r["nevents"] < 20000, (P["name"], P["d"], r["status"])
        assert r["nacc"] >= (3 if P["boom"] else 10), (P["name"], P["d"], r["nacc"])
        assert r["nrefresh"] >= 2, (P["name"], P["d"], r["nrefresh"])


# --------------------------------------------------------------------------------------------------------------------------- sticky loop

STICKY_CASES = [(flow, d) for d in W for flow in ("bps", "boom")]
STICKY_NCH = 2
STICKY_C = 20.0


def sticky_problem(pkg, flow, d):
    """The P of tests/test_gpu_sticky_bps_parity.py (problem / ref_run / check) on the coupling Γ, with the run's options beside it."""
    rng = np.random.default_rng(7400 + 31 * d + (flow == "boom"))
    G, mu = coupling_gamma(d), coupling_mean(d)
    t0 = t0_of(d)
    h = 8.0 * min(1.0, 100.0 / d) if flow == "bps" else max(12.0 * min(1.0, 300.0 / d), 5.0)
    P = dict(flow=flow, d=d, G=G, lam=max(0.8, 8.0 / h), rho=0.95 if t0 else (0.5 if W.index(d) % 4 == 0 else 0.0), target=None, t0=t0, T=t0 + h,
             c=STICKY_C, adapt=True, strong=W.index(d) % 4 in (1, 2), kappa=rng.uniform(0.3, 3.0, d), seed=7500 + d)
    x0, th0 = rng.standard_normal((STICKY_NCH, d)), rng.standard_normal((STICKY_NCH, d))
    x0[:, d - 1], th0[:, d - 1] = 0.05, -1.0
    P["x0"], P["th0"] = x0, th0
    if flow == "bps":
        P.update(mu=mu, F=pkg.BouncyParticle(G, mu, P["lam"], P["rho"]))
    else:  # the target's mean 3 away from the flow's
        P.update(mu=mu + 3.0 * rng.choice([-1.0, 1.0], d), mu_flow=mu, F=pkg.Boomerang(sp.identity(d, format="csc"), mu, P["lam"], P["rho"]))
    if t0:
        # the driver draws tref without t0 (src/ss_not_fact.jl:190): the first event is a refreshment at tref < t0, which moves the state BACK by
        # t0 − tref.  tref is draw 0 of the chain, whatever the state: read it from a probe run that ends at once, and start the last coordinate
        # where that move brings it to 0.05 (ρ = 0.95 keeps its θ < 0 through the refreshment).
        for k in range(STICKY_NCH):
            probe = sticky_ref(dict(P, T=t0 + 1e-9), k)
            if probe["nrefresh"] and probe["t"][1] < t0:  # (else tref > t0: nothing moves back)
                x0[k, d - 1] = 0.05 - (t0 - probe["t"][1])
    return P


def sticky_ref(P, k, x0=None, th0=None):
    kw = dict(flow_kind=0 if P["flow"] == "bps" else 1, gamma=P["G"], mu=P["mu"], lambda_ref=P["lam"], rho=P["rho"], strong_upperbounds=P["strong"],
              adapt=P["adapt"], factor=2.0, seed=P["seed"] + k, ev_cap=16384)
    if P["flow"] == "bps":
        kw["target"] = P["target"]
    else:
        kw["mu_flow"] = P["mu_flow"]
    return R.sspdmp_notfact(P["t0"], P["x0"][k] if x0 is None else x0, P["th0"][k] if th0 is None else th0, P["T"], P["c"], P["kappa"], **kw)


_sticky_cache = {}


def sticky_refs(pkg, flow, d):
    if (flow, d) not in _sticky_cache:
        P = sticky_problem(pkg, flow, d)
        _sticky_cache[(flow, d)] = (P, [sticky_ref(P, k) for k in range(STICKY_NCH)])
    return _sticky_cache[(flow, d)]


def freezes_and_thaws(f):
    """(freezes, thaws, slots in which a freeze happened) of an event list's free masks [n x d]."""
    k, i = np.nonzero(f[1:] != f[:-1])
    froze = ~f[k + 1, i]
    return int(froze.sum()), int((~froze).sum()), set((i[froze] // 64).tolist())


def guard_sticky(P, refs):
    d = P["d"]
    for r in refs:
        assert r["status"] == R.REF_OK and r["nevents"] == len(r["t"]), (P["flow"], d, r["status"])
        assert r["nacc"] >= (3 if P["flow"] == "boom" else 10), (P["flow"], d, r["nacc"])
        assert r["nrefresh"] >= 2, (P["flow"], d, r["nrefresh"])
        nf, nt, where = freezes_and_thaws(r["f"])
        assert nf >= 10 and nt >= 10, (P["flow"], d, nf, nt)
        assert (~r["f"][:, d - 1]).any(), (P["flow"], d)  # the last coordinate of the last occupied slot froze
        assert len(where) >= 2, (P["flow"], d, where)


# ------------------------------------------------------------------------------------------------------------------- speed-recorded loop

MODERN_FORMS = ["I", "U", "oscn", "L"]
_MODERN_AT = {
    "I": [65, 128, 129, 256, 257, 512, 513],
    "U": [129, 193, 256, 257, 513, 1023],
    "oscn": [129, 193, 257, 512, 513, 1023],
    "L": [65, 129, 193, 257, 513, 1023],
}
MODERN_CASES = [(form, d) for d in W for form in MODERN_FORMS if d in _MODERN_AT[form]]
MODERN_NCH, MODERN_RECORDS, MODERN_C = 3, 40, 5.0


def slot_crossing_factor(d, seed=0):
    """A sparse lower-triangular L: the diagonal, a sub-diagonal, and one at offset 70 -- the solve with L and L' crosses slots and lanes."""
    rng = np.random.default_rng(7600 + d + seed)
    diags, offs = [0.8 + 0.4 * rng.random(d)], [0]
    for o, s in ((1, 0.3), (70, 0.2)):
        if d > o:
            diags.append(s * rng.standard_normal(d - o))
            offs.append(-o)
    Ls = sp.csc_matrix(sp.diags(diags, offs, format="csc"))
    Ls.sort_indices()
    return Ls


def modern_problem(form, d):
    """The P of tests/test_gpu_modern_bps_parity.py (problem / ref_runs / open_ensemble) on the coupling Γ."""
    rng = np.random.default_rng(7700 + 31 * d + MODERN_FORMS.index(form))
    return dict(d=d, G=coupling_gamma(d), mu=coupling_mean(d), form=form, L=slot_crossing_factor(d) if form == "L" else None,
                u=(0.5 + rng.random(d) * 1.5) if form == "U" else None, oscn=form == "oscn", rho=0.9, lam=1.0, t0=t0_of(d),
                x0=rng.standard_normal((MODERN_NCH, d)), th0=rng.standard_normal((MODERN_NCH, d)),
                seeds=np.uint64(7800 + d) + np.arange(MODERN_NCH, dtype=np.uint64))


def modern_ref(P, k, T, c, adapt=False, factor=2.0, ev_cap=4096):
    return M.pdmp(P.get("t0", 0.0), P["x0"][k], P["th0"][k], T, c, gamma=P["G"], mu=P["mu"], lambda_ref=P["lam"], rho=P["rho"], L=P["L"],
                  u_diag=P["u"], oscn=P["oscn"], adapt=adapt, factor=factor, seed=int(P["seeds"][k]), ev_cap=ev_cap)


_modern_cache = {}


def modern_refs(form, d):
    if (form, d) not in _modern_cache:
        P = modern_problem(form, d)
        _modern_cache[(form, d)] = (P, [modern_ref(P, k, MODERN_RECORDS, MODERN_C) for k in range(MODERN_NCH)])
    return _modern_cache[(form, d)]


def guard_modern(P, refs):
    for r in refs:
        assert r["status"] == M.REF_OK and r["nevents"] == MODERN_RECORDS == len(r["t"]), (P["form"], P["d"], r["status"], r["nevents"])
        assert r["nacc"] >= 10 and r["nrefresh"] >= 2, (P["form"], P["d"], r["nacc"], r["nrefresh"])
        if P["oscn"]:
            assert r["noscn_draws"] == r["nacc"] > 0, (P["form"], P["d"], r["noscn_draws"], r["nacc"])
        else:
            assert r["noscn_draws"] == 0
