"""The mode table of zz_general_run_kernel (csrc/pdmp_general.hip): one case table for tests/test_general_cases_ref.py (the oracle alone, no
device) and tests/test_gpu_general_modes.py (the device against it, bit for bit, in one launch sequence and in slices).  TEST INFRASTRUCTURE ONLY.

The general kernel is the only one that serves adaptscale, c::LocalBound on the factorised samplers, an explicit neighbourhood G ⊋ G1, G = All()
for FactBoomerang and wide graphs, sspdmp on wide graphs, and FactBoomerang itself.  Each mode keeps per-chain state in global memory BETWEEN
launches -- the tuned σ (sig_chain), LocalBound's renew flags, θ_f of frozen coordinates, the adapted c, the refresh clock's key slot d -- and
a launch that resumed with one of them stale would still leave a self-consistent trace.  So every case is run to T once, and once cut at
three interior times with a trace buffer that refills, and both runs are held to the oracle.

What the kernel does depends on
  d        the clock's slot d lies in key block d / 64: with coordinates (d % 64 != 0) or alone (d = 64); several blocks beyond d = 64;
  |G1[i]|  the re-bound walks G1[i] in chunks of 64 members, the products in chunks of 128; beyond 64 the rank of a member -- its draw --
           is carried from chunk to chunk (reb_count), for sticky and masked chains;
  |G[i]|   with pdmp_ensemble_set_neighbourhood the tables' pattern is G: members of G[i] ∖ G1[i] are moved, not re-bounded, and take no draw.

The table, case x what it reaches.  Two chains per case, seeds fixed; c = cmul · column norms of Γ; counts are per chain on the oracle.
Graphs: lattice(n) = gmrf_precision(n); maintest(d); dense(d, ρ, seed) = R Rᵀ + 2I of a sparse R; hub = the same with a dense first row;
chunk2 = Γ without the couplings between its two halves of d / 2 coordinates (the bounding matrix of test/testparallel.jl).

  case        graph               d   |G| |G1|  T−t0  t0   events      proposals     end   what it is for
  adaptscale (σ0 = 0.5 + U(0,1), its own tuned copy per chain)
  as_zz81     lattice(9)          81    5   5   40    1.5  2069..2694   9192..11157  tail  ZigZag, λref = 1, bound 0.9 Γ, flow and target mean, adapt (24..29 c_i
                                                                                           raised); clock in block 1 with 17 coordinates; σ moved on 32..43 %
  as_zz144    lattice(12)        144    5   5   10    0.7  1106..1214  37875..37959  stop  the same without adapt, λref = 2; clock in block 2; 17..21 refreshes
  as_zz64     lattice(8)          64    5   5   40    0    1725..1818   5991..6155   stop  d a multiple of 64: the clock alone in block 1; adapt
  as_boom81   lattice(9)          81    5   5   30    0.5  1839..2098  66470..69620  tail  FactBoomerang, λref = 4, ρ = 0.4, flow mean = target mean, adapt; the step acts
                                                                                           once (1 + 2ρ/(1−ρ))/(t λref) < 0.2, i.e. t > 2.9: 112..149 refreshes, σ moved on 46..54 %
  as_boom144  lattice(12)        144    5   5   10    0    846..867    78001..85185  stop  λref = 5, ρ = 0.3 (t > 1.9), no adapt, flow mean only
  LocalBound (ZigZag, no refresh; c_i distinct: equal horizons give exactly tied keys, the documented divergence; speeds 0.5, 1, 1.5)
  lb_lat      lattice(12)        144    5   5   12    0.7  1259..1327   4387..4441   tail  target mean, adapt on; 152..187 renew events
  lb_main     maintest(20)        20   11  11  120    0    1592..1664  16013..16350  stop  adapt on; 2067..2191 renews
  lb_dense    dense(130,.07,11)  130   93  93    4    0.4   558..596   17969..18261  stop  56 columns above 64 members: two chunks per re-bound; 631..643 renews
  lb_own      dense(150,.08,3)   150  134 134    3    0     375..398   19052..19298  tail  flow Γ = 0.8 Γ and a flow mean that LocalBound must not read; 192..334 renews
  explicit G = pattern of Γ ⊋ G1 = pattern of chunk2(Γ): 103 columns of G above 64 members (up to 112), |G1| <= 62, up to 55 masked members
  g_adapt     dense(160,.06,5)   160  112  62    3    0     525..534    2702..2743   tail  c starts too small (20..21 c_i raised); 363..366 events on the wide columns
  g_clock     "                  160  112  62    3    0.5   587..619   31875..31983  stop  λref = 3, σ != 1, both means; 8..10 refreshes
  g_sticky    "                  160  112  62    3    0     673..718    2774..2790   tail  sspdmp: 221..252 freezes, 139..159 thaws; frozen AND masked members skipped
  g_local     "                  160  112  62    2    0     234..252   10675..11096  tail  LocalBound: REFUSED by the device (PDMP_ERR_UNSUPPORTED from set_state), see below
  g_ascale    "                  160  112  62    6    0    1156..1203  13268..13595  stop  adaptscale, λref = 3, adapt: σ moved on 11..15 %, 21..25 refreshes
  g_boom      "                  160  112  62    3    0     392..397   32954..36924  stop  FactBoomerang, ρ = 0.3, flow mean: the bound sums over G1[i] alone
  g_wide192   dense(192,.06,5)   192  150  77    2.5  0     540..562    3213..3264   stop  G1 itself has 10 columns above 64: masked members in both chunks
  G = All()
  all_boom    maintest(24)        24   16  16   60    0     588..762    7799..12376  tail  FactBoomerang on a small graph, bound 0.85 Γ, flow mean, adapt; 28..33 refreshes
  all_dense   dense(150,.08,3)   150  134 134    4    0     733..778   26101..26139  stop  ZigZag, λref = 2, σ != 1: 3..13 refreshes
  sspdmp on the general kernel (bound 0.9 Γ; proposals are counted from the last adaptation, src/ss_fact.jl:134)
  st_hub      hub(120,.04,31)    120  120 120    5    0     737..763      49..257    tail  flow and target mean, adapt; 251..256 freezes, 183..197 thaws
  st_hub_rev  "                  120  120 120    5    0     749..779    8793..9150   tail  reversible, no adapt, two different means
  st_hub_str  "                  120  120 120    5    0     793..853       4..39     tail  strong_upperbounds, adapt (28..31 c_i raised)

Explicit G together with the other modes -- what the reference does, what the oracle does, what the device does:
  sspdmp, a refresh clock, adaptscale, FactBoomerang   src/sfact.jl:73-145,162-201 re-bound G1[i] = pattern of F.Γ[:, i] and move G[i] (:82) and
      G2[i] = two-hop(G1) ∖ G[i] (:85,129,178); FactBoomerang's ab sums over neighbours(G1, i) (src/fact_samplers.jl:58-65).  Read against
      oracle/pdmp_oracle.c's orc_spdmp_zigzag line by line: they agree.  The device equals the oracle in all four (g_sticky, g_clock, g_ascale, g_boom).
      g_boom found a device bug: zz_init_kernel summed FactBoomerang's first bound over the tables' pattern, which is G's after set_neighbourhood.
  LocalBound   src/local.jl:95-149 has ONE graph: its argument G is moved (:43), re-bounded member by member with a draw each (:61-67), and G2 comes
      from G's own two-hop sets (:108); F.Γ's pattern is G only when no G is given (:148).  The oracle re-bounded pattern(F.Γ) as sfact.jl does:
      fixed (tests/test_general_cases_ref.py pins it).  The device's neighbourhood tables re-bound G1 only, so it refuses the combination when the
      state is set; a flow matrix that carries G's pattern gives the reference's chain.
LocalBound and adapt: between two re-bounds of i the Gaussian rate is pos(∇ϕ_i θ_i + v_i s) exactly and the bound is that plus c_i (1 + s/100),
so no c_i is ever raised; the guard asserts that c comes back unchanged instead.

Over the table: the clock's slot inside a coordinate block (81, 144, 160) and alone (64); |G1| > 64 (lb_dense, lb_own, all_dense, st_hub*,
g_wide192); |G| > 64 with masked members (g_*); every mode with adapt on and off; t0 > 0 in adaptscale, LocalBound and explicit-G cases; the last
launch runs the reference's tail in 11 cases and stops before T in 10.  In slices every case is cut at t0 + (0.3, 0.55, 0.8)(T − t0) and its trace
buffer holds min(32, events / 16) events (14..32), so every chain comes back with a full trace at least three times (asserted).

Stress: 12 seeded draws (stress_problem) over the same options: every mode once (draws 0..7: adaptscale, adaptscale + FactBoomerang, LocalBound,
explicit G plain / with a clock / sticky, All(), sspdmp) and four more at random; d = 30..168; T doubled until every chain has 150 events.
guard_case says what "not vacuous" means; the device test asserts it on the oracle's chains before anything is compared with them."""
import functools

import numpy as np
import scipy.sparse as sp

import oracle_lib as O

NCH = 2
FACTOR = 1.7
GENERAL_KERNEL, LOCAL_KERNEL = "zz_general_run_kernel", "zz_local_run_kernel"
CUT_FRACTIONS = (0.3, 0.55, 0.8)  # the three interior cut times of a run in slices, as fractions of T − t0
MAX_PROPOSALS = 100000
MIN_EVENTS = 150


def _pkg():
    from __graft_entry__ import load_package
    return load_package()


# ------------------------------------------------------------------------------------------------------------------------------- graphs

def _csc(G):
    G = sp.csc_matrix(G)
    G.sort_indices()
    return G


def lattice(n):
    return _csc(_pkg().problems.gmrf_precision(n))


def maintest(d):
    return _csc(_pkg().problems.maintest_precision(d))


def dense(d, density, seed):
    """R Rᵀ + 2I of a sparse R: two-hop sets and, at these sizes, columns beyond one wavefront (tests/test_gpu_stress_general.py's _graph)."""
    rng = np.random.default_rng(seed)
    R = sp.random(d, d, density=density, random_state=rng, data_rvs=rng.standard_normal, format="csc")
    return _csc(R @ R.T + 2.0 * sp.identity(d))


def hub(d, density, seed):
    """A sparse precision with a dense hub column, the shape of a regression's intercept (test_sticky_on_large_neighbourhoods)."""
    rng = np.random.default_rng(seed)
    R = sp.random(d, d, density=density, random_state=rng, data_rvs=rng.standard_normal, format="lil")
    R[0, :] = 0.3 * rng.standard_normal(d)
    A = sp.csc_matrix(R)
    return _csc(A.T @ A + 2.0 * sp.identity(d))


def chunk_diagonal_part(G, K):
    """Γ without the couplings between K chunks of d // K coordinates (test/testparallel.jl's bounding matrix)."""
    k = G.shape[0] // K
    coo = sp.coo_matrix(G)
    keep = (coo.row // k) == (coo.col // k)
    return _csc(sp.csc_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), shape=G.shape))


def col_sizes(G):
    return np.diff(sp.csc_matrix(G).indptr)


def dk_of(d):
    """Length of the key array: d coordinates and the refresh clock's slot d, in blocks of 64."""
    return 64 * ((d + 1 + 63) // 64)


def clock_shares_block(d):
    """Does slot d (the refresh clock) lie in a 64-key block that also holds coordinates?"""
    return d % 64 != 0


# -------------------------------------------------------------------------------------------------------------------------------- cases
# name: (graph, options).  Options (defaults in _DEFAULTS):
#   mode      "adaptscale" | "local" | "masked" | "all" | "sticky" (what the guard asks of the case; a case may combine: see the flags)
#   boom      FactBoomerang instead of ZigZag          lam, rho   refresh rate, ρ           sig      "nonuni" σ0 = 0.5 + U(0, 1) | "one"
#   bound     factor of the bounding Γ (1 = the target's) | "chunk2" = chunk_diagonal_part(Γ, 2)      mu_b, mu_t   flow / target mean (scale)
#   nbr       explicit G = the target's pattern           local, adaptscale, adapt, move_all, sticky (reversible, strong)
#   speeds    |θ0| drawn from these (ZigZag without σ)    cmul       c = cmul · column norms of Γ (· 1 + 0.01 U for LocalBound: no tied horizons)
#   t0, T     start, horizon T − t0                       tail       the last launch runs the reference's tail (else it stops before T)
#   expect    "equal" | "refuse" (the device returns PDMP_ERR_UNSUPPORTED from set_state)
_DEFAULTS = dict(boom=False, lam=0.0, rho=0.0, sig="one", bound=1.0, mu_b=0.0, mu_t=0.0, nbr=False, local=False, adaptscale=False, adapt=False,
                 move_all=False, sticky=None, speeds=(1.0,), cmul=2.0, t0=0.0, tail=True, expect="equal", kappa=(0.2, 1.5), same_mu=False)

_WIDE = lambda: dense(160, 0.06, 5)   # noqa: E731  the explicit-G target: 103 columns of G above 64 members
_WIDE192 = lambda: dense(192, 0.06, 5)  # noqa: E731  ... whose chunk-diagonal part itself has columns above 64
_DENSE = lambda: dense(150, 0.08, 3)  # noqa: E731
_HUB = lambda: hub(120, 0.04, 31)     # noqa: E731

_T = {
    # ---- adaptscale: σ per chain in global memory, tuned in the refresh branch
    "as_zz81":    (lambda: lattice(9), dict(mode="adaptscale", adaptscale=True, lam=1.0, sig="nonuni", bound=0.9, mu_b=0.3, mu_t=0.3, t0=1.5, T=40.0, adapt=True, cmul=0.5)),
    "as_zz144":   (lambda: lattice(12), dict(mode="adaptscale", adaptscale=True, lam=2.0, sig="nonuni", bound=0.9, mu_b=0.3, mu_t=0.2, t0=0.7, T=10.0, cmul=6.0, tail=False)),
    "as_zz64":    (lambda: lattice(8), dict(mode="adaptscale", adaptscale=True, lam=1.0, sig="nonuni", mu_t=0.3, T=40.0, adapt=True, cmul=0.5, tail=False)),
    "as_boom81":  (lambda: lattice(9), dict(mode="adaptscale", adaptscale=True, boom=True, lam=4.0, rho=0.4, sig="nonuni", mu_b=0.3, same_mu=True, t0=0.5, T=30.0,
                                            adapt=True, cmul=1.0)),
    "as_boom144": (lambda: lattice(12), dict(mode="adaptscale", adaptscale=True, boom=True, lam=5.0, rho=0.3, sig="nonuni", mu_b=0.2, T=10.0, cmul=3.0, tail=False)),
    # ---- LocalBound: renew flags per chain in global memory
    "lb_lat":     (lambda: lattice(12), dict(mode="local", local=True, speeds=(0.5, 1.0, 1.5), mu_t=0.3, t0=0.7, T=12.0, adapt=True, cmul=0.6)),
    "lb_main":    (lambda: maintest(20), dict(mode="local", local=True, speeds=(0.5, 1.0, 1.5), mu_t=0.3, T=120.0, adapt=True, cmul=2.5, tail=False)),
    "lb_dense":   (lambda: dense(130, 0.07, 11), dict(mode="local", local=True, speeds=(0.5, 1.0, 1.5), mu_t=0.2, t0=0.4, T=4.0, adapt=False, cmul=2.5, tail=False)),
    "lb_own":     (_DENSE, dict(mode="local", local=True, speeds=(0.5, 1.0), bound=0.8, mu_b=0.4, mu_t=0.2, T=3.0, cmul=2.5)),
    # ---- explicit G ⊋ G1 with columns of G above 64 members
    "g_adapt":    (_WIDE, dict(mode="masked", nbr=True, bound="chunk2", adapt=True, cmul=0.4, T=3.0)),
    "g_clock":    (_WIDE, dict(mode="masked", nbr=True, bound="chunk2", lam=3.0, sig="nonuni", mu_b=0.2, mu_t=0.2, t0=0.5, T=3.0, cmul=4.0, tail=False)),
    "g_sticky":   (_WIDE, dict(mode="masked", nbr=True, bound="chunk2", sticky=(False, False), adapt=True, cmul=0.8, T=3.0)),
    "g_local":    (_WIDE, dict(mode="masked", nbr=True, bound="chunk2", local=True, speeds=(0.5, 1.0), adapt=False, cmul=2.5, T=2.0, expect="refuse")),
    "g_ascale":   (_WIDE, dict(mode="masked", nbr=True, bound="chunk2", adaptscale=True, lam=3.0, sig="nonuni", adapt=True, cmul=1.0, T=6.0, tail=False)),
    "g_boom":     (_WIDE, dict(mode="masked", nbr=True, bound="chunk2", boom=True, lam=1.0, rho=0.3, sig="nonuni", mu_b=0.2, adapt=False, cmul=0.3, T=3.0, tail=False)),
    "g_wide192":  (_WIDE192, dict(mode="masked", nbr=True, bound="chunk2", adapt=True, cmul=0.4, T=2.5, tail=False)),
    # ---- G = All()
    "all_boom":   (lambda: maintest(24), dict(mode="all", move_all=True, boom=True, lam=0.5, rho=0.2, mu_b=0.2, bound=0.85, adapt=True, cmul=0.1, T=60.0)),
    "all_dense":  (_DENSE, dict(mode="all", move_all=True, lam=2.0, sig="nonuni", T=4.0, cmul=2.5, tail=False)),
    # ---- sspdmp on the general kernel (no explicit G)
    "st_hub":     (_HUB, dict(mode="sticky", sticky=(False, False), bound=0.9, mu_b=0.1, mu_t=0.1, adapt=True, cmul=0.3, T=5.0)),
    "st_hub_rev": (_HUB, dict(mode="sticky", sticky=(True, False), bound=0.9, mu_b=0.1, mu_t=0.15, cmul=3.0, T=5.0)),
    "st_hub_str": (_HUB, dict(mode="sticky", sticky=(False, True), bound=0.9, mu_t=0.1, adapt=True, cmul=0.15, T=5.0)),
}
NAMES = list(_T)
STRESS_N = 12


def _build(name, index, graph, opt, seed_base):
    """The problem of one table line or stress draw: every array drawn from default_rng(seed_base + index) in a fixed order."""
    o = dict(_DEFAULTS)
    o.update(opt)
    rng = np.random.default_rng(seed_base + index)
    G = graph()
    d = G.shape[0]
    Gb = chunk_diagonal_part(G, 2) if o["bound"] == "chunk2" else (G if o["bound"] == 1.0 else _csc(o["bound"] * G))
    mu_b = o["mu_b"] * rng.standard_normal(d) if o["mu_b"] else None
    mu_t = o["mu_t"] * rng.standard_normal(d) if o["mu_t"] else None
    if o["same_mu"]:
        mu_t = mu_b
    sig = 0.5 + rng.random(d) if o["sig"] == "nonuni" else np.ones(d)
    x0 = rng.standard_normal((NCH, d))
    if o["boom"]:
        th0 = sig * rng.standard_normal((NCH, d))
    else:
        th0 = sig * rng.choice([-1.0, 1.0], (NCH, d)) * rng.choice(np.asarray(o["speeds"]), (NCH, d))
    c = o["cmul"] * _pkg().problems.column_norms(G)
    if o["local"]:  # distinct c_i: equal horizons 2/c_i/|θ_i| give exactly tied queue keys (the documented tie divergence)
        c = c * (1.0 + 0.01 * rng.random(d))
    kappa = rng.uniform(o["kappa"][0], o["kappa"][1], d) if o["sticky"] is not None else None
    t0 = float(o["t0"])
    P = dict(o)
    P.update(name=name, G=G, Gb=Gb, d=d, mu_b=mu_b, mu_t=mu_t, sigma=sig, X0=x0, TH0=th0, c=c, kappa=kappa, t0=t0, T=t0 + float(o["T"]),
             nbrG=G if o["nbr"] else None, seeds=np.uint64(seed_base + 1000 + 10 * index) + np.arange(NCH, dtype=np.uint64))
    small_all = o["move_all"] and not o["boom"] and int(col_sizes(Gb).max()) <= 64 and _two_hop_max(Gb) <= 64
    P["kernel"] = LOCAL_KERNEL if small_all else GENERAL_KERNEL
    P["cuts"] = tuple(t0 + f * float(o["T"]) for f in CUT_FRACTIONS)
    return P


def _two_hop_max(G):
    A = sp.csc_matrix((np.ones(G.nnz), G.indices, G.indptr), shape=G.shape)
    return int(np.diff(sp.csc_matrix(A @ A).indptr).max())


@functools.lru_cache(maxsize=None)
def problem(name):
    graph, opt = _T[name]
    return _build(name, NAMES.index(name), graph, opt, 41000)


def oracle_run(P, k):
    kw = dict(t0=P["t0"], target_mu=P["mu_t"], adapt=P["adapt"], factor=FACTOR, seed=int(P["seeds"][k]))
    if P["sticky"] is not None:
        return O.sspdmp_zigzag(P["Gb"], P["mu_b"], P["G"], P["X0"][k], P["TH0"][k], P["c"], P["kappa"], P["T"], reversible=P["sticky"][0],
                               strong_upperbounds=P["sticky"][1], G=P["nbrG"], **kw)
    return O.spdmp_zigzag(P["Gb"], P["mu_b"], P["G"], P["X0"][k], P["TH0"][k], P["c"], P["T"], sigma=P["sigma"], lambda_ref=P["lam"], rho=P["rho"],
                          move_all=P["move_all"], stop_before_T=not P["tail"], factboomerang=P["boom"], adaptscale=P["adaptscale"],
                          local_bound=P["local"], G=P["nbrG"], **kw)


@functools.lru_cache(maxsize=None)
def refs(name):
    """The oracle's chains of a case, computed once per session and never written to."""
    P = problem(name)
    return tuple(oracle_run(P, k) for k in range(NCH))


# -------------------------------------------------------------------------------------------------------------------------------- guards

def rebound_set_sizes(P):
    """|what an accepted event of i re-bounds|: G1[i] = the pattern of the bounding Γ; under LocalBound with an explicit G, G[i] (src/local.jl:61)."""
    return col_sizes(P["G"] if (P["local"] and P["nbr"]) else P["Gb"])


def renew_events(P, r):
    """Events of LocalBound's `renew` branch (src/local.jl:34-41, one draw each): the main stream's draws that nothing else accounts for --
    d initial clocks, one coin per proposal, |G1[i]| draws per accepted event of i, one per rejection."""
    return int(r["ndraw_main"]) - P["d"] - int(r["num"]) - int(np.dot(r["acc"], rebound_set_sizes(P))) - (int(r["num"]) - int(r["nacc"]))


def wide_events(P, r):
    """Events on coordinates whose column of G has more than 64 members."""
    wide = col_sizes(P["G"]) > 64
    return int(np.sum(wide[r["events"]["i"]]))


def freezes_thaws(r):
    ev = r["events"]
    return int(np.sum(ev["theta"] == 0.0)), int(np.sum((ev["x"] == 0.0) & (ev["theta"] != 0.0)))


def slice_cap(rs):
    """trace_capacity of the run in slices: a sixteenth of the shortest chain, 32 at the most (the bound asked for is a quarter): the four
    slices hold 30, 25, 25 and 20 % of a chain's events, so every one of them fills the buffer at least three times."""
    return max(4, min(32, min(len(r["events"]) for r in rs) // 16))


def guard_common(P, rs):
    for r in rs:
        w = (P["name"], r["status"], len(r["events"]), r["num"], r["nacc"])
        assert r["status"] == 0, w
        assert len(r["events"]) >= MIN_EVENTS and r["num"] <= MAX_PROPOSALS, w
        assert r["num"] > r["nacc"], w  # rejections occur
        assert len(r["events"]) >= 4 * slice_cap(rs), w


def guard_case(P, rs):
    """Not vacuous: conditions on the oracle's chains alone (tests/test_general_cases_ref.py asserts them on the CPU, the device test before it
    compares anything): every chain healthy with >= 150 events, <= 10^5 proposals and rejections; then what the case's mode is about."""
    guard_common(P, rs)
    for r in rs:
        w = (P["name"], P["mode"])
        if P["adaptscale"]:
            assert np.mean(r["sigma"] != P["sigma"]) >= 0.10 and r["nrefresh"] >= 10, (w, float(np.mean(r["sigma"] != P["sigma"])), r["nrefresh"])
        if P["local"]:
            assert int(r["ndraw_main"]) - int(r["num"]) - int(r["nacc"]) >= 50 and renew_events(P, r) >= 50, (w, renew_events(P, r))
        if P["mode"] == "masked":
            assert wide_events(P, r) >= 50, (w, wide_events(P, r))
        if P["sticky"] is not None:
            fz, tw = freezes_thaws(r)
            assert fz >= 20 and tw >= 1, (w, fz, tw)
        if P["adapt"] and not P["local"]:
            assert np.any(r["c"] > P["c"]), w
        if P["adapt"] and P["local"]:
            # a LocalBound on a Gaussian target cannot be violated: between two re-bounds of i the rate is pos(∇ϕ_i θ_i + v_i s) exactly, and the
            # bound is that plus c_i (1 + s/100) > 0 -- so `adapt` switches the kernel to the per-chain c and never changes a value
            assert np.array_equal(r["c"], P["c"]), w
        if P["move_all"] and not P["boom"]:
            assert r["nrefresh"] >= 2, (w, r["nrefresh"])


# ------------------------------------------------------------------------------------------------------------------------------- stress

_STRESS_MODES = ("adaptscale", "adaptscale_boom", "local", "masked", "masked_clock", "masked_sticky", "all", "sticky")


@functools.lru_cache(maxsize=None)
def stress_problem(case):
    """One seeded draw over the table's option space: the mode, a graph that suits it (lattice 8..12, maintest 20..40, dense 100..170), means, a
    bounding Γ of its own, σ0, speeds, t0, adapt, the tail; T is doubled from a first guess until every chain of the oracle has 150 events."""
    rng = np.random.default_rng(42000 + case)
    mode = _STRESS_MODES[case % len(_STRESS_MODES)] if case < len(_STRESS_MODES) else _STRESS_MODES[int(rng.integers(0, len(_STRESS_MODES)))]
    adapt = bool(rng.integers(0, 2))
    o = dict(mode=mode.split("_")[0], adapt=adapt, t0=float(rng.choice([0.0, 0.0, rng.uniform(0.1, 2.0)])), tail=bool(rng.integers(0, 2)),
             mu_t=float(rng.choice([0.0, 0.2, 0.4])), cmul=float(rng.uniform(0.4, 1.0)) if adapt else float(rng.uniform(3.0, 4.5)))
    if mode.startswith("masked"):
        dd, dens, gs = int(rng.integers(130, 171)), float(rng.uniform(0.055, 0.075)), int(rng.integers(0, 1000))
        graph = lambda: dense(2 * (dd // 2), dens, gs)  # noqa: E731
        o.update(nbr=True, bound="chunk2")
        if mode == "masked_clock":
            o.update(lam=float(rng.uniform(0.5, 2.0)), sig="nonuni", mu_b=0.2)
        if mode == "masked_sticky":
            o.update(sticky=(bool(rng.integers(0, 2)), bool(rng.integers(0, 2))), tail=True)
        T = 1.5
    elif mode in ("adaptscale", "adaptscale_boom"):
        n = int(rng.integers(8, 13))
        graph = lambda: lattice(n)  # noqa: E731
        o.update(adaptscale=True, sig="nonuni", mu_b=float(rng.choice([0.0, 0.3])), bound=float(rng.choice([1.0, 0.9])))
        if mode == "adaptscale_boom":
            o.update(boom=True, lam=float(rng.uniform(3.0, 6.0)), rho=float(rng.choice([0.0, 0.3, 0.5])), bound=1.0, mu_t=0.0)
        else:
            o.update(lam=float(rng.uniform(0.5, 2.0)))
        if not adapt and mode == "adaptscale":  # (the tuned σ raises the ZigZag's rates: a fixed c needs the room)
            o.update(cmul=float(rng.uniform(6.0, 8.0)))
        T = 8.0
    elif mode == "local":
        kind = int(rng.integers(0, 3))
        n, dm, dd, gs = int(rng.integers(8, 13)), int(rng.integers(20, 41)), int(rng.integers(100, 171)), int(rng.integers(0, 1000))
        graph = (lambda: lattice(n)) if kind == 0 else (lambda: maintest(dm)) if kind == 1 else (lambda: dense(dd, 0.07, gs))  # noqa: E731
        o.update(local=True, speeds=(0.5, 1.0, 1.5), bound=float(rng.choice([1.0, 0.8])))
        T = 2.0
    elif mode == "all":
        boom = bool(rng.integers(0, 2))
        dm, dd, gs = int(rng.integers(20, 41)), int(rng.integers(100, 171)), int(rng.integers(0, 1000))
        graph = (lambda: maintest(dm)) if boom else (lambda: dense(dd, 0.07, gs))  # noqa: E731
        o.update(move_all=True, boom=boom, lam=float(rng.uniform(0.5, 2.5)), rho=float(rng.choice([0.0, 0.3])) if boom else 0.0,
                 sig="one" if boom else "nonuni")
        if boom:
            o.update(mu_t=0.0)
        T = 2.0
    else:
        dd, gs = int(rng.integers(100, 161)), int(rng.integers(0, 1000))
        graph = lambda: hub(dd, 0.04, gs)  # noqa: E731
        o.update(sticky=(bool(rng.integers(0, 2)), bool(rng.integers(0, 2))), bound=float(rng.choice([1.0, 0.9])), mu_b=float(rng.choice([0.0, 0.1])),
                 tail=True)
        T = 2.0
    for _ in range(8):
        o["T"] = T
        P = _build("stress%d" % case, case, graph, o, 43000)
        P["stress_mode"] = mode
        rs = tuple(oracle_run(P, k) for k in range(NCH))
        if any(r["status"] != 0 for r in rs) or min(len(r["events"]) for r in rs) >= MIN_EVENTS:
            break
        T *= 2.0
    return P, rs


def stress_refs(case):
    return stress_problem(case)[1]


# --------------------------------------------------------------------------------------------------------------------- the device's side

def open_ensemble(pk, P, cap):
    """An ensemble on problem P up to (not including) set_state; the caller closes it."""
    L = pk._lib
    sampler = L.SAMPLER_STICKY_ZIGZAG if P["sticky"] is not None else (L.SAMPLER_ZIGZAG_ALL if P["move_all"] else L.SAMPLER_ZIGZAG_LOCAL)
    ens = pk.Ensemble(NCH, P["d"], sampler=sampler, adapt=P["adapt"], factor=FACTOR, trace_capacity=cap)
    try:
        mu_b = np.zeros(P["d"]) if P["mu_b"] is None else P["mu_b"]
        if P["boom"]:
            ens.set_flow(pk.FactBoomerang(P["Gb"], mu_b, P["lam"], σ=P["sigma"], ρ=P["rho"]))
        else:
            ens.set_flow(pk.ZigZag(P["Gb"], mu_b, P["sigma"], λref=P["lam"]))
        if P["nbrG"] is not None:
            ens.set_neighbourhood(P["nbrG"])
        ens.set_target(pk.GaussianTarget(P["G"], P["mu_t"]))
        if P["sticky"] is not None:
            ens.set_sticky(P["kappa"], *P["sticky"])
        if P["adaptscale"]:
            ens.set_adaptscale(True)
        if P["local"]:
            ens.set_local_bound(True)
    except Exception:
        ens.close()
        raise
    return ens


def device_run(pk, P, cap, cuts):
    """The chains of P on the device: slices ending at `cuts` (RUN_STOP_BEFORE) and at T (the reference's tail or not, as P says), the trace
    drained whenever a launch returns.  Counters, events, final state, σ, the kernel's name, and how often each chain came back with a full
    trace."""
    L = pk._lib
    with open_ensemble(pk, P, cap) as ens:
        ens.set_state(P["t0"], P["X0"], P["TH0"], P["c"], P["seeds"])
        evs = [[] for _ in range(NCH)]
        full = np.zeros(NCH, dtype=np.int64)
        names, launches = set(), 0
        for Tk, flag in [(float(v), L.RUN_STOP_BEFORE) for v in cuts] + [(P["T"], L.RUN_REFERENCE_TAIL if P["tail"] else L.RUN_STOP_BEFORE)]:
            while True:
                ens.run(Tk, flag)
                launches += 1
                names.add(ens.kernel_name())
                cnt = ens.counters()
                full += cnt["status"] == L.CHAIN_TRACE_FULL
                for k in range(NCH):
                    if cnt["ntrace"][k]:
                        evs[k].append(ens.trace(k, counters=cnt))
                ens.trace_reset()
                if not L.needs_rerun(cnt["status"]):
                    break
        return dict(cnt=cnt, evs=[np.concatenate(e) if e else np.empty(0, dtype=L.EVENT_DTYPE) for e in evs], fs=ens.final_state(),
                    sigma=ens.final_sigma() if P["adaptscale"] else None, kernels=names, launches=launches, full=full)


def compare_with_oracle(what, P, run, rs):
    """Bit for bit: events (i, t, x, θ); num, nacc, acc per coordinate; nrefresh and the main stream's position; final (t, x, θ) -- the free
    mask of a sticky chain is θ != 0 --; the adapted c; the tuned σ."""
    cnt, fs = run["cnt"], run["fs"]
    for k, r in enumerate(rs):
        w = (what, P["name"], k)
        assert cnt["status"][k] == 0 and r["status"] == 0, (w, cnt["status"][k])
        ev = run["evs"][k]
        assert len(ev) == len(r["events"]), (w, len(ev), len(r["events"]))
        for f in ("i", "t", "x", "theta"):
            assert np.array_equal(ev[f], r["events"][f]), (w, f, int(np.argmax(ev[f] != r["events"][f])))
        assert (int(cnt["num"][k]), int(cnt["nacc"][k])) == (r["num"], r["nacc"]), (w, cnt["num"][k], r["num"])
        assert int(cnt["ndraw_main"][k]) == r["ndraw_main"], (w, cnt["ndraw_main"][k], r["ndraw_main"])
        if P["sticky"] is None:
            assert int(cnt["nrefresh"][k]) == r["nrefresh"], w
            assert np.array_equal(fs["acc"][k], r["acc"]), w
        for f in ("t", "x", "theta"):
            assert np.array_equal(fs[f][k], r[f]), (w, f)
        if P["sticky"] is not None:
            assert np.array_equal(fs["theta"][k] != 0.0, r["theta"] != 0.0), w
        if P["adapt"]:
            assert np.array_equal(fs["c"][k], r["c"]), w
        if P["adaptscale"]:
            assert np.array_equal(run["sigma"][k], r["sigma"]), w
