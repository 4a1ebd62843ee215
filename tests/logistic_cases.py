"""The shape matrix of the logistic kernel family of config C4: one case table for tests/test_logistic_cases_ref.py (the oracle alone, no device),
tests/test_gpu_logistic_shapes.py, tests/test_gpu_violation_state.py and tests/test_gpu_stress_logistic.py (the device against it, bit for bit).
TEST INFRASTRUCTURE ONLY.

zz_logistic_lds_kernel (csrc/pdmp_logistic.hip) keeps a chain in LDS and its event times in eight registers per lane; what it does depends on
  d      the `d & 1` padding in front of the chunk buffers; the key slots per lane (coordinate j in lane j % 64, slot j / 64: lanes that own
         nothing below d = 64, the `k − 1` re-reads, a partly used last slot); the limit dk <= 512, where dk = 64·ceil((d + 1)/64) counts the
         refresh clock's slot -- d = 511 is the largest it takes, 512 the first that goes to zz_general_run_kernel;
  k_sub  the observation lanes [goff, goff + k_sub) of the 64-draw block, goff = k_sub · (proposals since the refill), refilled when
         goff + k_sub > 64; the partner lanes `lane ^ 32`, which straddle lane 63 / 0 only where goff + k_sub > 32 > goff; the LDS staging of
         the four terms per observation, full at k_sub = 32, with a tail of one for odd k_sub and no pair at k_sub = 1;
  ne     the `e < ne` guard over the six packed regressors of an observation; l = 1 (a column with one observation: every draw is entry 0);
  |G1|   the remainders of the re-bound's sums (k & 7) and the chunks of columns beyond 64 entries.
The parity build's zz_logistic_rows_kernel<W> (csrc/pdmp_logrows.hip) takes dk <= 448 and k_sub + 2 <= W; the tracked form <.., TRK> and the
form without ∫x dt share the LDS kernel's limits; PDMP_DEBUG_KERNEL_SEQ keeps the records in HBM (zz_general_run_kernel, LGFAST at k_sub = 10).

The covering table, case x what it reaches.  Designs: sparse_design (scripts/sparsedesign.jl) or random_design below; the set-up around them is
logistic_setup (y, Newton mode μ, Γ, Γdrop at droptol 1e-2, σ, c = 0.01, γ0 = 0.01); 3 chains, x0 near μ, θ0 = ±σ, adapt = true, factor = 5.
Counts are per chain on the oracle (tests/test_logistic_cases_ref.py asserts the conditions they satisfy).

  case  design                                  p  k_sub  T−t0  events    proposals     what it is for
  a     sparse_design((2,3), r=1, m=40)        12    1     30   202..226  2058..5626    d < 64 (52 lanes own no key); ne ∈ {1,2,4}; one observation per
                                                                                        gradient: no pair in the staging loop; REFERENCE_TAIL
  b     sparse_design((4,4,4), r=0, m=20)      60    7     20  1239..1325 16330..21918  ne ∈ {0,1,3,6} (60 rows without a regressor appended: 6 %);
        + 60 empty rows                                                                 odd k_sub; even d < 64; t0 = 2.5; in slices, trace of 48
  c     sparse_design((7,8), r=1, m=20)        72   32     10   500..516   975..1140    staging buffers full; goff ∈ {0, 32}
  d     random, intercept, ne 1..6, n = 2000   65   31     10   290..331   999..1483    odd d just above one slot; odd k_sub at the top; the intercept's
                                                                                        65-entry column accepted 92 times; in slices, trace of 40
  e     random, ne 1..6, n = 3000             129    3     10   430..458  1361..1635    49 columns above 64 entries (511 accepted events there);
                                                                                        goff up to 60; t0 = 2.5
  f     random, intercept, n = 8000           511   13      3   614..641   901..976     the largest d the LDS kernel takes, odd: last slot one short;
                                                                                        the intercept's G1 holds 510 coordinates (8 chunks)
  g     random, n = 8000                      512   32      3   643..683   868..884     dk = 576: the first d the LDS kernel does NOT take ->
                                                                                        zz_general_run_kernel, tracking refused
  g511  as g, one column fewer                511   32      3   676..682   876..929     the largest d with the staging buffers full; 145 columns
                                                                                        above 64 entries
  h     random, n = 1500, column 37 cut to     70    9     10   280..298   644..737     H.l = 1: the column is accepted 4..6 times per chain
        one entry
  i     as e                                  129   20     10   517..526  1004..1058    goff ∈ {0, 20, 40}: at 20 the partner lanes are 52..63, 0..7
  j63   random, ne ∈ {2,3,5}, n = 1200         63    2     10   208..221   566..698     one slot, its last lane empty
  j64   random, intercept, ne ∈ {1,4}          64   10     10   245..279   500..608     dk = 128 with one coordinate in the second block; LGFAST on
                                                                                        the HBM form; trace_capacity = 0 (counters and final state only)
  j128  random, ne ∈ {3,6}, n = 2500          128    2     10   391..430  1153..1625    two full slots; 81 columns above 64 entries
  k     sparse_design((3,3,3), r=2, m=20)      38    5     10   222..268   775..931     rows of up to 8 regressors: no packed tables ->
                                                                                        zz_general_run_kernel, unpacked gradient, tracking refused
  l     as g, one column more                 513   10      3   617..636   935..998     -> zz_general_run_kernel (LGFAST), tracking refused
  m     as c                                   72   33     10   446..471   767..881     the first k_sub the LDS kernel does not take; REFERENCE_TAIL

Forms x cases (tests/test_gpu_logistic_shapes.py asserts the kernel's name in each):
  lds, lds_noI, hbm, trk, trk_noI   every case a .. j128 (the LDS family); g, k, l, m run zz_general_run_kernel with and without ∫x dt
  rows32                            a b e h i j63 j64 j128        rows16   a b e h j63 j64 j128   (the others exceed dk <= 448 or k_sub + 2 <= W)
Over the table: ne = 0..6 all occur; every k & 7 among accepted coordinates; accepted coordinates with k > 64 under tracking and at odd d
(d, e, f, g511, i); odd k_sub 1, 3, 7, 9, 13, 31.  Two cases start at t0 = 2.5 (b, e); two run in slices with a trace buffer that refills
at least three times per slice sequence (b: even d, d: odd d), so the state leaves and re-enters LDS at every launch.

Violation state (adapt = false, six chains, uniform c; with c = 0.01 every chain is violated within its first proposals): a at c = 40 -- three
chains violated after 138, 24 and 202 events, three finish; d at c = 20 -- all six violated after 43..68 events.

Stress: 12 seeded draws (stress_problem), reaching slot counts ceil(p/64) ∈ {1, 2, 3, 4, 6, 7, 8} and k_sub ∈ {7, 9, 15, 16, 19, 21, 23, 24, 26, 27}.
guard_* say what "not vacuous" means; the device tests assert them on the oracle's chains before anything is compared with them."""
import functools

import numpy as np
import scipy.sparse as sp

import oracle_lib as O

NCH = 3
GAMMA0 = 0.01
FACTOR = 5.0


# ------------------------------------------------------------------------------------------------------------------------------ designs

def random_design(n, p, lens, intercept, seed, single=None):
    """A seeded CSC design [n x p]: every row's length is drawn uniformly from `lens` (a subset of 0..6); with `intercept`, column 0 is
    present in every non-empty row (Γ then has a dense column, and the G1 set of the intercept holds every coordinate); the other regressors
    of a row are distinct columns drawn uniformly; every column has at least one entry.  Values as in the scripts' mock designs: 1 (a level),
    0.3 (an interaction) or 0.1 N(0, 1) + a sign (a continuous regressor).  single = j: column j is cut down to its first entry."""
    lens = tuple(sorted(set(int(v) for v in lens)))
    assert lens and lens[0] >= 0 and lens[-1] <= 6 and lens[-1] <= p and max(lens) >= 1
    rng = np.random.default_rng(seed)
    ne = rng.choice(lens, size=n)
    first = 1 if intercept else 0
    rows = []
    count = np.zeros(p, dtype=np.int64)
    for r in range(n):
        m = int(ne[r])
        if m == 0:
            rows.append(np.empty(0, dtype=np.int64))
            continue
        if intercept:
            cols = np.concatenate([[0], first + rng.choice(p - first, size=m - 1, replace=False)]) if m > 1 else np.array([0])
        else:
            cols = rng.choice(p, size=m, replace=False)
        cols = np.sort(cols.astype(np.int64))
        count[cols] += 1
        rows.append(cols)
    # a column nobody drew takes the place of an entry of a column that has entries to spare
    for j in np.flatnonzero(count == 0):
        for r in rng.permutation(n):
            cand = [c for c in rows[r] if c >= first and count[c] > 1]
            if cand:
                c = cand[0]
                rows[r] = np.sort(np.where(rows[r] == c, j, rows[r]))
                count[c] -= 1
                count[j] += 1
                break
        else:
            raise ValueError("no row can give column %d an entry" % j)
    ri = np.concatenate([np.full(len(c), r, dtype=np.int64) for r, c in enumerate(rows)])
    ci = np.concatenate(rows)
    kind = rng.integers(0, 3, size=ci.size)
    vals = np.where(kind == 0, 1.0, np.where(kind == 1, 0.3, 0.1 * rng.standard_normal(ci.size) + rng.choice([-0.4, 0.4], ci.size)))
    if intercept:
        vals[ci == 0] = 1.0
    if single is not None:
        hit = np.flatnonzero(ci == single)
        keep = np.ones(ci.size, dtype=bool)
        keep[hit[1:]] = False
        ri, ci, vals = ri[keep], ci[keep], vals[keep]
    A = sp.csc_matrix((vals, (ri, ci)), shape=(n, p))
    A.sort_indices()
    assert np.diff(A.indptr).min() >= 1
    return A


def row_lengths(A):
    return np.diff(sp.csc_matrix(A.T).indptr)


def logistic_setup(A, seed, gamma0=GAMMA0, droptol=1e-2):
    """What problems.logistic_problem does after sparse_design (scripts/logistic.jl:21-158), for any design: y ~ Bernoulli(sigmoid(A xtrue)),
    the Newton mode μ, the Hessian Γ at μ, Γdrop (droptol 1e-2), σ = sqrt(diag(inv Γ)), c = 0.01."""
    rng = np.random.default_rng(seed)
    A = sp.csc_matrix(A)
    A.sort_indices()
    n, p = A.shape
    xtrue = 5 * rng.standard_normal(p)
    sig = lambda u: 1.0 / (1.0 + np.exp(-u))  # noqa: E731
    y = (rng.random(n) < sig(A @ xtrue)).astype(np.float64)
    ny = 1.0 - y
    x = 0.1 * rng.random(p)
    At = sp.csc_matrix(A.T)
    At.sort_indices()
    for _ in range(30):
        u = A @ x
        g = gamma0 * x - A.T @ (y * sig(-u)) + A.T @ (ny * sig(u))
        H = gamma0 * sp.identity(p, format="csc") + (A.T @ sp.diags(sig(u) * sig(-u)) @ A)
        x = x - np.linalg.solve(H.toarray(), g)
    mu = x
    u = A @ mu
    g = gamma0 * mu - A.T @ (y * sig(-u)) + A.T @ (ny * sig(u))
    assert np.all(np.isfinite(mu)) and np.linalg.norm(g) <= 1e-8 * (1.0 + np.linalg.norm(mu)), "Newton did not reach the mode"
    G = sp.csc_matrix(gamma0 * sp.identity(p, format="csc") + (A.T @ sp.diags(sig(u) * sig(-u)) @ A))
    G = sp.csc_matrix((G + G.T) * 0.5)
    Gd = G.copy()
    Gd.data[np.abs(Gd.data) <= droptol] = 0.0
    Gd.eliminate_zeros()
    Gd.sort_indices()
    sigma = np.sqrt(np.diag(np.linalg.inv(G.toarray())))
    return dict(A=A, At=At, y=y, ny=ny, mu=mu, gamma0=gamma0, G=G, Gdrop=Gd, sigma=sigma, x0=mu.copy(), c=0.01 * np.ones(p), n=n, p=p)


# -------------------------------------------------------------------------------------------------------------------------------- cases

def _pkg():
    from __graft_entry__ import load_package
    return load_package()


def _sd(levels, r, m, seed, empty=0):
    """scripts/sparsedesign.jl's mock design; empty: that many rows without a regressor appended (observations no column refers to)."""
    def make():
        A = _pkg().problems.sparse_design(levels, r, m, np.random.default_rng(seed))
        if empty:
            A = sp.vstack([A, sp.csc_matrix((empty, A.shape[1]))], format="csc")
            A.sort_indices()
        return A
    return make


def _rd(n, p, lens, intercept, seed, single=None):
    return lambda: random_design(n, p, lens, intercept, seed, single)


ALL = (1, 2, 3, 4, 5, 6)
SINGLE = 37  # case h: the column cut down to one observation
# name: (design, k_sub, horizon T − t0, t0, row lengths the line names, kernel family, options)
#   options: cap / cuts = trace capacity and slice boundaries (as fractions of the horizon) of a run in slices; tail = the last launch
#   runs the reference's tail (RUN_REFERENCE_TAIL: the first event at or past T is processed) -- no ∫x dt can be read then
_T = {
    "a":    (_sd((2, 3), 1, 40, 11), 1, 30.0, 0.0, (1, 2, 4), "lds", dict(tail=True)),
    "b":    (_sd((4, 4, 4), 0, 20, 12, empty=60), 7, 20.0, 2.5, (0, 1, 3, 6), "lds", dict(cap=48, cuts=(0.3, 0.55))),
    "c":    (_sd((7, 8), 1, 20, 13), 32, 10.0, 0.0, (2, 4), "lds", {}),
    "d":    (_rd(2000, 65, ALL, True, 14), 31, 10.0, 0.0, ALL, "lds", dict(cap=40, cuts=(0.25, 0.7))),
    "e":    (_rd(3000, 129, ALL, False, 15), 3, 10.0, 2.5, ALL, "lds", {}),
    "f":    (_rd(8000, 511, ALL, True, 16), 13, 3.0, 0.0, ALL, "lds", {}),
    "g":    (_rd(8000, 512, ALL, False, 17), 32, 3.0, 0.0, ALL, "general", {}),
    "g511": (_rd(8000, 511, ALL, False, 17), 32, 3.0, 0.0, ALL, "lds", {}),
    "h":    (_rd(1500, 70, ALL, False, 18, single=SINGLE), 9, 10.0, 0.0, ALL, "lds", {}),
    "i":    (_rd(3000, 129, ALL, False, 15), 20, 10.0, 0.0, ALL, "lds", {}),
    "j63":  (_rd(1200, 63, (2, 3, 5), False, 19), 2, 10.0, 0.0, (2, 3, 5), "lds", {}),
    "j64":  (_rd(1200, 64, (1, 4), True, 20), 10, 10.0, 0.0, (1, 4), "lds", dict(cap=0, tail=True)),
    "j128": (_rd(2500, 128, (3, 6), False, 21), 2, 10.0, 0.0, (3, 6), "lds", {}),
    "k":    (_sd((3, 3, 3), 2, 20, 22), 5, 10.0, 0.0, (3, 5, 8), "general", {}),
    "l":    (_rd(8000, 513, ALL, False, 17), 10, 3.0, 0.0, ALL, "general", {}),
    "m":    (_sd((7, 8), 1, 20, 13), 33, 10.0, 0.0, (2, 4), "general", dict(tail=True)),
}
NAMES = list(_T)
LDS_NAMES = [n for n in NAMES if _T[n][5] == "lds"]
GENERAL_NAMES = [n for n in NAMES if _T[n][5] == "general"]
ROWS_DK_MAX, LDS_DK_MAX = 448, 512


def dk_of(d):
    """Length of the key array: d coordinates and the refresh clock, in blocks of 64."""
    return 64 * ((d + 1 + 63) // 64)


def lds_takes(P):
    """zz_logistic_lds_supported (pdmp_logistic.hip), as far as the shape decides it."""
    return dk_of(P["p"]) <= LDS_DK_MAX and 1 <= P["ksub"] <= 32 and int(row_lengths(P["A"]).max()) <= 6


def rows_fit(P, W):
    """zz_logistic_rows_supported (pdmp_logrows.hip)."""
    return P["kernel"] == "lds" and dk_of(P["p"]) <= ROWS_DK_MAX and P["ksub"] + 2 <= W


@functools.lru_cache(maxsize=None)
def _setup(name):
    design, *_ = _T[name]
    return logistic_setup(design(), seed=7900 + NAMES.index(name))


def state_of(S, seed, nch=NCH):
    """x0 near the mode, θ0 = ±σ."""
    rng = np.random.default_rng(seed)
    p = S["p"]
    return S["mu"] + 0.05 * S["sigma"] * rng.standard_normal((nch, p)), S["sigma"] * rng.choice([-1.0, 1.0], (nch, p))


@functools.lru_cache(maxsize=None)
def problem(name):
    _, ksub, h, t0, lens, kernel, opt = _T[name]
    P = dict(_setup(name))
    x0, th0 = state_of(P, 8000 + NAMES.index(name))
    P.update(name=name, ksub=ksub, t0=t0, T=t0 + h, lens=lens, kernel=kernel, cap=opt.get("cap", 4096), cuts=tuple(t0 + f * h for f in opt.get("cuts", ())),
             tail=opt.get("tail", False), X0=x0, TH0=th0, seeds=np.uint64(8100 + 10 * NAMES.index(name)) + np.arange(NCH, dtype=np.uint64))
    return P


def guard_case(P, rs):
    """Not vacuous: every chain healthy, at least 150 events, at least 64 proposals (every value goff = (k_sub · proposal) mod the refill
    period can take has then occurred: the sequence is deterministic)."""
    for r in rs:
        assert r["status"] == 0, (P["name"], r["status"])
        assert len(r["events"]) >= 150 and r["num"] >= 64, (P["name"], len(r["events"]), r["num"])
    if P["cuts"]:
        assert min(len(r["events"]) for r in rs) >= 3 * P["cap"], (P["name"], P["cap"])  # the trace buffer refills three times at least


def lg_of(P, ksub=None):
    return dict(A=P["A"], At=P["At"], y=P["y"], ny=P["ny"], mu=P["mu"], gamma0=P["gamma0"], k=P["ksub"] if ksub is None else ksub)


def oracle_run(P, k, *, tracked=False, adapt=True, c=None, want_trace=True):
    return O.spdmp_zigzag(P["Gdrop"], P["mu"], P["Gdrop"], P["X0"][k], P["TH0"][k], P["c"] if c is None else c, P["T"], t0=P["t0"],
                          seed=int(P["seeds"][k]), adapt=adapt, factor=FACTOR, logistic=lg_of(P), sigma=P["sigma"], stop_before_T=not P["tail"],
                          tracked=tracked, want_trace=want_trace)


@functools.lru_cache(maxsize=None)
def refs(name, tracked=False):
    """The oracle's chains of a case, computed once per session and never written to."""
    P = problem(name)
    return tuple(oracle_run(P, k, tracked=tracked) for k in range(NCH))


# ---------------------------------------------------------------------------------------------------------------------- violation state

VIOLATION_NCH = 6
VIOLATION_C = {"a": 40.0, "d": 20.0}


@functools.lru_cache(maxsize=None)
def violation_problem(name):
    """Case `name` with adapt = false, six chains and a uniform c at which some chains run into a bound violation late, others never."""
    P = dict(problem(name))
    x0, th0 = state_of(P, 8300 + NAMES.index(name), VIOLATION_NCH)
    P.update(X0=x0, TH0=th0, c=np.full(P["p"], VIOLATION_C[name]), tail=True, cap=8192, cuts=(),
             seeds=np.uint64(8400 + 10 * NAMES.index(name)) + np.arange(VIOLATION_NCH, dtype=np.uint64))
    return P


@functools.lru_cache(maxsize=None)
def violation_refs(name):
    P = violation_problem(name)
    return tuple(oracle_run(P, k, adapt=False) for k in range(VIOLATION_NCH))


def guard_violation(refs):
    late = [r for r in refs if r["status"] == O.ORC_BOUND_VIOLATED and len(r["events"]) >= 20]
    assert len(late) >= 2, [(r["status"], len(r["events"])) for r in refs]
    assert all(r["status"] in (O.ORC_OK, O.ORC_BOUND_VIOLATED) for r in refs)


# ------------------------------------------------------------------------------------------------------------------------------- stress

STRESS_N = 12


@functools.lru_cache(maxsize=None)
def stress_problem(case):
    """One seeded draw: p in 8..512, the row-length set, intercept or not, k_sub in 1..32, tracked or not, integrals or not, t0, a trace
    buffer of 24..160 events and up to three slice boundaries."""
    rng = np.random.default_rng(9000 + case)
    # (uniform, or log-uniform for as many draws below one slot of 64 as above four)
    p = int(rng.integers(8, 513)) if rng.integers(0, 2) else min(512, int(round(8.0 * 64.0 ** rng.random())))
    intercept = bool(rng.integers(0, 2))
    lens = tuple(sorted(set(int(v) for v in rng.choice(np.arange(0, min(6, p) + 1), size=int(rng.integers(1, 5)), replace=False))))
    if max(lens) < (2 if intercept else 1):  # (rows that can hold a regressor beside the intercept)
        lens = lens + (min(3, p),)
    ksub = int(rng.integers(1, 33))
    tracked, integrals = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    t0 = float(rng.choice([0.0, 2.5, rng.uniform(0.0, 5.0)]))
    n = int(p * rng.uniform(12.0, 25.0)) + 40
    P = dict(logistic_setup(random_design(n, p, lens, intercept, 9100 + case), seed=9200 + case))
    h = min(25.0, 600.0 / p)
    x0, th0 = state_of(P, 9300 + case)
    lds = dk_of(p) <= LDS_DK_MAX
    P.update(name="stress%d" % case, ksub=ksub, t0=t0, T=t0 + h, lens=lens, intercept=intercept, kernel="lds" if lds else "general",
             tracked=tracked and lds, integrals=integrals, tail=not integrals, cap=int(rng.integers(24, 160)),
             cuts=tuple(np.sort(t0 + h * rng.random(int(rng.integers(0, 4)))).tolist()), X0=x0, TH0=th0,
             seeds=np.uint64(9400 + 10 * case) + np.arange(NCH, dtype=np.uint64))
    return P


@functools.lru_cache(maxsize=None)
def stress_refs(case):
    P = stress_problem(case)
    return tuple(oracle_run(P, k, tracked=P["tracked"]) for k in range(NCH))


# --------------------------------------------------------------------------------------------------------------------- the device's side

LDS_KERNEL, GENERAL_KERNEL, ROWS_KERNEL = "zz_logistic_lds_kernel", "zz_general_run_kernel", "zz_logistic_rows_kernel"


def open_ensemble(pk, P, *, kernel="auto", rows=0, tracked=False, integrals=True, adapt=True, ksub=None):
    """An ensemble on problem P up to (not including) set_state; the caller closes it."""
    ens = pk.Ensemble(P["X0"].shape[0], P["p"], adapt=adapt, factor=FACTOR, trace_capacity=P["cap"])
    try:
        ens.debug_set_kernel(kernel)
        if rows:
            ens.debug_set_logistic_rows(rows)
        ens.set_flow(pk.ZigZag(P["Gdrop"], P["mu"], P["sigma"]))
        ens.set_target(pk.LogisticTarget(P["A"], P["y"], P["ny"], P["mu"], P["gamma0"], P["ksub"] if ksub is None else ksub))
        ens.set_path_integrals(integrals)
        ens.set_gradient_tracking(tracked)
    except Exception:
        ens.close()
        raise
    return ens


def device_run(pk, P, **form):
    """The chains of P on the device, in P's slices, the trace drained whenever it fills: counters, events, final state, ∫x dt of every
    coordinate (where the form keeps it and the run ends before T), the kernel's name and the number of launches."""
    L = pk._lib
    nch = P["X0"].shape[0]
    with open_ensemble(pk, P, **form) as ens:
        ens.set_state(P["t0"], P["X0"], P["TH0"], P["c"], P["seeds"])
        evs = [[] for _ in range(nch)]
        launches = 0
        names = set()
        for Tk, flag in [(v, L.RUN_STOP_BEFORE) for v in P["cuts"]] + [(P["T"], L.RUN_REFERENCE_TAIL if P["tail"] else L.RUN_STOP_BEFORE)]:
            while True:
                ens.run(Tk, flag)
                launches += 1
                names.add(ens.kernel_name())
                cnt = ens.counters()
                for k in range(nch):
                    if P["cap"] and cnt["ntrace"][k]:
                        evs[k].append(ens.trace(k, counters=cnt))
                ens.trace_reset()
                if not L.needs_rerun(cnt["status"]):
                    break
        pj = ens.path_integrals(P["T"], np.arange(P["p"])) if form.get("integrals", True) and not P["tail"] else None
        assert len(names) == 1, names
        return dict(cnt=cnt, evs=[np.concatenate(e) if e else np.empty(0, dtype=L.EVENT_DTYPE) for e in evs], fs=ens.final_state(), pj=pj,
                    kernel=names.pop(), launches=launches)


def compare_with_oracle(what, P, run, rs):
    """Bit for bit: events (i, t, x, θ), num, acc, the adapted c, final (t, x, θ), both stream positions."""
    cnt, fs = run["cnt"], run["fs"]
    for k, r in enumerate(rs):
        w = (what, k)
        assert cnt["status"][k] == 0 and r["status"] == 0, w
        if P["cap"]:
            ev = run["evs"][k]
            assert len(ev) == len(r["events"]), (w, len(ev), len(r["events"]))
            for f in ("i", "t", "x", "theta"):
                assert np.array_equal(ev[f], r["events"][f]), (w, f)
        assert (int(cnt["num"][k]), int(cnt["nacc"][k])) == (r["num"], r["nacc"]), (w, cnt["num"][k], r["num"])
        assert (int(cnt["ndraw_main"][k]), int(cnt["ndraw_global"][k])) == (r["ndraw_main"], r["ndraw_global"]), w
        for f in ("t", "x", "theta", "acc", "c"):
            assert np.array_equal(fs[f][k], r[f]), (w, f)
