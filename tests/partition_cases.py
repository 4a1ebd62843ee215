"""The case table of zz_partitioned_run_kernel (csrc/pdmp_partition.hip, parallel_spdmp on the device: one chain over a workgroup of K wavefronts):
one table for tests/test_partition_cases_ref.py (the oracle alone, no device) and tests/test_gpu_partition_cases.py (the device against it, bit
for bit).  TEST INFRASTRUCTURE ONLY; numpy and scipy, no device.

What the kernel does depends on
  k = d / K   nbc = ceil(k / 64) key blocks per chunk: a partial last block (k % 64 != 0), nbc > 64 (the strided loop of peek), k = 1;
  K           1 (no border, no waiting), a power of two or not, 16 (the most);
  |G[i]|      one neighbour per lane, up to 64; members of G[i] outside G1[i] are moved, not re-bounded (explicit zeros of the bound, g1mask);
  |G2[i]|     two-hop(G1) without G, moved on an accepted event in passes of 64;
  the bound   with the chunk-diagonal of the TARGET's Γ as the bounding Γ the affine bound of an inner coordinate (all of G[i] inside its chunk)
              is exact, l = lb − c − c·Δt/100 < lb: worker waves can then neither violate nor adapt, only the coordinator can, on a border
              coordinate.  The weak_* cases halve the bound's values so that the workers do both;
  μ           of the target (gmu_t) and of the bound (gmu_b);
  t0          the reference enqueues the first times without t0 (src/parallel.jl:132-136);
  the end     a violation raised by a worker (the chunk parks for good at +Inf) or by the coordinator, a full trace, no trace.

The table, case x what it reaches.  test_partition_cases_ref.py asserts what a row claims and prints, with -s, the oracle's accepted events,
coordinator rounds and chunk-rounds spent waiting (rounds·K − spawns) of every case.

  case            shape                                   what it reaches
  tri_K1          tridiagonal d = 4160, K = 1             nbc = 65 (strided peek), no border, few rounds
  tri_K2_long     tridiagonal d = 8320, K = 2             nbc = 65 with a border
  tri_K7          tridiagonal d = 700, K = 7, k = 100     partial last block with nbc = 2, odd K
  tri_k1          tridiagonal d = 16, K = 16              k = 1: every coordinate is the coordinator's
  tri_k3_bigΔ     d = 48, K = 16, Δ = 50                  the horizon is never the reason to park
  tri_k3_tinyΔ    d = 48, K = 16, Δ = 1e-4                the horizon is always the reason to park: one look at the queue per wake
  band31_K3       bandwidth 31, d = 192, K = 3            kG = 63, most coordinates on the border, thousands of waits
  dense64_K4      four dense 64 x 64 blocks, d = 256      kG = 64 exactly, G2 = ∅, no border at all
  rand12_K2       ~12 random in-chunk neighbours per column + 6 cross-chunk links, k = 256: max |G2[i]| > 64
  rand12_K3_mu    the same with K = 3 and 9 links, target μ != 0 and bound μ != target μ
  tri_K7_t0neg    tri_K7 with t0 = −2.5, T = 1            } the reference's un-offset first times: the first events lie
  tri_K7_t0pos    tri_K7 with t0 = 0.75, T = 3.25         } at 0+, beyond t0 + Δ resp. before t0
  wide_G          16 x 16 lattice, K = 4, explicit G = pattern of (bound Γ)² ∪ the target's: explicit zeros, g1mask skips in ab, G2 = ∅
  weak_adapt      tri_K7, bound values x 0.5, c = 0.05‖Γ‖, adapt: adapt! from worker waves and from the coordinator
  weak_violate    the same bound, c = 1.5‖Γ‖ inside and 3‖Γ‖ on the border, Δ = 50: stopped by a violation raised in a WORKER
  border_violate  bound = chunk-diagonal of the target, c = 0.5‖Γ‖, no adapt: a violation raised in the coordinator
  overflow        tri_K7 with trace_capacity = 64         TRACE_FULL, the run still completes
  no_trace        tri_K7 with trace_capacity = 0          nevents = nacc
  ensemble        rand12_K2 with 8 chains                 several workgroups at once

weak_violate, why a worker: a worker parks on a border coordinate or on a head beyond its horizon tnext, and the coordinator proposes what the
workers parked on.  With Δ = 50 > T no head before T lies beyond a horizon (a tridiagonal bound has b_j >= c_j/100 + 1 − 0.8·0.5 > 0.6, so a
waiting time above 47 has probability < exp(−0.3·47²)), so the coordinator proposes border coordinates only and every inner coordinate is a
worker's.  The census asserts that the same inputs with adapt=True raise c at inner coordinates only: every violation is then a worker's.
weak_violate, why these inputs: the chunk that raised the violation parks at +Inf, so the coordinator of that (final) round visits it last and
skips it.  Parked at the proposal's own time instead, it would be sorted into its place and proposed once more, on the coordinator's stream:
that proposal moves nothing (dt = 0) and violates again, but it takes one draw, so every chunk visited after it in that round gets its border
proposal with the next uniform of the stream, and shows it wherever that flips an accept.  With a large c on the border (50‖Γ‖, say) hardly
any border proposal is accepted and the difference cannot show; the census asserts that this row's coordinator does accept.  That the FINAL
round holds such a proposal cannot be asserted from the oracle's result: c on the border and the seed were picked by running variants of the
row through the oracle with and without that one change and keeping one whose results differ (in events, x, t and nacc).  If the row's
inputs change, pick them again the same way."""
import functools

import numpy as np
import scipy.sparse as sp

import oracle_lib as O

OK, VIOLATED, TRACE_FULL = "ok", "violated", "trace_full"  # the expected end of a case (device: PDMP_CHAIN_OK / BOUND_VIOLATED / TRACE_FULL)
MIN_EVENTS = 100


# ------------------------------------------------------------------------------------------------------------------------------- graphs

def _csc(G):
    G = sp.csc_matrix(G, dtype=np.float64)
    G.sort_indices()
    return G


def chunk_diagonal(G, K):
    """The bounding Γ of test/testparallel.jl:40-47: the target's Γ without the entries that couple two chunks."""
    d = G.shape[0]
    k = d // K
    coo = sp.coo_matrix(G)
    keep = (coo.row // k) == (coo.col // k)
    G2 = sp.csc_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), shape=G.shape)
    G2.sort_indices()
    return G2


def pattern(A):
    """The structural pattern of A as a matrix of ones (explicit zeros count, as in Julia's rowvals / nzrange)."""
    A = sp.csc_matrix(A)
    P = sp.csc_matrix((np.ones(A.nnz), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    P.sort_indices()
    return P


def on_pattern(A, P):
    """A's values on P's pattern (⊇ A's), explicit zeros elsewhere: how a matrix is handed to the oracle together with an explicit G."""
    P = pattern(P)
    cols = np.repeat(np.arange(P.shape[1]), np.diff(P.indptr))
    vals = np.asarray(sp.csc_matrix(A)[P.indices, cols]).reshape(-1)
    return sp.csc_matrix((vals, P.indices.copy(), P.indptr.copy()), shape=P.shape)


def g2_sizes(G1, G):
    """|G2[i]|, G2[i] = ∪_{j ∈ G1[i]} G1[j] without G[i] (src/parallel.jl:121), per column."""
    P1, PG = pattern(G1), pattern(G)
    two = pattern(P1 @ P1)
    return np.asarray((two - two.multiply(PG)).astype(bool).sum(axis=0)).reshape(-1)


def inner_mask(G, K):
    """inner[i]: all of G[i] lies in i's chunk (src/parallel.jl:114)."""
    k = G.shape[0] // K
    coo = sp.coo_matrix(pattern(G))
    out = np.ones(G.shape[0], dtype=bool)
    out[coo.col[(coo.row // k) != (coo.col // k)]] = False
    return out


def column_norms(G):
    return np.sqrt(np.asarray(sp.csc_matrix(G).multiply(G).sum(axis=0)).reshape(-1))


def tridiagonal(d):
    """test/testparallel.jl:22-38: 1 on the diagonal, −0.4 beside it."""
    return _csc(sp.diags([np.ones(d), -0.4 * np.ones(d - 1), -0.4 * np.ones(d - 1)], [0, 1, -1]))


def banded(d, bw):
    """Bandwidth bw, diagonally dominant: Γ_ij = −0.6 / (bw (1 + |i − j|)) off the diagonal."""
    offs = [o for o in range(-bw, bw + 1) if o != 0]
    return _csc(sp.diags([np.ones(d)] + [np.full(d - abs(o), -0.6 / (bw * (1 + abs(o)))) for o in offs], [0] + offs))


def dense_blocks(nb, m, seed):
    """nb dense m x m blocks B Bᵀ/m + I on the diagonal, nothing between them."""
    rng = np.random.default_rng(seed)
    blocks = []
    for _ in range(nb):
        B = rng.standard_normal((m, m))
        blocks.append(B @ B.T / m + np.eye(m))
    return _csc(sp.block_diag(blocks))


def random_chunks(K, k, per_col, links, seed):
    """K chunks of k coordinates: every column draws per_col / 2 partners inside its chunk (symmetrised: about per_col neighbours), `links` pairs
    couple coordinates of different chunks; off-diagonal values in ±(0.02, 0.06), the diagonal 1 + the column's absolute sum."""
    rng = np.random.default_rng(seed)
    d = K * k
    rows, cols = [], []
    for i in range(d):
        base = (i // k) * k
        p = base + rng.choice(k, per_col // 2, replace=False)
        p = p[p != i]
        rows.extend(p)
        cols.extend([i] * len(p))
    for _ in range(links):
        a, b = rng.choice(K, 2, replace=False)
        rows.append(a * k + rng.integers(k))
        cols.append(b * k + rng.integers(k))
    A = sp.csc_matrix((np.ones(len(rows)), (rows, cols)), shape=(d, d))
    A = sp.triu(pattern(A + A.T), 1).tocoo()
    v = rng.uniform(0.02, 0.06, A.nnz) * rng.choice([-1.0, 1.0], A.nnz)
    S = sp.csc_matrix((v, (A.row, A.col)), shape=(d, d))
    S = S + S.T
    return _csc(S + sp.diags(1.0 + np.asarray(abs(S).sum(axis=0)).reshape(-1)))


def lattice(n):
    """n x n grid Laplacian + 0.5 I (the stencil of problems.gmrf_precision)."""
    T1 = sp.diags([2.0 * np.ones(n), -np.ones(n - 1), -np.ones(n - 1)], [0, 1, -1])
    I = sp.identity(n)
    return _csc(sp.kron(I, T1) + sp.kron(T1, I) + 0.5 * sp.identity(n * n))


# -------------------------------------------------------------------------------------------------------------------------------- cases
# name: dict(graph=(builder, args...), K, T and the options below).  kG = max |G[i]| and g2 = max |G2[i]| are the row's claims (asserted by the
# census on the built inputs); links: does the pattern couple chunks (then some chunk must have waited).
_DEFAULTS = dict(
    delta=0.1, t0=0.0, xscale=1.0, cscale=2.0,   # x0 = xscale·N(0, 1), c = cscale·‖Γt[:, i]‖·(0.9 + 0.2 U)
    bscale=1.0,                                   # the bounding Γ = bscale · chunk_diagonal(target Γ)
    mu_t=0.0, mu_b=0.0,                           # target μ = mu_t·N(0, 1) (0: none); bound μ = target μ + mu_b·N(0, 1) (0: zeros)
    wide=False,                                   # explicit G = pattern((bound Γ)²) ∪ the target's
    cborder=None,                                 # c on the border coordinates = cborder·‖Γt[:, i]‖ (None: cscale, like the rest)
    adapt=False, factor=1.8, nchains=1, trace_capacity=8192, expect=OK, links=True)

_TRI_K7 = dict(graph=(tridiagonal, 700), K=7, T=2.5, seed=107, kG=3, g2=2)

CASES = {
    "tri_K1": dict(graph=(tridiagonal, 4160), K=1, T=0.5, seed=101, kG=3, g2=2, links=False, delta=0.2),
    "tri_K2_long": dict(graph=(tridiagonal, 8320), K=2, T=0.4, seed=102, kG=3, g2=2),
    "tri_K7": dict(_TRI_K7),
    "tri_k1": dict(graph=(tridiagonal, 16), K=16, T=40.0, seed=104, kG=3, g2=0),
    "tri_k3_bigΔ": dict(graph=(tridiagonal, 48), K=16, T=15.0, seed=105, kG=3, g2=1, delta=50.0),
    "tri_k3_tinyΔ": dict(graph=(tridiagonal, 48), K=16, T=15.0, seed=106, kG=3, g2=1, delta=1e-4),
    "band31_K3": dict(graph=(banded, 192, 31), K=3, T=6.0, seed=108, kG=63, g2=31),
    "dense64_K4": dict(graph=(dense_blocks, 4, 64, 9), K=4, T=3.0, seed=109, kG=64, g2=0, links=False),
    "rand12_K2": dict(graph=(random_chunks, 2, 256, 12, 6, 21), K=2, T=2.0, seed=110, kG=21, g2=141),
    "rand12_K3_mu": dict(graph=(random_chunks, 3, 256, 12, 9, 22), K=3, T=1.5, seed=111, kG=19, g2=145, mu_t=0.7, mu_b=0.1),
    "tri_K7_t0neg": dict(_TRI_K7, t0=-2.5, T=1.0, seed=112),
    "tri_K7_t0pos": dict(_TRI_K7, t0=0.75, T=3.25, seed=113),
    "wide_G": dict(graph=(lattice, 16), K=4, T=3.0, seed=114, kG=12, g2=0, wide=True),
    "weak_adapt": dict(_TRI_K7, bscale=0.5, cscale=0.05, xscale=3.0, adapt=True, seed=115),
    "weak_violate": dict(_TRI_K7, bscale=0.5, cscale=1.5, cborder=3.0, delta=50.0, T=40.0, expect=VIOLATED, seed=201),
    "border_violate": dict(_TRI_K7, cscale=0.5, T=40.0, expect=VIOLATED, seed=117),
    "overflow": dict(_TRI_K7, trace_capacity=64, expect=TRACE_FULL, seed=118),
    "no_trace": dict(_TRI_K7, trace_capacity=0, seed=119),
    "ensemble": dict(graph=(random_chunks, 2, 256, 12, 6, 21), K=2, T=2.0, seed=120, kG=21, g2=141, nchains=8),
}
NAMES = tuple(CASES)


class Case:
    """The built inputs of one row: target Γt / μt, bounding Γb / μb, G (None: the bound's pattern ∪ the target's), the state and the options."""

    def __init__(self, name, **over):
        """over: options that replace the row's (a variant of the row; the table itself is never written to)."""
        o = dict(_DEFAULTS)
        o.update(CASES[name])
        o.update(over)
        self.name, self.opt = name, o
        self.K, self.delta, self.t0, self.T = o["K"], o["delta"], o["t0"], o["T"]
        self.adapt, self.factor, self.seed, self.nchains = o["adapt"], o["factor"], o["seed"], o["nchains"]
        self.trace_capacity, self.expect, self.links = o["trace_capacity"], o["expect"], o["links"]
        self.Gt = o["graph"][0](*o["graph"][1:])
        self.d = d = self.Gt.shape[0]
        self.k = d // self.K
        cd = chunk_diagonal(self.Gt, self.K)
        self.Gb = _csc(cd * o["bscale"])
        rng = np.random.default_rng(self.seed)
        self.x0 = o["xscale"] * rng.standard_normal((self.nchains, d))
        self.th0 = rng.choice([-1.0, 1.0], (self.nchains, d))
        nrm = column_norms(self.Gt)
        self.G = _csc(pattern(pattern(self.Gb) @ pattern(self.Gb)) + pattern(self.Gt)) if o["wide"] else None
        self.Gfull = pattern(self.G if self.G is not None else pattern(self.Gb) + pattern(self.Gt))  # G as the kernel and the oracle see it
        self.inner = inner_mask(self.Gfull, self.K)
        self.c = o["cscale"] * nrm * (0.9 + 0.2 * rng.random(d))
        if o["cborder"] is not None:
            self.c[~self.inner] = o["cborder"] * nrm[~self.inner]
        self.mu_t = o["mu_t"] * rng.standard_normal(d) if o["mu_t"] else None
        self.mu_b = (0.0 if self.mu_t is None else self.mu_t) + o["mu_b"] * rng.standard_normal(d) if o["mu_b"] else None
        self.kG = int(np.diff(self.Gfull.indptr).max())
        self.g2 = int(g2_sizes(self.Gb, self.Gfull).max())

    def oracle(self, chain=0, **over):
        """The oracle's run of one chain (seed + chain, like the device's ensemble); over: adapt=..., target_mu=..., bound_mu=..., T=... replace the case's."""
        kw = dict(t0=self.t0, adapt=self.adapt, factor=self.factor, seed=self.seed + chain, target_mu=self.mu_t)
        T, mu_b = over.pop("T", self.T), over.pop("bound_mu", self.mu_b)
        kw.update(over)
        Gt = self.Gt if self.G is None else on_pattern(self.Gt, self.Gfull)  # (the oracle's G is the pattern of the target matrix it is given)
        return O.parallel_spdmp(self.Gb, mu_b, Gt, self.x0[chain], self.th0[chain], self.c, T, self.K, self.delta, **kw)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def reference(name, chain=0):
    """The oracle's result of a case's chain: computed once, shared by the tests, never written to."""
    r = case(name).oracle(chain)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def expected_status(case_):
    return {OK: O.ORC_OK, VIOLATED: O.ORC_BOUND_VIOLATED, TRACE_FULL: O.ORC_OK}[case_.expect]  # (the oracle's trace has no capacity)


def waits(r, K):
    """Chunk-rounds spent waiting for a neighbouring chunk: rounds·K − spawns."""
    return int(r["rounds"]) * K - int(r["spawns"])


# ---------------------------------------------------------------------------------------------------------------------------- path check
def check_path(t0, x0, th0, events, t_end, x_end, th_end, m):
    """A trace and a final state against the path they describe, in rationals (exact_path.ExactPath), with no second implementation involved:
    between consecutive own events of a coordinate, and from its last event to its final (t_i, x_i), the recorded position is
    x_k + θ_k (t_{k+1} − t_k) up to 2u·X_i·m -- one move costs 2u·X_i and a coordinate moves at most m = num + nevents + 1 times (exact_path's
    docstring) -- with X_i the largest |x_i| on the path; every recorded θ is exactly the negative of the one before, the final θ the last one.
    events: time-sorted, complete.  Returns the largest error / bound ratio (for reports; the bound is asserted here)."""
    from fractions import Fraction

    from exact_path import U, ExactPath
    P = ExactPath(t0, x0, th0)
    d = len(x0)
    err = [Fraction(0)] * d
    for e in events:
        i = int(e["i"])
        want = P.x[i] + P.th[i] * (Fraction(float(e["t"])) - P.t[i])
        err[i] = max(err[i], abs(Fraction(float(e["x"])) - want))
        assert float(e["theta"]) == -float(P.th[i]), "coordinate %d: θ = %r after %r at t = %r" % (i, float(e["theta"]), float(P.th[i]), float(e["t"]))
        P.feed([e])
    worst = 0.0
    for i in range(d):
        want = P.x[i] + P.th[i] * (Fraction(float(t_end[i])) - P.t[i])
        err[i] = max(err[i], abs(Fraction(float(x_end[i])) - want))
        assert float(th_end[i]) == float(P.th[i]), "coordinate %d: final θ" % i
        X = max(P.X[i], abs(float(x_end[i])))
        bound = 2 * U * Fraction(X) * int(m)
        assert err[i] <= bound, "coordinate %d: off its own path by %.3e, allowed %.3e" % (i, float(err[i]), float(bound))
        if bound > 0:
            worst = max(worst, float(err[i] / bound))
    return worst


def stopping_proposal(c, r, ra):
    """(i, t) of the worker's proposal that stopped the run r (no adapt, a violated bound), told from r and ra, the same inputs with adapt=True.
    For a case whose coordinator proposes border coordinates only (Δ beyond T): inner coordinates are then the workers' alone, and the workers
    of r did what those of ra did up to the stop, where ra adapted and went on.  The violated proposal is an (adapted) inner event of ra that
    r lacks.  A worker takes its chunk's coordinates in the order of their times, so in the chunk that raised the violation the earliest inner
    event that r lacks is that proposal, and r has moved its coordinate to its time without recording it (final t_i = the event's time); in
    every other chunk r stopped before its earliest missing event, and that coordinate's final time is earlier.  None unless exactly one
    chunk qualifies."""
    have = set(map(tuple, r["events"].tolist()))
    missing = np.array([e for e in ra["events"].tolist() if tuple(e) not in have], dtype=ra["events"].dtype)
    missing = missing[c.inner[missing["i"]]]
    hits = []
    for v in range(c.K):
        mv = missing[missing["i"] // c.k == v]
        if len(mv):
            e = mv[np.argmin(mv["t"])]
            if r["t"][e["i"]] == e["t"]:
                hits.append((int(e["i"]), float(e["t"])))
    return hits[0] if len(hits) == 1 else None
