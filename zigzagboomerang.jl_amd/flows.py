"""Parameter carriers mirroring the reference's dynamics descriptors (src/types.jl).

The reference passes a gradient closure ∇ϕ; a closure cannot cross the C ABI, so targets are an
enumerated set of device-resident families (GaussianTarget so far: the closure of
scripts/gaussianrandomfield.jl:25 and test/maintest.jl:9).
"""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import scipy.sparse as sp


def _csc(A):
    A = sp.csc_matrix(A, dtype=np.float64)
    A.sort_indices()
    A.sum_duplicates()
    return A


@dataclass
class ZigZag:
    """ZigZag(Γ, μ, σ=diag(Γ).^(-0.5); λref=0.0, ρ=0.0)  -- src/types.jl:19-27.

    Γ is the sparse precision used for the affine bounds (and whose column pattern defines the local
    neighbourhoods G1/G2, src/sfact.jl:170-179); μ the approximate target mean.
    """
    Γ: sp.csc_matrix
    μ: np.ndarray
    σ: Optional[np.ndarray] = None
    λref: float = 0.0
    ρ: float = 0.0

    def __post_init__(self):
        self.Γ = _csc(self.Γ)
        self.μ = np.ascontiguousarray(self.μ, dtype=np.float64)
        if self.σ is None:
            self.σ = np.asarray(self.Γ.diagonal(), dtype=np.float64) ** (-0.5)
        self.σ = np.ascontiguousarray(self.σ, dtype=np.float64)

    @property
    def ρ̄(self):
        return float(np.sqrt(1 - self.ρ ** 2))


@dataclass
class StickyBarriers:
    """StickyBarriers(x, rule, κ) -- src/stickyzz.jl:19-25: the lower and the upper barrier of one coordinate.  x: their levels (−inf / inf:
    no barrier on that side); rule: what each does to the restored speed when the coordinate thaws ("sticky" keeps it, "reflect" negates it,
    "reversible" flips its sign by a coin); κ: their thaw rates (inf: an instantaneous wall).  StickyBarriers() is the reference's default:
    no barriers at all."""
    x: tuple = (-np.inf, np.inf)
    rule: tuple = ("reflect", "reflect")
    κ: tuple = (np.inf, np.inf)

    def __post_init__(self):
        self.x = (float(self.x[0]), float(self.x[1]))
        self.rule = (str(self.rule[0]).lstrip(":"), str(self.rule[1]).lstrip(":"))
        self.κ = (float(self.κ[0]), float(self.κ[1]))
        for r in self.rule:
            if r not in ("sticky", "reflect", "reversible"):
                raise ValueError("rule must be 'sticky', 'reflect' or 'reversible', got %r" % (r,))


@dataclass
class FactBoomerang:
    """FactBoomerang(Γ, μ, λ, σ=diag(Γ).^(-0.5); ρ=0.0) -- src/types.jl:71-79: factorised Boomerang dynamics preserving
    N(μ, inv(Diagonal(Γ))), refreshment rate λ > 0."""
    Γ: sp.csc_matrix
    μ: np.ndarray
    λref: float
    σ: Optional[np.ndarray] = None
    ρ: float = 0.0

    def __post_init__(self):
        self.Γ = _csc(self.Γ)
        self.μ = np.ascontiguousarray(self.μ, dtype=np.float64)
        if self.σ is None:
            self.σ = np.asarray(self.Γ.diagonal(), dtype=np.float64) ** (-0.5)
        self.σ = np.ascontiguousarray(self.σ, dtype=np.float64)


def _is_identity(G):
    return G.nnz == G.shape[0] and np.array_equal(G.indices, np.arange(G.shape[0])) and bool(np.all(G.data == 1.0))


def cholesky_lower(Γ):
    """L = cholesky(Symmetric(Γ)).L (src/types.jl:43,66) as a lower-triangular CSC matrix, factorised densely in the NATURAL
    ordering.  For a dense Γ this is the reference's factor up to LAPACK rounding; for a SparseMatrixCSC the reference calls
    CHOLMOD, whose `.L` is the factor of the fill-reducing PERMUTATION of Γ -- a different (equally valid) mass matrix that a
    caller who wants it bit for bit passes explicitly as `L=`."""
    A = Γ.toarray() if sp.issparse(Γ) else np.asarray(Γ, dtype=np.float64)
    A = np.triu(A) + np.triu(A, 1).T  # Symmetric(Γ) reads the upper triangle
    L = sp.csc_matrix(np.tril(np.linalg.cholesky(A)))
    L.sort_indices()
    return L


@dataclass
class BouncyParticle:
    """BouncyParticle(Γ, μ, λ; ρ=0.0) -- src/types.jl:35-45.  L is the mass factor the reference stores in the struct
    (`cholesky(Symmetric(Γ)).L`, :43): computed here when not given (None and Γ = I: identity); the 6-field constructor
    BouncyParticle(Γ, μ, λ, ρ, U, L) of the reference corresponds to passing `L=` (or `U=`) explicitly.
    Γ = None, μ = None is the reference's BouncyParticle(missing, missing, λ, ρ, U, L) of the speed-recorded driver
    (src/not_fact_samplers.jl:336-384): L stays as given (None: identity), U is the diagonal of a PDiagMat metric ([d] > 0) or None."""
    Γ: Optional[sp.csc_matrix]
    μ: Optional[np.ndarray]
    λref: float
    ρ: float = 0.0
    L: Optional[sp.csc_matrix] = None
    U: Optional[np.ndarray] = None

    def __post_init__(self):
        if self.U is not None:
            self.U = np.ascontiguousarray(self.U, dtype=np.float64)
        if self.Γ is None:
            if self.μ is not None:
                raise ValueError("BouncyParticle(missing, missing, ...): μ is given without Γ")
            if self.L is not None:
                self.L = _csc(self.L)
            return
        self.Γ = _csc(self.Γ)
        self.μ = np.ascontiguousarray(self.μ, dtype=np.float64)
        if self.L is None:
            self.L = None if _is_identity(self.Γ) else cholesky_lower(self.Γ)
        else:
            self.L = _csc(self.L)


@dataclass
class LocalBound:
    """LocalBound(c) -- src/types.jl:121-123: pass as `c` to spdmp to select the bounds of src/local.jl."""
    c: np.ndarray


@dataclass
class Boomerang:
    """Boomerang(Γ, μ, λ; ρ=0.0) -- src/types.jl:59-66: Hamiltonian dynamics preserving N(μ, ·) with refreshment rate λ; Γ enters
    through its factor L = cholesky(Symmetric(Γ)).L only (reflect!, refresh!, grad_correct!), see BouncyParticle."""
    Γ: sp.csc_matrix
    μ: np.ndarray
    λref: float
    ρ: float = 0.0
    L: Optional[sp.csc_matrix] = None

    def __post_init__(self):
        self.Γ = _csc(self.Γ)
        self.μ = np.ascontiguousarray(self.μ, dtype=np.float64)
        if self.L is None:
            self.L = None if _is_identity(self.Γ) else cholesky_lower(self.Γ)
        else:
            self.L = _csc(self.L)


@dataclass
class ZigZag1d:
    """ZigZag1d() -- src/types.jl:82-86: the 1-d ZigZag (x(τ), θ(τ)) = (x + θτ, θ), src/dynamics.jl:66-68."""


@dataclass
class Boomerang1d:
    """Boomerang1d(Σ, μ, λ) / Boomerang1d(μ, λ) / Boomerang1d(λ) -- src/types.jl:89-100: rotation around μ (src/dynamics.jl:79-82),
    refreshment θ ~ N(0, Σ) at rate λref."""
    Σ: float = 1.0
    μ: float = 0.0
    λref: float = 1.0

    def __init__(self, *a):
        if len(a) == 1:
            self.Σ, self.μ, self.λref = 1.0, 0.0, float(a[0])
        elif len(a) == 2:
            self.Σ, self.μ, self.λref = 1.0, float(a[0]), float(a[1])
        elif len(a) == 3:
            self.Σ, self.μ, self.λref = float(a[0]), float(a[1]), float(a[2])
        else:
            raise TypeError("Boomerang1d(λ), Boomerang1d(μ, λ) or Boomerang1d(Σ, μ, λ)")


@dataclass
class GaussianTarget1d:
    """∇ϕ(x) = (x − μ)/σ² [+ noise·(rand() − 0.5)]: the closures of test/test1d.jl:9-10 (`∇ϕ`, `∇ϕhat` with noise = 0.1)."""
    μ: float = 0.0
    σ2: float = 1.0
    noise: float = 0.0


@dataclass
class GaussianTarget:
    """∇ϕ(x, i) = Γ[:, i]·x  [− Γ[:, i]·μ]  (idot, src/common.jl:16-24): the device-resident stand-in
    for the reference's `∇ϕ(x, i, Γ) = idot(Γ, i, x)` closure + its `args... = (Γ,)`."""
    Γ: sp.csc_matrix
    μ: Optional[np.ndarray] = None

    def __post_init__(self):
        self.Γ = _csc(self.Γ)
        if self.μ is not None:
            self.μ = np.ascontiguousarray(self.μ, dtype=np.float64)


@dataclass
class LogisticTarget:
    """Subsampled logistic-regression gradient with a control variate at μ, evaluated with SelfMoving():
    ∇ϕmoving(t,x,θ,i,t′,F,A,At,μ,y,ny,k) = γ0*x[i] − fdot_moving(A,At,i,...)  (scripts/logistic.jl:78-95,107,167) --
    the device-resident stand-in for that closure and its `args = (SelfMoving(), A, At, μ, y, ny, k)`."""
    A: sp.csc_matrix      # n x p design
    y: np.ndarray         # [n] successes
    ny: np.ndarray        # [n] failures (m - y)
    μ: np.ndarray         # [p] control-variate point (the mode)
    γ0: float = 0.01
    k: int = 10

    def __post_init__(self):
        self.A = _csc(self.A)
        self.At = _csc(self.A.T)
        self.y = np.ascontiguousarray(self.y, dtype=np.float64)
        self.ny = np.ascontiguousarray(self.ny, dtype=np.float64)
        self.μ = np.ascontiguousarray(self.μ, dtype=np.float64)


@dataclass
class DiffusionBridgeTarget:
    """∇ϕmoving(t, ξ, θ, i, t′, F, L, T) of research/diffusion_bridge/faberschauder.jl:128-145 with its `args = (SelfMoving(), L, T)`: the
    bridge of dX = b(X) ds + dW on [0, T], b(x) = −βx + α sin(ωx), in the Faber-Schauder basis up to level L -- d = (2 << L) + 1
    coefficients, the first and last being the fixed end points u/√T, v/√T (problems.diffusion_bridge_problem builds ξ0, θ0, c).  b′, b″
    are the true derivatives (the script's carry a stray factor 2).  pdmp_ensemble_set_target_diffusion_bridge."""
    L: int
    T: float
    α: float = 1.5
    β: float = 0.1
    ω: float = 2 * np.pi

    def __post_init__(self):
        self.L = int(self.L)
        self.T, self.α, self.β, self.ω = float(self.T), float(self.α), float(self.β), float(self.ω)

    @property
    def d(self):
        return (2 << self.L) + 1


@dataclass
class PrecisionCholeskyTarget:
    """∇ϕ(u, i, YY, (𝕀, 𝕁), N) of casestudies/precision/precision.jl:42-53 (γ0 = 0) and research/newsticky/precision/precision4.jl:82-93
    (γ0 > 0) with its `args = (YY, (𝕀, 𝕁), N)`: N observations Y_k ~ N(0, (L Lᵀ)⁻¹) through YY = Σ Y_k Y_kᵀ ([n x n], symmetric), the
    coordinates being the lower triangle of L packed column by column (trace.pack_lower / unpack_lower; d = n(n+1)/2):
    ∇ϕ_i = Σ_q YY[r, c+q] L[c+q, c] + (r == c ? −N/L[c,c] + γ0 (L[c,c] − 1) : γ0 L[r,c]).  For sspdmp with a diagonal ZigZag(Γ̂, μ̂)
    (problems.precision_cholesky_problem builds it); n <= 64.  pdmp_ensemble_set_target_precision_cholesky."""
    YY: np.ndarray
    N: float
    γ0: float = 0.0

    def __post_init__(self):
        self.YY = np.ascontiguousarray(self.YY, dtype=np.float64)
        if self.YY.ndim != 2 or self.YY.shape[0] != self.YY.shape[1]:
            raise ValueError("YY must be a square matrix")
        self.N, self.γ0 = float(self.N), float(self.γ0)

    @property
    def n(self):
        return self.YY.shape[0]

    @property
    def d(self):
        return self.n * (self.n + 1) // 2


class ExtendedForm:
    """ExtendedForm() / SelfMoving() (src/types.jl:103-119, src/sfact.jl:57-68): as the first of spdmp's `args...` it says that ∇ϕ takes
    (t, x, θ, i, t′, F, args...) and moves the coordinates it reads itself.  The device targets that work this way (LogisticTarget,
    DiffusionBridgeTarget) carry the fact in their type: the marker is accepted, and required by nothing."""

    def __eq__(self, other):
        return isinstance(other, ExtendedForm)

    def __hash__(self):
        return hash(ExtendedForm)

    def __repr__(self):
        return "ExtendedForm()"


SelfMoving = ExtendedForm  # const SelfMoving = ExtendedForm, src/sfact.jl:64


@dataclass
class LogisticRegressionTarget:
    """dϕ and ∇ϕ! of a Bayesian logistic regression for the speed-recorded Bouncy Particle (turing/lr.jl:105-139, tilde/lr.jl:55-98):
    ϕ(x) = Σ_i [m_i log(1 + e^{η_i}) − y_i η_i] + (γ0/2)‖x‖² with η = A x.  A: n x d design (explicit zeros are kept), y: [n] successes,
    m: [n] trials (None: ones), γ0 >= 0 a scalar prior precision.  The device-resident stand-in for the closures `dϕ`, `∇ϕ!` of
    pdmp(dϕ, ∇ϕ!, t0, x0, θ0, T, c::LocalBound, flow::BouncyParticle) (pdmp_ensemble_set_target_bps_logistic)."""
    A: sp.csc_matrix
    y: np.ndarray
    m: Optional[np.ndarray] = None
    γ0: float = 0.0

    def __post_init__(self):
        A = sp.csc_matrix(self.A, dtype=np.float64)
        A.sort_indices()
        self.A = A
        At = sp.csc_matrix(sp.csr_matrix((A.data, A.indices, A.indptr), shape=(A.shape[1], A.shape[0])))  # (no entry dropped or merged)
        At.sort_indices()
        self.At = At
        self.y = np.ascontiguousarray(self.y, dtype=np.float64)
        self.m = np.ones_like(self.y) if self.m is None else np.ascontiguousarray(self.m, dtype=np.float64)
        if self.y.shape != (A.shape[0],) or self.m.shape != self.y.shape:
            raise ValueError("y and m have one entry per row of A")
        self.γ0 = float(self.γ0)


@dataclass
class FactTrace:
    """FactTrace(F, t0, x0, θ0, events) -- src/trace.jl:7-13; events are (t, i, x_i, θ_i), i 0-based."""
    F: object
    t0: float
    x0: np.ndarray
    θ0: np.ndarray
    events: np.ndarray = field(default_factory=lambda: np.empty(0))

    def __len__(self):  # Base.length(FT::Trace) = 1 + length(FT.events), src/trace.jl:42
        return 1 + len(self.events)


@dataclass
class PDMPTrace:
    """PDMPTrace(F, t0, x0, θ0, events) -- src/trace.jl:20-27; events are (t, copy(x), copy(θ)) (src/not_fact_samplers.jl:39-41)."""
    F: object
    t0: float
    x0: np.ndarray
    θ0: np.ndarray
    t: np.ndarray = field(default_factory=lambda: np.empty(0))
    x: np.ndarray = field(default_factory=lambda: np.empty((0, 0)))
    θ: np.ndarray = field(default_factory=lambda: np.empty((0, 0)))
    # sticky samplers (src/ss_not_fact.jl:100-102, Trace(t0, x0, θ0, f, Flow)): the free mask at t0 and after every event, [events x d] bool
    f0: Optional[np.ndarray] = None
    f: Optional[np.ndarray] = None

    def __len__(self):
        return 1 + len(self.t)
