"""The exact integral of the path a factorised trace describes, in rationals -- the reference every device ∫x dt is held to
(test_exact_path.py on the host, test_gpu_path_integrals.py on the device).  No device, no package arithmetic, no tolerance.

The path
--------
Coordinate i's path is DEFINED BY THE TRACE: it starts at (t0, x0_i) with slope θ0_i; each event (t_k, i, x_k, θ_k) of i restarts it
at the RECORDED (t_k, x_k) with slope θ_k (a freeze records θ_k = 0, a refresh or `adaptscale` whatever θ was drawn).  Every float is
a rational, so with fractions.Fraction each segment integral Δ·(x_k + θ_k·Δ/2) and their sum are exact.  Events with t_k > T are ignored.
A trace with a refresh clock is not globally time-ordered (the refreshed coordinate is recorded at its own, stale, clock): the events are
taken per coordinate in trace order (= a stable ordering by coordinate), and each coordinate's own times must not decrease from its first
own event on.  The FIRST segment is the exception and is integrated signed: with t0 != 0 the reference draws the first queue times
without adding t0, so a coordinate's first own event lies before t0 and its first Δ = t_1 − t0 is negative -- on the device
(dt = tnew − t0) as here.

The bound (derived, not picked)
-------------------------------
Device and reference differ by rounding only.  One move of coordinate i on the device is

    xn = x + θ·dt          the position picks up <= 2u·X_i (one product, one sum), and carries it at most until i's next own event,
                           where the reference restarts from the recorded value, i.e. from the device's own;
    term = dt·((x + xn)·0.5)   three roundings (dt, the sum, the product; ·0.5 is exact): <= 3u·|term|;
    I += term              <= u·|I|,

with u = 2⁻⁵³, X_i = max over [t0, T] of |x_i(s)| and |term|, |I| <= X_i·L_i, L_i = Σ_k |Δ_k| over i's segments (= T − t0 when t0 = 0).
A position error ε held over a stretch of length ℓ shifts the integral by ε·ℓ <= 2u·X_i·L_i per move in the worst case; so after m_i moves

    |J_dev,i − J_exact,i|  <=  3·(m_i + 1)·u·X_i·L_i                                                    (bound_J)

(the + 1 is the read itself: J = I + dt·(x + θ·dt/2) at T).  m_i:
  * tracked evaluation: a coordinate moves at its own accepted events only -- own events in the trace + 1 for the tail;
  * moving evaluation: it moves at every proposal inside its neighbourhood -- bounded by the chain's counters, num + nevents + 1
    (loose and safe).
The counters' bound is far from tight -- every move is charged the whole X_i·L_i where it costs about u·X_i·|Δ_k| -- and that slack is
also what covers the one thing the derivation does not name: under the moving evaluation with t0 != 0 a coordinate is carried back to
a neighbour's first proposal (t ≈ 0) and forward again before its own first event, a stretch of |t0| each way that L_i of the trace's
own path does not contain; it adds two moves' worth of rounding at |x| <= X_i + |θ|·t0, against thousands of moves charged in full.
Host float64 arithmetic (trace.moments, trace.mean) uses 0.05-0.15 of the own-events bound (test_exact_path.py).

Sums over chains (batch_means, ess_*): the reference is the same sums formed in Fraction from the device's own per-chain J at all d
coordinates, which isolates the reduction kernels from the event loops.  A sum of n terms in ANY order (atomicAdd) costs
<= (n − 1)·u·Σ|terms|; with up to 3u on each term

    |ΣY_dev − ΣY_exact|   <=  (n + 3)·u·Σ_chains |y|          |ΣY²_dev − ΣY²_exact|  <=  (n + 3)·u·Σ_chains y²      (bound_sum)

y = (J(T) − J(T_prev))·(1/ΔT) written plainly spends exactly those 3u (the difference, 1/ΔT rounded once, the product) -- and y·y then
carries 2·3u + u = 7u, which a sum of ONE chain's squares cannot keep inside (n + 3)u.  The reduction kernels therefore round y and y² once each (batch_mean_exactly_rounded, pdmp_kernels.hip:
exact differences as pairs, the quotient carried to ~u²), 1u per term, and both sums hold (n + 3)u with room.
"""
from fractions import Fraction

U = Fraction(1, 2 ** 53)


class ExactPath:
    """Per-coordinate exact state of the path described by the events fed so far (in trace order)."""

    def __init__(self, t0, x0, theta0):
        self.d = len(x0)
        self.t0 = Fraction(float(t0))
        self.t = [self.t0] * self.d            # time of the last restart
        self.x = [Fraction(float(v)) for v in x0]
        self.th = [Fraction(float(v)) for v in theta0]
        self.I = [Fraction(0)] * self.d        # exact integral up to self.t
        self.L = [Fraction(0)] * self.d        # Σ |Δ| of the closed segments
        self.X = [abs(float(v)) for v in x0]   # max |x| over the closed segments (floats: it enters the bound only)
        self.own = [0] * self.d                # own events fed

    def feed(self, events):
        """events: structured array / iterable of records with fields t, i, x, theta, in trace order."""
        for e in events:
            i = int(e["i"])
            tk = Fraction(float(e["t"]))
            if self.own[i] > 0:
                assert tk >= self.t[i], "coordinate %d: own event times decrease (%r after %r)" % (i, float(tk), float(self.t[i]))
            dt = tk - self.t[i]  # (signed: negative for a first event before t0)
            self.I[i] += dt * (self.x[i] + self.th[i] * dt / 2)
            self.L[i] += abs(dt)
            self.X[i] = max(self.X[i], abs(float(self.x[i] + self.th[i] * dt)), abs(float(e["x"])))
            self.t[i], self.x[i], self.th[i] = tk, Fraction(float(e["x"])), Fraction(float(e["theta"]))
            self.own[i] += 1

    def J(self, T):
        """[d] Fractions: ∫_{t0}^{T} x_i(s) ds, the open segment after each coordinate's last restart continued to T."""
        T = Fraction(float(T))
        out = []
        for i in range(self.d):
            dt = T - self.t[i]
            out.append(self.I[i] + dt * (self.x[i] + self.th[i] * dt / 2))
        return out

    def absmax(self, T):
        T = Fraction(float(T))
        return [max(self.X[i], abs(float(self.x[i] + self.th[i] * (T - self.t[i])))) for i in range(self.d)]

    def length(self, T):
        T = Fraction(float(T))
        return [self.L[i] + abs(T - self.t[i]) for i in range(self.d)]


def _upto(events, T):
    return [e for e in events if float(e["t"]) <= float(T)]


def exact_J(t0, x0, theta0, events, T):
    """list of d Fractions: ∫_{t0}^{T} x_i(s) ds of the path the trace describes (module docstring)."""
    p = ExactPath(t0, x0, theta0)
    p.feed(_upto(events, T))
    return p.J(T)


def exact_absmax(t0, x0, theta0, events, T):
    """list of d floats: X_i = max over [t0, T] of |x_i(s)| (piecewise linear: attained at a segment end)."""
    p = ExactPath(t0, x0, theta0)
    p.feed(_upto(events, T))
    return p.absmax(T)


def bound_J(m, X, L):
    """3·(m + 1)·u·X·L as a Fraction (m moves of the coordinate in [t0, T])."""
    return 3 * (int(m) + 1) * U * Fraction(float(X)) * Fraction(L)


def bound_sum(n, abs_terms):
    """(n + 3)·u·Σ|terms| for a device sum of n per-chain terms in any order."""
    return (int(n) + 3) * U * sum((abs(Fraction(v)) for v in abs_terms), Fraction(0))
