"""Inputs shared by tests/test_precision_ref.py (CPU) and tests/test_gpu_precision_parity.py (device): the n = 2 case with the closed-form sticky
posterior, random n x n cases, and the input on which a diagonal coordinate's freeze is popped.  numpy only."""
import numpy as np

N2 = dict(YY=np.array([[12.0, 1.5], [1.5, 9.0]]), N=10.0)

# the restatement on stalled_input(): PDMP_CHAIN_STALLED at the freeze of coordinate 0 (pinned by tests/test_precision_ref.py)
DIAGONAL_FREEZE = dict(nevents=21, num=404, ndraw_main=833)


def lower_index(n):
    """(rows, cols) of the packed lower triangle, column by column"""
    cols, rows = np.triu_indices(int(n))
    return rows.astype(np.int64), cols.astype(np.int64)


def flow_of(YY, N, gamma0=0.0):
    """(γ̂, μ̂) of problems.precision_cholesky_problem for any YY: the per-column mode of the flat-prior posterior and the curvature there"""
    n = YY.shape[0]
    r, c = lower_index(n)
    mu = np.empty(r.size)
    k0 = 0
    for col in range(n):
        A = YY[col:, col:]
        w = np.linalg.solve(A[1:, 1:], A[1:, 0]) if n - col > 1 else np.empty(0)
        s = A[0, 0] - A[0, 1:] @ w
        mu[k0] = np.sqrt(N / s)
        mu[k0 + 1:k0 + n - col] = -w * mu[k0]
        k0 += n - col
    gam = YY[r, r] + gamma0 + np.where(r == c, N / mu**2, 0.0)
    return gam, mu


def n2_flow():
    return flow_of(N2["YY"], N2["N"])


def random_case(n, N, seed, nch, spread=0.05):
    """YY of N standard-normal observations in n dimensions, the flow of flow_of, and nch starts around the mode with their own directions"""
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((n, int(max(N, n + 2))))
    YY = Y @ Y.T
    YY = 0.5 * (YY + YY.T)
    gam, mu = flow_of(YY, N)
    r, c = lower_index(n)
    x0 = mu[None, :] + spread * rng.standard_normal((nch, r.size)) * np.where(r == c, 0.2, 1.0)
    x0[:, r == c] = np.abs(x0[:, r == c]) + 1e-3
    th0 = rng.choice([-1.0, 1.0], size=(nch, r.size))
    return dict(YY=YY, N=float(N), gam=gam, mu=mu, x0=x0, th0=th0, n=n, d=r.size)


def stalled_input(seed=1):
    """n = 5: L11 starts at 0.1 and moves down, N = 1e-3 leaves −N/u too weak to keep it off 0, c = 50 keeps every bound above its rate.  With
    seed 1 (found by running the restatement over seeds 0 .. 3) L11 reflects once, 21 events are recorded -- 7 of them freezes of off-diagonal
    coordinates --, then the freeze of coordinate 0 is popped at t = 0.5997."""
    a = random_case(5, 30, 900, 1)
    r, c = lower_index(5)
    x0, th0 = a["x0"][0].copy(), a["th0"][0].copy()
    x0[0], th0[0] = 0.1, -1.0
    return dict(YY=a["YY"], N=1e-3, x0=x0, th0=th0, c=np.full(15, 50.0), gam=np.ones(15), mu=np.zeros(15), kappa=np.full(15, 1.0), seed=seed)
