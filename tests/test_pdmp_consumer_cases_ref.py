"""The two host statements of the PDMPTrace consumers on the hand-made traces of tests/pdmp_consumer_cases.py, held to each other without a device:
trace.py (vectorised numpy: mean, cummean, inclusion_prob, discretize) and tests/ref/pdmp_trace_ref.c (one event after the other, the arithmetic
of csrc/pdmp_consume_bps.hip).  tests/test_gpu_bps_consumers.py then holds the device to the C reference bit for bit.

They agree within the project's rtol = 1e-12, atol = 1e-15 (numpy sums the terms pairwise, the reference in event order); the grid times agree
bit for bit; on the dyadic cases everything is exact and the agreement is bit for bit.  A Boomerang's rows differ by what pdmp_sincos and libm's
sin / cos differ by: measured here and held to the absolute error bound tests/test_detmath_accuracy.py pins pdmp_sincos to, times |x − μ| + |θ|
in the maximum norm (test_boomerang_rows_within_the_sincos_bound; its docstring has the figures, also those of the entry-by-entry ratio)."""
import numpy as np
import pytest

import pdmp_consumer_cases as PC
from test_detmath_accuracy import SINCOS_ABS

TOL = dict(rtol=1e-12, atol=1e-15)  # the project's tolerance for mean / inclusion_prob (tests/test_gpu_consumers_synthetic.py)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b, bitwise):
    """bit for bit with NaNs by position (a 0/0 has one sign on the host and another on the device), or within TOL"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    if bitwise:
        return np.array_equal(bits(a[ok]), bits(b[ok]))
    fin = ok & np.isfinite(a)
    return np.array_equal(a[ok & ~fin], b[ok & ~fin]) and np.allclose(a[fin], b[fin], **TOL)


def host_trace(pkg, c, k, s):
    t, x, th, f = c.so_far(k, s)
    F = pkg.Boomerang(np.eye(c.d), c.mu, 1.0) if c.mu is not None else None
    tr = pkg.PDMPTrace(F, c.t0, c.x0[k], c.th0[k], t, x, th)
    if c.sticky:
        tr.f0, tr.f = np.ones(c.d, dtype=bool), f
    return tr


def test_the_table_holds_what_it_says():
    for name in PC.NAMES:
        c = PC.case(name)
        assert c.dyadic == (name in PC.DYADIC)
        for k in range(c.nchains):
            t = c.t[k]
            assert np.all(np.diff(t) >= 0) and c.x[k].shape == c.th[k].shape == (len(t), c.d)
            assert len(c.cuts[k]) == c.nseg + 1 and c.cuts[k][0] == 0 and c.cuts[k][-1] == len(t)
            if c.sticky:  # what set_state_bps writes itself
                assert c.cuts[k][1] == 1 and t[0] == c.t0 and np.array_equal(c.x[k][0], c.x0[k]) and np.array_equal(c.th[k][0], c.th0[k])
                assert c.f[k][0].all()
    assert sorted(PC.case(n).d for n in ("one", "d63", "d64", "d65", "sticky130", "c1024")) == [1, 63, 64, 65, 130, 1024]
    one = PC.case("one")
    assert sorted(np.diff(one.cuts[0]))[:2] == [0, 1] and max(np.diff(one.cuts[0])) >= 299
    g = one.t0 + one.dt * np.arange(one.K)
    assert np.isin(one.t[0], g).sum() > 60 and (np.diff(one.t[0]) == 0).sum() > 60  # events on grid times, events sharing a time
    assert PC.reference("short_grid", 0, 3)["npoints"] > PC.case("short_grid").K
    neg = PC.case("neg")
    assert neg.t0 < 0 and (neg.t[0] == 0.0).sum() == 1 and neg.grow
    sp_ = PC.case("sparse")
    assert max(np.diff(np.searchsorted(sp_.t0 + sp_.dt * np.arange(sp_.K), sp_.t[0]))) > 100  # many rows between two events
    b = PC.case("boom")
    assert np.any(b.mu != 0)
    g = b.t0 + b.dt * np.arange(b.K)
    tau = g[:, None] - np.where(b.t[0][None] <= g[:, None], b.t[0][None], -np.inf)
    tau = tau.min(1)[np.isfinite(tau.min(1))]
    assert tau.min() < 2e-9 and tau.max() > 2 * np.pi
    for name, flips in (("sticky130", (63, 64, 129)), ("boom_sticky", (0, 63, 64, 65))):
        f = PC.case(name).f[0]
        assert all(np.any(np.diff(f[:, q].astype(int)) != 0) for q in flips)


@pytest.mark.parametrize("name", PC.NAMES)
def test_trace_py_agrees_with_the_c_reference(pkg, name):
    c = PC.case(name)
    for k in range(c.nchains):
        for s in range(c.nseg):
            t, x, th, f = c.so_far(k, s)
            r = PC.reference(name, k, s)
            if len(t) == 0:
                assert r["npoints"] == 1 and r["T"] == c.t0 and np.array_equal(r["grid"][0], c.x0[k]) and not r["grid"][1:].any()
                continue
            tr = host_trace(pkg, c, k, s)
            assert r["T"] == t[-1]
            with np.errstate(divide="ignore", invalid="ignore"):
                assert same(pkg.trace.mean(tr), r["mean"], c.dyadic)
                assert same(pkg.trace.cummean(tr), r["cummean"], c.dyadic)
            if c.sticky:
                assert same(pkg.trace.inclusion_prob(tr), r["inclusion"], c.dyadic)
            if not t[-1] > c.t0:
                # trace.py returns an empty grid when the last event time equals t0; the consumers report row 0
                assert r["npoints"] == 1 and len(pkg.trace.discretize(tr, c.dt)[0]) == 0
                continue
            grid, X = pkg.trace.discretize(tr, c.dt)
            n = min(r["npoints"], c.K)
            assert len(grid) == r["npoints"] and np.array_equal(bits(grid[:n]), bits(r["grid_t"]))
            assert not r["grid"][n:].any()
            if c.mu is None:
                assert same(X[:n], r["grid"][:n], c.dyadic)
            else:  # (the values: test_boomerang_rows_within_the_sincos_bound)
                assert np.allclose(X[:n], r["grid"][:n], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", [n for n in PC.NAMES if n.startswith("boom")])
def test_boomerang_rows_within_the_sincos_bound(pkg, name):
    """trace.py rotates with np.sin / np.cos, the reference with pdmp_sincos.  On every trace of the case: the largest |row(trace.py) − row(reference)|
    against SINCOS_ABS = 2.5e-16 (the absolute error tests/test_detmath_accuracy.py holds pdmp_sincos to) times the magnitude of |x − μ| + |θ|, the
    largest over the events the rows flow from -- a bound in the maximum norm, the form in which an absolute error of s and c carries over to
    (x − μ)·c + θ·s + μ.

    Measured: the largest difference is 8.88e-16 in both cases (boom: against 2.5e-16 · 5.08 = 1.27e-15; boom_sticky: against 2.5e-16 · 5.15 =
    1.29e-15).  Entry by entry the same factor does NOT hold and is not asserted: the largest difference / (|x − μ| + |θ|) of a single entry is
    1.12e-15 (boom) and 7.68e-16 (boom_sticky), 79 of 10790 and 40 of 12078 entries lie above 2.5e-16 -- e.g. x − μ = 0.031, θ = 0.068, μ = 0.675:
    0.6624000607233674 against …675, ONE ulp of the row apart and each within 0.52 ulp of the exact value.  μ sets such a row's magnitude, and
    so its ulp, but is not part of |x − μ| + |θ|; no pair of correctly rounded evaluations meets the factor there."""
    c = PC.case(name)
    worst = worst_entry = 0.0
    for s in range(c.nseg):
        t, x, th, f = c.so_far(0, s)
        if len(t) == 0 or not t[-1] > c.t0:
            continue
        r = PC.reference(name, 0, s)
        grid, X = pkg.trace.discretize(host_trace(pkg, c, 0, s), c.dt)
        n = min(r["npoints"], c.K)
        te = np.concatenate([[c.t0], t])
        idx = np.searchsorted(te, grid[:n], side="right") - 1
        mag = np.abs(np.vstack([c.x0[0][None], x])[idx] - c.mu) + np.abs(np.vstack([c.th0[0][None], th])[idx])
        err = np.abs(X[:n] - r["grid"][:n])
        worst, worst_entry = max(worst, float(err.max())), max(worst_entry, float((err / mag).max()))
        print("%s, %d events: largest |row(trace.py) - row(reference)| = %.3g against %.3g * %.3g = %.3g; largest entry by entry / (|x - mu| + |theta|) = %.3g"
              % (name, len(t), err.max(), SINCOS_ABS, mag.max(), SINCOS_ABS * mag.max(), (err / mag).max()))
        assert err.max() <= SINCOS_ABS * mag.max(), (float(err.max()), float(mag.max()))
    assert worst > 0.0  # (the two sides do differ: the comparison is not vacuous)
