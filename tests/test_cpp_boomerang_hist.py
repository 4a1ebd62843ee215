"""The marginal histograms of a path through the C++ host mirror (include/pdmp_mi355.hpp: Options::consume with hist_coords / hist_lo / hist_hi /
hist_bins on pdmp with a Boomerang -- arcs -- and with a BouncyParticle -- lines --, Result::hist; examples/boomerang_quantiles.cpp): compile
check here, equality with the Python call on the GPU box."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp


def _exe(pkg):
    exes = pkg.build.build_examples()
    exe = [e for e in exes if e.endswith("boomerang_quantiles")]
    assert exe and os.access(exe[0], os.X_OK)
    return exe[0]


def _fnv1a(h, data):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_boomerang_quantiles_example_builds_and_fails_loudly_without_a_device(pkg):
    exe = _exe(pkg)
    if pkg._lib.device_count() > 0:
        return
    p = subprocess.run([exe, "8", "10", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("flow", [0, 1])
def test_cpp_histogram_matches_the_python_call(gpu_pkg, flow):
    """pdmp of the C++ mirror on a Boomerang (flow 0) and on a BouncyParticle (flow 1) with Options::consume and hist_bins = 64, a trace buffer of
    48 events: the event count, num, an FNV-1a of the trace and one of (H, Z, T_last) equal those of samplers.pdmp(..., consume=dict(hist=...)),
    and the printed quantiles are trace.histogram_quantiles of those rows, bit for bit (Histogram::quantile restates it)."""
    pkg = gpu_pkg
    exe = _exe(pkg)
    d, T, seed = 8, 200.0, 0x31
    p = subprocess.run([exe, str(d), repr(T), hex(seed), str(flow)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().split("\n")
    d_s, nev_s, num_s, h_s, g_s = lines[0].split()
    k = np.arange(d)
    mu = 0.125 + 0.0625 * k
    x0, th0 = mu + 0.25 * (k % 3 - 1), np.where(k % 2 == 1, -0.75, 1.25)
    I = sp.identity(d, format="csc")
    target = pkg.GaussianTarget(sp.csc_matrix(1.2 * I), mu)
    F, c = (pkg.Boomerang(I, mu, 0.5), 3.0) if flow == 0 else (pkg.BouncyParticle(I, mu, 0.5), 1e-3)
    tr, _, (acc, num), _, extra = pkg.pdmp(target, 0.0, x0, th0, T, c, F, adapt=True, factor=2.0, seed=seed, trace_capacity=48,
                                           consume=dict(hist=dict(coords=None, lo=mu - 5.0, hi=mu + 5.0, bins=64)))
    assert len(tr.t) > 2 * 48  # (at least three slices of the buffer)
    assert (int(d_s), int(nev_s), int(num_s)) == (d, len(tr.t), int(num))
    h = 14695981039346656037
    for a in (tr.t, tr.x, tr.θ):
        h = _fnv1a(h, np.ascontiguousarray(a, dtype=np.float64).tobytes())
    assert int(h_s, 16) == h
    g = 14695981039346656037
    for a in (extra["hist_H"], extra["hist_Z"], np.float64(extra["T"])):
        g = _fnv1a(g, np.ascontiguousarray(a, dtype=np.float64).tobytes())
    assert int(g_s, 16) == g
    Q = pkg.trace.histogram_quantiles(extra["hist_H"], mu - 5.0, mu + 5.0, [0.05, 0.5, 0.95])
    got = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[1:]])
    assert [int(ln.split()[0]) for ln in lines[1:]] == list(range(d))
    assert got.shape == (d, 3) and np.array_equal(got.view(np.uint64), np.ascontiguousarray(Q).view(np.uint64))
    assert np.all(Q[:, 0] < Q[:, 1]) and np.all(Q[:, 1] < Q[:, 2])
