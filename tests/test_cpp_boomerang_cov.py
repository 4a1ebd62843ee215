"""The covariance of a Boomerang path through the C++ host mirror (include/pdmp_mi355.hpp: Options::consume with cov_pi / cov_pj on pdmp with a
Boomerang, Result::pairs; examples/boomerang_cov.cpp): compile check here, equality with the Python call on the GPU box."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp


def _exe(pkg):
    exes = pkg.build.build_examples()
    exe = [e for e in exes if e.endswith("boomerang_cov")]
    assert exe and os.access(exe[0], os.X_OK)
    return exe[0]


def _fnv1a(h, data):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_boomerang_cov_example_builds_and_fails_loudly_without_a_device(pkg):
    exe = _exe(pkg)
    if pkg._lib.device_count() > 0:
        return
    p = subprocess.run([exe, "8", "10", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_cpp_boomerang_cov_matches_the_python_call(gpu_pkg):
    """pdmp of the C++ mirror on a Boomerang with Options::consume and the lower triangle as pair list, a trace buffer of 48 events: the event
    count, num, an FNV-1a of the trace and one of (S, J, T_last) equal those of samplers.pdmp(..., consume=dict(cov=..., center=...)), whose
    integrals are trace.arc_pair_integrals of the returned trace bit for bit (tests/test_gpu_arc_pairs.py)."""
    pkg = gpu_pkg
    exe = _exe(pkg)
    d, T, seed = 8, 200.0, 0x31
    p = subprocess.run([exe, str(d), repr(T), hex(seed)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    d_s, nev_s, num_s, h_s, g_s, worst_s = p.stdout.split()
    k = np.arange(d)
    mu = 0.125 + 0.0625 * k
    x0, th0 = mu + 0.25 * (k % 3 - 1), np.where(k % 2 == 1, -0.75, 1.25)
    cen = 0.03125 * k - 0.0625
    pi, pj = np.tril_indices(d)  # (row by row, as the example lists them)
    I = sp.identity(d, format="csc")
    tr, _, (acc, num), _, extra = pkg.pdmp(pkg.GaussianTarget(sp.csc_matrix(1.2 * I), mu), 0.0, x0, th0, T, 3.0, pkg.Boomerang(I, mu, 0.5), adapt=True,
                                           factor=2.0, seed=seed, trace_capacity=48, consume=dict(cov=(pi, pj), center=cen))
    assert len(tr.t) > 2 * 48  # (at least three slices of the buffer)
    assert (int(d_s), int(nev_s), int(num_s)) == (d, len(tr.t), int(num))
    h = 14695981039346656037
    for a in (tr.t, tr.x, tr.θ):
        h = _fnv1a(h, np.ascontiguousarray(a, dtype=np.float64).tobytes())
    assert int(h_s, 16) == h
    g = 14695981039346656037
    for a in (extra["pair_S"], extra["pair_J"], np.float64(extra["T"])):
        g = _fnv1a(g, np.ascontiguousarray(a, dtype=np.float64).tobytes())
    assert int(g_s, 16) == g
    cov, _ = pkg.trace.covariance(pi, pj, extra["pair_S"], extra["pair_J"], extra["T"], center=cen)
    worst = np.abs(cov.toarray() - np.eye(d) / 1.2)[pi, pj].max()
    assert abs(float(worst_s) - worst) <= 1e-13
