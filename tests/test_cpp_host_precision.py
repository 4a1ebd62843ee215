"""The precision case study through the C++ host mirror (include/pdmp_mi355.hpp, examples/precision_sticky.cpp): compile check here, equality
with the Python call on the GPU box."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp


def _exe(pkg):
    exes = pkg.build.build_examples()
    exe = [e for e in exes if e.endswith("precision_sticky")]
    assert exe and os.access(exe[0], os.X_OK)
    return exe[0]


def _fnv1a(h, data):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_precision_example_builds_and_fails_loudly_without_a_device(pkg):
    exe = _exe(pkg)
    if pkg._lib.device_count() > 0:
        return
    p = subprocess.run([exe, "6", "50", "2", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_cpp_precision_matches_the_python_call(gpu_pkg, tmp_path):
    """sspdmp of the C++ mirror on a PrecisionCholesky with a trace buffer of 4096 events, on the inputs the example writes out: the event
    count, num, acc, an FNV-1a of every event and of the final (t, x, θ, c) equal those of samplers.sspdmp; ‖L̂L̂ᵀ − Γtrue‖ and the sub-diagonals'
    inclusion probabilities equal trace.mean / trace.inclusion_prob of the Python trace to rounding."""
    pkg = gpu_pkg
    exe = _exe(pkg)
    n, N, T, seed = 12, 300, 6.0, 0x52
    dump = str(tmp_path / "inputs.bin")
    p = subprocess.run([exe, str(n), str(N), repr(T), hex(seed), dump], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    d_s, nev_s, num_s, acc_s, h_s, err_s, i1_s, i2_s, i3_s = p.stdout.split()
    raw = np.fromfile(dump)
    d = n * (n + 1) // 2
    assert (raw[0], raw[1], raw.size) == (n, N, 2 + n * n + 4 * d)
    YY, (gam, mu, x0, th0) = raw[2:2 + n * n].reshape(n, n), raw[2 + n * n:].reshape(4, d)
    tgt = pkg.PrecisionCholeskyTarget(YY, N)
    tr, (t, x, th), (acc, num), cc = pkg.sspdmp(tgt, 0.0, x0, th0, T, np.full(d, 10.0), pkg.ZigZag(sp.diags(gam, format="csc"), mu), np.full(d, 0.01),
                                                adapt=True, seed=seed)
    assert len(tr.events) > 1000
    assert (int(d_s), int(nev_s), int(num_s), int(acc_s)) == (d, len(tr.events), num, acc)
    h = 14695981039346656037
    for a in (tr.events.tobytes(), t.tobytes(), x.tobytes(), th.tobytes(), cc.tobytes()):
        h = _fnv1a(h, a)
    assert int(h_s, 16) == h
    L = pkg.trace.unpack_lower(pkg.trace.mean(tr))
    G = np.eye(n) - 0.3 * (np.eye(n, k=1) + np.eye(n, k=-1))
    assert abs(float(err_s) - np.linalg.norm(L @ L.T - G)) <= 1e-10
    inc = pkg.trace.unpack_lower(pkg.trace.inclusion_prob(tr))
    for k, s in ((1, i1_s), (2, i2_s), (3, i3_s)):
        assert abs(float(s) - np.diagonal(inc, -k).mean()) <= 1e-12
    assert float(i1_s) > 0.9 and float(i3_s) < float(i1_s)  # the first sub-diagonal is where the truth is not 0
