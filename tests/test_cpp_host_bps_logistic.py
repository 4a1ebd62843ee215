"""The speed-recorded Bouncy Particle on the logistic-regression target through the C++ host mirror (include/pdmp_mi355.hpp,
examples/bps_logistic.cpp): compile check and "no CPU fallback" here, parity with the restatement on the GPU box."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import bps_logistic_ref_lib as B


def _exe(pkg):
    exes = pkg.build.build_examples()
    exe = [e for e in exes if e.endswith("bps_logistic")]
    assert exe and os.access(exe[0], os.X_OK)
    return exe[0]


def _fnv1a(h, data):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def example_data(d, n):
    """The data set examples/bps_logistic.cpp builds from (d, n)."""
    rows, cols, vals = [], [], []
    for i in range(n):
        for j in sorted({i % d, (3 * i + 1) % d, (7 * i + 2) % d}):
            rows.append(i)
            cols.append(j)
            vals.append(((13 * i + 7 * j) % 11 - 5) / 8.0)
    A = sp.csc_matrix((vals, (rows, cols)), shape=(n, d))
    assert A.nnz == len(vals)  # (the explicit zeros stay)
    i = np.arange(n)
    m = 1 + i % 3
    y = (5 * i) % (m + 1)
    k = np.arange(d)
    return A, y.astype(np.float64), m.astype(np.float64), (((k * 37) % 101) / 50.0 - 1.0) / 4.0, np.where(k % 3 == 0, -1.0, 0.75)


def test_cpp_logistic_example_builds_and_fails_loudly_without_a_device(pkg):
    exe = _exe(pkg)
    if pkg._lib.device_count() > 0:
        return
    p = subprocess.run([exe, "8", "12", "4", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["", "u", "oscn"])
def test_cpp_bps_logistic_matches_the_restatement(gpu_pkg, mode):
    """pdmp(target, t0, x0, θ0, nrec, LocalBound(c), B) of the C++ mirror with a trace buffer of 16 records: the record count, (acc, num)
    and an FNV-1a of every record and of the final (t, x, θ, c) equal the restatement's."""
    exe = _exe(gpu_pkg)
    d, n, nrec, seed = 100, 130, 40, 0x51
    p = subprocess.run([exe, str(d), str(n), str(nrec), hex(seed)] + ([mode] if mode else []), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    d_s, n_s, nrec_s, num_s, acc_s, h_s, tl_s = p.stdout.split()
    A, y, m, x0, th0 = example_data(d, n)
    k = np.arange(d)
    r = B.pdmp(0.0, x0, th0, nrec, 30.0, A=A, y=y, m=m, gamma0=0.5, lambda_ref=1.0, rho=0.9, seed=seed, adapt=True,
               u_diag=(0.5 + 0.25 * (k % 7)) if mode == "u" else None, oscn=mode == "oscn")
    assert r["status"] == B.REF_OK and r["nacc"] > 10
    assert (int(d_s), int(n_s), int(nrec_s), int(num_s), int(acc_s)) == (d, n, nrec, r["num"], r["nacc"])
    h = 14695981039346656037
    for a in (r["t"], r["x"], r["theta"], np.array([r["t_final"]]), r["x_final"], r["theta_final"], np.array([r["c_final"]])):
        h = _fnv1a(h, np.ascontiguousarray(a, dtype=np.float64).tobytes())
    assert int(h_s, 16) == h and float(tl_s) == r["t"][-1]
