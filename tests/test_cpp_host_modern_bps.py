"""The speed-recorded Bouncy Particle through the C++ host mirror (include/pdmp_mi355.hpp, examples/bps_modern.cpp): compile check here,
parity with the restatement on the GPU box."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import modern_bps_ref_lib as M


def _exe(pkg):
    exes = pkg.build.build_examples()
    exe = [e for e in exes if e.endswith("bps_modern")]
    assert exe and os.access(exe[0], os.X_OK)
    return exe[0]


def _fnv1a(h, data):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_modern_example_builds_and_fails_loudly_without_a_device(pkg):
    exe = _exe(pkg)
    if pkg._lib.device_count() > 0:
        return
    p = subprocess.run([exe, "8", "4", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["", "u", "oscn"])
def test_cpp_modern_bps_matches_the_restatement(gpu_pkg, mode):
    """pdmp(target, t0, x0, θ0, n, LocalBound(c), B) of the C++ mirror with a trace buffer of 16 records: the record count, (acc, num) and
    an FNV-1a of every record and of the final (t, x, θ, c) equal the restatement's."""
    exe = _exe(gpu_pkg)
    d, n, seed = 100, 40, 0x51
    p = subprocess.run([exe, str(d), str(n), hex(seed)] + ([mode] if mode else []), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    d_s, nrec_s, num_s, acc_s, h_s, tl_s = p.stdout.split()
    k = np.arange(d)
    G = sp.diags([np.full(d - 1, -0.5), 2.0 + 0.125 * (k % 5), np.full(d - 1, -0.5)], [-1, 0, 1], format="csc")
    x0 = ((k * 37) % 101) / 50.0 - 1.0
    th0 = np.where(k % 3 == 0, -1.0, 0.75)
    r = M.pdmp(0.0, x0, th0, n, 5.0, gamma=G, lambda_ref=1.0, rho=0.9, seed=seed, u_diag=(0.5 + 0.25 * (k % 7)) if mode == "u" else None,
               oscn=mode == "oscn")
    assert r["status"] == M.REF_OK and r["nacc"] > 10
    assert (int(d_s), int(nrec_s), int(num_s), int(acc_s)) == (d, n, r["num"], r["nacc"])
    h = 14695981039346656037
    for a in (r["t"], r["x"], r["theta"], np.array([r["t_final"]]), r["x_final"], r["theta_final"], np.array([r["c_final"]])):
        h = _fnv1a(h, np.ascontiguousarray(a, dtype=np.float64).tobytes())
    assert int(h_s, 16) == h and float(tl_s) == r["t"][-1]
