"""The ZigZag with sticky and reflecting barriers through the C++ host mirror (include/pdmp_mi355.hpp, examples/stickyzz_box.cpp): compile
check here, equality with the Python call on the GPU box."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp


def _exe(pkg):
    exes = pkg.build.build_examples()
    exe = [e for e in exes if e.endswith("stickyzz_box")]
    assert exe and os.access(exe[0], os.X_OK)
    return exe[0]


def _fnv1a(h, data):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_stickyzz_example_builds_and_fails_loudly_without_a_device(pkg):
    exe = _exe(pkg)
    if pkg._lib.device_count() > 0:
        return
    p = subprocess.run([exe, "8", "4", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_cpp_stickyzz_matches_the_python_call(gpu_pkg):
    """stickyzz of the C++ mirror with a trace buffer of 64 events: the event count, (acc, num), the number of frozen coordinates, t′ and an
    FNV-1a of every event and of the final (t, x, θ, saved speeds) equal those of samplers.stickyzz on the same problem."""
    pkg = gpu_pkg
    exe = _exe(pkg)
    d, T, seed = 16, 50.0, 0x51
    p = subprocess.run([exe, str(d), repr(T), hex(seed)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    d_s, nev_s, num_s, acc_s, nfr_s, h_s, tp_s = p.stdout.split()
    k = np.arange(d)
    G = sp.diags([np.full(d - 1, -0.5), 2.0 + 0.125 * (k % 5), np.full(d - 1, -0.5)], [-1, 0, 1], format="csc")
    x0 = ((k * 37) % 101) / 100.0 - 0.75
    th0 = np.where(k % 3 == 0, -1.0, 0.75)
    inf = float("inf")
    barriers = [pkg.StickyBarriers((-1.0, 0.5), ("sticky", "reflect"), (0.8, 5.0)) if i % 2 else pkg.StickyBarriers((-1.0, 0.5), ("reflect", "reflect"), (inf, inf))
                for i in range(d)]
    Z = pkg.ZigZag(0.9 * G, np.zeros(d), np.ones(d))
    tr, tp, (t, x, th), (acc, num), det = pkg.stickyzz(pkg.GaussianTarget(G, None), 0.0, x0, th0, T, np.full(d, 2.0), Z, barriers, seed=seed, details=True)
    assert len(tr.events) > 200 and np.any(tr.events["theta"] == 0)
    assert (int(d_s), int(nev_s), int(num_s), int(acc_s), int(nfr_s)) == (d, len(tr.events), num, acc, int(det["frozen"].sum()))
    h = 14695981039346656037
    for a in (tr.events.tobytes(), t.tobytes(), x.tobytes(), th.tobytes(), det["θ_saved"].tobytes()):
        h = _fnv1a(h, a)
    assert int(h_s, 16) == h and float(tp_s) == tp
