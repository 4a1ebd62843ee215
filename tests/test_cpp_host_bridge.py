"""The diffusion bridge through the C++ host mirror (include/pdmp_mi355.hpp, examples/diffusion_bridge.cpp): compile check here, equality
with the Python call on the GPU box."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp


def _exe(pkg):
    exes = pkg.build.build_examples()
    exe = [e for e in exes if e.endswith("diffusion_bridge")]
    assert exe and os.access(exe[0], os.X_OK)
    return exe[0]


def _fnv1a(h, data):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_bridge_example_builds_and_fails_loudly_without_a_device(pkg):
    exe = _exe(pkg)
    if pkg._lib.device_count() > 0:
        return
    p = subprocess.run([exe, "3", "4", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_cpp_bridge_matches_the_python_call(gpu_pkg):
    """spdmp of the C++ mirror on a DiffusionBridge with a trace buffer of 256 events: the event count, num, the accepted reflections, an
    FNV-1a of every event and of the final (t, ξ, θ, c), and dotψ of the final coefficients at T/2 equal those of samplers.spdmp."""
    pkg = gpu_pkg
    exe = _exe(pkg)
    L, TP, seed = 5, 12.0, 0x52
    p = subprocess.run([exe, str(L), repr(TP), hex(seed)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    d_s, nev_s, num_s, acc_s, h_s, x_s = p.stdout.split()
    tgt = pkg.DiffusionBridgeTarget(L, 2.0)
    d = tgt.d
    k = np.arange(d)
    xi0, th0, c = np.zeros(d), np.where(k % 3 == 0, -1.0, 1.0), np.ones(d)
    xi0[0], xi0[-1] = 1.5 / np.sqrt(2.0), -0.5 / np.sqrt(2.0)
    th0[0] = th0[-1] = c[0] = c[-1] = 0.0
    tr, (t, x, th), (acc, num), cc = pkg.spdmp(tgt, 0.0, xi0, th0, TP, c, pkg.ZigZag(sp.identity(d, format="csc"), np.zeros(d)), pkg.SelfMoving(),
                                               adapt=True, seed=seed)
    assert len(tr.events) > 300
    assert (int(d_s), int(nev_s), int(num_s), int(acc_s)) == (d, len(tr.events), num, int(acc.sum()))
    h = 14695981039346656037
    for a in (tr.events.tobytes(), t.tobytes(), x.tobytes(), th.tobytes(), cc.tobytes()):
        h = _fnv1a(h, a)
    assert int(h_s, 16) == h
    assert abs(float(x_s) - pkg.trace.faber_schauder_path(x, 1.0, L, 2.0)) <= 1e-13 * (1 + abs(float(x_s)))  # (numpy sums the levels in the same order)
