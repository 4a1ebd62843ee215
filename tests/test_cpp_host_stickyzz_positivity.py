"""The device consumers of a barrier run through the C++ host mirror (include/pdmp_mi355.hpp: Options::consume, Ensemble::barrier_consume_*;
examples/stickyzz_positivity.cpp, the shape of the reference's examples/positivityconstraint.jl): compile check here, equality with the Python
call on the GPU box."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp


def _exe(pkg):
    exes = pkg.build.build_examples()
    exe = [e for e in exes if e.endswith("stickyzz_positivity")]
    assert exe and os.access(exe[0], os.X_OK)
    return exe[0]


def test_cpp_positivity_example_builds_and_fails_loudly_without_a_device(pkg):
    exe = _exe(pkg)
    if pkg._lib.device_count() > 0:
        return
    p = subprocess.run([exe, "10", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_cpp_positivity_matches_the_python_call(gpu_pkg):
    """T_last, the event count, the mean of the grid rows, mean(Ξ), the hits of the wall at 2.5 and the time frozen on it (none: κ = Inf) equal
    those of samplers.stickyzz(..., consume=dict(dt=0.5, points=...)) on the same problem; with consume_only no event reaches the host and the
    consumers' numbers stay what they were."""
    pkg = gpu_pkg
    exe = _exe(pkg)
    T, seed = 200.0, 0x51
    G = sp.csc_matrix(np.array([[1.0, 0.25], [0.25, 0.5]]))
    inf = float("inf")
    barriers = [pkg.StickyBarriers(), pkg.StickyBarriers((2.5, inf), ("reflect", "reflect"), (inf, inf))]
    out = pkg.stickyzz(pkg.GaussianTarget(G, np.array([-3.0, 3.0])), 0.0, np.array([2.0, 5.0]), np.array([-1.0, 1.0]), T, np.full(2, 20.0),
                       pkg.ZigZag(G, np.zeros(2), np.ones(2)), barriers, seed=seed, adapt=True, factor=1.5, trace_capacity=4096,
                       consume=dict(dt=0.5, points=int(T / 0.5) + 64))
    tr, res = out[0], out[-1]
    assert res["hits_lo"][1] > 10 and res["frozen_lo"][1] == 0 and res["hits_hi"][1] == 0 and not res["hits_lo"][0]
    assert np.all(res["grid_x"][:, 1] >= 2.5 - 1e-12)  # the path stays above the wall
    gm = [float(np.cumsum(res["grid_x"][:, i])[-1]) / len(res["grid_t"]) for i in range(2)]  # (summed row by row, as the example does)
    for only in (0, 1):
        p = subprocess.run([exe, repr(T), hex(seed), str(only)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        f = p.stdout.split()
        assert float(f[0]) == res["T"] and int(f[1]) == (0 if only else len(tr.events))
        assert [float(v) for v in f[2:6]] == [gm[0], gm[1], float(res["mean"][0]), float(res["mean"][1])]
        assert int(f[6]) == int(res["hits_lo"][1]) and float(f[7]) == res["frozen_lo"][1]
