"""Every event-loop kernel's ∫x dt against the exact integral of its own trace (-m gpu).

The kernels keep I_i = ∫ x_i dt per coordinate next to (x, θ, t); the oracle has no such field and the events do not carry it, so the
bit-exact parity suites cannot see it.  Here an ensemble runs through the C ABI in PDMP_RUN_STOP_BEFORE slices with a trace buffer small
enough to refill; at EVERY slice end pdmp_ensemble_path_integrals(T_k, arange(d)) of every chain is compared with exact_path.ExactPath of
the events drained so far (rationals: no tolerance in the reference), every coordinate, inside the derived bound 3 (m_i + 1) u X_i L_i of
exact_path.py's docstring.  Each event-loop case asserts the kernel that ran, >= 1000 events per chain and >= 1 refill.

The reductions (zz_batch_means_kernel, zz_ess_kernel) are held to the same sums formed in Fraction from the device's own per-chain J;
the validity rule of T (pdmp_capi_stats.hip: fact_integrals_at) to the statuses it must refuse.

Digits lost in S_w = ΣY² − B·ΣM² at |mean| >> spread (B = 3, mean 5; every reduction case measures and prints it): with 63 chains or more
ΣY² is 1.1e2 (d = 3) to 1.1e3 .. 4.3e3 (d = 255, 257 and the lattice) times S_w, i.e. 2.0 to 3.7 decimal digits of the sums are given
up by the subtraction, and the device's S_w is off the exact one by 2e2 .. 5e4 u·S_w; with a single chain single coordinates lose up to
6.4 digits.  Not fixed: centred accumulators are a change of their own.
"""
from fractions import Fraction as Fr

import numpy as np
import pytest
import scipy.sparse as sp

import exact_path as E

pytestmark = pytest.mark.gpu

WORST = {}  # case id -> largest |J_dev − J_exact| / bound seen (printed; documents the room the bound leaves, asserts nothing new)


def _explain(k, i, s, Tk, got, want, bound, seg):
    lines = ["chain %d coordinate %d slice %d (T = %r): device %r exact %r |diff| %.3e bound %.3e" %
             (k, i, s, Tk, got, float(want), abs(got - float(want)), float(bound)), "the coordinate's events inside the slice:"]
    lines += ["    t = %r x = %r theta = %r" % (float(e["t"]), float(e["x"]), float(e["theta"])) for e in seg]
    return "\n".join(lines)


def run_case(pkg, name, *, G, nch, slices, cap, expect, c, Gt=None, mu_f=None, mu_t=None, sigma=None, lam=0.0, t0=0.0, kernel=None,
             sampler=None, adapt=False, factor=1.8, tracked=False, kappa=None, adaptscale=False, local_bound=False, nbr=None,
             logistic=None, moves="counters", seed=1, x0=None, th0=None, min_events=1000, need_refill=True, setup=None,
             frozen_exact=False):
    """One ensemble, slice by slice.  moves: 'own' (tracked evaluation: own events + 1), 'counters' (moving evaluation:
    num + nevents + 1) or 'draws' (LocalBound: renew events move a coordinate without counting as a proposal; every pop of the queue
    draws from the main stream, so ndraw_main + nevents + 1).  Returns (J per slice [nch x d], counters, events per chain)."""
    L = pkg._lib
    d = G.shape[0]
    rng = np.random.default_rng(seed)
    sg = np.ones(d) if sigma is None else sigma
    if x0 is None:
        x0 = rng.standard_normal((nch, d)) + (0.0 if mu_t is None else mu_t)
    if th0 is None:
        th0 = sg * rng.choice([-1.0, 1.0], (nch, d))
    seeds = np.arange(nch, dtype=np.uint64) + np.uint64(1000 + seed)
    kw = dict(adapt=adapt, factor=factor, trace_capacity=cap)
    if sampler is not None:
        kw["sampler"] = sampler
    out_J, paths = [], [E.ExactPath(t0, x0[k], th0[k]) for k in range(nch)]
    nev, refills, worst = np.zeros(nch, dtype=np.int64), 0, 0.0
    with pkg.Ensemble(nch, d, **kw) as ens:
        if kernel is not None:
            ens.debug_set_kernel(kernel)
        if setup is not None:
            setup(ens)
        mu = np.zeros(d) if mu_f is None else mu_f
        ens.set_flow(pkg.ZigZag(G, mu, sigma, λref=lam) if sigma is not None else pkg.ZigZag(G, mu, λref=lam))
        if nbr is not None:
            ens.set_neighbourhood(nbr)
        if logistic is not None:
            P, ksub = logistic
            ens.set_target(pkg.LogisticTarget(P["A"], P["y"], P["ny"], P["mu"], P["gamma0"], ksub))
        else:
            ens.set_target(pkg.GaussianTarget(G if Gt is None else Gt, mu_t))
        if kappa is not None:
            ens.set_sticky(kappa)
        if adaptscale:
            ens.set_adaptscale(True)
        if local_bound:
            ens.set_local_bound(True)
        if tracked:
            ens.set_gradient_tracking(True)
        ens.set_path_integrals(True)
        ens.set_state(t0, x0, th0, c, seeds)
        assert np.array_equal(ens.path_integrals(t0, np.arange(d)), np.zeros((nch, d)))  # J(t0) = 0 before the first run
        prev_J = None
        for s, Tk in enumerate(slices):
            seg = [[] for _ in range(nch)]
            while True:
                ens.run(Tk, L.RUN_STOP_BEFORE)
                cnt = ens.counters()
                assert not np.any((cnt["status"] == L.CHAIN_BOUND_VIOLATED) | (cnt["status"] == L.CHAIN_STALLED)), cnt["status"]
                for k in range(nch):
                    ev = ens.trace(k, counters=cnt)
                    seg[k].append(ev)
                    paths[k].feed(ev)
                    nev[k] += len(ev)
                ens.trace_reset()
                if not L.needs_rerun(cnt["status"]):
                    break
                refills += int(np.any(cnt["status"] == L.CHAIN_TRACE_FULL))
            kname = ens.kernel_name()
            assert kname == expect or (isinstance(expect, tuple) and kname in expect), (name, kname)
            J = ens.path_integrals(Tk, np.arange(d))
            assert J.shape == (nch, d)
            for k in range(nch):
                p = paths[k]
                want, X, Ln = p.J(Tk), p.absmax(Tk), p.length(Tk)
                shared = {"counters": int(cnt["num"][k]) + int(cnt["nevents"][k]) + 1,
                          "draws": int(cnt["ndraw_main"][k]) + int(cnt["nevents"][k]) + 1, "own": None}[moves]
                for i in range(d):
                    m = p.own[i] + 1 if shared is None else shared
                    b = E.bound_J(m, X[i], Ln[i])
                    err = abs(Fr(float(J[k, i])) - want[i])
                    if err > b:
                        own = [e for e in np.concatenate(seg[k]) if e["i"] == i]
                        raise AssertionError(name + ": " + _explain(k, i, s, Tk, float(J[k, i]), want[i], b, own))
                    if b:
                        worst = max(worst, float(err / b))
                    if frozen_exact and prev_J is not None and p.th[i] == 0 and p.t[i] <= Fr(float(slices[s - 1])):
                        # frozen over the whole slice (θ = 0 since before it began, no own event inside): EXACTLY the same J at both ends
                        assert J[k, i] == prev_J[k, i], (name, k, i, s, J[k, i], prev_J[k, i])
            prev_J = J
            out_J.append(J)
    WORST[name] = worst
    print("%s [%s]: events per chain %s, refills %d, largest |J_dev - J_exact| / bound %.3g" % (name, kname, nev.tolist(), refills, worst))
    assert nev.min() >= min_events, (name, nev)
    if need_refill:
        assert refills >= 1, name
    return out_J, cnt, paths


# ---------------------------------------------------------------------------------------------- forms of the local ZigZag, Gaussian lattice

SPEC8G = ("zz_local_spec8g_kernel", "zz_local_spec8g_kernel<GW=16>")  # (8 or 16 lanes per event, by the graph's two-hop sets)
KNAME = {"seq": "zz_local_run_kernel", "spec4": "zz_local_spec_kernel", "spec8": "zz_local_spec8_kernel"}


@pytest.mark.parametrize("form", ["seq", "spec4", "spec8"])
def test_lattice128_moving_forms(gpu_pkg, monkeypatch, form):
    """d = 16384 (test_gpu_spec8_parity.py's size): the one-event, 4-event and 8-event kernels of the moving evaluation."""
    pkg = gpu_pkg
    monkeypatch.setenv("PDMP_KERNEL", form)
    G = pkg.problems.gmrf_precision(128)
    run_case(pkg, "lattice128-" + form, G=G, nch=2, slices=(0.06, 0.11), cap=700, expect=KNAME[form], c=pkg.problems.column_norms(G), seed=3)


@pytest.mark.parametrize("form,which", [("spec8g", "random6"), ("wide", "random6"), ("spec8g", "lattice3d")])
def test_generic_graph_moving_forms(gpu_pkg, monkeypatch, form, which):
    """Off the lattice (test_gpu_spec_wide.py's graphs): zz_local_spec8g_kernel (two records I, I2 in flight) and the wide-zone 4-event kernel."""
    pkg = gpu_pkg
    monkeypatch.setenv("PDMP_KERNEL", "auto" if form == "spec8g" else "spec4")
    G = pkg.problems.random_sparse_precision(2500, 6, seed=3) if which == "random6" else pkg.problems.lattice3d_precision(14)
    run_case(pkg, "%s-%s" % (which, form), G=G, nch=2, slices=(0.5, 1.0, 1.4), cap=900,
             expect=SPEC8G if form == "spec8g" else "zz_local_spec_kernel<WIDE>", c=pkg.problems.column_norms(G), seed=4)


def test_lattice48_tracked_forms(gpu_pkg, trackp_form):
    """The one-proposal-per-lane tracked kernel: one wave, two waves (o.Ia committed by the helper's line), the line layout (cc.I packed and
    unpacked around every read)."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(48)
    expect = {"one_wave": "zz_local_trackp_kernel", "two_waves": "zz_local_trackp2_kernel", "lines": "zz_local_trackl_kernel"}[trackp_form]
    run_case(pkg, "lattice48-tracked-" + trackp_form, G=G, nch=3, slices=(0.4, 0.9, 1.3), cap=800, expect=expect,
             c=pkg.problems.column_norms(G), tracked=True, moves="own", seed=5)


@pytest.mark.parametrize("form", ["one_wave", "two_waves"])  # (the line layout does not serve a generic graph)
def test_generic_graph_tracked_forms(gpu_pkg, monkeypatch, form):
    pkg = gpu_pkg
    trackp_form = form
    monkeypatch.setenv("PDMP_HELPER_WAVE", "1" if form == "two_waves" else "0")
    monkeypatch.setenv("PDMP_TRACK_LINES", "0")
    G = pkg.problems.random_sparse_precision(2500, 6, seed=3)
    expect = "zz_local_trackp2_kernel<LAT=false>" if trackp_form == "two_waves" else "zz_local_trackp_kernel<LAT=false>"
    run_case(pkg, "random6-tracked-" + trackp_form, G=G, nch=2, slices=(0.5, 1.0, 1.4), cap=900, expect=expect,
             c=pkg.problems.column_norms(G), tracked=True, moves="own", seed=6)


def test_lattice48_tracked_8_lane_groups(gpu_pkg):
    """zz_local_track_kernel: what a target mean of its own (Γμ_target ≠ Γμ_flow) keeps under gradient tracking."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(48)
    rng = np.random.default_rng(3)
    mu = 0.3 * rng.standard_normal(G.shape[0])
    run_case(pkg, "lattice48-tracked-groups-different-means", G=G, nch=2, slices=(0.5, 1.2), cap=900, expect="zz_local_track_kernel",
             c=3.0 * pkg.problems.column_norms(G), mu_f=mu, mu_t=0.5 * mu, tracked=True, moves="own", seed=7)


def test_lattice136_tracked_big_form(gpu_pkg):
    """d = 18496 > 16384: zz_local_trackp_big_kernel, one wave per chain."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(136)
    run_case(pkg, "lattice136-tracked-big", G=G, nch=2, slices=(0.05, 0.1), cap=700, expect="zz_local_trackp_big_kernel",
             c=pkg.problems.column_norms(G), tracked=True, moves="own", seed=8)


# ---------------------------------------------------------------------------------------------- options

def _lattice48(pkg):
    G = pkg.problems.gmrf_precision(48)
    return G, G.shape[0], pkg.problems.column_norms(G)


@pytest.mark.parametrize("form", ["seq", "spec8"])
def test_option_means_and_speeds(gpu_pkg, monkeypatch, form):
    """Target mean = flow mean ≈ 5 and speeds σ_i in [0.5, 2]."""
    pkg = gpu_pkg
    monkeypatch.setenv("PDMP_KERNEL", form)
    G, d, c = _lattice48(pkg)
    rng = np.random.default_rng(11)
    mu, sg = 5.0 + 0.3 * rng.standard_normal(d), rng.uniform(0.5, 2.0, d)
    run_case(pkg, "lattice48-%s-mean-speeds" % form, G=G, nch=2, slices=(0.4, 0.9), cap=900, expect=KNAME[form], c=4.0 * c, mu_f=mu, mu_t=mu,
             sigma=sg, seed=12)


@pytest.mark.parametrize("form", ["seq", "spec8", "tracked"])
def test_option_t0_is_3(gpu_pkg, monkeypatch, form):
    """t0 = 3: the first queue times are drawn without t0, so every coordinate's first move has dt < 0; J counts from t0."""
    pkg = gpu_pkg
    monkeypatch.setenv("PDMP_KERNEL", "auto" if form == "tracked" else form)
    monkeypatch.setenv("PDMP_HELPER_WAVE", "1")
    G, d, c = _lattice48(pkg)
    tracked = form == "tracked"
    _, _, paths = run_case(pkg, "lattice48-%s-t0=3" % form, G=G, nch=2, slices=(3.5, 4.0), cap=700, t0=3.0, c=c, tracked=tracked,
                             expect="zz_local_trackp2_kernel" if tracked else KNAME[form], moves="own" if tracked else "counters", seed=13)
    assert all(max(p.length(4.0)) > 3.0 for p in paths)  # (first events lie before t0: a path longer than T − t0 = 1)


@pytest.mark.parametrize("form", ["seq", "spec8", "tracked"])
def test_option_adapt_from_bounds_that_start_too_small(gpu_pkg, monkeypatch, form):
    pkg = gpu_pkg
    monkeypatch.setenv("PDMP_KERNEL", "auto" if form == "tracked" else form)
    monkeypatch.setenv("PDMP_HELPER_WAVE", "0")
    G, d, c = _lattice48(pkg)
    c = c.copy()
    c[::11] = 1e-300  # (test_tracked_adapt_on_the_one_proposal_per_lane_kernel: with Γ_bound = Γ_target only a vanishing c_i is ever violated)
    tracked = form == "tracked"
    run_case(pkg, "lattice48-%s-adapt" % form, G=G, nch=2, slices=(0.5, 1.1), cap=900, c=c, adapt=True, tracked=tracked,
                         expect="zz_local_trackp_kernel" if tracked else KNAME[form], moves="own" if tracked else "counters", seed=14)


@pytest.mark.parametrize("form", ["seq", "spec4", "spec8"])
def test_option_refresh_clock_on_the_lattice(gpu_pkg, monkeypatch, form):
    """λref = 2 (test_refresh_clock_on_the_speculative_kernel's configuration): the refreshed coordinate is recorded at its own stale clock."""
    pkg = gpu_pkg
    monkeypatch.setenv("PDMP_KERNEL", form)
    G, d, c = _lattice48(pkg)
    rng = np.random.default_rng(48)
    sg = 0.5 + rng.random(d)
    _, cnt, _ = run_case(pkg, "lattice48-%s-refresh" % form, G=G, nch=2, slices=(0.6, 1.2), cap=500, expect=KNAME[form], c=4.0 * c, sigma=sg,
                         lam=2.0, seed=15)
    assert cnt["nrefresh"].min() >= 2


@pytest.mark.parametrize("form", ["seq", "spec8g"])
def test_option_refresh_clock_off_the_lattice(gpu_pkg, monkeypatch, form):
    pkg = gpu_pkg
    monkeypatch.setenv("PDMP_KERNEL", "auto" if form == "spec8g" else form)
    G = pkg.problems.random_sparse_precision(2500, 6, seed=5)
    d = G.shape[0]
    sg = 0.5 + np.random.default_rng(d).random(d)
    _, cnt, _ = run_case(pkg, "random6-%s-refresh" % form, G=G, nch=2, slices=(0.7, 1.4), cap=1200,
                         expect=SPEC8G if form == "spec8g" else KNAME["seq"], c=4.0 * pkg.problems.column_norms(G), sigma=sg,
                         lam=3.0, seed=16)
    assert cnt["nrefresh"].min() >= 2


def test_option_adaptscale_general_kernel(gpu_pkg):
    """spdmp(...; adaptscale = true): |θ_i| changes at a refresh (zz_general_run_kernel is the only kernel that serves it)."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(12)
    d = G.shape[0]
    sg = np.full(d, 2.0)
    _, cnt, paths = run_case(pkg, "lattice12-general-adaptscale", G=G, nch=2, slices=(8.0, 16.0, 24.0), cap=700, expect="zz_general_run_kernel",
                             c=6.0 * pkg.problems.column_norms(G), sigma=sg, lam=0.5, adapt=True, adaptscale=True, seed=17)
    assert cnt["nrefresh"].min() > 5 and any(abs(p.th[i]) != 2 for p in paths for i in range(d))  # (speeds did change)


def test_option_local_bound_general_kernel(gpu_pkg):
    """c::LocalBound: renew events between the proposals."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(12)
    d = G.shape[0]
    rng = np.random.default_rng(9)
    c = pkg.problems.column_norms(G) * (1.0 + 0.01 * rng.random(d))
    run_case(pkg, "lattice12-general-localbound", G=G, nch=2, slices=(5.0, 10.0, 15.0), cap=500, expect="zz_general_run_kernel", c=c, adapt=True,
             local_bound=True, moves="draws", seed=18)


def test_option_neighbourhood_larger_than_G1_general_kernel(gpu_pkg):
    """G ⊋ G1 (test_gpu_neighbourhood.py): the bound's Γ lacks the couplings between chunks, G is the target's pattern; the clocks of
    G[i] minus G1[i] move at every proposal of i.  An explicit neighbourhood runs on zz_general_run_kernel whatever PDMP_KERNEL says."""
    pkg = gpu_pkg
    n, K = 20, 5
    G = pkg.problems.gmrf_precision(n)
    d = n * n
    coo = sp.coo_matrix(G)
    keep = (coo.row // (d // K)) == (coo.col // (d // K))
    Gb = sp.csc_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), shape=G.shape)
    Gb.sort_indices()
    P = sp.csc_matrix((np.ones(G.nnz), G.indices.copy(), G.indptr.copy()), shape=G.shape)
    run_case(pkg, "lattice20-general-G-larger-than-G1", G=Gb, Gt=G, nbr=P, nch=2, slices=(3.0, 6.0, 9.0), cap=600,
             expect="zz_general_run_kernel", c=0.5 * pkg.problems.column_norms(G), adapt=True, factor=1.7, seed=19)


def test_option_G_is_All(gpu_pkg):
    """pdmp = spdmp with G = All(): sweep_all moves every coordinate at every proposal."""
    pkg = gpu_pkg
    G = pkg.problems.gmrf_precision(8)
    run_case(pkg, "lattice8-seq-All", G=G, nch=3, slices=(12.0, 24.0, 40.0), cap=600, expect="zz_local_run_kernel", c=pkg.problems.column_norms(G),
             sampler=pkg._lib.SAMPLER_ZIGZAG_ALL, seed=20)


# ---------------------------------------------------------------------------------------------- sticky

@pytest.mark.parametrize("form", ["seq", "spec"])
def test_sticky_kernels(gpu_pkg, monkeypatch, form):
    """zz_sticky_run_kernel / zz_sticky_spec_kernel: a frozen coordinate has θ = 0 -- I stops growing, resumes at the thaw; a coordinate
    frozen over a whole slice has EXACTLY the same J at both ends."""
    pkg = gpu_pkg
    monkeypatch.setenv("PDMP_KERNEL", "seq" if form == "seq" else "auto")
    G = pkg.problems.gmrf_precision(48, 0.5)
    d = G.shape[0]
    _, cnt, paths = run_case(pkg, "lattice48-sticky-" + form, G=G, nch=2, slices=(0.6, 1.0, 1.4, 1.8), cap=900,
                             expect="zz_sticky_run_kernel" if form == "seq" else "zz_sticky_spec_kernel", c=1.5 * pkg.problems.column_norms(G),
                             sampler=pkg._lib.SAMPLER_STICKY_ZIGZAG, factor=1.5, kappa=np.full(d, 0.8), seed=21, frozen_exact=True)
    assert min(sum(1 for i in range(d) if p.th[i] == 0) for p in paths) > 20  # (frozen at the end; every one of them froze at an event)


# ---------------------------------------------------------------------------------------------- general / logistic

def test_general_kernel_dense_ish_gaussian(gpu_pkg):
    pkg = gpu_pkg
    rng = np.random.default_rng(3)
    d = 150
    R = sp.random(d, d, density=0.08, random_state=rng, data_rvs=rng.standard_normal, format="csc")
    G = sp.csc_matrix(R @ R.T + 2.0 * sp.identity(d))
    G.sort_indices()
    run_case(pkg, "dense150-general", G=sp.csc_matrix(0.8 * G), Gt=G, nch=3, slices=(20.0, 40.0, 60.0), cap=500, expect="zz_general_run_kernel",
             c=1.5 * pkg.problems.column_norms(G), adapt=True, seed=22)


def test_general_kernel_G_is_All_with_a_refresh_clock(gpu_pkg):
    """pdmp (G = All()) on a graph whose neighbourhoods exceed one wavefront: zz_general_run_kernel's move_everything -- a site no other
    case reaches (a left-endpoint mutation of it survived the rest of this file)."""
    pkg = gpu_pkg
    rng = np.random.default_rng(6)
    d = 150
    R = sp.random(d, d, density=0.08, random_state=rng, data_rvs=rng.standard_normal, format="csc")
    G = sp.csc_matrix(R @ R.T + 2.0 * sp.identity(d))
    G.sort_indices()
    _, cnt, _ = run_case(pkg, "dense150-general-All-refresh", G=G, nch=2, slices=(4.0, 8.0, 12.0), cap=500, expect="zz_general_run_kernel",
                         c=2.0 * pkg.problems.column_norms(G), sigma=np.ones(d), lam=0.3, sampler=pkg._lib.SAMPLER_ZIGZAG_ALL, seed=28)
    assert cnt["nrefresh"].min() >= 2


@pytest.mark.parametrize("form", ["lds", "lds-tracked-bounds", "hbm"])
def test_c4_logistic_kernels(gpu_pkg, form):
    """Config C4 (subsampled logistic target): the LDS-resident kernel with the integrals on (template WITH_I: II[j]), with tracked bounds,
    and the same chains with the records in HBM (zz_general_run_kernel)."""
    pkg = gpu_pkg
    P = pkg.problems.logistic_problem(m=20)
    d, nch = P["p"], 3
    rng = np.random.default_rng(4)
    x0 = np.tile(P["x0"], (nch, 1)) + 0.01 * rng.standard_normal((nch, d))
    th0 = P["sigma"] * rng.choice([-1.0, 1.0], (nch, d))
    run_case(pkg, "c4-" + form, G=P["Gdrop"], mu_f=P["mu"], sigma=P["sigma"], logistic=(P, 10), nch=nch, slices=(3.0, 6.0, 9.0), cap=300,
             expect="zz_general_run_kernel" if form == "hbm" else "zz_logistic_lds_kernel", kernel="seq" if form == "hbm" else "auto",
             c=P["c"], adapt=True, factor=5.0, tracked=form == "lds-tracked-bounds", x0=x0, th0=th0, seed=23)


def test_c5_sticky_logistic_small_p(gpu_pkg):
    """Config C5 (spike-and-slab logistic regression, sticky ZigZag under the subsampled logistic target) at p = 600."""
    pkg = gpu_pkg
    P = pkg.problems.spike_slab_logistic_problem(p=600, num_rows=300)
    p, nch = P["p"], 2
    rng = np.random.default_rng(5)
    x0 = rng.standard_normal((nch, p))
    th0 = P["sigma"] * rng.choice([-1.0, 1.0], (nch, p))
    _, cnt, paths = run_case(pkg, "c5-sticky-logistic-p600", G=P["G"], mu_f=P["mu"], sigma=P["sigma"], logistic=(P, 12), nch=nch,
                             slices=(2.0, 4.0, 6.0), cap=300, expect="zz_general_run_kernel", c=P["c"], adapt=True, factor=1.5,
                             sampler=pkg._lib.SAMPLER_STICKY_ZIGZAG, kappa=P["kappa"], x0=x0, th0=th0, seed=27, frozen_exact=True)
    assert min(sum(1 for i in range(p) if q.th[i] == 0) for q in paths) > 20


@pytest.mark.parametrize("rows", [16, 32])
def test_c4_logistic_rows_kernel(gpu_pkg_parity, rows):
    pkg = gpu_pkg_parity
    P = pkg.problems.logistic_problem(m=20)
    d, nch = P["p"], 6
    rng = np.random.default_rng(4)
    x0 = np.tile(P["x0"], (nch, 1))
    th0 = P["sigma"] * rng.choice([-1.0, 1.0], (nch, d))
    run_case(pkg, "c4-rows%d" % rows, G=P["Gdrop"], mu_f=P["mu"], sigma=P["sigma"], logistic=(P, 10), nch=nch, slices=(4.5, 9.0), cap=300,
             expect="zz_logistic_rows_kernel", setup=lambda e: e.debug_set_logistic_rows(rows), c=P["c"], adapt=True, factor=5.0, x0=x0, th0=th0,
             seed=24)


def test_lattice48_exactp_kernel(gpu_pkg_parity):
    """zz_local_exactp_kernel (parity library): the moving evaluation with one proposal per lane."""
    pkg = gpu_pkg_parity
    G = pkg.problems.gmrf_precision(48)
    run_case(pkg, "lattice48-exactp", G=G, nch=2, slices=(0.5, 1.1), cap=900, expect="zz_local_exactp_kernel", kernel="exactp",
             c=pkg.problems.column_norms(G), seed=25)


# ---------------------------------------------------------------------------------------------- relaunches

@pytest.mark.parametrize("form", ["spec8", "tracked"])
def test_paused_relaunches_leave_J_bit_for_bit(gpu_pkg, monkeypatch, form):
    """PDMP_LAUNCH_COUNT_LIMIT = 3000 (>= 5 pauses per slice): J(T) equals the unpaused run's bit for bit, and the exact one within the bound."""
    pkg = gpu_pkg
    G, d, c = _lattice48(pkg)
    tracked = form == "tracked"
    monkeypatch.setenv("PDMP_HELPER_WAVE", "1")
    res = []
    for limit in ("0", "3000"):
        monkeypatch.setenv("PDMP_LAUNCH_COUNT_LIMIT", limit)
        res.append(run_case(pkg, "lattice48-%s-pauses-limit=%s" % (form, limit), G=G, nch=2, slices=(0.7, 1.4), cap=100000, c=c, tracked=tracked,
                            expect="zz_local_trackp2_kernel" if tracked else KNAME["spec8"], moves="own" if tracked else "counters", seed=26,
                            need_refill=False))
    (J0, c0, _), (J1, c1, _) = res
    assert c1["ndraw_main"].min() > 5 * 3000
    for a, b in zip(J0, J1):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------- reductions

def _tridiagonal(d):
    main = 2.0 + 0.1 * np.arange(d)
    return sp.diags([main] + [[-1.0] * (d - 1)] * 2, [0, -1, 1], format="csc")


def _check_sum(name, got, terms, n):
    """got [d] device sums against Σ_chains terms[k][i] (Fractions), bound (n + 3) u Σ|terms|."""
    worst = 0.0
    for i in range(len(got)):
        col = [t[i] for t in terms]
        want, b = sum(col, Fr(0)), E.bound_sum(n, col)
        err = abs(Fr(float(got[i])) - want)
        assert err <= b, (name, i, float(got[i]), float(want), float(err), float(b))
        if b:
            worst = max(worst, float(err / b))
    return worst


def _reduction_case(pkg, name, G, nch, c, mu, tracked, Ts, kernel, t0=0.0):
    """batch_means over two consecutive batches, then ess_begin / three ess_batch / ess_end -- each against the same sums formed in Fraction
    from the device's own path_integrals at all d coordinates."""
    L = pkg._lib
    d = G.shape[0]
    rng = np.random.default_rng(nch * 1000 + d)
    x0 = mu + rng.standard_normal((nch, d))
    th0 = rng.choice([-1.0, 1.0], (nch, d))
    worst = 0.0
    sq = lambda rows: [[v * v for v in r] for r in rows]
    with pkg.Ensemble(nch, d) as ens:
        if not tracked:
            ens.debug_set_kernel("seq")
        ens.set_flow(pkg.ZigZag(G, mu))
        ens.set_target(pkg.GaussianTarget(G, mu))
        if tracked:
            ens.set_gradient_tracking(True)
        ens.set_state(t0, x0, th0, c, np.arange(nch, dtype=np.uint64) + np.uint64(77))
        Jf = [[[Fr(0)] * d for _ in range(nch)]]  # J(t0) = 0: the first batch_means starts at t0 with jprev = 0

        def advance(T):  # run to T and keep the device's own per-chain J(T) at all d coordinates, as rationals
            ens.run(T, L.RUN_STOP_BEFORE)
            J = ens.path_integrals(T, np.arange(d))
            Jf.append([[Fr(float(v)) for v in J[k]] for k in range(nch)])

        def batch(a, b, Ta, Tb):  # per chain and coordinate: y = (J(Tb) − J(Ta)) / (Tb − Ta), exactly
            w = Fr(float(Tb)) - Fr(float(Ta))
            return [[(Jf[b][k][i] - Jf[a][k][i]) / w for i in range(d)] for k in range(nch)]

        advance(Ts[0])
        sy, sy2 = ens.batch_means(t0, Ts[0])
        y = batch(0, 1, t0, Ts[0])
        worst = max(worst, _check_sum(name + " batch 1 ΣY", sy, y, nch), _check_sum(name + " batch 1 ΣY²", sy2, sq(y), nch))
        advance(Ts[1])
        sy, sy2 = ens.batch_means(Ts[0], Ts[1])
        y = batch(1, 2, Ts[0], Ts[1])
        worst = max(worst, _check_sum(name + " batch 2 ΣY", sy, y, nch), _check_sum(name + " batch 2 ΣY²", sy2, sq(y), nch))
        ens.ess_begin(Ts[1])
        ys = []
        for q in (2, 3, 4):
            advance(Ts[q])
            ens.ess_batch(Ts[q])
            ys.append(batch(q, q + 1, Ts[q - 1], Ts[q]))
        sy, sy2, sm, sm2, nb, t0, t1 = ens.ess_end()
        assert (nb, t0, t1) == (3, Ts[1], Ts[4])
        cnt = ens.counters()
        assert np.all(cnt["status"] == L.CHAIN_OK) and cnt["nevents"].min() > 0
        assert ens.kernel_name() == kernel, ens.kernel_name()
        allY = [r for yb in ys for r in yb]  # 3 nch terms per coordinate
        worst = max(worst, _check_sum(name + " ess ΣY", sy, allY, 3 * nch), _check_sum(name + " ess ΣY²", sy2, sq(allY), 3 * nch))
        M = batch(2, 5, Ts[1], Ts[4])
        worst = max(worst, _check_sum(name + " ess ΣM", sm, M, nch), _check_sum(name + " ess ΣM²", sm2, sq(M), nch))
        # what the caller forms next: S_w = ΣY² − B·ΣM² (B = 3).  Measured, not asserted: how much larger ΣY² is than S_w (the digits the
        # subtraction gives up) and the error of the device's S_w against the exact one, in units of u·S_w
        lost, err_u = [], []
        for i in range(d):
            ey2, em2 = sum((v[i] * v[i] for v in allY), Fr(0)), sum((v[i] * v[i] for v in M), Fr(0))
            sw = ey2 - 3 * em2
            if sw > 0:
                lost.append(float(ey2 / sw))
                err_u.append(float(abs(Fr(float(sy2[i])) - 3 * Fr(float(sm2[i])) - sw) / sw / E.U))
    WORST[name] = worst
    print("%s: largest |sum_dev - sum_exact| / bound %.3g; S_w = ΣY² − 3 ΣM²: ΣY² / S_w median %.3g max %.3g (digits lost %.1f .. %.1f), "
          "error of the device's S_w up to %.3g u" % (name, worst, float(np.median(lost)), max(lost), np.log10(np.median(lost)),
                                                       np.log10(max(lost)), max(err_u)))


@pytest.mark.parametrize("d", [3, 255, 257])
@pytest.mark.parametrize("nch", [1, 63, 64, 65, 130])
def test_reductions_tridiagonal_64_byte_records(gpu_pkg, nch, d):
    """zz_batch_means_kernel / zz_ess_kernel (all three modes) around the launcher's switch to 64 chain groups of ceil(n / 64) at n = 64
    (65 leaves groups empty), target mean ≈ 5.  n = 1 is the hard case for the sums of squares: a square of a thrice-rounded mean carries 7u,
    more than (n + 3) u = 4 u; the kernels round every batch mean and its square once (exact_path.py's docstring)."""
    pkg = gpu_pkg
    G = _tridiagonal(d)
    mu = 5.0 + 0.1 * np.cos(np.arange(d))
    _reduction_case(pkg, "reduce-tridiag-n%d-d%d" % (nch, d), G, nch, pkg.problems.column_norms(G) + 0.1, mu, False, (1.0, 2.0, 3.0, 4.0, 5.0),
                    kernel="zz_local_run_kernel")


def test_reductions_tridiagonal_t0_is_3(gpu_pkg):
    """t0 = 3: the first batch_means starts at t0 with jprev = 0 (J counts from t0), ess_begin later -- 65 chains, d = 257."""
    pkg = gpu_pkg
    G = _tridiagonal(257)
    mu = 5.0 + 0.1 * np.cos(np.arange(257))
    _reduction_case(pkg, "reduce-tridiag-n65-d257-t0=3", G, 65, pkg.problems.column_norms(G) + 0.1, mu, False, (3.5, 4.0, 4.5, 5.0, 5.5),
                    kernel="zz_local_run_kernel", t0=3.0)


def test_reductions_lattice48_tracked_128_byte_records(gpu_pkg):
    pkg = gpu_pkg
    G, d, c = _lattice48(pkg)
    mu = np.full(d, 5.0)  # (flow mean = target mean: the one-proposal-per-lane tracked kernel serves it; records of 128 bytes)
    _reduction_case(pkg, "reduce-lattice48-tracked-n65", G, 65, 3.0 * c, mu, True, (0.1, 0.2, 0.3, 0.4, 0.5), kernel="zz_local_trackp2_kernel")


# ---------------------------------------------------------------------------------------------- validity of T

def _validity_ensemble(pkg, nch=3, cap=400, tracked=False, c_scale=1.0, Gb_scale=1.0):
    G, d, c = _lattice48(pkg)
    ens = pkg.Ensemble(nch, d, trace_capacity=cap)
    ens.set_flow(pkg.ZigZag(sp.csc_matrix(Gb_scale * G), np.zeros(d)))
    ens.set_target(pkg.GaussianTarget(G))
    if tracked:
        ens.set_gradient_tracking(True)
    ens.set_state_synthetic(0.0, c_scale * c, 4242)
    return ens, d


def _refused_everywhere(pkg, ens, d, T, T_prev, words):
    """batch_means, ess_batch (after a valid ess_begin was made by the caller), path_integrals and ess_begin at T: PDMP_ERR_INVALID with a
    message naming what is wrong."""
    L = pkg._lib
    for call in (lambda: ens.batch_means(T_prev, T), lambda: ens.ess_batch(T), lambda: ens.path_integrals(T, np.arange(d)),
                 lambda: ens.ess_begin(T)):
        with pytest.raises(L.PdmpError) as ei:
            call()
        assert ei.value.code == L.PDMP_ERR_INVALID, str(ei.value)
        assert all(w in str(ei.value) for w in words), str(ei.value)


@pytest.mark.parametrize("why", ["trace_full", "paused", "bound_violated_chain_cannot_resume", "reference_tail_passed_T", "beyond_the_run"])
def test_reads_at_a_T_the_state_does_not_describe_are_refused(gpu_pkg, why):
    """J_i(T) extrapolates every coordinate linearly from its clock: it is the path's integral only where no event lies in between.  A chain
    short of T (TRACE_FULL, PAUSED, BOUND_VIOLATED), a reference-tail run that passed T, a T beyond what was run: each of batch_means,
    ess_begin, ess_batch and path_integrals returns PDMP_ERR_INVALID naming chain and times, and leaves jprev and the accumulators alone --
    the correct reads afterwards give exactly what an undisturbed twin ensemble gives.  A BOUND_VIOLATED chain never resumes, so no
    correct read can follow there: that case shows the accumulators untouched by ess_end finding no batch counted.
    (Before the rule existed every one of these returned PDMP_OK and a number.)"""
    pkg = gpu_pkg
    L = pkg._lib
    violated = why == "bound_violated_chain_cannot_resume"
    T1, T2, T3 = (1e-4 if violated else 0.3), 0.6, 0.9  # (violated: a first slice so short that no chain has met its bound yet)
    kw = dict(c_scale=1e-3, Gb_scale=0.5) if violated else {}
    cap = 150 if why == "trace_full" else 100000
    twin, d = _validity_ensemble(pkg, cap=100000, **kw)
    ens, _ = _validity_ensemble(pkg, cap=cap, **kw)
    with twin, ens:
        for e in (twin, ens):
            e.run(T1, L.RUN_STOP_BEFORE)
        if why == "trace_full":
            cnt = ens.counters()
            assert np.all(cnt["status"] == L.CHAIN_TRACE_FULL) and np.all(cnt["t_last"] < T1)
            with pytest.raises(L.PdmpError) as ei:
                ens.batch_means(0.0, T1)
            assert ei.value.code == L.PDMP_ERR_INVALID and "chain 0" in str(ei.value) and "status 3" in str(ei.value) and "%.17g" % T1 in str(ei.value)
            while L.needs_rerun(ens.counters()["status"]):
                ens.trace_reset()
                ens.run(T1, L.RUN_STOP_BEFORE)
            ens.trace_reset()
        assert violated or np.all(twin.counters()["status"] == L.CHAIN_OK)
        for e in (twin, ens):
            e.batch_means(0.0, T1)
            e.ess_begin(T1)
        Tr = T2  # where the correct reads are made afterwards
        if violated:
            assert np.all(ens.counters()["status"] == L.CHAIN_OK)
            ens.run(T2, L.RUN_STOP_BEFORE)
            cnt = ens.counters()
            assert np.any(cnt["status"] == L.CHAIN_BOUND_VIOLATED)
            k = int(np.flatnonzero(cnt["status"] != L.CHAIN_OK)[0])
            assert cnt["status"][k] == L.CHAIN_BOUND_VIOLATED and cnt["t_last"][k] < T2
            _refused_everywhere(pkg, ens, d, T2, T1, ("chain %d" % k, "status 1", "%.17g" % T2))
            with pytest.raises(L.PdmpError) as ei:  # the refused ess_batch counted no batch
                ens.ess_end()
            assert "no batch accumulated" in str(ei.value)
            return
        if why == "trace_full":
            ens.run(T2, L.RUN_STOP_BEFORE)
            assert np.all(ens.counters()["status"] == L.CHAIN_TRACE_FULL)
            _refused_everywhere(pkg, ens, d, T2, T1, ("chain 0", "status 3", "%.17g" % T2))
            while L.needs_rerun(ens.counters()["status"]):
                ens.trace_reset()
                ens.run(T2, L.RUN_STOP_BEFORE)
        elif why == "paused":
            L.check(ens._L.pdmp_debug_set_launch_count_limit(ens._h, 2000))
            ens.run(T2, L.RUN_STOP_BEFORE)
            cnt = ens.counters()
            assert np.all(cnt["status"] == L.CHAIN_PAUSED) and np.all(cnt["t_last"] < T2)
            _refused_everywhere(pkg, ens, d, T2, T1, ("chain 0", "status 4", "%.17g" % T2))
            while L.needs_rerun(ens.counters()["status"]):
                ens.run(T2, L.RUN_STOP_BEFORE)
        elif why == "reference_tail_passed_T":
            ens.run(T2, L.RUN_REFERENCE_TAIL)
            cnt = ens.counters()
            assert np.all(cnt["status"] == L.CHAIN_OK) and np.all(cnt["t_last"] >= T2)
            _refused_everywhere(pkg, ens, d, T2, T1, ("chain 0", "%.17g" % T2, "%.17g" % float(cnt["t_last"][0])))
            Tr = T3  # (the state has passed T2 for good: the next time both ensembles describe is the end of a further slice)
            ens.run(T3, L.RUN_STOP_BEFORE)
        elif why == "beyond_the_run":
            _refused_everywhere(pkg, ens, d, T2, T1, ("%.17g" % T2, "%.17g" % T1, "horizon"))
            ens.run(T2, L.RUN_STOP_BEFORE)
        twin.run(Tr, L.RUN_STOP_BEFORE)
        # the refused calls touched nothing: the correct reads equal the undisturbed twin's, bit for bit
        assert np.array_equal(ens.path_integrals(Tr, np.arange(d)), twin.path_integrals(Tr, np.arange(d)))
        a, b = ens.batch_means(T1, Tr), twin.batch_means(T1, Tr)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.all(a[1] > 0)
        for e in (twin, ens):
            e.ess_batch(Tr)
        ra, rb = ens.ess_end(), twin.ess_end()
        for u, v in zip(ra, rb):
            assert np.array_equal(u, v)
        # an earlier time is refused too once the chains have passed it
        with pytest.raises(L.PdmpError) as ei:
            ens.path_integrals(T1, np.arange(d))
        assert ei.value.code == L.PDMP_ERR_INVALID and "last proposal" in str(ei.value)


def test_partitioned_run_leaves_no_T_to_read(gpu_pkg):
    """pdmp_ensemble_run_partitioned ends once EVERY chunk has processed a proposal at or past T, each at its own time (t_last is the
    earliest of them): zz_partitioned_run_kernel writes I, but no T exists at which the whole chain's J is the integral of its path, and the
    rule refuses the read instead of extrapolating the chunks that went further backwards."""
    pkg = gpu_pkg
    L = pkg._lib
    n, K = 16, 4
    G = pkg.problems.gmrf_precision(n)
    d = n * n
    coo = sp.coo_matrix(G)
    keep = (coo.row // (d // K)) == (coo.col // (d // K))
    Gb = sp.csc_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), shape=G.shape)
    Gb.sort_indices()
    rng = np.random.default_rng(1)
    with pkg.Ensemble(1, d, trace_capacity=8192) as ens:
        ens.set_flow(pkg.ZigZag(Gb, np.zeros(d)))
        ens.set_target(pkg.GaussianTarget(Gb))
        ens.set_state(0.0, rng.standard_normal((1, d)), rng.choice([-1.0, 1.0], (1, d)), pkg.problems.column_norms(G), np.array([1], dtype=np.uint64))
        ens.run_partitioned(1.0, K, 0.1)
        cnt = ens.counters()
        assert cnt["status"][0] == L.CHAIN_OK and cnt["t_last"][0] > 1.0 and cnt["nevents"][0] > 50
        for T in (1.0, float(cnt["t_last"][0])):
            with pytest.raises(L.PdmpError) as ei:
                ens.path_integrals(T, np.arange(d))
            assert ei.value.code == L.PDMP_ERR_INVALID


def test_refresh_clock_reads_only_at_the_horizon(gpu_pkg):
    """λref > 0: the proposals are not processed in time order, t_last is not the latest of them -- T must equal the last run's horizon."""
    pkg = gpu_pkg
    L = pkg._lib
    G, d, c = _lattice48(pkg)
    with pkg.Ensemble(2, d) as ens:
        ens.set_flow(pkg.ZigZag(G, np.zeros(d), λref=2.0))
        ens.set_target(pkg.GaussianTarget(G))
        ens.set_state_synthetic(0.0, 4.0 * c, 99)
        ens.run(0.5, L.RUN_STOP_BEFORE)
        J = ens.path_integrals(0.5, np.arange(d))
        t_last = float(ens.counters()["t_last"].max())
        assert t_last < 0.5
        with pytest.raises(L.PdmpError) as ei:
            ens.path_integrals(0.5 * (t_last + 0.5), np.arange(d))  # t_last <= T < horizon: fine without a clock, refused with one
        assert ei.value.code == L.PDMP_ERR_INVALID and "refresh clock" in str(ei.value)
        assert np.array_equal(ens.path_integrals(0.5, np.arange(d)), J)
