"""Every entry point of the C ABI that takes a CSC matrix refuses a malformed one with PDMP_ERR_INVALID -- colptr[0] != 0, a colptr that
decreases, a row index outside the matrix, rows of a column that do not ascend -- and accepts a well-formed one afterwards.  Only set_* calls:
no kernel is launched."""
import numpy as np
import pytest

D = 4


def tridiagonal():
    cp = np.array([0, 2, 5, 8, 10], dtype=np.int64)
    rv = np.array([0, 1, 0, 1, 2, 1, 2, 3, 2, 3], dtype=np.int64)
    nz = np.where(rv == np.repeat(np.arange(D), np.diff(cp)), 2.0, -0.5)
    return cp, rv, nz


def lower_bidiagonal():
    cp = np.array([0, 2, 4, 6, 7], dtype=np.int64)
    rv = np.array([0, 1, 1, 2, 2, 3, 3], dtype=np.int64)
    nz = np.where(rv == np.repeat(np.arange(D), np.diff(cp)), 2.0, 0.5)
    return cp, rv, nz


def broken(defect, cp, rv):
    cp, rv = cp.copy(), rv.copy()
    if defect == "colptr0":
        cp[0] = 1
    elif defect == "colptr_decreases":
        cp[2] = cp[1] - 1
    elif defect == "row_out_of_range":
        rv[-1] = D  # (the last row of the last column: still ascending)
    elif defect == "rows_not_ascending":
        a = cp[1]
        rv[a], rv[a + 1] = rv[a + 1], rv[a]
    return cp, rv


def p(a):
    return a.ctypes.data


SITES = ["flow_zigzag", "neighbourhood", "target", "target_of_bps", "flow_bps", "mass_cholesky"]
DEFECTS = ["colptr0", "colptr_decreases", "row_out_of_range", "rows_not_ascending"]


@pytest.mark.gpu
@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("site", SITES)
def test_malformed_csc_is_invalid_and_a_good_matrix_is_accepted_after(gpu_pkg, site, defect):
    pkg = gpu_pkg
    L = pkg._lib
    lib = L.load()
    bps = site in ("target_of_bps", "flow_bps", "mass_cholesky")
    cp, rv, nz = lower_bidiagonal() if site == "mass_cholesky" else tridiagonal()
    gcp, grv, gnz = tridiagonal()
    with pkg.Ensemble(1, D, sampler=L.SAMPLER_BPS if bps else L.SAMPLER_ZIGZAG_LOCAL, trace_capacity=8) as ens:
        h = ens._h
        # what has to be in place before the call under test
        if site in ("neighbourhood", "target"):
            assert lib.pdmp_ensemble_set_flow_zigzag(h, p(gcp), p(grv), p(gnz), None, None, 0.0, 0.0) == L.PDMP_OK
        if site in ("target_of_bps", "mass_cholesky"):
            assert lib.pdmp_ensemble_set_flow_bps(h, p(gcp), p(grv), p(gnz), None, 1.0, 0.0) == L.PDMP_OK
        call = {"flow_zigzag": lambda c, r: lib.pdmp_ensemble_set_flow_zigzag(h, p(c), p(r), p(nz), None, None, 0.0, 0.0),
                "neighbourhood": lambda c, r: lib.pdmp_ensemble_set_neighbourhood(h, p(c), p(r)),
                "target": lambda c, r: lib.pdmp_ensemble_set_target_gaussian_csc(h, p(c), p(r), p(nz), None),
                "target_of_bps": lambda c, r: lib.pdmp_ensemble_set_target_gaussian_csc(h, p(c), p(r), p(nz), None),
                "flow_bps": lambda c, r: lib.pdmp_ensemble_set_flow_bps(h, p(c), p(r), p(nz), None, 1.0, 0.0),
                "mass_cholesky": lambda c, r: lib.pdmp_ensemble_set_mass_cholesky(h, p(c), p(r), p(nz))}[site]
        bcp, brv = broken(defect, cp, rv)
        assert call(bcp, brv) == L.PDMP_ERR_INVALID, lib.pdmp_last_error()
        assert call(cp, rv) == L.PDMP_OK, lib.pdmp_last_error()
