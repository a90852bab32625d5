"""Host half of the Chebyshev-filtered Lanczos solver (no GPU): the exported coefficients and symbols, and the numpy
restatement (tests/filter_reference.py) on the two models the device tests use."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_reference as fr  # noqa: E402


@pytest.mark.parametrize("tau,center,half,degree", [(0.3, 0.0, 3.03, 200), (-1.2, 0.1, 2.5, 1), (0.0, 0.0, 1.0, 2), (2.9, 0.5, 2.5, 40), (0.3, -0.02, 7.0, 100)])
def test_exported_coefficients_match_the_restatement(tau, center, half, degree):
    from cmpt_eigenex_amd import solver

    mu = solver.chebyshev_delta(tau, center, half, degree)
    ref = fr.delta_coefficients(tau, center, half, degree)
    assert mu.shape == (degree + 1,)
    ulp = np.spacing(np.abs(ref).max())
    print("max |mu - ref| = %.3e (%.2f ulp of max|mu|)" % (np.abs(mu - ref).max(), np.abs(mu - ref).max() / ulp))
    assert np.abs(mu - ref).max() <= 4 * ulp
    a = (tau - center) / half
    assert abs(fr.polynomial(mu, a) - 1.0) < 1e-13  # p(tau) = 1
    if degree >= 40:  # a peak: nowhere on the interval larger than at tau
        assert np.all(fr.polynomial(mu, np.linspace(-1, 1, 2001)) <= 1.0 + 1e-12)


def test_new_symbols_are_exported():
    from cmpt_eigenex_amd import capi, solver

    L, S = capi.lib(), solver.lib()
    for name in ("eigenex_basis_set_filter", "eigenex_filter_apply"):
        assert hasattr(L, name)
    assert L.eigenex_version() == 100
    for kind in ("flanczos", "zflanczos"):
        for fn in ("create", "destroy", "set_device_operator", "set_initial_vector", "set", "compute", "sizes", "get", "log_line"):
            assert hasattr(S, f"eigenex_{kind}_solver_{fn}")
    assert hasattr(S, "eigenex_solver_chebyshev_delta")
    assert S.eigenex_solver_chebyshev_delta(0.0, 0.0, -1.0, 3, np.zeros(4).ctypes.data_as(C.POINTER(C.c_double))) != 0
    assert hasattr(capi.Basis, "set_filter") and hasattr(capi.Basis, "filter_apply") and hasattr(solver, "FilteredLanczosEigenSolver")


def test_solver_without_a_spectral_range_is_invalid_input():
    from cmpt_eigenex_amd import solver

    es = solver.FilteredLanczosEigenSolver()
    es.set(numberOfEigenvalues=2, target=0.1)
    es.compute()
    r = es.results()
    assert r["info_name"] == "InvalidInput" and r["neig"] == 0
    assert es.log()[-1].startswith("ERROR")


def test_recurrence_in_double_follows_long_double():
    A = fr.anderson_chain(257)
    lo, hi = fr.gershgorin(A)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo) * 1.01
    x = np.random.RandomState(1).standard_normal(257)
    for d in (1, 2, 3, 40):
        mu = fr.delta_coefficients(0.3, c, h, d)
        y = fr.apply_filter(fr.csr_rowsum_matmul(A.indptr, A.indices, A.data, np.float64), x, mu, c, h)
        yl = fr.apply_filter(fr.csr_rowsum_matmul(A.indptr, A.indices, A.data, np.longdouble), x.astype(np.longdouble), mu, c, h)
        lam, Q = np.linalg.eigh(A.toarray())
        dense = Q @ (fr.polynomial(mu, (lam - c) / h) * (Q.T @ x))
        assert np.abs(y - yl.astype(np.float64)).max() <= 8 * np.finfo(float).eps * np.abs(mu).sum() * np.abs(x).max() * d
        np.testing.assert_allclose(yl.astype(np.float64), dense, rtol=0, atol=1e-12)


def test_long_double_matmul_with_empty_rows():
    """fr.csr_rowsum_matmul_any_rows on a 40-row matrix with empty rows (a run of them, the first and the last row) against the
    dense long double product: equal where every operation is exact (small integers), else within the two sums' rounding, a row
    of k products: 2 k eps sum|a||x|; empty rows give 0; without empty rows the bits of fr.csr_rowsum_matmul"""
    import scipy.sparse as sp

    rng = np.random.RandomState(4)
    n = 40
    D = np.where(rng.rand(n, n) < 0.2, rng.standard_normal((n, n)), 0.0)
    gone = [0, 7, 39] + list(range(16, 24))
    D[gone, :] = 0.0
    x = rng.standard_normal(n)
    eps = np.finfo(np.longdouble).eps
    for dense, v in ((np.rint(8 * D), np.rint(8 * x)), (D, x)):
        A = sp.csr_matrix(dense)
        A.sort_indices()
        assert np.all(np.diff(A.indptr)[gone] == 0) and A.nnz > n
        for dtype, xv in ((np.longdouble, v), (np.float64, v), (np.clongdouble, v + 1j * v[::-1])):
            y = fr.csr_rowsum_matmul_any_rows(A.indptr, A.indices, A.data, dtype)(xv.astype(dtype))
            assert y.dtype == dtype and np.all(y[gone] == 0)
            ld = np.clongdouble if np.iscomplexobj(xv) else np.longdouble
            want = dense.astype(np.longdouble) @ xv.astype(ld)
            if dense is not D:
                np.testing.assert_array_equal(y.astype(ld), want)
            elif dtype != np.float64:
                k = np.diff(A.indptr)
                bound = 2 * k * eps * (np.abs(dense).astype(np.longdouble) @ np.abs(xv).astype(np.longdouble)) * (2 if ld is np.clongdouble else 1)
                assert np.all(np.abs(y - want) <= bound)
    keep = np.setdiff1d(np.arange(n), gone)
    B = sp.csr_matrix(D[np.ix_(keep, keep)] + np.eye(keep.size))
    B.sort_indices()
    xl = x[keep].astype(np.longdouble)
    np.testing.assert_array_equal(fr.csr_rowsum_matmul_any_rows(B.indptr, B.indices, B.data, np.longdouble)(xl),
                                  fr.csr_rowsum_matmul(B.indptr, B.indices, B.data, np.longdouble)(xl))


@pytest.mark.parametrize("model", ["chain", "grid"])
def test_restatement_finds_the_interior_pairs(model):
    """the two CPU results of the design: the 1000-site chain (degree 200) and the 6 x 7 x 8 model (degree 100), m = 60"""
    A = fr.anderson_chain(1000) if model == "chain" else fr.anderson3d()
    n = A.shape[0]
    lo, hi = fr.gershgorin(A)
    init = np.random.RandomState(11).standard_normal(n)
    r = fr.filtered_lanczos(lambda x: A @ x, n, init, 0.3, lo, hi, 200 if model == "chain" else 100, 4, 60)
    want = fr.nearest(A, 0.3, 4)
    print(model, "eigenvalue error %.2e, residuals %.2e, restarts %d" % (np.abs(r["eigenvalues"] - want).max(), r["residuals"].max(), r["restarts"]))
    np.testing.assert_allclose(r["eigenvalues"], want, rtol=0, atol=1e-12)
    assert r["residuals"].max() < 1e-12
