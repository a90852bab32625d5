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
