"""Host half of the spectral density solver (no GPU): the C++ post-processing (kpmDensity, kpmCount, kpmWindow, jacksonFactor
behind libeigenex_solver.so) against the numpy restatement tests/density_reference.py, fed with exact moments from LAPACK
eigenvalues, and the restatement itself against the true eigenvalue counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_reference as dr  # noqa: E402
import filter_reference as fr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
M = 257
_MODELS = {}


def _model(name):
    """(eigenvalues, lo, hi, center, halfwidth, exact moments) -- once per module"""
    if name not in _MODELS:
        A = fr.anderson_chain(1000) if name == "chain" else fr.anderson3d()
        lam = np.linalg.eigvalsh(A.toarray())
        lo, hi = fr.gershgorin(A)
        c, h = dr.widened(lo, hi)
        _MODELS[name] = (lam, lo, hi, c, h, dr.exact_moments(lam, c, h, M))
    return _MODELS[name]


@pytest.mark.parametrize("name", ["chain", "grid"])
def test_post_processing_matches_the_restatement(name):
    """density and count of the C++ functions against numpy on exact moments; tolerance = the rounding bound of a sum of M
    terms, M eps sum|terms| (times the common factor), which also covers a last-place difference per term between the two
    libraries' cos / sin"""
    from cmpt_eigenex_amd import solver

    lam, lo, hi, c, h, mu = _model(name)
    N = lam.size
    for E in np.quantile(lam, [0.02, 0.25, 0.5, 0.77, 0.99]):
        terms, f = dr.density_terms(mu, c, h, E)
        got, ref = solver.kpm_density(mu, c, h, E)[0], dr.density(mu, c, h, E)
        bound = M * EPS * np.abs(terms).sum() * f
        print(f"{name} density({E:+.4f}) = {ref:.6f}: |C++ - numpy| {abs(got - ref):.3e}, bound {bound:.3e}")
        assert abs(got - ref) <= bound
    assert solver.kpm_density(mu, c, h, c + 1.5 * h)[0] == 0.0 and solver.kpm_density(mu, c, h, c - h)[0] == 0.0
    for qa, qb in dr.QUANTILE_WINDOWS:
        a, b, _ = dr.quantile_window(lam, qa, qb, lo, hi)
        got, ref = solver.kpm_count(mu, c, h, a, b, N), dr.count(mu, c, h, a, b, N)
        bound = M * EPS * np.abs(dr.count_terms(mu, c, h, a, b)).sum() * N
        print(f"{name} count[{qa}, {qb}] = {ref:.6f}: |C++ - numpy| {abs(got - ref):.3e}, bound {bound:.3e}")
        assert abs(got - ref) <= bound
    assert solver.kpm_count(mu, c, h, 1.0, 1.0, N) == 0.0
    full = solver.kpm_count(mu, c, h, c - 2 * h, c + 2 * h, N)  # end points outside the interval: everything
    assert abs(full - N) <= M * EPS * N


# measured with M = 257 on exact moments: the largest error over the four windows
_MEASURED = {"chain": 3.08, "grid": 0.61}


@pytest.mark.parametrize("name", ["chain", "grid"])
def test_restatement_counts_the_eigenvalues(name):
    """physical sanity of the reference alone: the count from exact moments against the true number of eigenvalues in windows
    whose ends sit between neighbouring eigenvalues at the 10-40 %, 45-55 %, 0-50 % and 70-100 % quantiles.  Measured with
    M = 257: chain (N = 1000) errors -3.08, +0.66, +0.30, +0.25 levels; 6 x 7 x 8 grid (N = 336) -0.61, +0.00, -0.60, +0.39.
    Asserted: twice the largest measured error of each model."""
    lam, lo, hi, c, h, mu = _model(name)
    worst = 0.0
    for qa, qb in dr.QUANTILE_WINDOWS:
        a, b, true = dr.quantile_window(lam, qa, qb, lo, hi)
        est = dr.count(mu, c, h, a, b, lam.size)
        print(f"{name} [{qa}, {qb}]: {true} eigenvalues, counted {est:.3f} (error {est - true:+.3f})")
        worst = max(worst, abs(est - true))
    assert worst <= 2 * _MEASURED[name]
    E = np.linspace(c - h, c + h, 4001)[1:-1]
    rho = np.array([dr.density(mu, c, h, e) for e in E])
    assert rho.min() >= -1e-12  # the Jackson kernel is positive
    assert abs(rho.sum() * (E[1] - E[0]) - 1.0) < 1e-3  # per state


@pytest.mark.parametrize("name", ["chain", "grid"])
def test_energy_window_inverts_the_count(name):
    """kpmWindow ends on neighbouring doubles lo < hi with computed count(lo) < want <= count(hi); a computed count is within
    B = M eps N sum|terms| of the monotone exact one, and between neighbouring doubles that one moves by far less than B: so
    |count(window) - want| <= 3 B, asserted with 4 B, for the C++ function and for the restatement of the other's result"""
    from cmpt_eigenex_amd import solver

    lam, lo, hi, c, h, mu = _model(name)
    N = lam.size
    for tau, want in ((c, 10.0), (0.3, 4.0), (lam[5], 25.0), (c, 0.5)):
        d_cpp, d_ref = solver.kpm_window(mu, c, h, tau, want, N), dr.window(mu, c, h, tau, want, N)
        B = M * EPS * N * np.abs(dr.count_terms(mu, c, h, tau - d_ref, tau + d_ref)).sum()
        back_cpp, back_ref = solver.kpm_count(mu, c, h, tau - d_cpp, tau + d_cpp, N), dr.count(mu, c, h, tau - d_cpp, tau + d_cpp, N)
        print(f"{name} tau={tau:+.4f} count={want}: half-width C++ {d_cpp:.12f}, numpy {d_ref:.12f}; count back {back_cpp - want:+.3e} / {back_ref - want:+.3e}, 4B {4 * B:.3e}")
        assert d_cpp > 0 and abs(back_cpp - want) <= 4 * B and abs(back_ref - want) <= 4 * B
        assert abs(dr.count(mu, c, h, tau - d_ref, tau + d_ref, N) - want) <= 4 * B
    assert solver.kpm_window(mu, c, h, c, 2.0 * N, N) == pytest.approx(h)  # more than there is: the whole interval
    assert solver.kpm_window(mu, c, h, c, 0.0, N) == 0.0


@pytest.mark.parametrize("tau,center,half,degree", [(0.3, 0.0, 3.03, 200), (-1.2, 0.1, 2.5, 1), (0.0, 0.0, 1.0, 2), (2.9, 0.5, 2.5, 40), (0.3, -0.02, 7.0, 100)])
def test_shared_jackson_function_leaves_the_filter_coefficients_alone(tau, center, half, degree):
    """chebyshevDeltaCoefficients now takes its Jackson factors from jacksonFactor: against filter_reference.delta_coefficients
    as tests/test_filter_host.py holds it (4 ulp of max|mu|), and the factors themselves against numpy"""
    from cmpt_eigenex_amd import solver

    mu, ref = solver.chebyshev_delta(tau, center, half, degree), fr.delta_coefficients(tau, center, half, degree)
    assert np.abs(mu - ref).max() <= 4 * np.spacing(np.abs(ref).max())
    g, gref = solver.jackson_factors(degree + 1), dr.jackson(degree + 1)
    assert g[0] == 1.0 or abs(g[0] - 1.0) <= 2 * EPS
    assert np.abs(g - gref).max() <= 4 * EPS  # two terms of size <= 1 each, rounded in either library
    assert np.all(g > 0) and np.all(np.diff(g) < 0)


def test_four_scalars_instantiate_under_cxx11():
    src = ('#include "cmpt/eigen_ex/spectral_density.hpp"\n'
           "template class cmpt::EigenEx::SpectralDensitySolver<double>;\n"
           "template class cmpt::EigenEx::SpectralDensitySolver<float>;\n"
           "template class cmpt::EigenEx::SpectralDensitySolver<std::complex<double>>;\n"
           "template class cmpt::EigenEx::SpectralDensitySolver<std::complex<float>>;\n"
           "int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-fsyntax-only", "-x", "c++", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"), "-"], input=src.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()


def test_new_symbols_and_invalid_input():
    from cmpt_eigenex_amd import capi, solver

    L, S = capi.lib(), solver.lib()
    for name in ("eigenex_kpm_moments", "eigenex_kpm_trace_moments", "eigenex_vec_random_signs"):
        assert hasattr(L, name)
    for kind in ("density", "zdensity"):
        for fn in ("create", "destroy", "set_device_operator", "set_initial_vector", "set", "set_seed", "compute", "continue", "sizes", "get",
                   "density", "eigenvalue_count", "energy_window", "log_line"):
            assert hasattr(S, f"eigenex_{kind}_solver_{fn}")
    es = solver.SpectralDensitySolver()
    es.set(moments=16, randomVectors=2, seed=3)
    es.compute()  # no operator, no spectral range
    r = es.results()
    assert r["info_name"] == "InvalidInput" and r["nmoments"] == 0 and es.log()[-1].startswith("ERROR")
    assert es.eigenvalueCount(-1.0, 1.0) == 0.0 and es.energyWindow(0.0, 3.0) == 0.0
    es.close()


def test_hash_restatement_is_a_fixed_function():
    """values written down once from the definition (splitmix64 finaliser, G = 0x9E3779B97F4A7C15): mix(G) is the first output
    of splitmix64 seeded with 0, a published constant"""
    assert int(dr._mix(np.array([0x9E3779B97F4A7C15], np.uint64))[0]) == 0xE220A8397B1DCDAF
    a, b = dr.random_signs(7, 0, 4096), dr.random_signs(7, 1, 4096)
    assert set(np.unique(a)) == {-1.0, 1.0} and abs(a.mean()) < 0.06 and abs((a * b).mean()) < 0.06
    np.testing.assert_array_equal(dr.random_signs(7, 0, 100), a[:100])  # entry = f(seed, stream, row) alone
    z = dr.random_signs(7, 0, 16, np.complex128)
    assert z.dtype == np.complex128 and np.all(z.imag == 0)
