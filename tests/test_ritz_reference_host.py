"""CPU checks of tests/ritz_reference.py, the extended-precision reference the Ritz vector tests compare against:
combine() against exact rational arithmetic, finish() against the oracle's fix_phase_and_normalize (lanczos.hpp:806-816)
and on the phase and scale edges, bound() against the errors of plain fp64 products."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import krylov_oracle as ko
from tests import ritz_reference as rr


def _exact(V, S):
    """sum_m S[m, e] V[m] with Fractions (real) or pairs of Fractions (complex)"""
    nvec, nev = S.shape
    out = []
    for e in range(nev):
        col = []
        for r in range(V.shape[1]):
            re = im = Fraction(0)
            for m in range(nvec):
                s, v = complex(S[m, e]), complex(V[m, r])
                sr, si, vr, vi = (Fraction(t) for t in (s.real, s.imag, v.real, v.imag))
                re += sr * vr - si * vi
                im += sr * vi + si * vr
            col.append((re, im))
        out.append(col)
    return out


@pytest.mark.parametrize("cplx_v, cplx_s", [(False, False), (False, True), (True, False), (True, True)])
def test_combine_against_fractions(cplx_v, cplx_s):
    rng = np.random.default_rng(7 + 2 * cplx_v + cplx_s)
    nvec, nev, n = 6, 3, 5

    def draw(shape, c):
        x = rng.standard_normal(shape) * 10.0 ** rng.integers(-8, 8, shape)
        return x + 1j * rng.standard_normal(shape) if c else x

    V, S = draw((nvec, n), cplx_v), draw((nvec, nev), cplx_s)
    X = rr.combine(V, S)
    assert X.shape == (n, nev) and np.iscomplexobj(X) == (cplx_v or cplx_s)
    ex = _exact(V, S)
    scale = np.abs(S).T @ np.abs(V)  # (nev, n)
    for e in range(nev):
        for r in range(n):
            got_re = Fraction(*np.real(X[r, e]).as_integer_ratio())
            got_im = Fraction(*np.imag(X[r, e]).as_integer_ratio()) if np.iscomplexobj(X) else Fraction(0)
            err = abs(got_re - ex[e][r][0]) + abs(got_im - ex[e][r][1])
            assert err <= Fraction(4 * nvec) * Fraction(2) ** -63 * Fraction(float(scale[e, r])), (e, r)
            # and far below one fp64 rounding of the products
            assert float(err) < 0.02 * rr.U * scale[e, r] or scale[e, r] == 0


@pytest.mark.parametrize("cplx", [False, True])
def test_finish_matches_the_oracle(cplx):
    rng = np.random.default_rng(11 + cplx)
    n, nvec, nev = 200, 9, 5
    V = rng.standard_normal((nvec, n)) + (1j * rng.standard_normal((nvec, n)) if cplx else 0)
    V[:, :7] = 0.0  # leading rows zero in every column: the phase comes from row 7
    S = rng.standard_normal((nvec, nev))
    X = rr.finish(rr.combine(V, S))
    tol = rr.bound(V, S, X)
    for e in range(nev):
        x_or = ko.fix_phase_and_normalize(V.T @ S[:, e])
        assert np.all(np.abs(X[:, e] - x_or) <= tol[:, e])
        assert rr.first_hit(X[:, e]) == 7 and np.real(X[7, e]) > 0 and abs(np.imag(X[7, e])) <= 4 * rr.U
        assert abs(np.linalg.norm(X[:, e]) - 1.0) < 1e-15


def test_finish_phase_edges():
    u = rr.U
    # -0.0 ahead of a negative first hit: the phase is -1
    x = rr.finish(np.array([-0.0, 0.0, -0.0, -3.0, 4.0]))
    assert rr.first_hit(x) == 3 and x[3] == 0.6 and x[4] == -0.8
    # a subnormal first hit decides the phase although later entries are far larger
    x = rr.finish(np.array([0.0, -5e-324, 0.6, 0.8]))
    assert rr.first_hit(x) == 1 and x[1] == 5e-324 and x[2] < 0
    # a purely imaginary first hit: the result is real positive there
    x = rr.finish(np.array([0.0, -2j, 1.0 + 1.0j]))
    assert rr.first_hit(x) == 1 and x[1].real > 0 and abs(x[1].imag) <= 4 * u
    np.testing.assert_allclose(x, np.array([0.0, 2.0, 1j * (1 + 1j)]) / np.sqrt(6.0), rtol=0, atol=4 * u)
    # an all-zero column comes back as zeros, not NaN
    for z in (np.zeros(6), np.zeros(6, complex), np.array([0.0, -0.0])):
        x = rr.finish(z)
        assert not np.isnan(x).any() and np.all(x == 0)
    # the oracle agrees on each of these
    for col in (np.array([-0.0, -3.0, 4.0]), np.array([0.0, -2j, 1.0 + 1j]), np.zeros(3)):
        np.testing.assert_allclose(rr.finish(col), ko.fix_phase_and_normalize(col), rtol=0, atol=4 * u)


def test_finish_scale_edges():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(50)
    # squares underflow in float64: normalized() leaves the column as it is (the phase still applies)
    small = -1e-200 * np.abs(x)
    small[3:] = -small[3:]
    y = rr.finish(small)
    np.testing.assert_array_equal(y, -small)
    assert np.sum(small ** 2) == 0.0  # (float64: what the reference sees)
    # squares overflow: x / sqrt(inf) = 0
    big = 1e200 * x
    y = rr.finish(big)
    assert np.all(y == 0) and not np.isnan(y).any()
    # complex: the same two rules
    yc = rr.finish(1e-200 * (x + 1j * x))
    assert np.abs(np.abs(yc) - 1e-200 * np.sqrt(2) * np.abs(x)).max() <= 4 * np.spacing(1e-200)
    assert np.all(rr.finish(1e200 * (x + 1j * x)) == 0)
    # raw bound: relative to the products, not to a normalised column
    S = np.array([[1e-200], [2e-200]])
    V = np.stack([x, x])
    b = rr.bound(V, S, rr.combine(V, S), raw=True)
    assert b.shape == (50, 1) and np.all(b[:, 0] <= 19 * rr.U * 3.0001e-200 * np.abs(x))


def test_bound_covers_fp64_products_but_is_not_flat():
    """a float64 product V S (numpy, a blocked sum) lies within the bound; the bound scales with the entries"""
    rng = np.random.default_rng(3)
    for nvec, n in ((100, 300), (5, 2000)):
        V = rng.standard_normal((nvec, n)) * np.logspace(-6, 6, n)
        S = rng.standard_normal((nvec, 4))
        X = rr.finish(rr.combine(V, S))
        b = rr.bound(V, S, X)
        Y = np.stack([ko.fix_phase_and_normalize(V.T @ S[:, e]) for e in range(4)], axis=1)
        assert np.all(np.abs(Y - X) <= b)
        assert b[:10].max() < 1e-6 * b[-10:].min()  # per entry, not one flat atol
