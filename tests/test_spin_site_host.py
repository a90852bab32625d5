"""The site operators on the host: eigenex_spin_site_apply_host against the Kronecker restatement of
tests/spin_dynamics_reference.py within the bound that the number of roundings gives, the adjoint identity, the operators that
leave the sectors, every refusal by its code and message, the exports, the numpy continued fraction of the reference module
against dense diagonalisation at the tolerances the GPU test asserts, and the host code (csrc/spin_site.hpp) together with the
kernel's row walk (csrc/spin_rows.hpp) under AddressSanitizer + UBSan in a stand-alone program.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_dynamics_reference as dr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
# (L, n_up, kinds): Kronecker products up to L = 10 (1024 x 1024); an odd L, one-row sources and destinations, the full space
SHAPES = [(3, None, (0, 1, 2)), (8, None, (0, 1, 2)), (4, 2, (0, 1, 2)), (6, 0, (0, 1)), (6, 6, (0, 2)), (6, 1, (2,)), (6, 5, (1,)), (9, 4, (0, 1, 2)),
          (10, 5, (0, 1, 2))]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g

    g.build()
    from cmpt_eigenex_amd import capi as c

    return c


def _coefficients(L, which):
    c = np.random.RandomState(50 + L).uniform(-1.0, 1.0, L)
    if which == "zeros":
        c[::2] = 0.0
    return c


@pytest.mark.parametrize("L,n_up,kinds", SHAPES)
def test_host_apply_equals_the_kronecker_restatement_within_the_bound(capi, L, n_up, kinds):
    x = np.random.RandomState(7 * L + (n_up or 0)).standard_normal(dr.states(capi, L, n_up).size)
    for kind in kinds:
        for which in ("dense", "zeros"):
            c = _coefficients(L, which)
            y, norm2 = capi.spin_site_apply_host(L, n_up, kind, c, x)
            O = dr.site_operator(capi, L, n_up, kind, c).astype(LD)
            ref = O @ x.astype(LD)
            assert y.dtype == np.float64 and y.shape == ref.shape
            if kind == dr.Z:  # n_sites roundings of w, each below eps * sum |c_i| / 2, and one of the product
                bound = L * dr.EPS * (np.abs(c).sum() / 2) * np.abs(x)
            else:             # at most n_sites fma, each rounding a partial sum below sum_i |c_i x_.|
                bound = L * dr.EPS * (dr.site_operator(capi, L, n_up, kind, c, absolute=True).astype(LD) @ np.abs(x).astype(LD))
            err = np.abs(y.astype(LD) - ref)
            print(f"({L},{n_up}) kind {kind} {which}: largest error / bound = {float(np.max(err / np.maximum(bound, LD(1e-300)))):.3f}")
            assert np.all(err <= bound)
            assert abs(norm2 - float(y @ y)) <= y.size * dr.EPS * norm2
            if kind != dr.Z:  # an entry without any term is exactly +0.0
                assert np.all(y[np.asarray(bound == 0)] == 0.0)
    # all coefficients zero: y = 0 and norm2 = 0, exactly
    y, norm2 = capi.spin_site_apply_host(L, n_up, kinds[0], np.zeros(L), x)
    assert not y.any() and norm2 == 0.0


@pytest.mark.parametrize("L,n_up", [(8, None), (9, 4), (10, 5), (6, 0)])
def test_plus_is_the_adjoint_of_minus(capi, L, n_up):
    """<y | S+ x> = <S- y | x> with the same coefficients: x on (L, n_up), y on (L, n_up + 1).  Both sides are sums of the same
    products in different orders: rows * n_sites terms, each side within that many roundings of the sum of their sizes."""
    rng = np.random.RandomState(3 * L)
    c = _coefficients(L, "dense")
    up = dr.dst_up(n_up, dr.PLUS)
    x, y = rng.standard_normal(dr.states(capi, L, n_up).size), rng.standard_normal(dr.states(capi, L, up).size)
    px, _ = capi.spin_site_apply_host(L, n_up, dr.PLUS, c, x)
    my, _ = capi.spin_site_apply_host(L, up, dr.MINUS, c, y)
    lhs, rhs = float(y @ px), float(my @ x)
    size = float(np.abs(y) @ (dr.site_operator(capi, L, n_up, dr.PLUS, c, absolute=True) @ np.abs(x)))
    print(f"({L},{n_up}): {lhs!r} against {rhs!r}, bound {2 * (L + max(x.size, y.size)) * dr.EPS * size:.3e}")
    assert abs(lhs - rhs) <= 2 * (L + max(x.size, y.size)) * dr.EPS * size and size > 0.0


def test_operators_that_leave_the_sectors_give_zero(capi):
    """S+ on the state with every site up and S- on the one with none: zero in the full space, where they are vectors like any
    other, and refused in the sectors (L, L) and (L, 0), whose destination does not exist."""
    L = 6
    c = np.arange(1.0, L + 1)
    for kind, s in ((dr.PLUS, (1 << L) - 1), (dr.MINUS, 0)):
        x = np.zeros(1 << L)
        x[s] = 2.5
        y, norm2 = capi.spin_site_apply_host(L, None, kind, c, x)
        assert not y.any() and norm2 == 0.0
        other, n2 = capi.spin_site_apply_host(L, None, dr.PLUS + dr.MINUS - kind, c, x)  # the other one moves it
        assert np.count_nonzero(other) == L and n2 == float(np.sum((2.5 * c) ** 2))
        with pytest.raises(capi.EigenexError, match="destination sector"):
            capi.spin_site_apply_host(L, L if kind == dr.PLUS else 0, kind, c, np.ones(1))
    # and Z on a product state is its magnetisation-weighted multiple: w = sum_i +-c_i / 2
    x = np.zeros(1 << L)
    x[0b010011] = -2.0
    y, _ = capi.spin_site_apply_host(L, None, dr.Z, c, x)
    w = sum((0.5 if (0b010011 >> i) & 1 else -0.5) * c[i] for i in range(L))
    assert y[0b010011] == w * -2.0 and np.count_nonzero(y) == 1


def _raw(capi, n_sites, n_up, kind, coef, x=True, y=True):
    dp = C.POINTER(C.c_double)
    cv = None if coef is None else np.ascontiguousarray(coef, np.float64)
    xv, yv, n2 = np.ones(1 << 6), np.full(1 << 6, -7.0), C.c_double(-7.0)
    rc = capi.lib().eigenex_spin_site_apply_host(n_sites, n_up, kind, None if cv is None else cv.ctypes.data_as(dp), xv.ctypes.data_as(dp) if x else None,
                                                yv.ctypes.data_as(dp) if y else None, C.byref(n2))
    return rc, capi.lib().eigenex_last_error().decode(), n2.value == -7.0 and bool(np.all(yv == -7.0))


def test_every_refusal_returns_its_code_and_a_message(capi):
    ok = np.ones(32)
    assert _raw(capi, 6, -1, 1, ok)[0] == 0 and _raw(capi, 6, 3, 2, ok)[0] == 0 and _raw(capi, 6, 3, 0, ok)[0] == 0
    bad = ok.copy()
    bad[4] = np.inf
    nan = ok.copy()
    nan[0] = np.nan
    cases = [("kind", (6, -1, 3, ok)), ("kind", (6, 3, -1, ok)), ("not finite", (6, 3, 0, bad)), ("not finite", (6, -1, 2, nan)),
             ("destination sector", (6, 6, 1, ok)), ("destination sector", (6, 0, 2, ok)), ("n_sites", (31, -1, 0, ok)), ("n_sites", (33, 2, 0, ok)),
             ("n_sites", (1, -1, 0, ok)), ("n_up", (6, 7, 0, ok)), ("n_up", (6, -2, 0, ok)), ("NULL", (6, 3, 0, None))]
    for word, args in cases:
        rc, msg, untouched = _raw(capi, *args)
        assert rc == -1 and word in msg and msg.startswith("eigenex_spin_site_apply_host: ") and untouched, (word, args, msg)
    assert bad[5] == 1.0 and _raw(capi, 4, 2, 0, bad)[0] == 0  # a coefficient beyond n_sites is not read
    for kw in (dict(x=False), dict(y=False)):
        rc, msg, untouched = _raw(capi, 6, 3, 0, ok, **kw)
        assert rc == -1 and "NULL" in msg and untouched
    # in place: Z only
    dp = C.POINTER(C.c_double)
    v = np.arange(1.0, 21.0)
    assert capi.lib().eigenex_spin_site_apply_host(6, -1, 1, ok.ctypes.data_as(dp), v.ctypes.data_as(dp), v.ctypes.data_as(dp), None) == -1
    assert "reads what it would write" in capi.lib().eigenex_last_error().decode()
    want, _ = capi.spin_site_apply_host(6, 3, 0, ok[:6], v)
    assert capi.lib().eigenex_spin_site_apply_host(6, 3, 0, ok.ctypes.data_as(dp), v.ctypes.data_as(dp), v.ctypes.data_as(dp), None) == 0
    assert np.array_equal(v, want)


def test_exports_are_declared_and_present(capi):
    text = open(os.path.join(ROOT, "include", "eigenex_hip.h")).read()
    for name in ("eigenex_spin_site_apply", "eigenex_spin_site_apply_host"):
        assert re.search(r"\bint %s\s*\(" % name, text)
        assert hasattr(capi.lib(), name) and name in capi.SIGNATURES
    for k, name in enumerate(("EIGENEX_SPIN_SITE_Z", "EIGENEX_SPIN_SITE_PLUS", "EIGENEX_SPIN_SITE_MINUS")):
        assert re.search(r"\b%s = %d\b" % (name, k), text)
    assert (capi.SPIN_SITE_Z, capi.SPIN_SITE_PLUS, capi.SPIN_SITE_MINUS) == (0, 1, 2) == (dr.Z, dr.PLUS, dr.MINUS)
    assert "i ascending" in text[text.index("EIGENEX_SPIN_SITE_Z      O"):]  # the order of summation is stated


@pytest.mark.parametrize("name", sorted(dr.moment_cases()))
def test_numpy_continued_fraction_meets_the_moment_tolerance(capi, name):
    model, n_up, parts, m = dr.moment_cases()[name]
    dense = dr.Dense(capi, model, n_up, parts)
    (kind, coef), = parts
    phi = dr.site_operator(capi, model[0], n_up, kind, coef) @ dense.psi
    p, w = dr.lanczos_fraction(dr.hamiltonian(capi, model, dr.dst_up(n_up, kind)), phi, m, dense.E0)
    for k in range(4):
        err = abs(float(np.sum(w * p ** k)) - dense.moment(k)) / dense.moment_scale(k)
        print(f"{name}: moment {k} relative error {err:.2e}")
        assert err <= dr.MOMENT_TOL


@pytest.mark.parametrize("name", sorted(dr.spectrum_cases()))
def test_numpy_continued_fraction_meets_the_spectrum_tolerance(capi, name):
    model, n_up, parts, m = dr.spectrum_cases()[name]
    dense = dr.Dense(capi, model, n_up, parts)
    (kind, coef), = parts
    phi = dr.site_operator(capi, model[0], n_up, kind, coef) @ dense.psi
    p, w = dr.lanczos_fraction(dr.hamiltonian(capi, model, dr.dst_up(n_up, kind)), phi, m, dense.E0)
    ref = dense.spectrum(dr.OMEGA, dr.ETA)
    err = float(np.max(np.abs(dr.lorentzians(p, w, dr.OMEGA, dr.ETA) - ref)) / ref.max())
    print(f"{name}: spectrum error / maximum {err:.2e}, lowest pole {p[w > 1e-12 * w.sum()].min():.6f} (dense {dense.lowest_pole():.6f})")
    assert err <= dr.SPECTRUM_TOL
    assert abs(p[w > 1e-12 * w.sum()].min() - dense.lowest_pole()) <= dr.MOMENT_TOL * max(1.0, abs(dense.lowest_pole()))


def test_site_host_code_under_sanitizers(tmp_path):
    """csrc/spin_site.hpp (argument check, kernel table, host evaluation) compiled into a stand-alone program with
    AddressSanitizer + UBSan, and the row loop of k_spin_site_apply -- the kernel's own functions (csrc/spin_rows.hpp, compiled
    into the program) with every load bounds-checked -- equal to the host evaluation over every row of every shape."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "spin_site_sanitize")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "spin_site_sanitize.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-1500:], out.stderr.decode()[-2000:])
    assert b"SPIN SITE OK" in out.stdout
