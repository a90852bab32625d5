"""The site operators of complex vectors on the host: eigenex_spin_site_apply_host_z against the longdouble restatement of
tests/spin_site_z_reference.py (state lists, and Kronecker products in the full space) within the bound that the number of
roundings gives; real coefficients (coef_im NULL, or all zero) against eigenex_spin_site_apply_host part by part, bit for bit;
the adjoint identity with conjugated coefficients; every refusal by its code and message; the exports; and the host code
(csrc/spin_site.hpp) together with the complex kernel's row walk (csrc/spin_rows.hpp) under AddressSanitizer + UBSan in a
stand-alone program.  No GPU."""
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
import spin_site_z_reference as zr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g

    g.build()
    from cmpt_eigenex_amd import capi as c

    return c


def _rows(capi, L, n_up):
    return dr.states(capi, L, n_up).size


@pytest.mark.parametrize("L,n_up,kinds", zr.HOST_SHAPES)
def test_host_apply_equals_the_restatement_within_the_bound(capi, L, n_up, kinds):
    x = zr.complex_vector(_rows(capi, L, n_up), 7 * L + (n_up or 0))
    for kind in kinds:
        for which in ("both signs", "zeros"):
            c = zr.coefficients(L, which)
            y, norm2 = capi.spin_site_apply_host_z(L, n_up, kind, c, x)
            ref_re, ref_im = zr.apply(capi, L, n_up, kind, c, x)
            assert y.dtype == np.complex128 and y.shape == ref_re.shape
            bound = zr.terms(L) * zr.EPS * zr.row_size(capi, L, n_up, kind, c, x)
            err = np.maximum(np.abs(y.real.astype(LD) - ref_re), np.abs(y.imag.astype(LD) - ref_im))
            print(f"({L},{n_up}) kind {kind} {which}: largest error / bound = {float(np.max(err / np.maximum(bound, LD(1e-300)))):.3f}")
            assert np.all(err <= bound)
            assert abs(norm2 - float(np.vdot(y, y).real)) <= 2 * y.size * zr.EPS * norm2
            if kind != dr.Z:  # an entry without any term is exactly +0.0 in both parts
                assert np.all(y[np.asarray(bound == 0)] == 0.0)
    y, norm2 = capi.spin_site_apply_host_z(L, n_up, kinds[0], np.zeros(L, np.complex128), x)  # all coefficients zero
    assert not y.any() and norm2 == 0.0


@pytest.mark.parametrize("L", [3, 8])
def test_the_state_list_restatement_is_the_kronecker_form_in_the_full_space(capi, L):
    w = np.random.RandomState(L).uniform(-1.0, 1.0, L)
    for kind in (dr.Z, dr.PLUS, dr.MINUS):
        K = zr.kronecker_matrix(L, kind, w)
        assert np.array_equal(zr.site_matrix(capi, L, None, kind, w), K)
        assert np.allclose(K.astype(np.float64), dr.site_operator(capi, L, None, kind, w), rtol=0, atol=1e-15)  # and the real yardstick's


@pytest.mark.parametrize("L,n_up,kinds", zr.HOST_SHAPES)
def test_real_coefficients_give_the_real_call_on_each_part(capi, L, n_up, kinds):
    """coef_im = NULL and an all-zero coef_im (also of negative zeros): real_coef, and each part of y is
    eigenex_spin_site_apply_host on that part of x, bit for bit"""
    x = zr.complex_vector(_rows(capi, L, n_up), 11 * L + (n_up or 0))
    for kind in kinds:
        c = zr.coefficients(L, "zeros").real.copy()
        want_re, _ = capi.spin_site_apply_host(L, n_up, kind, c, np.ascontiguousarray(x.real))
        want_im, _ = capi.spin_site_apply_host(L, n_up, kind, c, np.ascontiguousarray(x.imag))
        negative_zeros = c + 1j * np.where(np.arange(L) % 2 == 0, -0.0, 0.0)
        for coef, imaginary in ((c, False), (c, True), (negative_zeros, True)):
            y, norm2 = capi.spin_site_apply_host_z(L, n_up, kind, coef, x, imaginary=imaginary)
            assert y.real.tobytes() == want_re.tobytes() and y.imag.tobytes() == want_im.tobytes(), (L, n_up, kind, imaginary)
            assert abs(norm2 - float(np.vdot(y, y).real)) <= 2 * y.size * zr.EPS * norm2


@pytest.mark.parametrize("L,n_up", [(8, None), (9, 4), (11, 5), (6, 0), (13, 1)])
def test_plus_is_the_adjoint_of_minus_with_conjugated_coefficients(capi, L, n_up):
    """<y | S+(c) x> = <S-(conj c) y | x>: x on (L, n_up), y on (L, n_up + 1).  Each applied row is within terms * EPS * row_size
    of the exact one, and each numpy dot adds at most (rows + 2) roundings of a sum that `size` bounds; both sides together stay
    within 2 (terms + rows + 2) EPS size of each other in each part."""
    c = zr.coefficients(L, "both signs")
    up = dr.dst_up(n_up, dr.PLUS)
    x, y = zr.complex_vector(_rows(capi, L, n_up), 3 * L), zr.complex_vector(_rows(capi, L, up), 3 * L + 1)
    px, _ = capi.spin_site_apply_host_z(L, n_up, dr.PLUS, c, x)
    my, _ = capi.spin_site_apply_host_z(L, up, dr.MINUS, np.conj(c), y)
    lhs, rhs = np.vdot(y, px), np.vdot(my, x)
    size = float((np.abs(y.real) + np.abs(y.imag)) @ zr.row_size(capi, L, n_up, dr.PLUS, c, x).astype(np.float64))
    bound = 2 * (zr.terms(L) + max(x.size, y.size) + 2) * zr.EPS * size
    print(f"({L},{n_up}): {lhs!r} against {rhs!r}, bound {bound:.3e}")
    assert abs(lhs.real - rhs.real) <= bound and abs(lhs.imag - rhs.imag) <= bound and size > 0.0


def _raw(capi, n_sites, n_up, kind, cre, cim, x=True, y=True):
    dp = C.POINTER(C.c_double)
    ptr = lambda v: None if v is None else np.ascontiguousarray(v, np.float64).ctypes.data_as(dp)  # noqa: E731
    keep = [None if v is None else np.ascontiguousarray(v, np.float64) for v in (cre, cim)]
    xv, yv, n2 = np.ones(2 << 6), np.full(2 << 6, -7.0), C.c_double(-7.0)
    rc = capi.lib().eigenex_spin_site_apply_host_z(n_sites, n_up, kind, ptr(keep[0]), ptr(keep[1]), xv.ctypes.data_as(dp) if x else None,
                                                  yv.ctypes.data_as(dp) if y else None, C.byref(n2))
    return rc, capi.lib().eigenex_last_error().decode(), n2.value == -7.0 and bool(np.all(yv == -7.0))


def test_every_refusal_returns_its_code_and_a_message(capi):
    ok = np.ones(32)
    assert _raw(capi, 6, -1, 1, ok, ok)[0] == 0 and _raw(capi, 6, 3, 2, ok, None)[0] == 0 and _raw(capi, 6, 3, 0, ok, ok)[0] == 0
    bad = ok.copy()
    bad[4] = np.inf
    nan = ok.copy()
    nan[0] = np.nan
    cases = [("kind", (6, -1, 3, ok, ok)), ("kind", (6, 3, -1, ok, None)), ("not finite", (6, 3, 0, bad, ok)), ("not finite", (6, 3, 0, ok, bad)),
             ("not finite", (6, -1, 2, ok, nan)), ("not finite", (6, -1, 1, nan, None)), ("destination sector", (6, 6, 1, ok, ok)),
             ("destination sector", (6, 0, 2, ok, ok)), ("n_sites", (31, -1, 0, ok, ok)), ("n_sites", (33, 2, 0, ok, ok)), ("n_sites", (1, -1, 0, ok, ok)),
             ("n_up", (6, 7, 0, ok, ok)), ("n_up", (6, -2, 0, ok, ok)), ("NULL", (6, 3, 0, None, ok))]
    for word, args in cases:
        rc, msg, untouched = _raw(capi, *args)
        assert rc == -1 and word in msg and msg.startswith("eigenex_spin_site_apply_host_z: ") and untouched, (word, args, msg)
    assert bad[5] == 1.0 and _raw(capi, 4, 2, 0, ok, bad)[0] == 0  # an imaginary coefficient beyond n_sites is not read
    for kw in (dict(x=False), dict(y=False)):
        rc, msg, untouched = _raw(capi, 6, 3, 0, ok, ok, **kw)
        assert rc == -1 and "NULL" in msg and untouched
    # in place: Z only
    dp = C.POINTER(C.c_double)
    v = np.arange(1.0, 41.0)
    assert capi.lib().eigenex_spin_site_apply_host_z(6, -1, 1, ok.ctypes.data_as(dp), ok.ctypes.data_as(dp), v.ctypes.data_as(dp), v.ctypes.data_as(dp), None) == -1
    assert "reads what it would write" in capi.lib().eigenex_last_error().decode()
    want, _ = capi.spin_site_apply_host_z(6, 3, 0, ok[:6] + 1j * ok[:6], v.view(np.complex128))
    assert capi.lib().eigenex_spin_site_apply_host_z(6, 3, 0, ok.ctypes.data_as(dp), ok.ctypes.data_as(dp), v.ctypes.data_as(dp), v.ctypes.data_as(dp), None) == 0
    assert np.array_equal(v.view(np.complex128), want)


def test_exports_are_declared_and_present(capi):
    text = open(os.path.join(ROOT, "include", "eigenex_hip.h")).read()
    for name in ("eigenex_spin_site_apply_z", "eigenex_spin_site_apply_host_z"):
        assert re.search(r"\bint %s\s*\(" % name, text)
        assert hasattr(capi.lib(), name) and name in capi.SIGNATURES
    assert callable(capi.spin_site_apply_host_z) and callable(capi.Basis.spin_site_apply_z)
    assert "real_coef" in text and "may be NULL" in text[text.index("The same of a COMPLEX vector"):]  # the definition is stated


def test_site_z_host_code_under_sanitizers(tmp_path):
    """csrc/spin_site.hpp's complex code (argument check, kernel table, host evaluation) compiled into a stand-alone program with
    AddressSanitizer + UBSan, and the row loop of k_spin_site_apply<SECTOR, SpinZ> -- the kernel's own functions
    (csrc/spin_rows.hpp, compiled into the program) with every load bounds-checked -- equal to the host evaluation over every
    row of every shape.  Nothing is loaded into Python."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "spin_site_z_sanitize")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "spin_site_z_sanitize.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-1500:], out.stderr.decode()[-2000:])
    assert b"SPIN SITE Z OK" in out.stdout
