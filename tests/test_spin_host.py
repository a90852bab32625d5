"""eigenex_spin_csr -- the host-side definition of the spin-1/2 Hamiltonian that the matrix-free kernel is held against --
against the two numpy restatements of tests/spin_reference.py, the argument errors of both spin entry points, and the
host code under AddressSanitizer + UBSan in a stand-alone program.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_reference as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (2, 3, 6, 8, 10)
NAMES = ("open", "periodic", "random40", "fields", "random40_fields", "ising")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g

    g.build()
    from cmpt_eigenex_amd import capi as c

    return c


@pytest.mark.parametrize("L", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_rows_equal_the_restatement_bit_for_bit(capi, name, L):
    n_sites, bonds, hz, hx = sr.models(L)[name]
    rowptr, col, val = capi.spin_csr(n_sites, bonds, hz, hx)
    rp, cl, vl = sr.rows_csr(n_sites, bonds, hz, hx)
    assert rowptr.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.float64
    np.testing.assert_array_equal(rowptr, rp)
    np.testing.assert_array_equal(col, cl)
    assert val.tobytes() == vl.tobytes()
    assert np.all(col[rowptr[:-1]] == np.arange(1 << L))  # the diagonal is stored first, in every row
    if name == "ising":
        assert col.size == 1 << L  # no flip anywhere


@pytest.mark.parametrize("L", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_dense_form_equals_the_kronecker_hamiltonian(capi, name, L):
    n_sites, bonds, hz, hx = sr.models(L)[name]
    n = 1 << L
    H = sr.dense_from_csr(n, *capi.spin_csr(n_sites, bonds, hz, hx))
    K = sr.dense_kron(n_sites, bonds, hz, hx)
    err, scale = np.abs(H - K).max(), np.abs(K).max()
    print(f"{name} L={L}: |H - H_kron|_max = {err:.3e}, |H|_max = {scale:.3e}")
    assert np.array_equal(H, H.T)
    assert err <= 1e-14 * scale


def test_known_spectra(capi):
    H2 = sr.dense_from_csr(4, *capi.spin_csr(2, sr.chain(2)))
    np.testing.assert_allclose(np.linalg.eigvalsh(H2), [-0.75, 0.25, 0.25, 0.25], rtol=0, atol=1e-15)
    H4 = sr.dense_from_csr(16, *capi.spin_csr(4, sr.chain(4, periodic=True)))
    assert abs(np.linalg.eigvalsh(H4)[0] + 2.0) < 1e-14


@pytest.mark.parametrize("name", NAMES)
def test_row_window_and_count_only_call(capi, name):
    n_sites, bonds, hz, hx = sr.models(8)[name]
    rowptr, col, val = capi.spin_csr(n_sites, bonds, hz, hx)
    for rb, nr in ((0, 256), (0, 1), (37, 100), (255, 1), (200, 0), (256, 0)):
        rp, cl, vl = capi.spin_csr(n_sites, bonds, hz, hx, row_begin=rb, n_rows=nr)
        np.testing.assert_array_equal(rp, rowptr[rb : rb + nr + 1] - rowptr[rb])
        np.testing.assert_array_equal(cl, col[rowptr[rb] : rowptr[rb + nr]])
        assert vl.tobytes() == val[rowptr[rb] : rowptr[rb + nr]].tobytes()
        # the count-only form (col == val == NULL) of the raw entry point
        keep, args = capi._spin_model(n_sites, bonds, hz, hx)
        rp2, nnz = np.full(nr + 1, -1, np.int64), C.c_int64(-1)
        assert capi.lib().eigenex_spin_csr(*args, rb, nr, rp2.ctypes.data_as(C.POINTER(C.c_int64)), None, None, C.byref(nnz)) == 0
        np.testing.assert_array_equal(rp2, rp)
        assert nnz.value == cl.size == rp[-1]


def _raw_csr(capi, n_sites, bonds, hz=None, hx=None, n_rows=1):
    keep, args = capi._spin_model(n_sites, bonds, hz, hx)
    rp, nnz = np.zeros(n_rows + 1, np.int64), C.c_int64()
    rc = capi.lib().eigenex_spin_csr(*args, 0, n_rows, rp.ctypes.data_as(C.POINTER(C.c_int64)), None, None, C.byref(nnz))
    return rc, capi.lib().eigenex_last_error().decode()


def test_argument_errors_return_a_code_and_a_message(capi):
    ok = [(0, 1, 1.0, 1.0)]
    cases = {
        "n_sites": [(1, ok), (31, ok), (0, []), (-3, [])],
        "n_bonds": [(4, [(0, 1, 1.0, 1.0)] * 65)],
        "outside": [(4, [(0, 4, 1.0, 1.0)]), (4, [(-1, 2, 1.0, 1.0)]), (4, [(2, 17, 1.0, 1.0)])],
        "itself": [(4, [(2, 2, 1.0, 1.0)])],
        "finite": [(4, [(0, 1, np.nan, 1.0)]), (4, [(0, 1, 1.0, np.inf)])],
    }
    for word, models in cases.items():
        for n_sites, bonds in models:
            rc, msg = _raw_csr(capi, n_sites, bonds)
            assert rc != 0 and word in msg, (n_sites, bonds, rc, msg)
    for hz, hx in ((np.array([0.0, np.nan, 0.0, 0.0]), None), (None, np.array([0.0, 0.0, -np.inf, 0.0]))):
        rc, msg = _raw_csr(capi, 4, ok, hz, hx)
        assert rc != 0 and "finite" in msg
    # rows outside the matrix, col without val
    keep, args = capi._spin_model(4, ok, None, None)
    rp, nnz, cl = np.zeros(40, np.int64), C.c_int64(), np.zeros(64, np.int32)
    lp = rp.ctypes.data_as(C.POINTER(C.c_int64))
    L = capi.lib()
    assert L.eigenex_spin_csr(*args, 10, 7, lp, None, None, C.byref(nnz)) != 0 and "rows" in L.eigenex_last_error().decode()
    assert L.eigenex_spin_csr(*args, -1, 2, lp, None, None, C.byref(nnz)) != 0
    assert L.eigenex_spin_csr(*args, 0, 4, lp, cl.ctypes.data_as(C.POINTER(C.c_int32)), None, C.byref(nnz)) != 0
    assert L.eigenex_spin_csr(*args, 0, 4, None, None, None, C.byref(nnz)) != 0
    # the upload checks its model before it touches the context: the same errors without a GPU, and a NULL context is an error too
    with pytest.raises(capi.EigenexError):
        capi.spin_csr(1, ok)
    h = C.c_void_p()
    assert L.eigenex_spin_upload(None, *args, C.byref(h)) != 0 and not h.value
    with pytest.raises(ValueError):
        capi.spin_csr(4, ok, hz=np.zeros(3))


def test_exports_are_declared_and_present(capi):
    text = open(os.path.join(ROOT, "include", "eigenex_hip.h")).read()
    for name in ("eigenex_spin_upload", "eigenex_spin_csr"):
        assert re.search(r"\bint %s\s*\(" % name, text)
        assert hasattr(capi.lib(), name) and name in capi.SIGNATURES
    assert "EIGENEX_LAYOUT_MATRIX_FREE_SPIN = 5" in text


def test_spin_host_code_under_sanitizers(capi, tmp_path):
    """csrc/spin_model.hpp (argument checks, the CSR rows, the kernel's tables) compiled into a stand-alone program with
    AddressSanitizer + UBSan, together with SpinHalfModel of spin_operator.hpp: for every model above at L = 2..10 the rows
    are written into exactly-sized arrays and compared bitwise with the row sums of k_spin_spmv<false>, for which the kernel's
    own functions (csrc/spin_rows.hpp, compiled into the program) run on the kernel's tables through bounds-checked accessors."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "spin_model_sanitize")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "spin_model_sanitize.cpp"),
                           "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the HIP runtime's own start-up allocations are not ours to judge
    out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-1500:], out.stderr.decode()[-2000:])
    assert b"SPIN MODEL OK" in out.stdout
