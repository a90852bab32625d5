"""The fixed-magnetisation sector of the spin-1/2 Hamiltonian on the host: eigenex_spin_sector_dim / _states / _csr against the
numpy restatements of tests/spin_sector_reference.py (enumeration, searchsorted, the full-space rows restricted to the
sector), the union of the sector spectra against the Kronecker Hamiltonian, the argument errors of all four sector entry
points, and the host code (csrc/spin_sector.hpp) under AddressSanitizer + UBSan in a stand-alone program.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
from math import comb

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_reference as sr  # noqa: E402
import spin_sector_reference as ss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTORS = [(L, k) for L in (2, 3, 6, 8, 11, 12) for k in range(L + 1)]
EDGE = [(32, 1), (32, 2), (32, 31), (31, 2)]
NAMES = ("open", "periodic", "random40", "ising", "fields")  # spin_reference.models with hx removed


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g

    g.build()
    from cmpt_eigenex_amd import capi as c

    return c


def _model(L, name):
    return ss.without_hx(sr.models(L)[name])


@pytest.mark.parametrize("L,n_up", SECTORS + EDGE)
def test_dim_states_and_rank_equal_the_enumeration(capi, L, n_up):
    st = ss.states(L, n_up)
    assert capi.spin_sector_dim(L, n_up) == comb(L, n_up) == st.size
    got = capi.spin_sector_states(L, n_up)
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got.astype(np.uint64), st)
    # a window of ranks, and the empty one at the end
    a, b = st.size // 3, st.size - st.size // 4
    np.testing.assert_array_equal(capi.spin_sector_states(L, n_up, a, b - a).astype(np.uint64), st[a:b])
    assert capi.spin_sector_states(L, n_up, st.size, 0).size == 0
    # rank: a model whose only off-diagonal entry per row comes from one bond shows rank(s ^ mask) as the column; every pair
    # of sites (every pair with the top site where there are 31 or 32) covers masks inside the low half, inside the high half
    # and across the split
    pairs = [(i, j) for i in range(L) for j in range(i + 1, L)] if L <= 12 else [(i, L - 1) for i in range(L - 1)] + [(0, 1), (15, 16), (14, 17)]
    for (i, j) in pairs:
        rowptr, col, _ = capi.spin_sector_csr(L, n_up, [(i, j, 1.0, 1.0)])
        np.testing.assert_array_equal(col[rowptr[:-1]], np.arange(st.size))  # the diagonal: rank(state(r)) = r
        flips = ((st >> np.uint64(i)) ^ (st >> np.uint64(j))) & np.uint64(1) == 1
        assert np.array_equal(np.diff(rowptr), 1 + flips.astype(np.int64))
        want = ss.rank(st, st[flips] ^ np.uint64((1 << i) | (1 << j)))
        np.testing.assert_array_equal(col[rowptr[:-1][flips] + 1], want)


ROW_CASES = [(L, k) for L in (2, 3, 6, 8) for k in range(L + 1)] + [(11, 5), (12, 6), (31, 2), (32, 2), (32, 31)]


@pytest.mark.parametrize("name", NAMES)
def test_rows_equal_the_restatement_bit_for_bit(capi, name):
    for (L, n_up) in ROW_CASES:
        n_sites, bonds, hz = _model(L, name)
        rowptr, col, val = capi.spin_sector_csr(n_sites, n_up, bonds, hz)
        rp, cl, vl = ss.rows_csr(n_sites, n_up, bonds, hz)
        assert rowptr.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.float64
        np.testing.assert_array_equal(rowptr, rp, err_msg=f"{name} ({L},{n_up})")
        np.testing.assert_array_equal(col, cl, err_msg=f"{name} ({L},{n_up})")
        assert val.tobytes() == vl.tobytes(), (name, L, n_up)
        assert np.all(col[rowptr[:-1]] == np.arange(rowptr.size - 1))  # the diagonal is stored first, in every row
        if name == "ising":
            assert col.size == comb(L, n_up)
        # an all-zero transverse field is no transverse field
        rp0, cl0, vl0 = capi.spin_sector_csr(n_sites, n_up, bonds, hz, np.zeros(n_sites))
        assert np.array_equal(rp0, rowptr) and np.array_equal(cl0, col) and vl0.tobytes() == val.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_row_window_and_count_only_call(capi, name):
    n_sites, bonds, hz = _model(8, name)
    n_up, dim = 4, 70
    rowptr, col, val = capi.spin_sector_csr(n_sites, n_up, bonds, hz)
    for rb, nr in ((0, 70), (0, 1), (17, 40), (69, 1), (50, 0), (70, 0)):
        rp, cl, vl = capi.spin_sector_csr(n_sites, n_up, bonds, hz, row_begin=rb, n_rows=nr)
        np.testing.assert_array_equal(rp, rowptr[rb : rb + nr + 1] - rowptr[rb])
        np.testing.assert_array_equal(cl, col[rowptr[rb] : rowptr[rb + nr]])
        assert vl.tobytes() == val[rowptr[rb] : rowptr[rb + nr]].tobytes()
        keep, args = capi._spin_model(n_sites, bonds, hz, None)
        rp2, nnz = np.full(nr + 1, -1, np.int64), C.c_int64(-1)
        assert capi.lib().eigenex_spin_sector_csr(*capi._sector_args(args, n_up), rb, nr, rp2.ctypes.data_as(C.POINTER(C.c_int64)), None, None, C.byref(nnz)) == 0
        np.testing.assert_array_equal(rp2, rp)
        assert nnz.value == cl.size == rp[-1]
    assert dim == rowptr.size - 1


@pytest.mark.parametrize("name", NAMES)
def test_dense_sector_matrix_is_symmetric(capi, name):
    for (L, n_up) in ((6, 3), (8, 3), (11, 5)):
        n_sites, bonds, hz = _model(L, name)
        rowptr, col, val = capi.spin_sector_csr(n_sites, n_up, bonds, hz)
        H = sr.dense_from_csr(rowptr.size - 1, rowptr, col, val)
        assert np.array_equal(H, H.T), (name, L, n_up)


@pytest.mark.parametrize("name", NAMES)
def test_union_of_the_sector_spectra_is_the_full_spectrum(capi, name):
    """L = 8: the eigenvalues of the nine sector matrices together are those of the Kronecker Hamiltonian of the full model.
    Compared sorted, within 1e-12 |H|_max: the margin scale of the Kronecker test of tests/test_spin_host.py (1e-14 |H|_max for
    entries), loosened for the eigensolver's own error (a few n eps |H|_2 at n = 256)."""
    n_sites, bonds, hz = _model(8, name)
    K = sr.dense_kron(n_sites, bonds, hz, None)
    lam = np.linalg.eigvalsh(K)
    parts = []
    for n_up in range(9):
        rowptr, col, val = capi.spin_sector_csr(n_sites, n_up, bonds, hz)
        parts.append(np.linalg.eigvalsh(sr.dense_from_csr(rowptr.size - 1, rowptr, col, val)))
    got = np.sort(np.concatenate(parts))
    assert got.size == 256
    err, scale = np.abs(got - lam).max(), np.abs(K).max()
    print(f"{name}: max eigenvalue difference {err:.3e}, |H|_max {scale:.3e}")
    assert err <= 1e-12 * scale


def _raw_csr(capi, n_sites, n_up, bonds, hz=None, hx=None, rb=0, nr=1):
    keep, args = capi._spin_model(n_sites, bonds, hz, hx)
    rp, nnz = np.zeros(max(nr, 0) + 1, np.int64), C.c_int64()
    rc = capi.lib().eigenex_spin_sector_csr(*capi._sector_args(args, n_up), rb, nr, rp.ctypes.data_as(C.POINTER(C.c_int64)), None, None, C.byref(nnz))
    return rc, capi.lib().eigenex_last_error().decode()


def test_argument_errors_return_a_code_and_a_message(capi):
    ok = [(0, 1, 1.0, 1.0)]
    L = capi.lib()
    dim, st = C.c_int64(-7), np.zeros(8, np.uint32)
    sp = st.ctypes.data_as(C.POINTER(C.c_uint32))
    for n_sites in (1, 33, 0, -2):
        rc, msg = _raw_csr(capi, n_sites, 1, ok if n_sites > 1 else [])
        assert rc != 0 and "n_sites" in msg, (n_sites, msg)
        assert L.eigenex_spin_sector_dim(n_sites, 1, C.byref(dim)) != 0 and "n_sites" in L.eigenex_last_error().decode()
        assert L.eigenex_spin_sector_states(n_sites, 1, 0, 1, sp) != 0
    for n_sites, n_up in ((4, -1), (4, 5), (32, 33)):
        rc, msg = _raw_csr(capi, n_sites, n_up, ok)
        assert rc != 0 and "n_up" in msg, (n_sites, n_up, msg)
        assert L.eigenex_spin_sector_dim(n_sites, n_up, C.byref(dim)) != 0 and "n_up" in L.eigenex_last_error().decode()
        assert L.eigenex_spin_sector_states(n_sites, n_up, 0, 1, sp) != 0
    assert dim.value == -7 and not st.any()  # nothing written
    # 31 and 32 sites are sectors, and only sectors
    assert _raw_csr(capi, 32, 2, ok)[0] == 0 and _raw_csr(capi, 31, 30, ok)[0] == 0
    with pytest.raises(capi.EigenexError, match="n_sites"):
        capi.spin_csr(31, ok)
    # the model checks of the full-space operator
    for word, bonds in (("n_bonds", ok * 65), ("outside", [(0, 4, 1.0, 1.0)]), ("itself", [(2, 2, 1.0, 1.0)]), ("finite", [(0, 1, np.nan, 1.0)])):
        rc, msg = _raw_csr(capi, 4, 2, bonds)
        assert rc != 0 and word in msg, (word, msg)
    rc, msg = _raw_csr(capi, 4, 2, ok, np.array([0.0, np.nan, 0.0, 0.0]))
    assert rc != 0 and "finite" in msg
    # a transverse field does not conserve Sz; an all-zero one is none
    rc, msg = _raw_csr(capi, 4, 2, ok, None, np.array([0.0, 0.0, 0.25, 0.0]))
    assert rc != 0 and "transverse" in msg
    assert _raw_csr(capi, 4, 2, ok, None, np.zeros(4))[0] == 0
    with pytest.raises(capi.EigenexError, match="transverse"):
        capi.spin_sector_csr(4, 2, ok, hx=[0.0, 1.0, 0.0, 0.0])
    # rows outside 0..dim (C(4,2) = 6), col without val, no rowptr
    for rb, nr in ((3, 4), (-1, 2), (0, 7), (7, 0), (0, -1)):
        rc, msg = _raw_csr(capi, 4, 2, ok, rb=rb, nr=nr)
        assert rc != 0 and "rows" in msg, (rb, nr, msg)
    assert _raw_csr(capi, 4, 2, ok, rb=6, nr=0)[0] == 0
    for first, count in ((3, 4), (-1, 2), (7, 0), (0, -1)):
        assert L.eigenex_spin_sector_states(4, 2, first, count, sp) != 0 and "ranks" in L.eigenex_last_error().decode()
    assert L.eigenex_spin_sector_states(4, 2, 0, 2, None) != 0
    assert L.eigenex_spin_sector_dim(4, 2, None) != 0
    keep, args = capi._spin_model(4, ok, None, None)
    sargs = capi._sector_args(args, 2)
    rp, nnz, cl = np.zeros(8, np.int64), C.c_int64(), np.zeros(64, np.int32)
    lp = rp.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.eigenex_spin_sector_csr(*sargs, 0, 4, lp, cl.ctypes.data_as(C.POINTER(C.c_int32)), None, C.byref(nnz)) != 0
    assert L.eigenex_spin_sector_csr(*sargs, 0, 4, None, None, None, C.byref(nnz)) != 0
    # the upload checks its model before it touches the context: the same errors without a GPU, and a NULL context is an error too
    h = C.c_void_p()
    assert L.eigenex_spin_sector_upload(None, *sargs, C.byref(h)) != 0 and not h.value
    with pytest.raises(ValueError):
        capi.spin_sector_csr(4, 2, ok, hz=np.zeros(3))


def test_exports_are_declared_and_present(capi):
    text = open(os.path.join(ROOT, "include", "eigenex_hip.h")).read()
    for name in ("eigenex_spin_sector_dim", "eigenex_spin_sector_states", "eigenex_spin_sector_csr", "eigenex_spin_sector_upload"):
        assert re.search(r"\bint %s\s*\(" % name, text)
        assert hasattr(capi.lib(), name) and name in capi.SIGNATURES
    assert "EIGENEX_LAYOUT_MATRIX_FREE_SPIN_SECTOR = 6" in text
    assert "EIGENEX_LAYOUT_MATRIX_FREE_SPIN = 5" in text


def test_sector_host_code_under_sanitizers(capi, tmp_path):
    """csrc/spin_sector.hpp (argument checks, binomials, unrank, the rank tables, the sector rows, the kernel's view) compiled
    into a stand-alone program with AddressSanitizer + UBSan, together with the sector calls of SpinHalfModel: rank and unrank
    round trips, rows written into exactly-sized arrays, and the row sum of k_spin_spmv<true> compared bitwise with the rows:
    the kernel's own functions (csrc/spin_rows.hpp, compiled into the program) run on its tables, every load bounds-checked."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "spin_sector_sanitize")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "spin_sector_sanitize.cpp"),
                           "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the HIP runtime's own start-up allocations are not ours to judge
    out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-1500:], out.stderr.decode()[-2000:])
    assert b"SPIN SECTOR OK" in out.stdout
