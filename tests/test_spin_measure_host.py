"""The spin measurement on the host: eigenex_spin_measure_host against the long double restatement of
tests/spin_measure_reference.py within the rounding bound of an n-term sum, physics with known answers (total spin of the
levels of the 12-site Heisenberg ring, magnetisation, product states, the singlet, <Sx> in a transverse field against the
Kronecker operators), every refusal of the argument check by its message, and the host code (csrc/spin_measure.hpp) under
AddressSanitizer + UBSan in a stand-alone program.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_measure_reference as mr  # noqa: E402
import spin_reference as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
SHAPES = [(3, None), (6, None), (9, None), (4, 2), (6, 0), (6, 6), (11, 5), (31, 2), (32, 2), (32, 31)]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g

    g.build()
    from cmpt_eigenex_amd import capi as c

    return c


@pytest.mark.parametrize("L,n_up", SHAPES)
def test_host_sums_equal_the_restatement_within_the_bound(capi, L, n_up):
    diag_masks, flip_masks = mr.term_lists(L, n_up)
    x = mr.vector(L, n_up)
    got = capi.spin_measure_host(L, n_up, x, diag_masks, flip_masks)
    assert got[0].dtype == np.float64 and got[0].size == diag_masks.size and got[1].size == flip_masks.size
    mr.check(f"host ({L},{n_up})", L, n_up, x, diag_masks, flip_masks, got)
    # the duplicate of the first pair is the first pair, bit for bit; a term does not depend on its neighbours in the lists
    assert got[0][-1] == got[0][L] and got[1][len(mr.pairs(L))] == got[1][0]
    alone = capi.spin_measure_host(L, n_up, x, diag_masks[L : L + 1], flip_masks[:1])
    assert alone[0][0] == got[0][L] and alone[1][0] == got[1][0] and alone[2] == got[2]
    # empty lists: norm2 alone
    d, f, n2 = capi.spin_measure_host(L, n_up, x, [], [])
    assert d.size == 0 and f.size == 0 and n2 == got[2]


def _s_squared(capi, L, n_up, x):
    d, f, n2 = capi.spin_measure_host(L, n_up, x, mr.site_masks(L) + mr.pair_masks(L), mr.pair_masks(L))
    sz, zz, xy, dot = mr.correlations(L, d[:L], d[L:], f, n2)
    return mr.total_spin_squared(dot), sz, dot


def test_total_spin_of_the_levels_of_the_heisenberg_ring(capi):
    """Periodic 12-site Heisenberg ring, eigenvectors of the dense sector matrices by numpy.linalg.eigh: <S^2> = S(S + 1) is 0 and
    2 for the two lowest levels of (12,6), 2 for the lowest of (12,5), 6 for the lowest of (12,4); sum_i <Sz_i> = n_up - L/2.
    1e-9: eigh's eigenvectors limit the accuracy, not the measurement."""
    L, bonds = 12, sr.chain(12, periodic=True)
    for n_up, want in ((6, (0.0, 2.0)), (5, (2.0,)), (4, (6.0,))):
        rowptr, col, val = capi.spin_sector_csr(L, n_up, bonds)
        _, X = np.linalg.eigh(sr.dense_from_csr(rowptr.size - 1, rowptr, col, val))
        for level, s2 in enumerate(want):
            got, sz, dot = _s_squared(capi, L, n_up, X[:, level])
            print(f"(12,{n_up}) level {level}: <S^2> = {float(got):.12f}, sum <Sz> = {float(sz.sum(dtype=LD)):.12f}")
            assert abs(got - s2) < 1e-9
            assert abs(sz.sum(dtype=LD) - (n_up - L / 2)) < 1e-12
            if level == 0 and n_up == 6:  # the ring is translation invariant: every bond carries E0 / 12
                nn = np.array([dot[i, (i + 1) % L] for i in range(L)], LD)
                assert np.abs(nn - (-5.387390917445 / 12)).max() < 1e-9


def test_product_states_and_the_singlet_exactly(capi):
    L = 5
    masks = mr.site_masks(L) + mr.pair_masks(L)
    for s in (0, 0b10110, 0b11111, 0b00001):
        x = np.zeros(1 << L)
        x[s] = -1.5
        d, f, n2 = capi.spin_measure_host(L, None, x, masks, mr.pair_masks(L) + mr.site_masks(L))
        sz, zz, xy, dot = mr.correlations(L, d[:L], d[L:], f[: len(mr.pairs(L))], n2)
        sigma = np.array([1.0 if (s >> i) & 1 else -1.0 for i in range(L)])
        assert n2 == 2.25 and not f.any()
        assert np.array_equal(sz.astype(np.float64), sigma / 2)
        for (i, j) in mr.pairs(L):
            assert zz[i, j] == sigma[i] * sigma[j] / 4 and dot[i, j] == zz[i, j]
        # the same state in its sector
        n_up = bin(s).count("1")
        xs = np.zeros(mr.rows(L, n_up))
        xs[int(np.searchsorted(mr.states(L, n_up), s))] = -1.5
        ds, fs, n2s = capi.spin_measure_host(L, n_up, xs, masks, mr.pair_masks(L))
        assert np.array_equal(ds, d) and not fs.any() and n2s == n2
    # (|up down> - |down up>) / sqrt(2), unnormalised: Sz Sz = -1/4, Sx Sx + Sy Sy = -1/2, S.S = -3/4
    for n_up, x in ((None, [0.0, 1.0, -1.0, 0.0]), (1, [1.0, -1.0])):
        d, f, n2 = capi.spin_measure_host(2, n_up, x, [1, 2, 3], [3])
        assert (d[0], d[1], n2) == (0.0, 0.0, 2.0)
        assert d[2] / (4 * n2) == -0.25 and f[0] / (2 * n2) == -0.5 and d[2] / (4 * n2) + f[0] / (2 * n2) == -0.75
    # the triplet partner (|up down> + |down up>): S.S = +1/4
    d, f, n2 = capi.spin_measure_host(2, 1, [1.0, 1.0], [3], [3])
    assert d[0] / (4 * n2) + f[0] / (2 * n2) == 0.25


def test_transverse_magnetisation_against_the_kronecker_operators(capi):
    """full space with hx: the ground state of the 'fields' model at L = 6 by eigh of the Kronecker Hamiltonian; <Sx_i>, <Sz_i> and
    <Sz_i Sz_j> of the measurement against x^T O x with O from Kronecker products, both sides from the same x, the reference
    in long double.  The bound is that of the sums (n eps sum |terms|) plus the rounding of the reference's operator entries,
    which are exact here (0, 1/2, 1/4)."""
    L = 6
    n_sites, bonds, hz, hx = sr.models(L)["fields"]
    assert np.count_nonzero(hx) > 0
    _, X = np.linalg.eigh(sr.dense_kron(n_sites, bonds, hz, hx))
    x = X[:, 0]
    xl = x.astype(LD)
    d, f, n2 = capi.spin_measure_host(L, None, x, mr.site_masks(L) + mr.pair_masks(L), mr.site_masks(L))
    n, largest = 1 << L, 0.0
    for i in range(L):
        Ox, Oz = sr._site_operator(L, {i: sr._SX}).astype(LD), sr._site_operator(L, {i: sr._SZ}).astype(LD)
        ref_x, ref_z = xl @ (Ox @ xl), xl @ (Oz @ xl)
        bound_x = n * mr.EPS * (np.abs(xl) @ (np.abs(Ox) @ np.abs(xl)))
        bound_z = n * mr.EPS * (np.abs(xl) @ (np.abs(Oz) @ np.abs(xl)))
        assert abs(LD(f[i]) / 2 - ref_x) <= bound_x and abs(LD(d[i]) / 2 - ref_z) <= bound_z
        largest = max(largest, abs(float(ref_x)))
    for k, (i, j) in enumerate(mr.pairs(L)):
        O = sr._site_operator(L, {i: sr._SZ, j: sr._SZ}).astype(LD)
        assert abs(LD(d[L + k]) / 4 - xl @ (O @ xl)) <= n * mr.EPS * (np.abs(xl) @ (np.abs(O) @ np.abs(xl)))
    assert abs(n2 - 1.0) < 1e-12 and largest > 1e-2  # the field polarises the chain: the comparison is not 0 = 0


def _raw(capi, n_sites, n_up, n_diag, diag, n_flip, flip, x=True, outs=True):
    up = C.POINTER(C.c_uint32)
    dm = None if diag is None else np.ascontiguousarray(diag, np.uint32)
    fm = None if flip is None else np.ascontiguousarray(flip, np.uint32)
    xv, do, fo, n2 = np.ones(1 << 6), np.full(1100, -7.0), np.full(1100, -7.0), C.c_double(-7.0)
    dp = C.POINTER(C.c_double)
    rc = capi.lib().eigenex_spin_measure_host(n_sites, n_up, xv.ctypes.data_as(dp) if x else None, n_diag, None if dm is None else dm.ctypes.data_as(up), n_flip,
                                             None if fm is None else fm.ctypes.data_as(up), do.ctypes.data_as(dp) if outs else None,
                                             fo.ctypes.data_as(dp) if outs else None, C.byref(n2))
    untouched = n2.value == -7.0 and np.all(do == -7.0) and np.all(fo == -7.0)
    return rc, capi.lib().eigenex_last_error().decode(), untouched


def test_every_refusal_returns_a_code_and_a_message(capi):
    ok = [3, 5]
    assert _raw(capi, 6, -1, 2, ok, 2, ok)[0] == 0 and _raw(capi, 6, 3, 2, ok, 2, ok)[0] == 0
    cases = [
        ("zero", (6, -1, 2, [3, 0], 0, None)),
        ("zero", (6, 3, 0, None, 2, [0, 3])),
        ("outside", (6, -1, 1, [1 << 6], 0, None)),
        ("outside", (6, 3, 0, None, 1, [(1 << 6) | 1])),
        ("outside", (31, 2, 1, [1 << 31], 0, None)),
        ("one or two", (6, -1, 0, None, 1, [7])),
        ("one or two", (6, 3, 0, None, 1, [15])),
        ("conserve total Sz", (6, 3, 0, None, 1, [4])),
        ("n_diag", (6, -1, -1, ok, 0, None)),
        ("n_diag", (6, -1, 1025, [1] * 1025, 0, None)),
        ("n_flip", (6, -1, 0, None, 1025, [3] * 1025)),
        ("n_flip", (6, -1, 0, None, -3, ok)),
        ("NULL", (6, -1, 2, None, 0, None)),
        ("NULL", (6, 3, 0, None, 1, None)),
        ("n_sites", (31, -1, 0, None, 0, None)),
        ("n_sites", (33, 2, 0, None, 0, None)),
        ("n_sites", (1, -1, 0, None, 0, None)),
        ("n_up", (6, 7, 0, None, 0, None)),
        ("n_up", (6, -2, 0, None, 0, None)),
    ]
    for word, args in cases:
        rc, msg, untouched = _raw(capi, *args)
        assert rc != 0 and word in msg and msg.startswith("eigenex_spin_measure_host: ") and untouched, (word, args, msg)
    rc, msg, untouched = _raw(capi, 6, -1, 2, ok, 0, None, x=False)
    assert rc != 0 and "x is NULL" in msg and untouched
    rc, msg, untouched = _raw(capi, 6, -1, 2, ok, 0, None, outs=False)
    assert rc != 0 and "output" in msg
    # 1024 terms are allowed, duplicates and all; a one-bit flip is fine in the full space; an unused output may be NULL
    assert _raw(capi, 6, -1, 1024, [5] * 1024, 1024, [1] * 1024)[0] == 0
    assert _raw(capi, 6, -1, 0, None, 0, None, outs=False)[0] == 0
    with pytest.raises(capi.EigenexError, match="conserve total Sz"):
        capi.spin_measure_host(4, 2, np.ones(6), [1], [2])


def test_exports_are_declared_and_present(capi):
    text = open(os.path.join(ROOT, "include", "eigenex_hip.h")).read()
    for name in ("eigenex_spin_measure", "eigenex_spin_measure_host", "eigenex_spin_geometry"):
        assert re.search(r"\bint %s\s*\(" % name, text)
        assert hasattr(capi.lib(), name) and name in capi.SIGNATURES


def test_measure_host_code_under_sanitizers(tmp_path):
    """csrc/spin_measure.hpp (argument check, chunk table, host evaluation) compiled into a stand-alone program with
    AddressSanitizer + UBSan: outputs into exactly-sized arrays, and the row loop of k_spin_measure on its chunk table -- the
    kernel's own functions (csrc/spin_rows.hpp, compiled into the program) with every load bounds-checked -- bit-identical to
    the host evaluation."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "spin_measure_sanitize")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "spin_measure_sanitize.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-1500:], out.stderr.decode()[-2000:])
    assert b"SPIN MEASURE OK" in out.stdout
