"""The observables of one vector against a set of columns on the host: eigenex_spin_measure_columns_host against the long double
restatement of tests/spin_measure_columns_reference.py within the rounding bound of an n-term sum, the bit-for-bit tie to
eigenex_spin_measure_host where the column is the vector itself, the independence of a sum from what shares its call, every
refusal of the argument check by its message with the outputs untouched, and the host code (csrc/spin_measure_columns.hpp)
with the kernel's row loop under AddressSanitizer + UBSan in a stand-alone program.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_measure_columns_reference as cr  # noqa: E402
import spin_measure_reference as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, None), (6, None), (9, None), (4, 2), (6, 0), (6, 6), (11, 5), (31, 2), (32, 2), (32, 31)]
COUNT = 5  # one above the kernel's column chunk


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g

    g.build()
    from cmpt_eigenex_amd import capi as c

    return c


@pytest.mark.parametrize("L,n_up", SHAPES)
def test_host_sums_equal_the_restatement_within_the_bound(capi, L, n_up):
    diag_masks, flip_masks = mr.term_lists(L, n_up)
    x, V = mr.vector(L, n_up), cr.columns(L, n_up, COUNT)
    got = capi.spin_measure_columns_host(L, n_up, x, V, diag_masks, flip_masks)
    assert got[0].shape == (diag_masks.size, COUNT) and got[1].shape == (flip_masks.size, COUNT)
    cr.check(f"host ({L},{n_up})", L, n_up, got, cr.measure(L, n_up, x, V, diag_masks, flip_masks))
    # the duplicate of the first pair is the first pair, bit for bit
    assert got[0][-1].tobytes() == got[0][L].tobytes() and got[1][len(mr.pairs(L))].tobytes() == got[1][0].tobytes()
    # a sum does not depend on the terms and columns it shares the call with
    alone = capi.spin_measure_columns_host(L, n_up, x, V[2:3], diag_masks[L : L + 1], flip_masks[:1])
    assert alone[0][0, 0] == got[0][L, 2] and alone[1][0, 0] == got[1][0, 2]
    # one list may be empty
    d, f = capi.spin_measure_columns_host(L, n_up, x, V, diag_masks, [])
    assert f.shape == (0, COUNT) and d.tobytes() == got[0].tobytes()


@pytest.mark.parametrize("L,n_up", SHAPES)
def test_a_column_that_is_the_vector_gives_the_bits_of_the_measurement(capi, L, n_up):
    """V_j = x: diag[t] has the fma chain of eigenex_spin_measure_host's diag[t]; the flip sums agree within the bound (there the
    measurement adds x_s * x_partner, the same product, so they are the same bits too)"""
    diag_masks, flip_masks = mr.term_lists(L, n_up)
    x = mr.vector(L, n_up)
    d1, f1, _ = capi.spin_measure_host(L, n_up, x, diag_masks, flip_masks)
    d2, f2 = capi.spin_measure_columns_host(L, n_up, x, np.stack([x, -x]), diag_masks, flip_masks)
    assert d2[:, 0].tobytes() == d1.tobytes() and d2[:, 1].tobytes() == (-d1).tobytes()
    assert f2[:, 0].tobytes() == f1.tobytes()


def test_known_answers(capi):
    # the singlet and the triplet of two sites against each other (row 0 is site 0 up): <t| sigma_0 |s> = 2, <t| sigma_1 |s> = -2,
    # sigma_0 sigma_1 = -1 on both rows, and S+S- + S-S+ takes |s> to -|s>
    s, t = np.array([1.0, -1.0]), np.array([1.0, 1.0])
    d, f = capi.spin_measure_columns_host(2, 1, s, np.stack([s, t]), [1, 2, 3], [3])
    assert d.tolist() == [[0.0, 2.0], [0.0, -2.0], [-2.0, 0.0]] and f.tolist() == [[-2.0, 0.0]]
    # full space, 2 Sx_0 moves |00> to |01>
    x = np.array([1.0, 0.0, 0.0, 0.0])
    d, f = capi.spin_measure_columns_host(2, None, x, np.eye(4), [], [1, 2, 3])
    assert f.tolist() == [[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0]]
    # ldv larger than the rows: the columns are strided
    V = np.arange(24.0).reshape(3, 8)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    out, mask, xs = np.zeros(3), np.array([1], np.uint32), np.ones(4)
    assert capi.lib().eigenex_spin_measure_columns_host(2, -1, xs.ctypes.data_as(dp), V.ctypes.data_as(dp), 8, 3, 1, mask.ctypes.data_as(up), 0, None,
                                                        out.ctypes.data_as(dp), None) == 0
    assert out.tolist() == [float((V[j, :4] * [-1, 1, -1, 1]).sum()) for j in range(3)]


def _raw(capi, n_sites, n_up, count, n_diag, diag, n_flip, flip, x=True, v=True, outs=True, ldv=64):
    up, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    dm = None if diag is None else np.ascontiguousarray(diag, np.uint32)
    fm = None if flip is None else np.ascontiguousarray(flip, np.uint32)
    xv, vv, do, fo = np.ones(1 << 6), np.ones(2 << 6), np.full(2200, -7.0), np.full(2200, -7.0)
    rc = capi.lib().eigenex_spin_measure_columns_host(n_sites, n_up, xv.ctypes.data_as(dp) if x else None, vv.ctypes.data_as(dp) if v else None, ldv, count,
                                                     n_diag, None if dm is None else dm.ctypes.data_as(up), n_flip,
                                                     None if fm is None else fm.ctypes.data_as(up), do.ctypes.data_as(dp) if outs else None,
                                                     fo.ctypes.data_as(dp) if outs else None)
    return rc, capi.lib().eigenex_last_error().decode(), bool(np.all(do == -7.0) and np.all(fo == -7.0))


def test_every_refusal_returns_a_code_and_a_message(capi):
    ok = [3, 5]
    assert _raw(capi, 6, -1, 2, 2, ok, 2, ok)[0] == 0 and _raw(capi, 6, 3, 2, 2, ok, 2, ok)[0] == 0
    cases = [
        ("zero", (6, -1, 1, 2, [3, 0], 0, None)),
        ("zero", (6, 3, 1, 0, None, 2, [0, 3])),
        ("outside", (6, -1, 1, 1, [1 << 6], 0, None)),
        ("outside", (6, 3, 1, 0, None, 1, [(1 << 6) | 1])),
        ("outside", (31, 2, 1, 1, [1 << 31], 0, None)),
        ("one or two", (6, -1, 1, 0, None, 1, [7])),
        ("conserve total Sz", (6, 3, 1, 0, None, 1, [4])),
        ("n_diag", (6, -1, 1, -1, ok, 0, None)),
        ("n_diag", (6, -1, 1, 1025, [1] * 1025, 0, None)),
        ("n_flip", (6, -1, 1, 0, None, 1025, [3] * 1025)),
        ("NULL", (6, -1, 1, 2, None, 0, None)),
        ("NULL", (6, 3, 1, 0, None, 1, None)),
        ("n_sites", (31, -1, 1, 0, None, 0, None)),
        ("n_sites", (33, 2, 1, 0, None, 0, None)),
        ("n_up", (6, 7, 1, 0, None, 0, None)),
        ("count must be at least 1", (6, -1, 0, 2, ok, 0, None)),
        ("count must be at least 1", (6, 3, -2, 2, ok, 2, ok)),
    ]
    for word, args in cases:
        rc, msg, untouched = _raw(capi, *args)
        assert rc == -1 and word in msg and msg.startswith("eigenex_spin_measure_columns_host: ") and untouched, (word, args, msg)
    for kw, word in ((dict(x=False), "x or V is NULL"), (dict(v=False), "x or V is NULL"), (dict(outs=False), "output"), (dict(ldv=63), "ldv")):
        rc, msg, untouched = _raw(capi, 6, -1, 2, 2, ok, 0, None, **kw)
        assert rc == -1 and word in msg and untouched, (kw, msg)
    assert _raw(capi, 6, 3, 2, 2, ok, 0, None, ldv=20)[0] == 0  # 20 rows
    # 1024 terms are allowed; an unused output may be NULL
    assert _raw(capi, 6, -1, 2, 1024, [5] * 1024, 1024, [1] * 1024)[0] == 0
    assert _raw(capi, 6, -1, 2, 0, None, 0, None, outs=False)[0] == 0
    with pytest.raises(capi.EigenexError, match="conserve total Sz"):
        capi.spin_measure_columns_host(4, 2, np.ones(6), np.ones((1, 6)), [1], [2])
    with pytest.raises(ValueError, match="rows of x"):
        capi.spin_measure_columns_host(4, 2, np.ones(6), np.ones((1, 5)), [1], [])


def test_exports_are_declared_and_present(capi):
    text = open(os.path.join(ROOT, "include", "eigenex_hip.h")).read()
    for name in ("eigenex_spin_measure_columns", "eigenex_spin_measure_columns_host"):
        assert re.search(r"\bint %s\s*\(" % name, text)
        assert hasattr(capi.lib(), name) and name in capi.SIGNATURES
    assert hasattr(capi.Basis, "spin_measure_columns")


def test_columns_host_code_under_sanitizers(tmp_path):
    """csrc/spin_measure_columns.hpp (range check, host evaluation) compiled into a stand-alone program with AddressSanitizer +
    UBSan: outputs into exactly-sized arrays, and the row loop of k_spin_measure_columns over its chunk tables and column chunks
    -- the kernel's own function (csrc/spin_rows.hpp: spin_measure_columns_row) with every load bounds-checked -- bit-identical
    to the host evaluation."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "spin_measure_columns_sanitize")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "spin_measure_columns_sanitize.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-1500:], out.stderr.decode()[-2000:])
    assert b"SPIN MEASURE COLUMNS OK" in out.stdout
