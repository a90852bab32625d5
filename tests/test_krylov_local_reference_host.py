"""tests/krylov_local_reference.py on the host: the fp64 numpy recurrences pass the local check with room to spare, and every
single fault of the kind a matrix-free kernel could have fails it.  No GPU, no library.

Operators: the dense momentum blocks of tests/spin_momentum_reference.py at (12,6,1), (12,6,2), (16,8,1) and the two-row sectors
of (4,2,1); the full-space rows of tests/spin_reference.py ('fields', L = 8) and the sector rows of tests/spin_sector_reference.py
('fields', (10,5)).  Recurrences: one_sweep_reference.batched and one_sweep (real), krylov_local_reference.lanczos_fp64 (complex)
and arnoldi_fp64 with one and two Gram-Schmidt passes.

Measured (the worst ratio error / bound over recurrences and shifts): momentum blocks of 75 to 810 rows 5.6e-3, full space and
sector 2.4e-3, the two-row sectors 0.31 (an error of one or two units in the last place against a bound of about ten).
profiles/spin_krylov_passes.md has the figures per recurrence beside those of the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import krylov_local_reference as kl  # noqa: E402
import one_sweep_reference as osr  # noqa: E402
import spin_momentum_reference as mref  # noqa: E402
import spin_reference as sr  # noqa: E402
import spin_sector_reference as ssr  # noqa: E402

STEPS = 8
SHIFTS = (0.0, -0.37)
_BLOCKS = {}


def _momentum_rows(L, n_up, cell, m):
    key = (L, n_up, cell, m)
    if key not in _BLOCKS:
        bonds, hz = (mref.xxz_ring(L, 1.0, 0.7), None) if cell == 1 else mref.cell_model(L, cell)
        H = mref.dense_block(L, n_up, cell, m, bonds, hz)
        real = m == 0 or 2 * m == L // cell
        assert np.abs(H - H.conj().T).max() < 1e-15 and (not real or not H.imag.any())
        _BLOCKS[key] = kl.dense_to_csr(H.real.copy() if real else H)
    return _BLOCKS[key]


def _start(n, cplx, seed=3):
    rs = np.random.RandomState(seed)
    return rs.standard_normal(n) + 1j * rs.standard_normal(n) if cplx else rs.standard_normal(n)


def _run_all(rows, what):
    """every recurrence that fits the operator's scalar type, at both shifts; returns the worst ratio"""
    n = rows[0].size - 1
    cplx = np.iscomplexobj(rows[2])
    apply = kl.csr_matmul(rows)
    worst = 0.0
    for shift in SHIFTS:
        reports = []
        if not cplx:
            a, b, V = osr.batched(apply, _start(n, False), STEPS - 1, shift)
            reports.append(("batched", kl.check_lanczos(rows, shift, V, a, b)))
            a, b, V, _, _ = osr.one_sweep(apply, _start(n, False), STEPS - 1, shift)
            reports.append(("one_sweep", kl.check_lanczos(rows, shift, V, a, b)))
        a, b, V = kl.lanczos_fp64(apply, _start(n, True), STEPS - 1, shift)
        reports.append(("lanczos_z", kl.check_lanczos(rows, shift, V, a, b)))
        for passes in (1, 2):
            for z in ((False, True) if not cplx else (True,)):
                V, H, residue, w = kl.arnoldi_fp64(apply, _start(n, z), STEPS, shift, passes)
                reports.append((f"arnoldi{passes}{'_z' if z else ''}", kl.check_arnoldi(rows, shift, V, H, residue, w)))
        for name, rep in reports:
            print(rep.line(f"{what} n={n} shift={shift} {name}"))
            assert rep.ok(), rep.line(name)
            worst = max(worst, rep.ratio())
    return worst


@pytest.mark.parametrize("L,n_up,cell,m", [(12, 6, 1, 0), (12, 6, 1, 6), (12, 6, 1, 1), (12, 6, 1, 11), (12, 6, 2, 0), (12, 6, 2, 3), (12, 6, 2, 1),
                                           (16, 8, 1, 0), (16, 8, 1, 1)])
def test_fp64_recurrences_pass_on_momentum_blocks(L, n_up, cell, m):
    worst = _run_all(_momentum_rows(L, n_up, cell, m), f"({L},{n_up},{cell}) m={m}")
    print(f"({L},{n_up},{cell}) m={m}: worst ratio {worst:.3e}")


@pytest.mark.parametrize("m", [0, 2])
def test_fp64_recurrences_pass_on_the_two_row_sectors(m):
    """(4,2,1) at m = 0 and m = 2: two rows, every recurrence breaks down after two vectors; the steps before the stop pass"""
    rows = _momentum_rows(4, 2, 1, m)
    assert rows[0].size - 1 == 2
    worst = _run_all(rows, f"(4,2,1) m={m}")
    print(f"(4,2,1) m={m}: worst ratio {worst:.3e}")


def test_fp64_recurrences_pass_on_full_space_and_sector_rows():
    L, bonds, hz, hx = sr.models(8)["fields"]
    worst = _run_all(sr.rows_csr(L, bonds, hz, hx), "full space L=8 fields")
    L, bonds, hz, _ = sr.models(10)["fields"]
    worst = max(worst, _run_all(ssr.rows_csr(L, 5, bonds, hz), "sector (10,5) fields"))
    print(f"full space and sector: worst ratio {worst:.3e}")


# ---- single faults -------------------------------------------------------------------------------------------------------------
Z_ROWS = (12, 6, 1, 1)  # a complex momentum
SHIFT_Z = 0.3 - 0.2j


def _fails(rep, what):
    print(rep.line(what))
    assert not rep.ok(), what
    assert rep.worst() > 1e3 * rep["bound"], what  # far outside, not a near miss


def test_rejects_one_wrong_entry_of_one_column():
    for key, cplx in ((Z_ROWS, True), ((12, 6, 1, 0), False)):
        rows = _momentum_rows(*key)
        n = rows[0].size - 1
        apply = kl.csr_matmul(rows)
        a, b, V = kl.lanczos_fp64(apply, _start(n, cplx), STEPS - 1)
        assert kl.check_lanczos(rows, 0.0, V, a, b).ok()
        V[3, 5] += 1e-9
        _fails(kl.check_lanczos(rows, 0.0, V, a, b), "lanczos, entry 5 of column 3 off by 1e-9")
        U, H, residue, w = kl.arnoldi_fp64(apply, _start(n, cplx), STEPS)
        assert kl.check_arnoldi(rows, 0.0, U, H, residue, w).ok()
        U[STEPS - 1, n - 1] += 1e-9  # the newest column
        _fails(kl.check_arnoldi(rows, 0.0, U, H, residue, w), "arnoldi, the last entry of the newest column off by 1e-9")


def test_rejects_the_operator_applied_to_the_unnormalised_vector():
    """what a lane that reads xraw where it should read xr computes"""
    for key, cplx in ((Z_ROWS, True), ((12, 6, 1, 0), False)):
        rows = _momentum_rows(*key)
        n = rows[0].size - 1
        apply = kl.csr_matmul(rows)
        for shift in SHIFTS:
            a, b, V = kl.lanczos_fp64(apply, _start(n, cplx), STEPS - 1, shift, scaled_input=False)
            _fails(kl.check_lanczos(rows, shift, V, a, b), f"lanczos on the raw vector, shift {shift}")
            U, H, residue, w = kl.arnoldi_fp64(apply, _start(n, cplx), STEPS, shift, scaled_input=False)
            _fails(kl.check_arnoldi(rows, shift, U, H, residue, w), f"arnoldi on the raw vector, shift {shift}")


def test_rejects_a_dropped_imaginary_part_of_the_shift():
    rows = _momentum_rows(*Z_ROWS)
    n = rows[0].size - 1
    apply = kl.csr_matmul(rows)
    for passes in (1, 2):
        U, H, residue, w = kl.arnoldi_fp64(apply, _start(n, True), STEPS, SHIFT_Z, passes)
        assert kl.check_arnoldi(rows, SHIFT_Z, U, H, residue, w).ok()
        U, H, residue, w = kl.arnoldi_fp64(apply, _start(n, True), STEPS, SHIFT_Z.real, passes)
        _fails(kl.check_arnoldi(rows, SHIFT_Z, U, H, residue, w), f"arnoldi with {passes} passes, shift_im dropped")


def test_rejects_one_conjugated_value_at_a_complex_momentum():
    rowptr, col, val = _momentum_rows(*Z_ROWS)
    n = rowptr.size - 1
    e = int(np.argmax(np.abs(val.imag)))
    assert abs(val[e].imag) > 0.1
    bad = val.copy()
    bad[e] = np.conj(bad[e])
    apply = kl.csr_matmul((rowptr, col, bad))
    a, b, V = kl.lanczos_fp64(apply, _start(n, True), STEPS - 1)
    _fails(kl.check_lanczos((rowptr, col, val), 0.0, V, a, b), "lanczos, one value conjugated")
    U, H, residue, w = kl.arnoldi_fp64(apply, _start(n, True), STEPS)
    _fails(kl.check_arnoldi((rowptr, col, val), 0.0, U, H, residue, w), "arnoldi, one value conjugated")


def test_rejects_alpha_taken_as_the_norm_of_the_output():
    """what a stuck kPassSelfNorm would do: the partial sums of |hu|^2 where those of u^H hu belong"""
    for key, cplx in ((Z_ROWS, True), ((12, 6, 1, 0), False)):
        rows = _momentum_rows(*key)
        n = rows[0].size - 1
        a, b, V = kl.lanczos_fp64(kl.csr_matmul(rows), _start(n, cplx), STEPS - 1, alpha_of=lambda u, v: np.vdot(v, v).real)
        _fails(kl.check_lanczos(rows, 0.0, V, a, b), "lanczos, alpha = |hu|^2")


# ---- rows without entries -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_empty_rows_against_a_dense_product_in_longdouble(cplx):
    """empty first, last and interior rows (two of them adjacent), and an operator without any entry: applied(), csr_matmul() and
    norm1() against the dense product in long double; an empty row's result is shift u.  On rows that all have entries the
    results are those of np.add.reduceat over every row start, bit for bit (what the module computed before)."""
    rs = np.random.RandomState(23)
    n = 12
    T = np.clongdouble if cplx else np.longdouble
    A = rs.standard_normal((n, n)) + (1j * rs.standard_normal((n, n)) if cplx else 0.0)
    A[rs.uniform(size=(n, n)) < 0.5] = 0.0
    u = _start(n, cplx, 5)
    for empty in ([0], [n - 1], [4], [0, 5, 6, n - 1], list(range(n))):
        B = A.copy()
        B[empty] = 0.0
        keep = B != 0
        rowptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
        rows = (rowptr, np.nonzero(keep)[1].astype(np.int32), B[keep])
        assert all(rowptr[i] == rowptr[i + 1] for i in empty)
        scale = max(float(np.abs(B).sum(1).max()), 1.0) * float(np.abs(u).max())
        for shift in (0.0, -0.37) + ((SHIFT_Z,) if cplx else ()):
            want = B.astype(T) @ u.astype(T) + T(shift) * u.astype(T)
            got = kl.applied(rows, shift, u)
            assert got.shape == (n,) and got.dtype == T
            assert np.abs(got - want).max() <= 4 * n * float(np.finfo(np.longdouble).eps) * scale
            assert np.array_equal(got[empty], T(shift) * u[empty].astype(T))  # exactly shift u
        got64 = kl.csr_matmul(rows)(u)
        assert got64.shape == (n,) and not got64[empty].any()
        assert np.abs(got64 - B @ u).max() <= 4 * n * kl.EPS * scale
        assert kl.norm1(n, rows[1], rows[2]) == pytest.approx(float(np.abs(B).sum(0).max()), rel=1e-15, abs=0.0)
    full = kl.dense_to_csr(A)  # every diagonal entry stored: no row is empty
    prod = full[2].astype(T) * u.astype(T)[full[1]]
    assert np.array_equal(kl.applied(full, -0.37, u), np.add.reduceat(prod, full[0][:-1]) + T(-0.37) * u.astype(T))
    assert np.array_equal(kl.csr_matmul(full)(u), np.add.reduceat(full[2] * u[full[1]], full[0][:-1]))
