"""Momentum sectors of the spin-1/2 Hamiltonian on the host: the numpy restatement tests/spin_momentum_reference.py against itself
(these pass without the library's momentum code), eigenex_spin_momentum_dim / _states / _csr / _expand_host against it, the
refusals with their messages, and the host code and the kernels' row walk (csrc/spin_momentum.hpp, csrc/spin_rows.hpp) under
AddressSanitizer + UBSan in a stand-alone program.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
from math import comb, sqrt

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_momentum_reference as ref  # noqa: E402
import spin_momentum64_reference as ref64  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
RINGS = [(8, 1), (8, 2), (6, 3), (9, 1)]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g

    g.build()
    from cmpt_eigenex_amd import capi as c

    return c


def _model(L, cell):
    return (ref.xxz_ring(L, 1.0, 0.7), None) if cell == 1 else ref.cell_model(L, cell)


# ---- 1. the reference against itself ----
@pytest.mark.parametrize("L,cell", RINGS)
def test_reference_blocks_are_hermitian_and_tile_the_sector(L, cell):
    bonds, hz = _model(L, cell)
    N = L // cell
    for n_up in range(L + 1):
        Hs = ref.dense_sector(L, n_up, bonds, hz)
        levels, total = [], 0
        for m in range(N):
            Hk = ref.dense_block(L, n_up, cell, m, bonds, hz)
            total += Hk.shape[0]
            if Hk.shape[0]:
                assert np.abs(Hk - Hk.conj().T).max() <= 1e-13
                levels += list(np.linalg.eigvalsh(Hk))
        assert total == comb(L, n_up)
        assert np.abs(np.sort(levels) - np.linalg.eigvalsh(Hs)).max() <= 1e-12 * max(np.abs(Hs).sum(0).max(), 1.0)


# ---- 2. dim and states ----
@pytest.mark.parametrize("L,cell", RINGS + [(12, 1), (12, 2), (12, 3), (13, 1)])
def test_dim_states_and_periods_equal_the_reference(capi, L, cell):
    N = L // cell
    for n_up in range(L + 1):
        for m in range(N):
            want = ref.representatives(L, n_up, cell, m)
            if not want:
                with pytest.raises(capi.EigenexError, match="empty"):
                    capi.spin_momentum_dim(L, n_up, m, cell)
                continue
            assert capi.spin_momentum_dim(L, n_up, m, cell) == len(want)
            states, periods = capi.spin_momentum_states(L, n_up, m, cell)
            assert states.dtype == np.uint32 and periods.dtype == np.uint8
            assert states.tolist() == [s for s, _ in want] and periods.tolist() == [p for _, p in want]
            a, b = len(want) // 3, len(want) - len(want) // 4  # a window of rows
            st, pr = capi.spin_momentum_states(L, n_up, m, cell, a, b - a)
            assert st.tolist() == [s for s, _ in want[a:b]] and pr.tolist() == [p for _, p in want[a:b]]


def test_dimensions_of_larger_sectors(capi):
    assert [capi.spin_momentum_dim(16, 8, m) for m in (0, 8, 1)] == [810, 810, 800]
    assert all(capi.spin_momentum_dim(32, 3, m) == 155 for m in range(32))
    assert all(capi.spin_momentum_dim(32, 31, m) == 1 for m in range(32))
    assert all(capi.spin_momentum_dim(31, 2, m) == 15 for m in range(31))  # N = 31 is odd: there is no N/2
    assert capi.spin_momentum_dim(6, 0, 0) == 1 and capi.spin_momentum_dim(6, 6, 0) == 1
    with pytest.raises(capi.EigenexError, match="eigenex_spin_momentum_dim: the sector is empty"):
        capi.spin_momentum_dim(6, 0, 1)
    states, periods = capi.spin_momentum_states(32, 31, 5)
    assert states.tolist() == [0x7FFFFFFF] and periods.tolist() == [32]  # bit 31 rotates into bit 0


@pytest.mark.parametrize("L,n_up,cell", [(20, 5, 1), (22, 4, 2)])
def test_chunked_enumeration_equals_the_pure_python_reference(capi, L, n_up, cell):
    """From 20 sites the rows come from 2^16 pruned prefixes on several threads: the list and the periods must be those of
    tests/spin_momentum64_reference.py, which walks the necklaces in pure Python and shares nothing with the C code."""
    N = L // cell
    for m in (0, 1, N // 2):
        want = ref64.representatives(L, n_up, cell, m)
        if not want:
            with pytest.raises(capi.EigenexError, match="empty"):
                capi.spin_momentum_dim(L, n_up, m, cell)
            continue
        assert capi.spin_momentum_dim(L, n_up, m, cell) == len(want)
        states, periods = capi.spin_momentum_states(L, n_up, m, cell)
        assert states.dtype == np.uint32 and states.tolist() == [s for s, _ in want] and periods.tolist() == [p for _, p in want]


# ---- 3. the rows ----
def _entry_bounds(L, n_up, cell, m, bonds):
    """B[r, c]: the bound of |library - reference| on the summed entry, from the roundings of value = ((jxy * 0.5) * ratio) * phase
    on both sides.  jxy * 0.5 is exact.  ratio = sqrt(p / q): the division's u = eps / 2 halves under the root, then the root's own
    u; the product with it u: c is within 2.5 u.  phase: the angle 2 pi q / N carries three roundings (the constant, a product, a
    quotient), 3 u of at most 2 pi or 19 u absolute, which cos and sin pass on at most one to one, and their own rounding is u: 20 u.
    The last product u.  One side: (3.5 + 20) u |c|; two sides 47 u = 23.5 eps: K = 24 in units of eps |jxy| / 2 ratio.  The sum
    of duplicates is rounded once per addition on either side: eps |sum|, added by the caller."""
    N = L // cell
    reps = ref.representatives(L, n_up, cell, m)
    index = {s: r for r, (s, _) in enumerate(reps)}
    B = np.zeros((len(reps), len(reps)))
    for r, (a, ra) in enumerate(reps):
        for i, j, _, jxy in bonds:
            if jxy != 0.0 and ((a >> i) ^ (a >> j)) & 1:
                rep, _, rs = ref.orbit(a ^ (1 << i | 1 << j), L, cell)
                if (m * rs) % N == 0:
                    B[r, index[rep]] += 24 * EPS * abs(jxy) / 2 * sqrt(ra / rs)
    return B


@pytest.mark.parametrize("L,n_up,cell", [(8, 4, 1), (8, 3, 2), (6, 3, 3), (9, 4, 1), (12, 6, 2), (12, 4, 3), (4, 2, 1), (2, 1, 1)])
def test_rows_equal_the_dense_reference(capi, L, n_up, cell):
    bonds, hz = _model(L, cell)
    N = L // cell
    sp, sc, sv = capi.spin_sector_csr(L, n_up, bonds, hz)
    sector_states = capi.spin_sector_states(L, n_up)
    for m in range(N):
        reps = ref.representatives(L, n_up, cell, m)
        if not reps:
            continue
        n = len(reps)
        rowptr, col, val = capi.spin_momentum_csr(L, n_up, m, bonds, hz, cell)
        assert rowptr.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.complex128 and rowptr[-1] == col.size == val.size
        # the diagonal: first in its row, and the bits of the sector CSR's diagonal of the representative's row
        assert np.array_equal(col[rowptr[:-1]], np.arange(n))
        ranks = np.searchsorted(sector_states, np.array([s for s, _ in reps], np.uint32))
        assert val[rowptr[:-1]].real.tobytes() == sv[sp[:-1][ranks]].tobytes() and not val[rowptr[:-1]].imag.any()
        # entry by entry after summing duplicates, in stored order
        H = np.zeros((n, n), np.complex128)
        for r in range(n):
            for p in range(rowptr[r], rowptr[r + 1]):
                H[r, col[p]] += val[p]
        want = ref.dense_block(L, n_up, cell, m, bonds, hz)
        bound = _entry_bounds(L, n_up, cell, m, bonds) + EPS * np.abs(want) * len(bonds)
        worst = (np.abs(H - want) - bound).max()
        print(f"({L},{n_up},{cell}) m={m}: largest error {np.abs(H - want).max():.3e}, largest bound {bound.max():.3e}")
        assert worst <= 0.0
        if m == 0 or 2 * m == N:
            assert not val.imag.any() and not np.signbit(val.imag).any()
        # a range of rows from the middle; counting alone
        a, b = n // 3, n - n // 4
        rp, cl, vl = capi.spin_momentum_csr(L, n_up, m, bonds, hz, cell, row_begin=a, n_rows=b - a)
        assert np.array_equal(rp, rowptr[a : b + 1] - rowptr[a]) and np.array_equal(cl, col[rowptr[a] : rowptr[b]])
        assert vl.tobytes() == val[rowptr[a] : rowptr[b]].tobytes()
        keep, args = capi._spin_model(L, bonds, hz, None)
        margs = capi._momentum_args(args, n_up, cell, m)
        only, nnz = np.zeros(n + 1, np.int64), C.c_int64()
        assert capi.lib().eigenex_spin_momentum_csr(*margs, 0, n, only.ctypes.data_as(C.POINTER(C.c_int64)), None, None, C.byref(nnz)) == 0
        assert nnz.value == col.size and np.array_equal(only, rowptr)


# ---- 4. expand ----
@pytest.mark.parametrize("L,n_up,cell", [(8, 4, 1), (12, 6, 2)])
def test_expand_host_preserves_the_norm_and_intertwines(capi, L, n_up, cell):
    """H_sector expand(x) = expand(H_k x).  Either side is a product with at most n_bonds + 1 terms per row, each term rounded and
    added, behind or before an expand of four roundings: (n_bonds + 8) eps sum |H_rc| |x_c| per side.  |expand(x)_r| <= max |x|, a
    row of |H_sector| sums to at most |H|_1 and one of |H_k| to at most sqrt(N) |H|_1 (the ratios): 2 (n_bonds + 8) eps sqrt(N)
    |H|_1 max |x|."""
    bonds, hz = _model(L, cell)
    N = L // cell
    Hs = ref.dense_sector(L, n_up, bonds, hz)
    H1 = np.abs(Hs).sum(0).max()
    rs = np.random.RandomState(L + cell)
    for m in range(N):
        n = capi.spin_momentum_dim(L, n_up, m, cell)
        Hk = ref.dense_block(L, n_up, cell, m, bonds, hz)
        x = rs.standard_normal(n) + 1j * rs.standard_normal(n)
        y = capi.spin_momentum_expand_host(L, n_up, m, x, cell)
        assert y.dtype == np.complex128 and y.size == comb(L, n_up)
        # four roundings per entry, and the two sums of len(y) terms
        assert abs(np.vdot(y, y).real - np.vdot(x, x).real) <= (8 + len(y)) * EPS * np.vdot(x, x).real
        assert np.abs(y - ref.expand(L, n_up, cell, m, x)).max() <= 24 * EPS * np.abs(x).max()
        tol = 2 * (len(bonds) + 8) * EPS * sqrt(N) * H1 * np.abs(x).max()
        err = np.abs(Hs @ y - capi.spin_momentum_expand_host(L, n_up, m, Hk @ x, cell)).max()
        print(f"({L},{n_up},{cell}) m={m}: intertwining error {err:.3e}, bound {tol:.3e}")
        assert err <= tol
        if m == 0 or 2 * m == N:
            xr = np.ascontiguousarray(x.real)
            yr = capi.spin_momentum_expand_host(L, n_up, m, xr, cell)
            assert yr.dtype == np.float64
            if m == 0:  # the complex form on a real x: the real form's bytes in the real parts, +0 elsewhere
                yz = capi.spin_momentum_expand_host(L, n_up, m, xr.astype(np.complex128), cell)
                assert np.ascontiguousarray(yz.real).tobytes() == yr.tobytes()
                assert not yz.imag.any() and not np.signbit(yz.imag).any()
        else:
            with pytest.raises(capi.EigenexError, match="real momentum"):
                capi.spin_momentum_expand_host(L, n_up, m, np.ones(n), cell)


# ---- 5. refusals ----
def test_refusals_and_their_messages(capi):
    L, n_up = 8, 4
    ring = ref.xxz_ring(L, 1.0, 0.7)
    with pytest.raises(capi.EigenexError, match=r"eigenex_spin_momentum_csr: .*not invariant.*bond 6 \(sites 6, 7\)"):
        capi.spin_momentum_csr(L, n_up, 0, ring[:-1])  # a chain with open ends: bond (6,7) has no image (7,0)
    altered = list(ring)
    altered[3] = (3, 4, 1.0, 0.7000000000000001)
    with pytest.raises(capi.EigenexError, match=r"not invariant.*bond 2 \(sites 2, 3\)"):
        capi.spin_momentum_csr(L, n_up, 0, altered)  # one altered coupling, by one bit
    with pytest.raises(capi.EigenexError, match=r"not invariant.*hz at site 3 differs from hz at site 5"):
        capi.spin_momentum_csr(L, n_up, 0, ring, hz=[0.1, 0.2, 0.1, 0.2, 0.1, 0.5, 0.1, 0.2], cell=2)
    assert capi.spin_momentum_csr(L, n_up, 0, ring, hz=[0.1, 0.2] * 4, cell=2)[0].size > 1
    with pytest.raises(capi.EigenexError, match="cell must be at least 1 and divide n_sites"):
        capi.spin_momentum_dim(L, n_up, 0, cell=3)
    with pytest.raises(capi.EigenexError, match="cell must be at most n_sites / 2"):
        capi.spin_momentum_dim(L, n_up, 0, cell=8)
    for m in (-1, 8):
        with pytest.raises(capi.EigenexError, match="momentum must be 0..n_sites/cell - 1"):
            capi.spin_momentum_dim(L, n_up, m)
    with pytest.raises(capi.EigenexError, match="momentum must be"):
        capi.spin_momentum_states(L, n_up, 4, cell=2)  # N = 4
    with pytest.raises(capi.EigenexError, match="eigenex_spin_momentum_states: the sector is empty"):
        capi.spin_momentum_states(6, 0, 1, count=1)
    with pytest.raises(capi.EigenexError, match="eigenex_spin_momentum_csr: the sector is empty"):
        capi.spin_momentum_csr(6, 0, 1, ref.xxz_ring(6))
    with pytest.raises(capi.EigenexError, match="n_sites must be 2..32"):
        capi.spin_momentum_dim(33, 3, 0)
    with pytest.raises(capi.EigenexError, match="n_up must be"):
        capi.spin_momentum_dim(8, 9, 0)
    with pytest.raises(capi.EigenexError, match="rows outside"):
        capi.spin_momentum_csr(L, n_up, 0, ring, row_begin=3, n_rows=100)
    # the uploads check everything before they look at the context: the same refusals without a GPU, with a NULL context
    with pytest.raises(capi.EigenexError, match="eigenex_spin_momentum_upload: real states take a real momentum only"):
        capi.Csr.spin_half_momentum(None, L, n_up, 1, ring)
    with pytest.raises(capi.EigenexError, match="eigenex_spin_momentum_upload_z: .*not invariant"):
        capi.Csr.spin_half_momentum(None, L, n_up, 1, ring[:-1], complex_states=True)
    with pytest.raises(capi.EigenexError, match="eigenex_spin_momentum_upload_z: NULL argument"):
        capi.Csr.spin_half_momentum(None, L, n_up, 1, ring, complex_states=True)


# ---- 6. the sanitizer program ----
def test_momentum_host_code_under_sanitizers(tmp_path):
    """csrc/spin_momentum.hpp on 32-bit states (checks, threaded enumeration, buckets, tables, rows, expand, measure) and the
    momentum walk of csrc/spin_rows.hpp -- the functions k_spin_momentum_spmv<E>, k_spin_momentum_measure<E, uint32_t> and
    k_spin_momentum_expand<E> call -- compiled into a stand-alone program with AddressSanitizer + UBSan: every load bounds-checked,
    the enumeration compared with the plain walk, each row's sum bitwise with the sum over the stored entries, the expand walk
    bitwise with spin_momentum_expand_host; 19, 20, 22 and 32 sites among the shapes."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "spin_momentum_sanitize")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "spin_momentum_sanitize.cpp"),
                           "-o", exe])
    out = subprocess.run([exe, "32"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-1500:], out.stderr.decode()[-2000:])
    assert b"SPIN MOMENTUM OK" in out.stdout


# ---- 7. the header ----
def test_exports_are_declared_and_present(capi):
    text = open(os.path.join(ROOT, "include", "eigenex_hip.h")).read()
    for name in ("eigenex_spin_momentum_dim", "eigenex_spin_momentum_states", "eigenex_spin_momentum_csr", "eigenex_spin_momentum_upload",
                 "eigenex_spin_momentum_upload_z", "eigenex_spin_momentum_geometry", "eigenex_spin_momentum_expand", "eigenex_spin_momentum_expand_host"):
        assert re.search(r"\bint %s\s*\(" % name, text)
        assert hasattr(capi.lib(), name) and name in capi.SIGNATURES
    assert "EIGENEX_LAYOUT_MATRIX_FREE_SPIN_MOMENTUM = 7" in text
    assert "EIGENEX_LAYOUT_MATRIX_FREE_SPIN_SECTOR = 6" in text
