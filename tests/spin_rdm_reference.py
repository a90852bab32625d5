"""numpy restatement of the reduced density matrix (include/eigenex_hip.h: eigenex_spin_rdm, eigenex_spin_rdm_host), written
from the definition at the top of csrc/spin_rdm.hpp and sharing no code with the library: its own enumeration of the words of
n bits with k set (ascending: their rank), its own deposit and its own rank (searchsorted over the sector's states).  M_k is
built explicitly in np.longdouble and rho_k = M_k M_k^T.  Shared by tests/test_spin_rdm_host.py and tests/test_gpu_spin_rdm.py.

The bound: |out - ref| <= n_b eps (|M_k| |M_k|^T) elementwise, n_b the number of b's of the block, eps = 2^-52 -- the rounding
of an n_b-term sum in any grouping, so it holds for every launch grid, slice count and tile size."""
from __future__ import annotations

from itertools import combinations
from math import comb, log

import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def words(n, k):
    """the n-bit words with k bits set, ascending (uint64): index = rank"""
    if k < 0 or k > n:
        return np.zeros(0, np.uint64)
    if n <= 22:  # by filtering every word; beyond that by choosing the set bits
        a = np.arange(1 << n, dtype=np.uint64)
        count = np.zeros(a.size, np.int64)
        for p in range(n):
            count += ((a >> np.uint64(p)) & np.uint64(1)).astype(np.int64)
        return a[count == k]
    return np.sort(np.array([sum(1 << p for p in c) for c in combinations(range(n), k)], np.uint64))


def deposit(w, mask):
    """bit j of every word of w goes to the j-th lowest set bit of mask"""
    w = np.asarray(w, np.uint64)
    s, j = np.zeros(w.shape, np.uint64), 0
    for p in range(32):
        if (mask >> p) & 1:
            s |= ((w >> np.uint64(j)) & np.uint64(1)) << np.uint64(p)
            j += 1
    return s


def rows(n_sites, n_up):
    return 1 << n_sites if n_up is None else comb(n_sites, n_up)


def geometry(n_sites, n_up, mask_a):
    """(nA, nB, mask_b, [k of every block])"""
    nA = bin(mask_a).count("1")
    nB = n_sites - nA
    mask_b = ((1 << n_sites) - 1) & ~mask_a
    ks = [0] if n_up is None else list(range(max(0, n_up - nB), min(nA, n_up) + 1))
    return nA, nB, mask_b, ks


def panels(n_sites, n_up, x, mask_a):
    """[(k, M_k)]: M_k[i, j] = x[row(dep_A(a_i) | dep_B(b_j))] in np.longdouble"""
    nA, nB, mask_b, ks = geometry(n_sites, n_up, mask_a)
    xl = np.asarray(x, np.float64).astype(LD)
    assert xl.size == rows(n_sites, n_up)
    sector = None if n_up is None else words(n_sites, n_up)
    out = []
    for k in ks:
        a = np.arange(1 << nA, dtype=np.uint64) if n_up is None else words(nA, k)
        b = np.arange(1 << nB, dtype=np.uint64) if n_up is None else words(nB, n_up - k)
        s = deposit(a, mask_a)[:, None] | deposit(b, mask_b)[None, :]
        if n_up is None:
            idx = s.astype(np.int64)
        else:
            idx = np.searchsorted(sector, s.ravel()).reshape(s.shape)
            assert np.array_equal(sector[idx], s)
        out.append((k, xl[idx]))
    return out


def rdm(n_sites, n_up, x, mask_a):
    """[(k, rho_k, bound_k)]: rho_k = M_k M_k^T and n_b eps |M_k| |M_k|^T, both np.longdouble"""
    out = []
    for k, M in panels(n_sites, n_up, x, mask_a):
        out.append((k, M @ M.T, M.shape[1] * EPS * (np.abs(M) @ np.abs(M).T)))
    return out


def check(label, got, ref):
    """assert got = [(k, ndarray)] equals ref = rdm(...) within its bound, entry by entry, and is symmetric bit for bit; prints the
    largest error over its bound"""
    assert [k for k, _ in got] == [k for k, _, _ in ref], label
    worst = 0.0
    for (k, g), (_, want, bound) in zip(got, ref):
        assert g.dtype == np.float64 and g.shape == want.shape, (label, k, g.shape, want.shape)
        assert g.tobytes() == np.ascontiguousarray(g.T).tobytes(), f"{label}: block {k} is not symmetric bit for bit"
        err = np.abs(g.astype(LD) - want)
        pos = bound > 0
        if pos.any():
            worst = max(worst, float((err[pos] / bound[pos]).max()))
        bad = err > bound
        assert not bad.any(), f"{label}: block {k}: {int(bad.sum())} entries off, the first at {tuple(np.argwhere(bad)[0])}: error {float(err[bad][0]):.3e} > bound {float(bound[bad][0]):.3e}"
    print(f"{label}: largest error / bound = {worst:.3e}")


def vector(n_sites, n_up, seed=None):
    return np.random.RandomState(2000 * n_sites + (91 if n_up is None else n_up) if seed is None else seed).standard_normal(rows(n_sites, n_up))


def spectrum(blocks):
    """all eigenvalues of the unit-trace rho from raw blocks [(k, array)], descending, clamped at 0 (np.float64)"""
    tr = sum(float(np.trace(np.asarray(b, np.float64))) for _, b in blocks)
    lam = np.concatenate([np.linalg.eigvalsh(np.asarray(b, np.float64) / tr) for _, b in blocks])
    return np.sort(np.maximum(lam, 0.0))[::-1]


def entropy(lam):
    lam = np.asarray(lam, np.float64)
    lam = lam[lam > 0]
    return float(-(lam * np.log(lam)).sum())


def entropy_tolerance(d, n_b):
    """|S - S'| <= d (-delta ln delta), delta = (n_b + d) eps: by Weyl an eigenvalue of the unit-trace rho moves by at most the
    Frobenius norm of the perturbation, n_b eps for the sums (Cauchy-Schwarz on the elementwise bound) plus d eps for the
    eigen-solver's backward error, and |x ln x - y ln y| <= -delta ln delta for |x - y| <= delta <= 1/2; d eigenvalues"""
    delta = (n_b + d) * float(EPS)
    assert delta <= 0.5
    return d * (-delta * log(delta))


def t_plus_e(d, complex_entries=False):
    """tridiag(1, 3 + 0.1 i, 1) + E, E = +-1e-9 (or +-1e-9 i) on every entry with |i - j| >= 2 (the signs from a fixed seed), brought
    to unit trace: a positive definite rho whose columns are tridiagonal up to 1e-9 of the sub-diagonal.  Shared by
    tests/test_small_eigen_hard_cases_host.py and the GPU tests of the entanglement spectrum."""
    T = np.diag(3.0 + 0.1 * np.arange(d)) + np.diag(np.ones(d - 1), 1) + np.diag(np.ones(d - 1), -1)
    low = 1e-9 * np.where(np.random.default_rng(100 + d).random((d, d)) < 0.5, -1.0, 1.0) * np.tril(np.ones((d, d)), -2)
    if complex_entries:
        low = 1j * low
    A = T + low + low.conj().T
    return A / np.trace(A).real


def t_plus_e_state(d, complex_entries=False):
    """psi[a + d e] = M[a, e] with M the Cholesky factor of t_plus_e(d): the state of 2 log2(d) sites whose reduced density matrix
    on the low log2(d) sites is M M^H = t_plus_e(d) up to rounding"""
    M = np.linalg.cholesky(t_plus_e(d, complex_entries))
    return np.ascontiguousarray(M.T).ravel()
