"""numpy restatements of the spin-1/2 Hamiltonian of eigenex_spin_csr / eigenex_spin_upload (include/eigenex_hip.h), two of
them and independent of each other: the row definition (the stored order, one rounded operation at a time) and the dense
matrix from Kronecker products of Sz, S+, S-, Sx.  Also the models the tests run.  Shared by tests/test_spin_host.py and
tests/test_gpu_spin_operator.py.

A model is (n_sites, bonds, hz, hx): bonds = [(i, j, Jz, Jxy), ...], hz / hx = arrays of n_sites fields or None."""
from __future__ import annotations

import numpy as np


def rows_csr(n_sites, bonds, hz=None, hx=None, row_begin=0, n_rows=None):
    """Row s: the diagonal (always stored), d = 0.0, for b ascending d += +-(Jz_b * 0.25) (+ where the two spins are equal),
    for i ascending d += +-(hz_i * 0.5) (+ where site i is up); then for b ascending with Jxy_b != 0 and different spins the
    entry (s ^ (1<<i | 1<<j), Jxy_b * 0.5); then for i ascending with hx_i != 0 the entry (s ^ (1<<i), hx_i * 0.5).
    Vectorised over the rows; every addition is one float64 addition, in that order."""
    n = 1 << n_sites
    if n_rows is None:
        n_rows = n - row_begin
    s = np.arange(row_begin, row_begin + n_rows, dtype=np.int64)
    up = lambda i: (s >> i) & 1  # noqa: E731
    d = np.zeros(n_rows, np.float64)
    for (i, j, jz, _) in bonds:
        c = np.float64(jz) * 0.25
        d = d + np.where(up(i) == up(j), c, -c)
    if hz is not None:
        for i in range(n_sites):
            c = np.float64(hz[i]) * 0.5
            d = d + np.where(up(i) == 1, c, -c)
    cols, vals, present = [s], [d], [np.ones(n_rows, bool)]
    for (i, j, _, jxy) in bonds:
        if jxy != 0.0:
            cols.append(s ^ ((1 << i) | (1 << j)))
            vals.append(np.full(n_rows, np.float64(jxy) * 0.5))
            present.append(up(i) != up(j))
    if hx is not None:
        for i in range(n_sites):
            if hx[i] != 0.0:
                cols.append(s ^ (1 << i))
                vals.append(np.full(n_rows, np.float64(hx[i]) * 0.5))
                present.append(np.ones(n_rows, bool))
    cols, vals, present = np.stack(cols, 1), np.stack(vals, 1), np.stack(present, 1)
    rowptr = np.concatenate([[0], np.cumsum(present.sum(1))]).astype(np.int64)
    return rowptr, cols[present].astype(np.int32), vals[present]


def dense_from_csr(n, rowptr, col, val):
    H = np.zeros((n, n))
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    np.add.at(H, (rows, col), val)
    return H


_SZ = np.array([[-0.5, 0.0], [0.0, 0.5]])  # index 0 = down (bit clear), 1 = up
_SP = np.array([[0.0, 0.0], [1.0, 0.0]])   # S+ |down> = |up>
_SM = _SP.T.copy()
_SX = 0.5 * (_SP + _SM)
_ID = np.eye(2)


def _site_operator(n_sites, ops):
    """kron over the sites with ops = {site: 2x2}; site 0 is the LOWEST bit of the state index, i.e. the last Kronecker factor"""
    out = np.eye(1)
    for site in range(n_sites - 1, -1, -1):
        out = np.kron(out, ops.get(site, _ID))
    return out


def dense_kron(n_sites, bonds, hz=None, hx=None):
    n = 1 << n_sites
    H = np.zeros((n, n))
    for (i, j, jz, jxy) in bonds:
        H += jz * _site_operator(n_sites, {i: _SZ, j: _SZ})
        H += 0.5 * jxy * (_site_operator(n_sites, {i: _SP, j: _SM}) + _site_operator(n_sites, {i: _SM, j: _SP}))
    for i in range(n_sites):
        if hz is not None:
            H += hz[i] * _site_operator(n_sites, {i: _SZ})
        if hx is not None:
            H += hx[i] * _site_operator(n_sites, {i: _SX})
    return H


def chain(L, jz=1.0, jxy=1.0, periodic=False):
    bonds = [(i, i + 1, jz, jxy) for i in range(L - 1)]
    if periodic and L > 2:
        bonds.append((L - 1, 0, jz, jxy))
    return bonds


def random_bonds(L, count, seed):
    """`count` random bonds with random couplings, every fifth Jz and every third Jxy zero, bond 1 a repeat of the pair of bond 0"""
    rng = np.random.RandomState(seed)
    bonds = []
    for b in range(count):
        i = int(rng.randint(L))
        j = int((i + 1 + rng.randint(L - 1)) % L)
        bonds.append((i, j, 0.0 if b % 5 == 4 else float(rng.standard_normal()), 0.0 if b % 3 == 2 else float(rng.standard_normal())))
    if count > 1:
        bonds[1] = (bonds[0][1], bonds[0][0], bonds[1][2], bonds[1][3] or 0.75)
    return bonds


def models(L):
    """name -> (n_sites, bonds, hz, hx): the models of the issue's CPU test, at L sites"""
    rng = np.random.RandomState(100 + L)
    hz, hx = rng.standard_normal(L), rng.standard_normal(L)
    hx_some = np.where(np.arange(L) % 2 == 0, hx, 0.0)
    return {
        "open": (L, chain(L), None, None),
        "periodic": (L, chain(L, 1.0, 0.7, periodic=True), None, None),
        "random40": (L, random_bonds(L, 40, L), None, None),
        "fields": (L, chain(L, 0.8, 1.1), hz, hx_some),
        "random40_fields": (L, random_bonds(L, 40, 7 * L), hz, hx),
        "ising": (L, [(i, j, jz, 0.0) for (i, j, jz, _) in random_bonds(L, 12, 3 * L)], hz, None),
    }
