"""numpy restatements of the fixed-magnetisation sector of the spin-1/2 Hamiltonian (include/eigenex_hip.h:
eigenex_spin_sector_*), independent of csrc/spin_sector.hpp: the states by enumeration, the rank by searchsorted, and the
sector rows as the rows of tests/spin_reference.py (rows_csr, the full-space definition) at the sector's states with every
column replaced by its rank.  Shared by tests/test_spin_sector_host.py and tests/test_gpu_spin_sector.py."""
from __future__ import annotations

import itertools
from math import comb

import numpy as np
import spin_reference as sr


def states(n_sites, n_up):
    """the states with n_up bits set among n_sites, ascending (uint64).  Up to 20 sites by a popcount over all 2^n_sites words,
    beyond that (the few-spin sectors of 31 and 32 sites) from the combinations of the up positions."""
    if n_sites <= 20:
        s = np.arange(1 << n_sites, dtype=np.uint64)
        pc = np.zeros(s.size, np.int64)
        for i in range(n_sites):
            pc += ((s >> np.uint64(i)) & np.uint64(1)).astype(np.int64)
        return s[pc == n_up]
    k = min(n_up, n_sites - n_up)
    assert comb(n_sites, k) <= 1 << 16, "enumeration by combinations is for the small sectors only"
    full = (1 << n_sites) - 1
    out = [sum(1 << p for p in pos) for pos in itertools.combinations(range(n_sites), k)]
    if k != n_up:  # the complement: n_up ups = k downs
        out = [full ^ w for w in out]
    return np.array(sorted(out), dtype=np.uint64)


def rank(sector_states, s):
    r = np.searchsorted(sector_states, s)
    assert np.all(sector_states[r] == s), "a state outside the sector"
    return r


def rows_csr(n_sites, n_up, bonds, hz=None):
    """(rowptr int64, col int32, val float64) of the sector; no transverse field"""
    st = states(n_sites, n_up)
    if n_sites <= 14:
        rp, cl, vl = sr.rows_csr(n_sites, bonds, hz, None)
        pieces = [(cl[rp[s] : rp[s + 1]], vl[rp[s] : rp[s + 1]]) for s in st.astype(np.int64)]
    else:  # row by row: the full space is too large to write down
        pieces = []
        for s in st.astype(np.int64):
            _, cl, vl = sr.rows_csr(n_sites, bonds, hz, None, row_begin=int(s), n_rows=1)
            pieces.append((cl, vl))
    rowptr = np.concatenate([[0], np.cumsum([c.size for c, _ in pieces])]).astype(np.int64)
    full_cols = np.concatenate([c for c, _ in pieces]).view(np.uint32).astype(np.uint64)  # bit 31 is a site, not a sign
    return rowptr, rank(st, full_cols).astype(np.int32), np.concatenate([v for _, v in pieces])


def dense(n_sites, n_up, bonds, hz=None):
    rowptr, col, val = rows_csr(n_sites, n_up, bonds, hz)
    return sr.dense_from_csr(rowptr.size - 1, rowptr, col, val)


def without_hx(model):
    n_sites, bonds, hz, _ = model
    return n_sites, bonds, hz
