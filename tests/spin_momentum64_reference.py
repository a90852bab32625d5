"""Momentum sectors of the spin-1/2 Hamiltonian on rings of up to 48 sites, restated from the definition at the top of
csrc/spin_momentum.hpp with Python integers and independent of the library.  tests/spin_momentum_reference.py moves a state bit by
bit, which is too slow at 40 sites; here a translation is two shifts, T s = ((s << cell) | (s >> (L - cell))) & (2^L - 1).

  bonds = [(i, j, Jz, Jxy), ...], hz = n_sites fields or None; cell divides L, N = L // cell translations, momentum m in 0..N-1.
  The rows of sector (L, n_up, cell, m) are the smallest states of the orbits whose period R satisfies (m R) mod N == 0, ascending.
"""
from __future__ import annotations

import itertools
import math

import numpy as np


def translate(s: int, L: int, cell: int) -> int:
    return ((s << cell) | (s >> (L - cell))) & ((1 << L) - 1)


_ORBITS = {}


def orbit(s: int, L: int, cell: int):
    """(representative, j* = the smallest j >= 0 with T^j s = representative, period); remembered, since the blocks of all momenta
    of a sector ask for the same states"""
    key = (s, L, cell)
    if key not in _ORBITS:
        rep, jstar, t, r = s, 0, s, 0
        while True:
            t = translate(t, L, cell)
            r += 1
            if t == s:
                break
            if t < rep:
                rep, jstar = t, r
        _ORBITS[key] = (rep, jstar, r)
    return _ORBITS[key]


def representatives(L: int, n_up: int, cell: int, m: int):
    """[(state, period)] of the rows, ascending"""
    N = L // cell
    out = []
    for c in itertools.combinations(range(L), n_up):
        s = sum(1 << i for i in c)
        t, r = s, 0
        while True:
            t = translate(t, L, cell)
            r += 1
            if t <= s:
                break
        if t == s and (m * r) % N == 0:
            out.append((s, r))
    out.sort()
    return out


def necklace_count(L: int, n_up: int) -> int:
    """the number of orbits of the translation by one site among the states with n_up sites up (the rows at m = 0)"""
    g = math.gcd(L, n_up)
    total = 0
    for d in range(1, g + 1):
        if g % d == 0:
            phi = sum(1 for k in range(1, d + 1) if math.gcd(k, d) == 1)
            total += phi * math.comb(L // d, n_up // d)
    return total // L


def phase(m: int, l: int, N: int) -> complex:
    q = (m * l) % N
    if (4 * q) % N == 0:
        return (1.0 + 0j, -1j, -1.0 + 0j, 1j)[4 * q // N]
    return complex(math.cos(2.0 * math.pi * q / N), -math.sin(2.0 * math.pi * q / N))


def diagonal(s: int, L: int, bonds, hz) -> float:
    d = 0.0
    for i, j, jz, _ in bonds:
        d += -jz * 0.25 if ((s >> i) ^ (s >> j)) & 1 else jz * 0.25
    if hz is not None:
        for i in range(L):
            d += hz[i] * 0.5 if (s >> i) & 1 else -(hz[i] * 0.5)
    return d


def dense_block(L: int, n_up: int, cell: int, m: int, bonds, hz=None, reps=None):
    """H_k as a dense complex matrix over the rows of representatives(), duplicates summed"""
    N = L // cell
    reps = representatives(L, n_up, cell, m) if reps is None else reps
    index = {s: r for r, (s, _) in enumerate(reps)}
    h = np.zeros((len(reps), len(reps)), np.complex128)
    for r, (a, ra) in enumerate(reps):
        h[r, r] += diagonal(a, L, bonds, hz)
        for i, j, _, jxy in bonds:
            if jxy != 0.0 and ((a >> i) ^ (a >> j)) & 1:
                rep, jstar, rs = orbit(a ^ (1 << i | 1 << j), L, cell)
                if (m * rs) % N != 0:
                    continue
                h[r, index[rep]] += (jxy * 0.5) * math.sqrt(ra / rs) * phase(m, (N - jstar) % N, N)
    return h


def block_entries(L: int, n_up: int, cell: int, m: int, bonds, hz=None, reps=None):
    """the non-zero entries of H_k as {(row, column): value}, duplicates summed, and {(row, column): bound} with the per-entry
    bound of entry_bounds -- for blocks that are too large to hold densely three times over"""
    N = L // cell
    eps = np.finfo(np.float64).eps
    reps = representatives(L, n_up, cell, m) if reps is None else reps
    index = {s: r for r, (s, _) in enumerate(reps)}
    h, bound = {}, {}
    for r, (a, ra) in enumerate(reps):
        h[(r, r)] = h.get((r, r), 0.0) + diagonal(a, L, bonds, hz)
        for i, j, _, jxy in bonds:
            if jxy != 0.0 and ((a >> i) ^ (a >> j)) & 1:
                rep, jstar, rs = orbit(a ^ (1 << i | 1 << j), L, cell)
                if (m * rs) % N != 0:
                    continue
                key = (r, index[rep])
                h[key] = h.get(key, 0.0) + (jxy * 0.5) * math.sqrt(ra / rs) * phase(m, (N - jstar) % N, N)
                bound[key] = bound.get(key, 0.0) + 24 * eps * abs(jxy) / 2 * math.sqrt(ra / rs)
    return h, bound


def entry_bounds(L: int, n_up: int, cell: int, m: int, bonds, reps=None):
    """the per-entry bound of |library - reference| that tests/test_spin_momentum_host.py derives (_entry_bounds): 24 eps |jxy| / 2
    ratio per stored term; the caller adds eps |sum| per addition of duplicates"""
    N = L // cell
    eps = np.finfo(np.float64).eps
    reps = representatives(L, n_up, cell, m) if reps is None else reps
    index = {s: r for r, (s, _) in enumerate(reps)}
    B = np.zeros((len(reps), len(reps)))
    for r, (a, ra) in enumerate(reps):
        for i, j, _, jxy in bonds:
            if jxy != 0.0 and ((a >> i) ^ (a >> j)) & 1:
                rep, _, rs = orbit(a ^ (1 << i | 1 << j), L, cell)
                if (m * rs) % N == 0:
                    B[r, index[rep]] += 24 * eps * abs(jxy) / 2 * math.sqrt(ra / rs)
    return B


def orbit_sums(reps, L: int, cell: int, masks):
    """c[t][a] = sum over the N rotations T^r a of prod_{i in mask_t} sigma_i, sigma = +1 for an up site and -1 for a down one"""
    N = L // cell
    out = np.zeros((len(masks), len(reps)), np.int64)
    for a, (s, _) in enumerate(reps):
        t = s
        for _r in range(N):
            for k, mask in enumerate(masks):
                out[k, a] += -1 if bin(~t & mask).count("1") & 1 else 1
            t = translate(t, L, cell)
    return out


def measure(reps, L: int, cell: int, masks, x):
    """(diag, norm2) of eigenex_spin_momentum_measure in extended precision (math.fsum)"""
    w = [abs(complex(v)) ** 2 for v in x]
    c = orbit_sums(reps, L, cell, masks)
    return np.array([math.fsum(float(c[k, a]) * w[a] for a in range(len(reps))) for k in range(len(masks))]), math.fsum(w)


def xxz_ring(L: int, jz: float = 1.0, jxy: float = 1.0, reach=(1,)):
    """the periodic ring with bonds (i, i + d) for d in reach; couplings divided by d (a J1-J2 ring for reach (1, 2))"""
    bonds = []
    for d in reach:
        for i in range(L):
            bonds.append((i, (i + d) % L, jz / d, jxy / d))
    return bonds


def cell_model(L: int, cell: int):
    """a model that is invariant under the translation by `cell` sites and by no smaller one (cell >= 2), with a bond that crosses
    bit 32 of the state word and a cell-periodic hz"""
    bonds = []
    far = max(2, L // 2 - 1)
    for i in range(L):
        p = i % cell
        bonds.append((i, (i + 1) % L, 1.0 + 0.25 * p, 0.75 + 0.125 * p))
        bonds.append((i, (i + far) % L, 0.3 - 0.05 * p, 0.2 + 0.0625 * p))
    hz = [0.1 * (1 + (i % cell)) for i in range(L)]
    return bonds, hz
