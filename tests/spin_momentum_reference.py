"""Momentum sectors of the spin-1/2 Hamiltonian, restated in numpy from the definition at the top of csrc/spin_momentum.hpp and
independent of the library: orbits by explicit rotation, dictionaries for the row index, dense H_k.

  bonds = [(i, j, Jz, Jxy), ...], hz = n_sites fields or None; cell divides L, N = L // cell translations, momentum m in 0..N-1.
  T moves site i to site (i + cell) mod L.  The rows of sector (L, n_up, cell, m) are the smallest states of the orbits whose
  period R satisfies (m R) mod N == 0, ascending.
"""
from __future__ import annotations

import itertools
import math

import numpy as np


def translate(s: int, L: int, cell: int) -> int:
    out = 0
    for i in range(L):
        if (s >> i) & 1:
            out |= 1 << ((i + cell) % L)
    return out


def orbit(s: int, L: int, cell: int):
    """(representative, j* = the smallest j >= 0 with T^j s = representative, period)"""
    states = [s]
    while True:
        t = translate(states[-1], L, cell)
        if t == s:
            break
        states.append(t)
    rep = min(states)
    return rep, states.index(rep), len(states)


def sector_states(L: int, n_up: int):
    return sorted(sum(1 << i for i in c) for c in itertools.combinations(range(L), n_up))


def representatives(L: int, n_up: int, cell: int, m: int):
    """[(state, period)] of the rows, ascending"""
    N = L // cell
    out = []
    for s in sector_states(L, n_up):
        rep, _, period = orbit(s, L, cell)
        if rep == s and (m * period) % N == 0:
            out.append((s, period))
    return out


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


def dense_block(L: int, n_up: int, cell: int, m: int, bonds, hz=None):
    """H_k as a dense complex matrix over the rows of representatives(), duplicates summed"""
    N = L // cell
    reps = representatives(L, n_up, cell, m)
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


def dense_sector(L: int, n_up: int, bonds, hz=None):
    """the Sz-sector matrix over sector_states(), real"""
    states = sector_states(L, n_up)
    index = {s: r for r, s in enumerate(states)}
    h = np.zeros((len(states), len(states)))
    for r, s in enumerate(states):
        h[r, r] += diagonal(s, L, bonds, hz)
        for i, j, _, jxy in bonds:
            if jxy != 0.0 and ((s >> i) ^ (s >> j)) & 1:
                h[r, index[s ^ (1 << i | 1 << j)]] += jxy * 0.5
    return h


def expand(L: int, n_up: int, cell: int, m: int, x):
    """the Sz-sector vector of the momentum vector x"""
    N = L // cell
    reps = representatives(L, n_up, cell, m)
    index = {s: r for r, (s, _) in enumerate(reps)}
    states = sector_states(L, n_up)
    y = np.zeros(len(states), np.complex128)
    for r, s in enumerate(states):
        rep, jstar, period = orbit(s, L, cell)
        if rep in index:
            y[r] = x[index[rep]] * phase(m, (N - jstar) % N, N) / math.sqrt(period)
    return y


def xxz_ring(L: int, jz: float = 1.0, jxy: float = 1.0, reach=(1,)):
    """the periodic ring with bonds (i, i + d) for d in reach (a ring of two sites has one bond)"""
    bonds = []
    for d in reach:
        for i in range(L):
            j = (i + d) % L
            if L == 2 and i == 1:
                continue
            bonds.append((i, j, jz / d, jxy / d))
    return bonds


def cell_model(L: int, cell: int):
    """a model that is invariant under the translation by `cell` sites and by no smaller one (cell >= 2): different couplings on the
    bonds of a cell, a further-neighbour bond of reach L // 2 - 1 or so that crosses the split between the two halves of the state
    word, and a cell-periodic hz"""
    bonds = []
    far = max(2, L // 2 - 1)
    for i in range(L):
        p = i % cell
        bonds.append((i, (i + 1) % L, 1.0 + 0.25 * p, 0.75 + 0.125 * p))
        bonds.append((i, (i + far) % L, 0.3 - 0.05 * p, 0.2 + 0.0625 * p))
    hz = [0.1 * (1 + (i % cell)) for i in range(L)]
    return bonds, hz
