"""Site operators between momentum sectors, restated from the definition at the top of csrc/spin_momentum_site.hpp in numpy
longdouble, independent of the library and of that header: states are Python integers / uint64 arrays, a translation is two shifts,
every sum also carries the number of its terms and the sum of their moduli, from which the tests take their bounds.

  sector (L, n_up, cell, m): N = L // cell translations, T moves site i to site (i + cell) mod L, rows = the smallest states of the
  orbits whose period R has (m R) mod N == 0, ascending; |a(k)> = (sqrt(R_a) / N) sum_r e^{-ikr} T^r |a>, k = 2 pi m / N.
  operator (kind, cc, p): c[j + cell r] = cc[j] e^{+2 pi i p r / N}; O = sum_i c[i] S^kind_i; kind 0 Z, 1 PLUS, 2 MINUS.
  destination: n_up' = n_up, n_up + 1, n_up - 1; m' = (m - p) mod N.
"""
from __future__ import annotations

import itertools

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
Z, PLUS, MINUS = 0, 1, 2
PI = 4 * np.arctan(LD(1))


def unit(q: int, N: int):
    """e^{+2 pi i q / N} in longdouble, exact at quarter turns"""
    q %= N
    if (4 * q) % N == 0:
        return (CLD(1), CLD(1j), CLD(-1), CLD(-1j))[4 * q // N]
    a = 2 * PI * LD(q) / LD(N)
    return CLD(np.cos(a) + 1j * np.sin(a))


def destination(L: int, n_up: int, cell: int, m: int, kind: int, p: int):
    N = L // cell
    return n_up + (0, 1, -1)[kind], (m - p) % N


def site_coefficients(L: int, cell: int, p: int, cc):
    N = L // cell
    c = np.zeros(L, CLD)
    for r in range(N):
        for j in range(cell):
            c[j + cell * r] = CLD(cc[j]) * unit(p * r, N)
    return c


def sector_states(L: int, n_up: int):
    """the states with n_up of L sites up, ascending (uint64)"""
    s = np.fromiter((sum(1 << i for i in c) for c in itertools.combinations(range(L), n_up)), np.uint64)
    s.sort()
    return s


def orbits(states, L: int, cell: int):
    """(representative, j* = the smallest j >= 0 with T^j s = representative, period) of every state of the array"""
    states = np.asarray(states, np.uint64)
    mask = np.uint64((1 << L) - 1)
    rep, jstar, period = states.copy(), np.zeros(states.size, np.int64), np.zeros(states.size, np.int64)
    t = states.copy()
    for r in range(1, L // cell + 1):
        t = ((t << np.uint64(cell)) | (t >> np.uint64(L - cell))) & mask
        back = (t == states) & (period == 0)
        period[back] = r
        smaller = (t < rep) & (period == 0)  # before the orbit closes
        rep[smaller], jstar[smaller] = t[smaller], r
    return rep, jstar, period


_ROWS = {}


def rows(L: int, n_up: int, cell: int, m: int):
    """(representatives, periods) of the sector's rows, ascending; empty arrays for a sector without rows"""
    key = (L, n_up, cell)
    if key not in _ROWS:
        if not 0 <= n_up <= L:
            _ROWS[key] = (np.zeros(0, np.uint64), np.zeros(0, np.int64))
        else:
            s = sector_states(L, n_up)
            rep, _, period = orbits(s, L, cell)
            _ROWS[key] = (s[rep == s], period[rep == s])
    reps, period = _ROWS[key]
    ok = (m * period) % (L // cell) == 0
    return reps[ok], period[ok]


def _row_index(reps, states):
    """(index of each state in the ascending list reps, whether it is there)"""
    if reps.size == 0:
        return np.zeros(states.size, np.int64), np.zeros(states.size, bool)
    idx = np.minimum(np.searchsorted(reps, states), reps.size - 1)
    return idx, reps[idx] == states


def apply(L: int, n_up: int, cell: int, m: int, kind: int, cc, p: int, x):
    """(y, terms, moduli): y = O x over the rows of the destination sector in longdouble, the number of terms of each row and the
    sum of their moduli"""
    N = L // cell
    up2, m2 = destination(L, n_up, cell, m, kind, p)
    src, _ = rows(L, n_up, cell, m)
    dst, Rb = rows(L, up2, cell, m2)
    c = site_coefficients(L, cell, p, cc)
    x = np.asarray(x).astype(CLD)
    y, terms, moduli = np.zeros(dst.size, CLD), np.zeros(dst.size, np.int64), np.zeros(dst.size, LD)
    src_phase = np.array([np.conj(unit(m * l, N)) for l in range(N)], CLD)  # phase[l] = e^{-2 pi i m l / N}
    for i in range(L):
        bit = np.uint64(1 << i)
        up = (dst & bit) != 0
        if kind == Z:
            idx, there = _row_index(src, dst)
            live = there & ((m * Rb) % N == 0)
            term = np.where(up, c[i] / 2, -c[i] / 2) * x[idx]
        else:
            has = up if kind == PLUS else ~up
            rep, jstar, period = orbits(dst ^ bit, L, cell)
            idx, there = _row_index(src, rep)
            live = has & ((m * period) % N == 0)
            assert np.all(there[live])  # a compatible representative of the source's magnetisation is a row of the source
            term = c[i] * np.sqrt(Rb.astype(LD) / period.astype(LD)) * src_phase[(N - jstar) % N] * x[idx]
        term = np.where(live, term, CLD(0))
        y += term
        terms += live
        moduli += np.abs(term)
    return y, terms, moduli


def expand(L: int, n_up: int, cell: int, m: int, x):
    """the Sz-sector vector of the momentum vector x, in longdouble: psi(s) = x[idx(rep s)] e^{-2 pi i m ((N - j*) mod N) / N} / sqrt(R)"""
    N = L // cell
    reps, _ = rows(L, n_up, cell, m)
    s = sector_states(L, n_up)
    rep, jstar, period = orbits(s, L, cell)
    idx, there = _row_index(reps, rep)
    ph = np.array([np.conj(unit(m * l, N)) for l in range(N)], CLD)
    return np.where(there, np.asarray(x).astype(CLD)[idx] * ph[(N - jstar) % N] / np.sqrt(period.astype(LD)), CLD(0))


def apply_sites_in_sector(L: int, n_up: int, kind: int, c, psi):
    """(phi, terms, moduli) of phi = sum_i c[i] S^kind_i psi over the states of the destination Sz sector, in longdouble.  Z has
    L terms per state, +-c[i]/2 psi(s)."""
    up2 = n_up + (0, 1, -1)[kind]
    src, dst = sector_states(L, n_up), sector_states(L, up2)
    psi = np.asarray(psi).astype(CLD)
    phi, terms, moduli = np.zeros(dst.size, CLD), np.zeros(dst.size, np.int64), np.zeros(dst.size, LD)
    for i in range(L):
        bit = np.uint64(1 << i)
        up = (dst & bit) != 0
        if kind == Z:
            live, term = np.ones(dst.size, bool), np.where(up, CLD(c[i]) / 2, -CLD(c[i]) / 2) * psi
        else:
            live = up if kind == PLUS else ~up
            idx, there = _row_index(src, dst ^ bit)
            assert np.all(there[live])
            term = np.where(live, CLD(c[i]) * psi[idx], CLD(0))
        phi += term
        terms += live
        moduli += np.abs(term)
    return phi, terms, moduli
