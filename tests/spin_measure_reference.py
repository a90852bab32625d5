"""numpy restatement of the spin measurement (include/eigenex_hip.h: eigenex_spin_measure, eigenex_spin_measure_host),
independent of csrc/spin_measure.hpp: every sum and the sum of its terms' magnitudes in np.longdouble, the sector's states by
enumeration and the rank by searchsorted (tests/spin_sector_reference.py).  Also the term lists the tests run, the rounding
bound they share and the physical quantities that follow from the raw sums.  Shared by tests/test_spin_measure_host.py and
tests/test_gpu_spin_measure.py.

The bound: |out - ref| <= n eps sum_s |term_s|, n the number of rows, eps = 2^-52 -- the rounding of an n-term sum in any
grouping, the bound the spin tests use for partial dots."""
from __future__ import annotations

from math import comb

import numpy as np
import spin_sector_reference as ss

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def rows(n_sites, n_up):
    return 1 << n_sites if n_up is None else comb(n_sites, n_up)


def states(n_sites, n_up):
    """the state of every row, ascending (uint64)"""
    return np.arange(1 << n_sites, dtype=np.uint64) if n_up is None else ss.states(n_sites, n_up)


def _sigma_product(s, mask):
    """prod over the sites of the mask of sigma_i(s) = +1 (bit i set: up) or -1"""
    p = np.ones(s.size, np.int64)
    for i in range(32):
        if (mask >> i) & 1:
            p *= 2 * ((s >> np.uint64(i)) & np.uint64(1)).astype(np.int64) - 1
    return p


def measure(n_sites, n_up, x, diag_masks, flip_masks):
    """(diag, flip, norm2) and the sums of magnitudes (diag_abs, flip_abs, norm_abs), all np.longdouble"""
    st = states(n_sites, n_up)
    xl = np.asarray(x, np.float64).astype(LD)
    assert xl.size == st.size
    x2 = xl * xl
    norm2 = x2.sum(dtype=LD)
    diag, flip, flip_abs = np.zeros(len(diag_masks), LD), np.zeros(len(flip_masks), LD), np.zeros(len(flip_masks), LD)
    for t, m in enumerate(diag_masks):
        diag[t] = (_sigma_product(st, int(m)).astype(LD) * x2).sum(dtype=LD)
    for t, m in enumerate(flip_masks):
        m = int(m)
        on = np.ones(st.size, bool) if bin(m).count("1") == 1 else _sigma_product(st, m) == -1
        partner = st[on] ^ np.uint64(m)
        idx = partner.astype(np.int64) if n_up is None else ss.rank(st, partner)
        terms = xl[on] * xl[idx]
        flip[t], flip_abs[t] = terms.sum(dtype=LD), np.abs(terms).sum(dtype=LD)
    return diag, flip, norm2, np.full(len(diag_masks), norm2, LD), flip_abs, norm2


def check(label, n_sites, n_up, x, diag_masks, flip_masks, got, ref=None):
    """assert got = (diag, flip, norm2) within the bound of the restatement; prints the largest error over its bound"""
    ref = measure(n_sites, n_up, x, diag_masks, flip_masks) if ref is None else ref
    n = rows(n_sites, n_up)
    worst = 0.0
    for name, out, want, mag in (("diag", got[0], ref[0], ref[3]), ("flip", got[1], ref[1], ref[4]), ("norm2", [got[2]], [ref[2]], [ref[5]])):
        assert len(out) == len(want), (label, name)
        for t in range(len(out)):
            err, bound = abs(LD(out[t]) - want[t]), n * EPS * mag[t]
            if bound > 0:
                worst = max(worst, float(err / bound))
            assert err <= bound, f"{label}: {name}[{t}] = {out[t]!r}, reference {want[t]!r}, error {float(err):.3e} > bound {float(bound):.3e}"
    print(f"{label}: largest error / bound = {worst:.3e}")
    return ref


def site_masks(n_sites):
    return [1 << i for i in range(n_sites)]


def pairs(n_sites):
    return [(i, j) for i in range(n_sites) for j in range(i + 1, n_sites)]


def pair_masks(n_sites):
    return [(1 << i) | (1 << j) for (i, j) in pairs(n_sites)]


def term_lists(n_sites, n_up):
    """the lists of the tests: diag = every site, every pair, a string of (up to) four sites spread over the chain with the top
    site among them, the all-sites mask and a duplicate of the first pair; flip = every pair, the same duplicate and, in the full
    space, every site"""
    string = 0
    for i in sorted({0, n_sites // 3, (2 * n_sites) // 3, n_sites - 1}):
        string |= 1 << i
    pm = pair_masks(n_sites)
    diag = site_masks(n_sites) + pm + [string, (1 << n_sites) - 1, pm[0]]
    flip = pm + [pm[0]] + (site_masks(n_sites) if n_up is None else [])
    return np.array(diag, np.uint32), np.array(flip, np.uint32)


def vector(n_sites, n_up, seed=None):
    return np.random.RandomState(1000 * n_sites + (77 if n_up is None else n_up) if seed is None else seed).standard_normal(rows(n_sites, n_up))


def correlations(n_sites, diag_sites, diag_pairs, flip_pairs, norm2):
    """(sz[i], szsz[i, j], sxy[i, j], dot[i, j]) in np.longdouble from the raw sums of site_masks and pair_masks; i = j holds
    1/4, 1/2 and 3/4"""
    n2 = LD(norm2)
    sz = np.asarray(diag_sites, LD) / (2 * n2)
    zz, xy = np.eye(n_sites, dtype=LD) / 4, np.eye(n_sites, dtype=LD) / 2
    for k, (i, j) in enumerate(pairs(n_sites)):
        zz[i, j] = zz[j, i] = LD(diag_pairs[k]) / (4 * n2)
        xy[i, j] = xy[j, i] = LD(flip_pairs[k]) / (2 * n2)
    return sz, zz, xy, zz + xy


def total_spin_squared(dot):
    return dot.sum(dtype=LD)
