"""numpy longdouble restatement of the site operators with complex coefficients (eigenex_spin_site_apply_z), independent of the
library's row walk and of its ranking: the matrix of sum_i c_i O_i between the state lists of two sectors, built from bit
operations on the states, and, in the full space, the same matrix from Kronecker products.  A complex matrix is the pair of its
real and imaginary parts in longdouble (numpy has no portable extended complex type worth relying on).  Also the size of what a
row sums, from which the tests take their bounds, and the shapes the host test runs.  NOT part of the reference project."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_dynamics_reference as dr  # noqa: E402

Z, PLUS, MINUS = dr.Z, dr.PLUS, dr.MINUS
EPS = dr.EPS
LD = np.longdouble

# (L, n_up or None, kinds) of the host test: the smallest sector, odd L, a partial batch of sites, a sector of one up spin, one-row
# sources and destinations, bit 31, the full space
HOST_SHAPES = [(4, 2, (Z, PLUS, MINUS)), (9, 4, (Z, PLUS, MINUS)), (11, 5, (Z, PLUS, MINUS)), (13, 1, (Z, PLUS, MINUS)), (6, 0, (PLUS,)), (6, 6, (MINUS,)),
               (32, 1, (MINUS,)), (3, None, (Z, PLUS, MINUS)), (8, None, (Z, PLUS, MINUS))]


def coefficients(L, which, seed=0):
    """complex coefficients of both signs in both parts; "zeros": some of them zero, in either part or in both; "none": all zero"""
    rng = np.random.RandomState(300 + 7 * L + seed)
    c = rng.uniform(-1.0, 1.0, L) + 1j * rng.uniform(-1.0, 1.0, L)
    if which == "zeros":
        c[::3] = c[::3].real
        c[1::3] = 1j * c[1::3].imag
        c[L // 2] = 0.0
    if which == "none":
        c[:] = 0.0
    return c


def complex_vector(n, seed):
    rng = np.random.RandomState(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def site_matrix(capi, L, n_up, kind, weights):
    """the real longdouble matrix of sum_i weights[i] O_i from the rows of (L, n_up) to those of the destination, entry by entry
    from the states: Sz_i has +-1/2 on the diagonal; S+_i has a 1 from s to s | bit where site i is down in s; S-_i the reverse"""
    src, dst = dr.states(capi, L, n_up), dr.states(capi, L, dr.dst_up(n_up, kind))
    O = np.zeros((dst.size, src.size), LD)
    rows = np.arange(dst.size)
    for i in range(L):
        bit = np.int64(1) << i
        up = (dst & bit) != 0
        if kind == Z:
            O[rows, rows] += np.where(up, LD(weights[i]) / 2, -LD(weights[i]) / 2)
            continue
        has = up if kind == PLUS else ~up  # the destination row has the term: S+ raised site i, S- lowered it
        cols = np.searchsorted(src, dst[has] ^ bit)
        assert np.array_equal(src[cols], dst[has] ^ bit)
        O[rows[has], cols] += LD(weights[i])
    return O


def kronecker_matrix(L, kind, weights):
    """the same in the full space as sum_i weights[i] 1 x ... x O x ... x 1, site 0 the lowest bit"""
    one = {Z: np.diag([-LD(1) / 2, LD(1) / 2]), PLUS: np.array([[0, 0], [1, 0]], LD), MINUS: np.array([[0, 1], [0, 0]], LD)}[kind]
    O = np.zeros((1 << L, 1 << L), LD)
    for i in range(L):
        M = np.ones((1, 1), LD)
        for site in range(L - 1, -1, -1):  # the leftmost factor is the highest bit
            M = np.kron(M, one if site == i else np.eye(2, dtype=LD))
        O += LD(weights[i]) * M
    return O


def apply(capi, L, n_up, kind, coef, x):
    """(real part, imaginary part) of O x in longdouble"""
    coef = np.asarray(coef, np.complex128)
    Or, Oi = site_matrix(capi, L, n_up, kind, coef.real), site_matrix(capi, L, n_up, kind, coef.imag)
    xr, xi = np.asarray(x).real.astype(LD), np.asarray(x).imag.astype(LD)
    return Or @ xr - Oi @ xi, Or @ xi + Oi @ xr


def row_size(capi, L, n_up, kind, coef, x):
    """sum_i |c_i| |x_i| per row, with |c| = |Re c| + |Im c| and |x| = |Re x| + |Im x|: what bounds every partial sum of either
    part of a row (for Z the row's sum_i |c_i| / 2 times its own |x|)"""
    coef = np.asarray(coef, np.complex128)
    A = np.abs(site_matrix(capi, L, n_up, kind, np.abs(coef.real) + np.abs(coef.imag)))
    if kind == Z:  # |sum of signed halves| would cancel: the size of what is added is the sum of the halves
        A = np.eye(A.shape[0], dtype=LD) * LD(np.sum(np.abs(coef.real) + np.abs(coef.imag))) / 2
    return A @ (np.abs(np.asarray(x).real) + np.abs(np.asarray(x).imag)).astype(LD)


def terms(L):
    """roundings behind one part of one row.  Z: L - 1 additions for each of the two weights (their halves are exact), one product
    and one fma -- at most 2 L + 2.  A flip: two fma per term the row has, at most 2 L.  Each is below eps/2 of a partial sum that
    row_size bounds, so terms(L) * EPS * row_size is twice what the roundings can add up to."""
    return 2 * L + 2
