"""numpy restatement of the observables of one vector against a set of columns (include/eigenex_hip.h:
eigenex_spin_measure_columns, eigenex_spin_measure_columns_host), independent of csrc/spin_measure_columns.hpp: every sum and
the sum of its terms' magnitudes in np.longdouble, the sector's states by enumeration and the rank by searchsorted, as in
tests/spin_measure_reference.py, whose shapes, term lists and vectors the tests reuse.  Shared by
tests/test_spin_measure_columns_host.py and tests/test_gpu_spin_measure_columns.py.

    diag[t, j] = sum_s (prod_{i in mask_t} sigma_i(s)) V_j(s) x_s
    flip[t, j] = sum_s [the row has the entry] V_j(s) x_{s ^ mask_t}

The bound is spin_measure_reference.check's: |out - ref| <= n eps sum_s |term_s|, n the number of rows, eps = 2^-52 -- the
rounding of an n-term sum in any grouping."""
from __future__ import annotations

import numpy as np
import spin_measure_reference as mr
import spin_sector_reference as ss

EPS = mr.EPS
LD = np.longdouble


def applied(n_sites, n_up, x, diag_masks, flip_masks):
    """w_d[t, s] = (A_t x)(s) of the diagonal masks and w_f[t, s] of the flip masks, np.longdouble (exact: a sign or a copy)"""
    st = mr.states(n_sites, n_up)
    xl = np.asarray(x, np.float64).astype(LD)
    assert xl.size == st.size
    wd, wf = np.zeros((len(diag_masks), st.size), LD), np.zeros((len(flip_masks), st.size), LD)
    for t, m in enumerate(diag_masks):
        wd[t] = mr._sigma_product(st, int(m)).astype(LD) * xl
    for t, m in enumerate(flip_masks):
        m = int(m)
        on = np.ones(st.size, bool) if bin(m).count("1") == 1 else mr._sigma_product(st, m) == -1
        partner = st[on] ^ np.uint64(m)
        idx = partner.astype(np.int64) if n_up is None else ss.rank(st, partner)
        wf[t, on] = xl[idx]
    return wd, wf


def measure(n_sites, n_up, x, columns, diag_masks, flip_masks):
    """(diag[n_diag, count], flip[n_flip, count], diag_abs, flip_abs): the sums and the sums of magnitudes, np.longdouble"""
    wd, wf = applied(n_sites, n_up, x, diag_masks, flip_masks)
    v = np.asarray(columns, np.float64).astype(LD)
    assert v.ndim == 2 and v.shape[1] == wd.shape[1]
    return wd @ v.T, wf @ v.T, np.abs(wd) @ np.abs(v).T, np.abs(wf) @ np.abs(v).T


def check(label, n_sites, n_up, got, ref):
    """assert got = (diag, flip) within the bound of ref = measure(...); prints the largest error over its bound"""
    n = mr.rows(n_sites, n_up)
    worst = 0.0
    for name, out, want, mag in (("diag", got[0], ref[0], ref[2]), ("flip", got[1], ref[1], ref[3])):
        out = np.asarray(out)
        assert out.shape == want.shape and out.dtype == np.float64, (label, name, out.shape, want.shape)
        err, bound = np.abs(out.astype(LD) - want), n * EPS * mag
        if err.size:
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)
            worst = max(worst, float(ratio.max()))
            bad = np.argwhere(err > bound)
            assert bad.size == 0, f"{label}: {name}{tuple(bad[0])} = {out[tuple(bad[0])]!r}, reference {want[tuple(bad[0])]!r}, " \
                                  f"error {float(err[tuple(bad[0])]):.3e} > bound {float(bound[tuple(bad[0])]):.3e}"
    print(f"{label}: largest error / bound = {worst:.3e}")


def columns(n_sites, n_up, count, seed=None):
    """count test columns, a (count, rows) array"""
    rs = np.random.RandomState(7000 + 100 * n_sites + (77 if n_up is None else n_up) if seed is None else seed)
    return rs.standard_normal((count, mr.rows(n_sites, n_up)))
