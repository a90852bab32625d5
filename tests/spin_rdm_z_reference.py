"""numpy restatement of the reduced density matrix of a COMPLEX vector (include/eigenex_hip.h: eigenex_spin_rdm_z,
eigenex_spin_rdm_host_z), on top of tests/spin_rdm_reference.py, whose panels M_k (its own enumeration, deposit and rank) are
taken of the real and of the imaginary part in np.longdouble:

    rho_k = M_k M_k^H:   re = Mr Mr^T + Mi Mi^T,   im = Mi Mr^T - Mr Mi^T.

The bound, elementwise: 2 n_b eps times the same expressions in absolute values,
    bound_re = 2 n_b eps (|Mr| |Mr|^T + |Mi| |Mi|^T),   bound_im = 2 n_b eps (|Mi| |Mr|^T + |Mr| |Mi|^T)
-- each part is a sum of 2 n_b products, and a sum of N terms in any grouping is within N eps sum |terms| of the exact one (the
real kernel's n_b eps |M| |M|^T, for twice the terms).  It holds for every launch grid, slice count and tile size.

Shared by tests/test_spin_rdm_z_host.py and tests/test_gpu_spin_rdm_z.py."""
from __future__ import annotations

from math import log

import numpy as np
import spin_rdm_reference as rr

EPS = rr.EPS
LD = rr.LD


def rdm_z(n_sites, n_up, x, mask_a):
    """[(k, re, im, bound_re, bound_im)], all np.longdouble"""
    x = np.asarray(x, np.complex128)
    pr = rr.panels(n_sites, n_up, np.ascontiguousarray(x.real), mask_a)
    pi = rr.panels(n_sites, n_up, np.ascontiguousarray(x.imag), mask_a)
    out = []
    for (k, Mr), (k2, Mi) in zip(pr, pi):
        assert k == k2
        ar, ai = np.abs(Mr), np.abs(Mi)
        scale = 2 * Mr.shape[1] * EPS
        out.append((k, Mr @ Mr.T + Mi @ Mi.T, Mi @ Mr.T - Mr @ Mi.T, scale * (ar @ ar.T + ai @ ai.T), scale * (ai @ ar.T + ar @ ai.T)))
    return out


def check_z(label, got, ref, factor=1):
    """assert got = [(k, complex128 ndarray)] equals ref = rdm_z(...) within factor times its bound, part by part and entry by
    entry; that the imaginary part of the diagonal is +0.0 (the sign bit too) and that (j, i) is the conjugate of (i, j) bit for
    bit.  Prints the largest error over its bound."""
    assert [k for k, _ in got] == [r[0] for r in ref], label
    worst = 0.0
    for (k, g), (_, re, im, bre, bim) in zip(got, ref):
        assert g.dtype == np.complex128 and g.shape == re.shape, (label, k, g.shape, re.shape)
        diag = np.ascontiguousarray(g.imag.diagonal())
        assert diag.tobytes() == np.zeros(diag.size).tobytes(), f"{label}: block {k}: the diagonal's imaginary part is not +0.0"
        mirror_im, minus_im = np.ascontiguousarray(g.T.imag), np.ascontiguousarray(-g.imag)
        np.fill_diagonal(mirror_im, 0.0), np.fill_diagonal(minus_im, 0.0)  # the diagonal is +0.0 on both sides, checked above
        assert np.ascontiguousarray(g.T.real).tobytes() == np.ascontiguousarray(g.real).tobytes() and mirror_im.tobytes() == minus_im.tobytes(), \
            f"{label}: block {k} is not Hermitian bit for bit"
        for part, want, bound in (("re", re, bre), ("im", im, bim)):
            err = np.abs(getattr(g, "real" if part == "re" else "imag").astype(LD) - want)
            pos = bound > 0
            if pos.any():
                worst = max(worst, float((err[pos] / bound[pos]).max()))
            bad = err > factor * bound
            assert not bad.any(), (f"{label}: block {k} ({part}): {int(bad.sum())} entries off, the first at {tuple(np.argwhere(bad)[0])}: "
                                   f"error {float(err[bad][0]):.3e} > bound {float((factor * bound)[bad][0]):.3e}")
    print(f"{label}: largest error / bound = {worst:.3e}")


def trace_check(got, x, n):
    """the trace is sum |x|^2: 2n terms in some grouping on either side"""
    x = np.asarray(x, np.complex128)
    n2 = float(np.vdot(x, x).real)
    trace = sum(float(np.trace(m).real) for _, m in got)
    assert abs(trace - n2) <= 2 * n * EPS * n2, (trace, n2)


def spectrum_z(blocks):
    """all eigenvalues of the unit-trace rho from raw complex blocks [(k, array)], descending, clamped at 0"""
    tr = sum(float(np.trace(np.asarray(b)).real) for _, b in blocks)
    lam = np.concatenate([np.linalg.eigvalsh(np.asarray(b, np.complex128) / tr) for _, b in blocks])
    return np.sort(np.maximum(lam, 0.0))[::-1]


def rho_of_state(n_sites, n_up, psi, mask_a):
    """numpy's own raw complex blocks [(k, M_k M_k^H)] of a state in float64 (the reference of the entropy tests)"""
    psi = np.asarray(psi, np.complex128)
    pr = rr.panels(n_sites, n_up, np.ascontiguousarray(psi.real), mask_a)
    pi = rr.panels(n_sites, n_up, np.ascontiguousarray(psi.imag), mask_a)
    out = []
    for (k, Mr), (_, Mi) in zip(pr, pi):
        M = Mr.astype(np.float64) + 1j * Mi.astype(np.float64)
        out.append((k, M @ M.conj().T))
    return out


def entropy_tolerance_z(d, n_b):
    """rr.entropy_tolerance re-derived for the complex sums and the embedded eigen-solve: an entry of the unit-trace rho is off by at
    most 2 n_b eps (|M| |M|^H)[i, j], whose Frobenius norm is at most 2 n_b eps (Cauchy-Schwarz, trace 1), for each of the two parts:
    ||Delta||_F <= 2 sqrt(2) n_b eps < 3 n_b eps; the eigen-solver (the real symmetric embedding of order 2d) adds 2d eps.  By Weyl
    every eigenvalue moves by at most delta = (3 n_b + 2 d) eps, and |x ln x - y ln y| <= -delta ln delta for |x - y| <= delta <=
    1/2, over d eigenvalues."""
    delta = (3 * n_b + 2 * d) * float(EPS)
    assert delta <= 0.5
    return d * (-delta * log(delta))
