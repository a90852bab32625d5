"""numpy restatement of the Chebyshev-filtered Lanczos solver (filtered_lanczos.hpp, eigenex_basis_set_filter): the
coefficients, the recurrence in float64 (the device's order of operations) and in np.longdouble, and the filtered
thick-restart Lanczos with its final Rayleigh-Ritz step.  Shared by tests/test_filter_host.py and tests/test_gpu_filter.py."""
from __future__ import annotations

import math

import numpy as np

from oracle.krylov_oracle import fix_phase_and_normalize
from oracle.thick_restart_oracle import thick_restart_lanczos


def delta_coefficients(tau, center, halfwidth, degree):
    """mu_0..mu_degree of the Jackson-damped Chebyshev expansion of a delta peak at tau on [center - halfwidth,
    center + halfwidth], normalised so that p(tau) = 1 (Weisse et al., Rev. Mod. Phys. 78 (2006) 275, eq. 71)"""
    N = degree + 1
    a = min(1.0, max(-1.0, (tau - center) / halfwidth))
    th, q = np.arccos(a), np.pi / (N + 1)
    k = np.arange(N, dtype=np.float64)
    g = ((N - k + 1) * np.cos(q * k) + np.sin(q * k) / np.tan(q)) / (N + 1)
    t = np.cos(k * th)
    mu = np.where(k == 0, 1.0, 2.0) * g * t
    return mu / math.fsum(mu * t)  # (the product sums with compensation: the correctly rounded sum)


def polynomial(mu, x):
    """p(x) = sum_k mu_k T_k(x) for x in [-1, 1]"""
    return np.polynomial.chebyshev.chebval(x, mu)


def csr_rowsum_matmul(rowptr, col, val, dtype):
    """x -> A x with products and row sums in `dtype` (np.longdouble / np.clongdouble for the reference); rows are non-empty"""
    rowptr = np.asarray(rowptr, np.int64)
    v = np.asarray(val).astype(dtype)
    assert np.all(np.diff(rowptr) > 0)

    def matmul(x):
        return np.add.reduceat(v * x[col], rowptr[:-1])

    return matmul


def csr_rowsum_matmul_any_rows(rowptr, col, val, dtype):
    """csr_rowsum_matmul for matrices that may have rows without entries (their result is 0): the same products and the same
    sum of every non-empty row (krylov_local_reference.row_sums)"""
    from krylov_local_reference import row_sums

    rowptr = np.asarray(rowptr, np.int64)
    v = np.asarray(val).astype(dtype)
    return lambda x: row_sums(v * x[col], rowptr)


def apply_filter(matmul, x, mu, center, halfwidth):
    """p(A) x by the recurrence of eigenex_basis_set_filter, one rounded operation at a time, in the precision of x and matmul:
    a = A t_k - center t_k;  t_1 = (1/h) a,  t_{k+1} = (2/h) a - t_{k-1};  acc_1 = mu0 x + mu1 t_1,  acc_{k+1} = acc_k + mu_{k+1} t_{k+1}."""
    real = np.float64 if x.dtype in (np.float64, np.complex128) else np.longdouble
    mu = np.asarray(mu).astype(real)
    c1, c2 = real(1.0) / real(halfwidth), real(2.0) / real(halfwidth)
    if real is np.float64:  # the factors the device forms on the host, in double
        c1, c2 = np.float64(1.0 / halfwidth), np.float64(2.0 / halfwidth)
    shift = real(-center)
    d = len(mu) - 1
    assert d >= 1
    t_prev, t = None, x
    acc = None
    for k in range(d):
        a = matmul(t)
        if shift != 0:
            a = a + shift * t
        if k == 0:
            t_next = c1 * a
            acc = mu[0] * x + mu[1] * t_next
        else:
            t_next = c2 * a - t_prev
            acc = acc + mu[k + 1] * t_next
        t_prev, t = t, t_next
    return acc


def filtered_lanczos(matmul, n, init, tau, lo, hi, degree, nev, m, keep=-1, tol=1e-10, max_restarts=1000):
    """The solver: range widened by 1 %, thick-restart Lanczos (oracle/thick_restart_oracle.py) on -p(A) for the nev pairs of
    largest p, then Rayleigh-Ritz in A.  Eigenvalues sorted by |lambda - tau|; residuals are ||A x - lambda x||."""
    center, half = 0.5 * (lo + hi), 0.5 * (hi - lo) * 1.01
    mu = delta_coefficients(tau, center, half, degree)
    r = thick_restart_lanczos(lambda x: -apply_filter(matmul, x, mu, center, half), n, init, nev, m, keep=keep, tol=tol, max_restarts=max_restarts)
    X = r["eigenvectors"]
    AX = np.stack([matmul(np.ascontiguousarray(X[:, i])) for i in range(X.shape[1])], axis=1)
    G = X.conj().T @ AX
    lam, S = np.linalg.eigh(0.5 * (G + G.conj().T))
    order = np.argsort(np.abs(lam - tau), kind="stable")
    lam, S = lam[order], S[:, order]
    Y = np.stack([fix_phase_and_normalize(X @ S[:, i]) for i in range(len(lam))], axis=1)
    res = np.array([np.linalg.norm(matmul(np.ascontiguousarray(Y[:, i])) - lam[i] * Y[:, i]) for i in range(len(lam))])
    return dict(eigenvalues=lam, eigenvectors=Y, residuals=res, restarts=r["restarts"], filter_applications=r["matvecs"],
                p_residuals=r["residuals"], log=r["log"], mu=mu, center=center, halfwidth=half)


# ---- the inputs the issue names -------------------------------------------------------------------------------------
def anderson_chain(n=1000, seed=7):
    """1-D Anderson chain: diag(2 (rand - 0.5)) - hopping, as CSR (ascending columns)"""
    import scipy.sparse as sp

    d = 2.0 * (np.random.RandomState(seed).rand(n) - 0.5)
    A = (sp.diags(d) - sp.eye(n, k=1) - sp.eye(n, k=-1)).tocsr()
    A.sort_indices()
    return A


def anderson3d(shape=(6, 7, 8), W=2.0, seed=7):
    """3-D Anderson model on an open nx x ny x nz grid: on-site energies W (rand - 0.5), hopping -1"""
    import scipy.sparse as sp

    nx, ny, nz = shape
    n = nx * ny * nz
    eps = W * (np.random.RandomState(seed).rand(n) - 0.5)
    hop = lambda k: -(sp.eye(k, k=1) + sp.eye(k, k=-1))
    ix, iy, iz = sp.eye(nx), sp.eye(ny), sp.eye(nz)
    A = sp.diags(eps) + sp.kron(sp.kron(hop(nx), iy), iz) + sp.kron(sp.kron(ix, hop(ny)), iz) + sp.kron(sp.kron(ix, iy), hop(nz))
    A = A.tocsr()
    A.sort_indices()
    return A


def hermitian_tridiagonal(n=300, seed=3):
    import scipy.sparse as sp

    rng = np.random.RandomState(seed)
    d = rng.standard_normal(n)
    e = rng.standard_normal(n - 1) + 1j * rng.standard_normal(n - 1)
    A = (sp.diags(d.astype(np.complex128)) + sp.diags(e, 1) + sp.diags(e.conj(), -1)).tocsr()
    A.sort_indices()
    return A


def gershgorin(A):
    A = A.tocsr()
    d = A.diagonal().real
    r = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(A.diagonal())
    return float((d - r).min()), float((d + r).max())


def nearest(A, tau, k):
    lam = np.linalg.eigvalsh(A.toarray())
    return lam[np.argsort(np.abs(lam - tau), kind="stable")[:k]]
