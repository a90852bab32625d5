"""Dense float64 numpy restatement of the Krylov-Schur restart (Stewart, SIAM J. Matrix Anal. Appl. 23 (2001) 601), the
reference of tests/test_krylov_schur_host.py and tests/test_gpu_krylov_schur.py.

A Krylov decomposition  A Z_k = Z_k B_top + u b^T  (Z_k orthonormal, u a unit vector orthogonal to it) is kept as
Z (N x k), Ht ((k+1) x k: B_top over b^T) and the unnormalised residual w = |w| u.  An Arnoldi run is the special case
with B_top upper Hessenberg and b = |w| e_k.
"""
from __future__ import annotations

import numpy as np


def sorted_ritz(H):
    """Ritz values and vectors of the square projected matrix, |theta| descending, ties in numpy.linalg.eig's order"""
    theta, S = np.linalg.eig(H)
    order = np.argsort(-np.abs(theta), kind="stable")
    return theta[order], S[:, order]


def select(theta, keep, real):
    """indices (ascending) of the Ritz values a restart keeps: the first `keep`; for a real matrix a conjugate pair is never
    split: the partner joins (keep + 1), or the half pair leaves if that would fill the whole basis"""
    m = theta.size
    keep = max(1, min(keep, m - 1))
    taken = list(range(keep))
    if real:
        for i in range(keep):
            if theta[i].imag == 0.0:
                continue
            j = int(np.argmin([abs(theta[j] - np.conj(theta[i])) if j != i and theta[j].imag != 0.0 else np.inf for j in range(m)]))
            if j not in taken:
                if len(taken) + 1 <= m - 1:
                    taken.append(j)
                else:
                    taken.remove(i)
    return sorted(taken)


def restart_basis(H, keep, residue):
    """keep', Q (m x keep'), B ((keep'+1) x keep'), theta (all, sorted) of one restart of the m x m projected matrix H"""
    H = np.asarray(H)
    real = not np.iscomplexobj(H)
    theta, S = sorted_ritz(H)
    taken = select(theta, keep, real)
    cols = []
    for i in taken:
        s = S[:, i]
        if not real:
            cols.append(s)
        elif theta[i].imag == 0.0:
            cols.append(s.real)  # eig returns real vectors for the real eigenvalues of a real matrix
        elif theta[i].imag > 0.0:
            cols += [s.real, s.imag]  # once per pair: eig lists theta and conj(theta) side by side, and select() keeps both
    if not cols:  # m = 2 and one conjugate pair: a real basis cannot keep half of it
        return 0, np.zeros((H.shape[0], 0)), np.zeros((1, 0)), theta
    Q, _ = np.linalg.qr(np.stack(cols, axis=1))  # Householder
    k = Q.shape[1]
    B = np.empty((k + 1, k), Q.dtype)
    B[:k] = Q.conj().T @ H @ Q
    B[k] = residue * Q[-1]
    return k, Q, B, theta


def arnoldi_extend(A, Z, Ht, w, m):
    """continue the decomposition (Z: N x k, Ht: (k+1) x k, residual w) to m vectors by Arnoldi steps with Gram-Schmidt
    applied twice; k = 0: start from w.  Returns Z (N x m), Ht ((m+1) x m, last row = (0 .. 0 |w|)) and the new w."""
    N = w.size
    k = 0 if Z is None else Z.shape[1]
    dt = np.result_type(A.dtype, w.dtype)
    Zn = np.zeros((N, m), dt)
    Hn = np.zeros((m + 1, m), dt)
    if k:
        Zn[:, :k] = Z
        Hn[: k + 1, :k] = Ht
    for j in range(k, m):
        q = w / np.linalg.norm(w)
        Zn[:, j] = q
        v = A @ q
        h = np.zeros(j + 1, dt)
        for _ in range(2):
            c = Zn[:, : j + 1].conj().T @ v
            v = v - Zn[:, : j + 1] @ c
            h += c
        Hn[: j + 1, j] = h
        Hn[j + 1, j] = 0.0
        if j + 1 < m:
            Hn[j + 1, j] = np.linalg.norm(v)
        w = v
    Hn[m, m - 1] = np.linalg.norm(w)
    return Zn, Hn, w


def restarted_decomposition(A, v0, m, keep):
    """one cycle of m Arnoldi steps, one restart keeping `keep`, and the continuation back to m vectors.
    Returns the first cycle (Z1, H1, w1), the restart (k, Q, B) and the second cycle (Z2, H2, w2)."""
    Z1, H1, w1 = arnoldi_extend(A, None, None, np.asarray(v0), m)
    k, Q, B, _ = restart_basis(H1[:m], keep, np.linalg.norm(w1))
    Z2, H2, w2 = arnoldi_extend(A, Z1 @ Q, B, w1, m)
    return (Z1, H1, w1), (k, Q, B), (Z2, H2, w2)


def krylov_relation_residual(A, Z, Ht, w):
    """max |A Z_m - [Z_m, w/|w|] Ht|  for a decomposition of m vectors"""
    u = w / np.linalg.norm(w)
    return np.abs(A @ Z - np.concatenate([Z, u[:, None]], axis=1) @ Ht).max()
