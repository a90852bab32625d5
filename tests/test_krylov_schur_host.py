"""The dense host part of a Krylov-Schur restart (small_eigen::krylov_schur_basis through
eigenex_solver_krylov_schur_basis) against the numpy restatement in krylov_schur_reference.py.  No GPU needed."""
from __future__ import annotations

import numpy as np
import pytest

import krylov_schur_reference as ref
from cmpt_eigenex_amd import solver

RESIDUE = 0.37  # any positive number: it only scales the coupling row


def _random(m, cplx, seed):
    rng = np.random.default_rng([seed, m, int(cplx)])
    H = rng.standard_normal((m, m))
    return H + 1j * rng.standard_normal((m, m)) if cplx else H


def _hessenberg(m, cplx, seed):
    return np.triu(_random(m, cplx, seed), -1)


def _restart_shape(m, k, cplx, seed):
    """what a restart leaves: a full (k+1) x k leading block, Hessenberg behind it"""
    H = _hessenberg(m, cplx, seed)
    H[: k + 1, :k] = _random(m, cplx, seed + 1)[: k + 1, :k]
    return H


def _split_pair(seed):
    """real 12 x 12 with eigenvalues 6, 5, 3 +- 2.5i (|.| = 3.9), 2, 1.5, ...: keep = 3 cuts the pair in two"""
    rng = np.random.default_rng([seed, 12])
    D = np.zeros((12, 12))
    D[0, 0], D[1, 1] = 6.0, 5.0
    D[2:4, 2:4] = [[3.0, 2.5], [-2.5, 3.0]]
    D[4:, 4:] = np.diag(np.linspace(2.0, 0.25, 8))
    X = np.eye(12) + 0.3 * rng.standard_normal((12, 12))
    return X @ D @ np.linalg.inv(X)


CASES = {}
for _m in (2, 3, 10, 33):
    CASES[f"real-{_m}"] = (_random(_m, False, 1), max(1, _m // 2))
    CASES[f"complex-{_m}"] = (_random(_m, True, 1), max(1, _m // 2))
CASES["hessenberg-real-20"] = (_hessenberg(20, False, 2), 8)
CASES["hessenberg-complex-20"] = (_hessenberg(20, True, 2), 8)
CASES["restart-shape-real-24"] = (_restart_shape(24, 9, False, 3), 11)
CASES["restart-shape-complex-24"] = (_restart_shape(24, 9, True, 3), 11)
CASES["split-pair-12"] = (_split_pair(4), 3)


def _match(found, wanted):
    """largest distance after pairing every wanted value with its nearest unused found value"""
    found = list(found)
    worst = 0.0
    for w in wanted:
        j = int(np.argmin([abs(f - w) for f in found]))
        worst = max(worst, abs(found.pop(j) - w))
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_restart_basis_against_numpy(name):
    """Q orthonormal to 1e-12 (the symmetric solver's tolerance), keep as the reference's, eig(B_top) = the selected Ritz
    values, coupling row = residue * Q[m-1, :] exactly, and the invariance residual max|H Q - Q B_top| within 10x the
    reference's on the same input (eigenvector conditioning dominates it; the reference stays below 1e-10 on every case).

    Measured (this code / numpy reference): real-2 1.1e-16/2.2e-16, complex-2 2.2e-16/4.0e-16, real-3 4.4e-16/3.3e-16,
    complex-3 1.2e-15/1.2e-15, real-10 1.3e-15/2.2e-15, complex-10 1.8e-15/3.1e-15, real-33 4.0e-15/5.1e-15,
    complex-33 4.7e-15/5.8e-15, hessenberg-real-20 1.8e-15/3.4e-15, hessenberg-complex-20 1.8e-15/2.2e-15,
    restart-shape-real-24 3.7e-15/2.9e-15, restart-shape-complex-24 2.9e-15/4.3e-15, split-pair-12 2.7e-15/1.6e-15.
    Other seeds of the restart shape gave ratios up to 11 (4.1e-14 / 3.8e-15 on a real 20 x 20): the 10x is not loose.
    """
    H, keep = CASES[name]
    m = H.shape[0]
    k, Q, B, theta = solver.krylov_schur_basis(H, keep, RESIDUE)
    k_ref, Q_ref, B_ref, theta_ref = ref.restart_basis(H, keep, RESIDUE)
    res = np.abs(H @ Q - Q @ B[:k]).max(initial=0.0)
    res_ref = np.abs(H @ Q_ref - Q_ref @ B_ref[:k_ref]).max(initial=0.0)
    print(f"{name}: keep {keep} -> {k} (reference {k_ref}), invariance residual {res:.2e}, reference {res_ref:.2e}")
    assert res_ref < 1e-10
    assert k == k_ref
    assert Q.shape == (m, k) and B.shape == (k + 1, k)
    assert Q.dtype == H.dtype and B.dtype == H.dtype  # a real matrix gets a real basis
    assert np.abs(Q.conj().T @ Q - np.eye(k)).max(initial=0.0) <= 1e-12
    assert np.array_equal(B[k], RESIDUE * Q[m - 1])
    # all Ritz values, |theta| descending, as numpy finds them.  Bauer-Fike: a backward-stable eigensolver (error m eps |H|)
    # moves an eigenvalue by at most cond(S) m eps |H|_2; both solvers may, hence the factor 2, and 10 for the constants
    S_ref = ref.sorted_ritz(H)[1]
    bound = 20 * max(np.linalg.cond(S_ref) * m * np.finfo(float).eps * np.linalg.norm(H, 2), _match(np.linalg.eigvals(B_ref[:k_ref]), theta_ref[:k_ref]) if k_ref else 0.0)
    assert np.all(np.diff(np.abs(theta)) <= bound)
    assert _match(theta, theta_ref) <= bound
    # eig(B_top) = the selected Ritz values: the first k of the sorted list (a real matrix's selection is closed under
    # conjugation, and a pair shares one modulus, so the first k are the selection)
    if k:
        assert _match(np.linalg.eigvals(B[:k]), theta_ref[:k]) <= bound
    assert res <= 10 * res_ref


def test_conjugate_pair_is_not_split():
    H, keep = CASES["split-pair-12"]
    k, Q, B, theta = solver.krylov_schur_basis(H, keep, RESIDUE)
    assert k == keep + 1
    assert abs(theta[2] - np.conj(theta[3])) < 1e-10 and abs(abs(theta[2].imag) - 2.5) < 1e-10
    ev = np.linalg.eigvals(B[:k])
    assert _match(ev, [6.0, 5.0, 3.0 + 2.5j, 3.0 - 2.5j]) < 1e-10
    # the same matrix as complex data has no pairs to respect
    assert solver.krylov_schur_basis(H.astype(np.complex128), keep, RESIDUE)[0] == keep


def test_half_pair_leaves_when_the_basis_would_be_full():
    """m = 3, keep = 2 and the pair second: keeping both would leave no room (keep must stay below m)"""
    H = np.array([[5.0, 0.0, 0.0], [0.0, 1.0, 2.0], [0.0, -2.0, 1.0]]) + 1e-3 * np.arange(9.0).reshape(3, 3)
    k, Q, B, _ = solver.krylov_schur_basis(H, 2, RESIDUE)
    assert k == ref.restart_basis(H, 2, RESIDUE)[0] == 1
    assert abs(B[0, 0] - ref.sorted_ritz(H)[0][0].real) < 1e-12


def test_bad_arguments_are_errors():
    from cmpt_eigenex_amd import capi

    with pytest.raises(capi.EigenexError):
        solver.krylov_schur_basis(np.eye(1), 1, RESIDUE)
