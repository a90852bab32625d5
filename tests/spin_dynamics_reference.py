"""numpy yardsticks for the site operators (eigenex_spin_site_apply) and for SpinDynamicsSolver, independent of the library's
row walk: the operators sum_i c_i Sz_i, sum_i c_i S+_i, sum_i c_i S-_i as Kronecker products on the full space, restricted to
sectors by their state lists; the dynamical response from a dense diagonalisation of the destination's matrix; and a plain
Lanczos continued fraction with full re-orthogonalisation, which tests/test_spin_site_host.py holds to the tolerances the GPU
test asserts, so that a failure there is the device's.  Also the cases both tests run.  NOT part of the reference project.

A model is (n_sites, bonds, hz, hx) as in tests/spin_reference.py; n_up = None is the full space."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_reference as sr  # noqa: E402

Z, PLUS, MINUS = 0, 1, 2
EPS = 2.0 ** -52
LD = np.longdouble


def dst_up(n_up, kind):
    return n_up if n_up is None or kind == Z else n_up + (1 if kind == PLUS else -1)


def states(capi, L, n_up):
    return np.arange(1 << L, dtype=np.int64) if n_up is None else capi.spin_sector_states(L, n_up).astype(np.int64)


def site_operator(capi, L, n_up, kind, coef, absolute=False):
    """the matrix of sum_i c_i O_i from the rows of (L, n_up) to those of the destination, from Kronecker products; absolute:
    sum_i |c_i| O_i instead (the entries of Sz taken as +1/2), the size of what is summed"""
    one = {Z: np.abs(sr._SZ) if absolute else sr._SZ, PLUS: sr._SP, MINUS: sr._SM}[kind]
    O = np.zeros((1 << L, 1 << L))
    for i in range(L):
        O += (abs(coef[i]) if absolute else coef[i]) * sr._site_operator(L, {i: one})
    return O[np.ix_(states(capi, L, dst_up(n_up, kind)), states(capi, L, n_up))]


def hamiltonian(capi, model, n_up):
    L, bonds, hz, hx = model
    if n_up is None:
        rowptr, col, val = capi.spin_csr(L, bonds, hz, hx)
    else:
        rowptr, col, val = capi.spin_sector_csr(L, n_up, bonds, hz)
    return sr.dense_from_csr(rowptr.size - 1, rowptr, col, val)


def random_model(L, seed, with_hx=False):
    """random couplings on the open chain and on one long bond (0, L/2), random fields"""
    rng = np.random.RandomState(seed)
    bonds = [(i, i + 1, float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.5, 1.5))) for i in range(L - 1)]
    bonds.append((0, L // 2, float(rng.uniform(0.3, 0.9)), float(rng.uniform(0.3, 0.9))))
    hz = rng.uniform(-0.5, 0.5, L)
    hx = rng.uniform(-0.5, 0.5, L) if with_hx else None
    return (L, bonds, hz, hx)


def ring(L):
    return (L, sr.chain(L, periodic=True), None, None)


def random_coefficients(L, seed):
    return np.random.RandomState(1000 + seed).uniform(-1.0, 1.0, L)


def sz_q(L, q):
    """(cos part, sin part) of Sz_q = L^{-1/2} sum_r e^{iqr} Sz_r"""
    r = np.arange(L)
    return np.cos(q * r) / np.sqrt(L), np.sin(q * r) / np.sqrt(L)


class Dense:
    """ground state of the source and the exact response of a list of (kind, coef) parts, by numpy.linalg.eigh"""

    def __init__(self, capi, model, n_up, parts):
        L = model[0]
        Es, Vs = np.linalg.eigh(hamiltonian(capi, model, n_up))
        self.E0, self.psi = float(Es[0]), np.ascontiguousarray(Vs[:, 0])
        self.gap_levels = Es
        poles, weights = [], []
        for kind, coef in parts:
            phi = site_operator(capi, L, n_up, kind, coef) @ self.psi
            En, Vn = np.linalg.eigh(hamiltonian(capi, model, dst_up(n_up, kind)))
            poles.append(En - self.E0)
            weights.append((Vn.T @ phi) ** 2)
        self.poles, self.weights = np.concatenate(poles), np.concatenate(weights)

    def moment(self, k):
        return float(np.sum(self.weights * self.poles ** k))

    def moment_scale(self, k):
        return float(np.sum(self.weights * np.abs(self.poles) ** k))

    def spectrum(self, omega, eta):
        return lorentzians(self.poles, self.weights, omega, eta)

    def lowest_pole(self, floor=1e-12):
        """the lowest pole that carries weight"""
        return float(self.poles[self.weights > floor * self.weights.sum()].min())


def lorentzians(poles, weights, omega, eta):
    omega = np.asarray(omega, np.float64)
    return np.sum(weights[None, :] * (eta / np.pi) / ((omega[:, None] - poles[None, :]) ** 2 + eta ** 2), axis=1)


def lanczos_fraction(H, phi, m, E0, vv=1.0):
    """(poles, weights) of the m-step continued fraction of <phi| delta(w - (H - E0)) |phi> / vv by plain Lanczos with full
    re-orthogonalisation (twice); stops at a breakdown"""
    n2 = float(phi @ phi)
    if n2 == 0.0:
        return np.zeros(0), np.zeros(0)
    V = [phi / np.sqrt(n2)]
    alpha, beta = [], []
    for k in range(min(m, H.shape[0])):
        w = H @ V[k]
        alpha.append(float(V[k] @ w))
        for _ in range(2):
            for u in V:
                w = w - (u @ w) * u
        b = float(np.sqrt(w @ w))
        if k + 1 == min(m, H.shape[0]) or b <= 1e-12:
            break
        beta.append(b)
        V.append(w / b)
    T = np.diag(alpha) + np.diag(beta[: len(alpha) - 1], 1) + np.diag(beta[: len(alpha) - 1], -1)
    theta, S = np.linalg.eigh(T)
    return theta - E0, n2 / vv * S[0, :] ** 2


# ---- the cases of the dynamics tests: name -> (model, n_up, [(kind, coef), ...], m) ----
def moment_cases():
    """m = 40, k = 0..3 against the dense values to 1e-10 of sum w |p|^k"""
    out = {}
    for name, L, n_up, kind, seed in (("(10,5) Z", 10, 5, Z, 1), ("(10,5) MINUS", 10, 5, MINUS, 2), ("(9,4) PLUS", 9, 4, PLUS, 3)):
        out[name] = (random_model(L, seed), n_up, [(kind, random_coefficients(L, seed))], 40)
    for kind, word in ((Z, "Z"), (PLUS, "PLUS"), (MINUS, "MINUS")):
        out["full 8 hx " + word] = (random_model(8, 4, with_hx=True), None, [(kind, random_coefficients(8, 4 + kind))], 40)
    return out


def spectrum_cases():
    """spectrum(w, eta = 0.1) on 141 points of [-1, 6] against the dense spectrum to 1e-9 of its maximum: the Heisenberg ring at
    q = pi, and one random model with m = the destination's dimension (56 rows of (8,3))"""
    return {
        "ring (10,5) q=pi": (ring(10), 5, [(Z, sz_q(10, np.pi)[0])], 40),
        "ring (12,6) q=pi": (ring(12), 6, [(Z, sz_q(12, np.pi)[0])], 60),
        "(8,4) MINUS complete": (random_model(8, 5), 4, [(MINUS, random_coefficients(8, 5))], 56),
    }


OMEGA = np.linspace(-1.0, 6.0, 141)
ETA = 0.1
MOMENT_TOL = 1e-10   # the project's asserted tolerance for Ritz values against the oracle
SPECTRUM_TOL = 1e-9  # a pole error of 1e-10 divided by eta
