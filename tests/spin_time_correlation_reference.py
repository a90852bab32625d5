"""numpy restatement of SpinTimeCorrelationSolver (spin_time_correlation.hpp), independent of csrc/ and of the header:
C_n(t) = <A_n psi(t) | phi(t)> with psi(t) = exp(-iHt) psi_0 on the source sector and phi(t) = exp(-iHt) B psi_0 on the
destination's, both propagated as unit vectors by spin_evolution_reference.KrylovPropagator (the algorithm of the sub-step,
restated on dense matrices) or, for the exact values, by spin_evolution_reference.Dense.  The operators are dense matrices from
the Kronecker yardstick of spin_dynamics_reference.site_operator, real and imaginary coefficients apart.  Also the cases of
tests/test_gpu_spin_time_correlation.py and their floors.  NOT part of the reference project.

The bound of the restatement is the solver's: |delta C_n| <= ||A_n|| |B psi_0| (eps_psi + eps_phi), eps the accumulated sub-step
bounds of the two unit vectors, ||A|| <= sum_i |a_i| / 2 for Z and sum_i |a_i| for the flips."""
from __future__ import annotations

import functools

import numpy as np
import spin_dynamics_reference as dr
import spin_evolution_reference as er

EPS = np.finfo(np.float64).eps
CALLS, DT, M, TOL = 8, 0.25, 12, 1e-9


def operator(capi, L, n_up, kind, coef):
    """the dense complex matrix of sum_i c_i S^kind_i from (L, n_up) to the destination"""
    c = np.asarray(coef, np.complex128)
    return dr.site_operator(capi, L, n_up, kind, c.real) + 1j * dr.site_operator(capi, L, n_up, kind, c.imag)


def norm_bound(kind, coef):
    s = float(np.sum(np.abs(np.asarray(coef, np.complex128))))
    return 0.5 * s if kind == dr.Z else s


def momentum_z(L, q):
    return np.exp(1j * q * np.arange(L)) / np.sqrt(L)


class Case:
    """model = (L, bonds, hz, hx); psi0 a unit vector of (L, n_up); source and measured: coefficient arrays of one kind"""

    def __init__(self, capi, model, n_up, psi0, kind, source, measured, eigen_energy=None):
        L = model[0]
        self.model, self.n_up, self.kind, self.source, self.measured = model, n_up, kind, np.asarray(source, np.complex128), [np.asarray(a, np.complex128) for a in measured]
        self.H_src, self.H_dst = dr.hamiltonian(capi, model, n_up), dr.hamiltonian(capi, model, dr.dst_up(n_up, kind))
        self.psi0 = np.asarray(psi0, np.complex128) / np.linalg.norm(psi0)
        self.B = operator(capi, L, n_up, kind, self.source)
        self.A = [operator(capi, L, n_up, kind, a) for a in self.measured]
        self.phi0 = self.B @ self.psi0
        self.source_norm = float(np.linalg.norm(self.phi0))
        self.norms = np.array([norm_bound(kind, a) for a in self.measured])
        self.eigen_energy = eigen_energy
        self._dense = (er.Dense(self.H_src), er.Dense(self.H_dst))

    def dense_values(self, t):
        psi, phi = self._dense[0].propagate(self.psi0, t), self._dense[1].propagate(self.phi0, t)
        return np.array([np.vdot(A @ psi, phi) for A in self.A])

    def restatement(self, m, tol):
        return Restatement(self, m, tol)


class Restatement:
    def __init__(self, case, m, tol):
        self.case, self.time = case, 0.0
        self.psi = er.KrylovPropagator(case.H_src, case.psi0, m, tol)
        self.phi = er.KrylovPropagator(case.H_dst, case.phi0, m, tol)  # normalises: a unit vector, like the solver's
        self.eps_psi = self.eps_phi = 0.0

    def evolve(self, dt):
        if self.case.eigen_energy is None:
            self.psi.evolve(dt)
            self.eps_psi += self.psi.bound
        self.phi.evolve(dt)
        self.eps_phi += self.phi.bound
        self.time += dt

    def values(self):
        c = self.case
        psi = self.psi.psi if c.eigen_energy is None else np.exp(-1j * c.eigen_energy * self.time) * c.psi0
        return np.array([c.source_norm * np.vdot(A @ psi, self.phi.psi) for A in c.A])

    def bounds(self):
        return self.case.norms * self.case.source_norm * (self.eps_psi + self.eps_phi)

    @property
    def applications(self):
        return self.psi.applications + self.phi.applications


@functools.lru_cache(maxsize=None)
def _ring_ground_state(capi):
    E, V = np.linalg.eigh(dr.hamiltonian(capi, dr.ring(10), 5))
    return float(E[0]), np.ascontiguousarray(V[:, 0])


def case(capi, name):
    """(a) "neel": the Neel state of the open XXZ chain (10,5), B = S-_4, A_j = S-_j for every site, (10,5) -> (10,4).
    (b) "ring" / "ring eigen": the ground state of the Heisenberg ring (10,5), A = B = Sz_q at q = 2 pi 3 / 10, psi evolved or
    declared an eigenstate."""
    if name == "neel":
        L, n_up, bonds, hz, hx, bits = er.QUENCHES["neel_xxz_10_5"]
        states = dr.states(capi, L, n_up)
        psi0 = np.zeros(states.size)
        psi0[int(np.searchsorted(states, bits))] = 1.0
        return Case(capi, (L, bonds, hz, hx), n_up, psi0, dr.MINUS, np.eye(L)[4], list(np.eye(L)))
    E0, psi = _ring_ground_state(capi)
    c = momentum_z(10, 2 * np.pi * 3 / 10)
    return Case(capi, dr.ring(10), 5, psi, dr.Z, c, [c], eigen_energy=E0 if name == "ring eigen" else None)


def excess(case_):
    """the restatement's own rounding error: the largest excess of its error over its own bound, over the eight calls at
    tol = 1e-13 (0 if it stays inside)"""
    r = case_.restatement(M, 1e-13)
    worst = 0.0
    for k in range(CALLS):
        r.evolve(DT)
        worst = max(worst, float(np.max(np.abs(r.values() - case_.dense_values(DT * (k + 1))) - r.bounds())))
    return max(worst, 0.0)
