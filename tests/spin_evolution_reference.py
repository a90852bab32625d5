"""numpy restatements for complex spin states and their time evolution, independent of csrc/ and of spin_evolution.hpp.

1. measure_z / check_z: the Hermitian spin measurement (include/eigenex_hip.h: eigenex_spin_measure on a complex state,
   eigenex_spin_measure_host_z) of a complex128 vector, every sum and the sum of its terms' magnitudes in np.longdouble.  The
   bound is that of tests/spin_measure_reference.py: a sum of N terms accumulated one fma at a time, in any grouping, is within
   (N - 1) u sum |terms| of the exact sum to first order, u = eps / 2.  A complex row has two terms per sum (real parts,
   imaginary parts), N = 2 rows, so the bound is rows * eps * sum |terms| -- the same expression as for the real vector.

2. KrylovPropagator: the algorithm of SpinTimeEvolutionSolver restated on a dense Hermitian matrix -- m Lanczos steps with full
   re-orthogonalisation from the normalised state, T_m = S theta S^T (numpy.linalg.eigh), c(tau) = S exp(-i tau theta) S^T e_1,
   psi <- V c; the error bound B(tau) = beta_m int_0^tau |[exp(-i s T_m)]_{m,1}| ds by the composite Simpson rule with 512
   panels; the largest tau <= remaining with B(tau) <= tol tau / |dt|, by exactly 60 halvings where the whole remainder does not
   pass; a breakdown (beta <= 1e-12, or m at least the dimension) makes the step exact.

3. dense_propagate: exp(-i H t) psi through numpy.linalg.eigh of H, the reference of the quench tests; models and start states
   of those tests; floor(): the rounding error of the restatement itself, its distance from the dense exponential when run at
   tol = 1e-13.

Shared by tests/test_spin_complex_host.py, tests/test_gpu_spin_complex.py and tests/test_gpu_spin_evolution.py."""
from __future__ import annotations

import functools

import numpy as np
import spin_measure_reference as mr
import spin_reference as sr
import spin_sector_reference as ss

EPS = np.finfo(np.float64).eps
LD = np.longdouble
QUAD_PANELS = 512
BISECTIONS = 60
BREAKDOWN = 1e-12


def vector_z(n_sites, n_up, seed=None):
    rs = np.random.RandomState(5000 + 1000 * n_sites + (77 if n_up is None else n_up) if seed is None else seed)
    n = mr.rows(n_sites, n_up)
    return rs.standard_normal(n) + 1j * rs.standard_normal(n)


def measure_z(n_sites, n_up, x, diag_masks, flip_masks):
    """(diag, flip, norm2) and the sums of magnitudes (diag_abs, flip_abs, norm_abs), all np.longdouble"""
    st = mr.states(n_sites, n_up)
    x = np.asarray(x, np.complex128)
    xr, xi = x.real.astype(LD), x.imag.astype(LD)
    assert xr.size == st.size
    x2 = xr * xr + xi * xi
    norm2 = x2.sum(dtype=LD)
    diag, flip, flip_abs = np.zeros(len(diag_masks), LD), np.zeros(len(flip_masks), LD), np.zeros(len(flip_masks), LD)
    for t, m in enumerate(diag_masks):
        diag[t] = (mr._sigma_product(st, int(m)).astype(LD) * x2).sum(dtype=LD)
    for t, m in enumerate(flip_masks):
        m = int(m)
        on = np.ones(st.size, bool) if bin(m).count("1") == 1 else mr._sigma_product(st, m) == -1
        partner = st[on] ^ np.uint64(m)
        idx = partner.astype(np.int64) if n_up is None else ss.rank(st, partner)
        tr, ti = xr[on] * xr[idx], xi[on] * xi[idx]  # Re(conj(a) b) = Re a Re b + Im a Im b
        flip[t], flip_abs[t] = tr.sum(dtype=LD) + ti.sum(dtype=LD), np.abs(tr).sum(dtype=LD) + np.abs(ti).sum(dtype=LD)
    return diag, flip, norm2, np.full(len(diag_masks), norm2, LD), flip_abs, norm2


def check_z(label, n_sites, n_up, x, diag_masks, flip_masks, got, ref=None):
    """assert got = (diag, flip, norm2) within rows * eps * sum |terms| of the restatement; prints the largest error over its bound"""
    ref = measure_z(n_sites, n_up, x, diag_masks, flip_masks) if ref is None else ref
    n = mr.rows(n_sites, n_up)
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


# ---- time evolution ----
def error_integral(theta, S, beta_m, tau):
    """B(tau): composite Simpson, QUAD_PANELS panels, of beta_m |sum_j S[m-1, j] exp(-i s theta_j) S[0, j]|"""
    w = S[-1, :] * S[0, :]
    s = np.linspace(0.0, tau, QUAD_PANELS + 1)
    g = np.abs(np.exp(-1j * np.outer(s, theta)) @ w)
    weights = np.ones(QUAD_PANELS + 1)
    weights[1:-1:2], weights[2:-1:2] = 4.0, 2.0
    return beta_m * float(weights @ g) * (tau / QUAD_PANELS) / 3.0


class KrylovPropagator:
    def __init__(self, H, psi0, m, tol):
        self.H = np.asarray(H)
        self.n = self.H.shape[0]
        self.psi = np.asarray(psi0, np.complex128) / np.linalg.norm(psi0)
        self.m, self.tol = m, tol
        self.applications = 0
        self.bound = 0.0  # of the last evolve()

    def _lanczos(self, m, want_next):
        """V (k columns), alpha[k], beta[k - 1], beta_m or None, breakdown flag"""
        v = self.psi / np.linalg.norm(self.psi)
        V, alpha, beta = [v], [], []
        w = self.H @ v
        self.applications += 1
        alpha.append(float(np.vdot(v, w).real))
        while True:
            k = len(V)
            if k == m and not want_next:
                return np.array(V).T, alpha, beta, None, True
            Vm = np.array(V).T
            w = w - Vm @ (Vm.conj().T @ w)  # full re-orthogonalisation
            b = float(np.linalg.norm(w))
            if b <= BREAKDOWN:
                return Vm, alpha, beta, None, True
            if k == m:
                return Vm, alpha, beta, b, False
            beta.append(b)
            v = w / b
            V.append(v)
            w = self.H @ v
            self.applications += 1
            alpha.append(float(np.vdot(v, w).real))

    def _sub_step(self, remaining, total, sign):
        m = min(self.m, self.n)
        V, alpha, beta, beta_m, exact = self._lanczos(m, want_next=m < self.n)
        k = len(alpha)
        T = np.diag(alpha) + np.diag(beta[: k - 1], 1) + np.diag(beta[: k - 1], -1)
        theta, S = np.linalg.eigh(T)
        tau, bound = remaining, 0.0
        if not exact:
            passes = lambda t: (lambda B: (B <= self.tol * t / total, B))(error_integral(theta, S, beta_m, t))
            ok, B = passes(remaining)
            if ok:
                bound = B
            else:
                lo, hi, b_lo = 0.0, remaining, 0.0
                for _ in range(BISECTIONS):
                    mid = 0.5 * (lo + hi)
                    ok, B = passes(mid)
                    if ok:
                        lo, b_lo = mid, B
                    else:
                        hi = mid
                assert lo > 0.0
                tau, bound = lo, b_lo
        c = S @ (np.exp(-1j * sign * tau * theta) * S[0, :])
        self.psi = V @ c
        return tau, bound

    def evolve(self, dt):
        total, sign, remaining, steps = abs(dt), (-1.0 if dt < 0 else 1.0), abs(dt), 0
        self.bound = 0.0
        while remaining > 0.0:
            tau, bound = self._sub_step(remaining, total, sign)
            self.bound += bound
            remaining = 0.0 if tau >= remaining else remaining - tau
            steps += 1
        return steps


class Dense:
    """exp(-i H t) psi through the eigendecomposition of the dense Hermitian H"""

    def __init__(self, H):
        self.H = np.asarray(H, np.float64)
        self.lam, self.U = np.linalg.eigh(self.H)

    def propagate(self, psi0, t):
        return self.U @ (np.exp(-1j * self.lam * t) * (self.U.conj().T @ np.asarray(psi0, np.complex128)))


# the quenches of tests/test_gpu_spin_evolution.py: name -> (n_sites, n_up, bonds, hz, hx, product state bits)
def neel(L):
    return sum(1 << i for i in range(0, L, 2))


QUENCHES = {
    "neel_xxz_10_5": (10, 5, sr.chain(10, 0.6, 1.0), None, None, neel(10)),
    "all_up_ising_8": (8, None, sr.chain(8, 1.0, 0.0), None, np.full(8, 0.9), (1 << 8) - 1),
}
QUENCH_CALLS, QUENCH_DT, QUENCH_M, QUENCH_TOL = 8, 0.25, 12, 1e-9


@functools.lru_cache(maxsize=None)
def quench_reference(name):
    """(H dense, psi0, [psi_dense after call 1..8]) of one quench"""
    L, n_up, bonds, hz, hx, bits = QUENCHES[name]
    H = sr.dense_kron(L, bonds, hz, hx) if n_up is None else ss.dense(L, n_up, bonds, hz)
    psi0 = np.zeros(H.shape[0], np.complex128)
    psi0[bits if n_up is None else int(np.searchsorted(mr.states(L, n_up), bits))] = 1.0
    d = Dense(H)
    return H, psi0, [d.propagate(psi0, QUENCH_DT * (k + 1)) for k in range(QUENCH_CALLS)]


@functools.lru_cache(maxsize=None)
def quench_floor(name):
    """the restatement's own rounding error: its largest distance from the dense exponential over the eight calls at tol = 1e-13"""
    H, psi0, dense = quench_reference(name)
    p = KrylovPropagator(H, psi0, QUENCH_M, 1e-13)
    worst = 0.0
    for k in range(QUENCH_CALLS):
        p.evolve(QUENCH_DT)
        worst = max(worst, float(np.linalg.norm(p.psi - dense[k])))
    return worst


# the invariants test at (20,10) takes its bound from the restatement's drift on (12,6)
INVARIANT_SMALL = (12, 6, sr.chain(12, 0.6, 1.0, periodic=True) + [(2, 9, 0.3, 0.4)], np.linspace(-0.5, 0.5, 12))
INVARIANT_M, INVARIANT_DT, INVARIANT_TOL = 20, 0.5, 1e-10


@functools.lru_cache(maxsize=None)
def invariant_drift():
    """(|<psi|psi> - 1|, |E(t) - E(0)|, floor, operator applications) of the restatement on (12,6): evolve(0.5) from the Neel state at
    m = 20; floor is its distance from the dense exponential"""
    L, n_up, bonds, hz = INVARIANT_SMALL
    H = ss.dense(L, n_up, bonds, hz)
    psi0 = np.zeros(H.shape[0], np.complex128)
    psi0[int(np.searchsorted(mr.states(L, n_up), neel(L)))] = 1.0
    p = KrylovPropagator(H, psi0, INVARIANT_M, INVARIANT_TOL)
    e0 = float(np.vdot(psi0, H @ psi0).real)
    p.evolve(INVARIANT_DT)
    n2 = float(np.vdot(p.psi, p.psi).real)
    e1 = float(np.vdot(p.psi, H @ p.psi).real) / n2
    floor = max(float(np.linalg.norm(p.psi - Dense(H).propagate(psi0, INVARIANT_DT))) - p.bound, 0.0)
    return abs(n2 - 1.0), abs(e1 - e0), floor, p.applications
