"""ctypes view of libeigenex_solver.so: the flat C wrapper (csrc/solver_capi.cpp) around the
header-only C++ solver classes LanczosEigenSolver<S> / ArnoldiEigenSolver<S>, S = double or
std::complex<double> (cmpt-eigenex_amd/include/cmpt/eigen_ex/).  Plumbing for tests/ and
bench.py: the Python side holds no algorithm, the method names mirror the C++ (= reference) names.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import capi

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libeigenex_solver.so")
_dp = C.POINTER(C.c_double)
_lp = C.POINTER(C.c_int64)
_vp = C.c_void_p

UNLIMITED = -1
INFO = {0: "Success", 1: "NumericalIssue", 2: "NoConvergence", 3: "InvalidInput"}
FAMILIES = ("lanczos", "zlanczos", "arnoldi", "zarnoldi")

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        capi.lib()  # libeigenex_hip.so first (RTLD_GLOBAL)
        if not os.path.exists(LIB_PATH):
            raise capi.EigenexError(f"{LIB_PATH} is missing: run `python -m cmpt_eigenex_amd.build`")
        L = C.CDLL(LIB_PATH)
        L.eigenex_solver_last_error.restype = C.c_char_p
        L.eigenex_solver_default_start_vector.argtypes = [C.c_int64, _dp]
        L.eigenex_solver_random_vector.argtypes = [C.c_uint32, C.c_int64, _dp]
        L.eigenex_solver_random_vector_z.argtypes = [C.c_uint32, C.c_int64, _dp]
        L.eigenex_solver_stl_normal.argtypes = [C.c_uint32, C.c_int64, _dp]
        L.eigenex_solver_random_csr.argtypes = [C.c_int64, C.c_int, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp]
        L.eigenex_solver_tridiagonal_eigen.argtypes = [C.c_int, _dp, _dp, _dp, _dp]
        L.eigenex_solver_hessenberg_eigen.argtypes = [C.c_int, _dp, _dp, _dp]
        L.eigenex_solver_symmetric_eigen.argtypes = [C.c_int, _dp, _dp, _dp]
        L.eigenex_solver_hessenberg_values_real.argtypes = [C.c_int, _dp, _dp]
        _ip32 = C.POINTER(C.c_int32)
        L.eigenex_solver_triplets_to_csr.argtypes = [C.c_int64, C.c_int64, _lp, _lp, _dp, C.c_int, _ip32, _ip32, _dp, _lp]
        L.eigenex_solver_gershgorin_range.argtypes = [C.c_int64, C.c_int64, _lp, _lp, _dp, C.c_int, _dp]
        L.eigenex_solver_blocks_to_csr.argtypes = [C.c_int, _lp, C.c_int, _lp, C.c_int, _lp, _lp, _dp, _ip32, _ip32, _dp, _lp]
        L.eigenex_solver_krylov_schur_basis.argtypes = [C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int), _dp, _dp, _dp]
        L.eigenex_solver_chebyshev_delta.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, _dp]
        for kind in ("trlanczos", "ztrlanczos", "kschur", "zkschur", "flanczos", "zflanczos"):
            p = f"eigenex_{kind}_solver_"
            getattr(L, p + "create").restype = _vp
            getattr(L, p + "destroy").argtypes = [_vp]
            getattr(L, p + "destroy").restype = None
            getattr(L, p + "set_device_operator").argtypes = [_vp, _vp, _vp]
            getattr(L, p + "set_host_operator").argtypes = [_vp, _vp, capi.MATVEC_FN, _vp, C.c_int64]
            getattr(L, p + "set").argtypes = [_vp, C.c_char_p, C.c_double, C.c_double]
            getattr(L, p + "set_initial_vector").argtypes = [_vp, _dp, C.c_int64]
            getattr(L, p + "compute").argtypes = [_vp]
            getattr(L, p + "sizes").argtypes = [_vp, _lp]
            getattr(L, p + "get").argtypes = [_vp, _dp, _dp, _dp]
            getattr(L, p + "log_line").argtypes = [_vp, C.c_int64]
            getattr(L, p + "log_line").restype = C.c_char_p
        L.eigenex_solver_jackson_factors.argtypes = [C.c_int, _dp]
        L.eigenex_solver_kpm_density.argtypes = [_dp, C.c_int, C.c_double, C.c_double, _dp, C.c_int64, _dp]
        L.eigenex_solver_kpm_count.argtypes = [_dp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _dp]
        L.eigenex_solver_kpm_window.argtypes = [_dp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _dp]
        for kind in ("density", "zdensity"):
            p = f"eigenex_{kind}_solver_"
            getattr(L, p + "create").restype = _vp
            getattr(L, p + "destroy").argtypes = [_vp]
            getattr(L, p + "destroy").restype = None
            getattr(L, p + "set_device_operator").argtypes = [_vp, _vp, _vp]
            getattr(L, p + "set").argtypes = [_vp, C.c_char_p, C.c_double, C.c_double]
            getattr(L, p + "set_seed").argtypes = [_vp, C.c_uint64]
            getattr(L, p + "set_initial_vector").argtypes = [_vp, _dp, C.c_int64]
            getattr(L, p + "compute").argtypes = [_vp]
            getattr(L, p + "continue").argtypes = [_vp]
            getattr(L, p + "sizes").argtypes = [_vp, _lp]
            getattr(L, p + "get").argtypes = [_vp, _dp, _dp, _dp, _dp]
            getattr(L, p + "density").argtypes = [_vp, _dp, C.c_int64, _dp]
            getattr(L, p + "eigenvalue_count").argtypes = [_vp, C.c_double, C.c_double, _dp, _dp]
            getattr(L, p + "energy_window").argtypes = [_vp, C.c_double, C.c_double, _dp]
            getattr(L, p + "log_line").argtypes = [_vp, C.c_int64]
            getattr(L, p + "log_line").restype = C.c_char_p
        _up32 = C.POINTER(C.c_uint32)
        for kind in ("thermal", "zthermal"):
            p = f"eigenex_{kind}_solver_"
            getattr(L, p + "create").restype = _vp
            getattr(L, p + "destroy").argtypes = [_vp]
            getattr(L, p + "destroy").restype = None
            getattr(L, p + "set_device_operator").argtypes = [_vp, _vp, _vp]
            getattr(L, p + "set").argtypes = [_vp, C.c_char_p, C.c_double, C.c_double]
            getattr(L, p + "set_seed").argtypes = [_vp, C.c_uint64, C.c_uint64]
            getattr(L, p + "set_sample_vectors").argtypes = [_vp, _dp, C.c_int64, C.c_int64]
            getattr(L, p + "set_spin_observables").argtypes = [_vp, C.c_int, _up32, C.c_int, _up32, C.POINTER(C.c_int)]
            getattr(L, p + "compute").argtypes = [_vp]
            getattr(L, p + "sizes").argtypes = [_vp, _lp]
            getattr(L, p + "value").argtypes = [_vp, C.c_int, C.c_int64, C.c_double, _dp, _dp]
            getattr(L, p + "correlation").argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_double, _dp]
            getattr(L, p + "sample").argtypes = [_vp, C.c_int64, _lp, _dp, _dp]
            getattr(L, p + "add_to_ensemble").argtypes = [_vp, _vp, C.c_double, C.c_double]
            getattr(L, p + "log_line").argtypes = [_vp, C.c_int64]
            getattr(L, p + "log_line").restype = C.c_char_p
        L.eigenex_thermal_ensemble_create.argtypes = [C.c_int]
        L.eigenex_thermal_ensemble_create.restype = _vp
        L.eigenex_thermal_ensemble_destroy.argtypes = [_vp]
        L.eigenex_thermal_ensemble_destroy.restype = None
        L.eigenex_thermal_ensemble_value.argtypes = [_vp, C.c_int, C.c_int64, C.c_double, _dp]
        _ip32 = C.POINTER(C.c_int32)
        p = "eigenex_spin_momentum_dynamics_solver_"
        getattr(L, p + "set_model").argtypes = [_vp, _vp, C.c_int, C.c_int, _ip32, _ip32, _dp, _dp, _dp, C.c_int, C.c_int, C.c_int]
        getattr(L, p + "set_state").argtypes = [_vp, _dp, C.c_int64, C.c_int]
        getattr(L, p + "set_state_energy").argtypes = [_vp, C.c_double]
        getattr(L, p + "set_site_operator").argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, C.c_int]
        getattr(L, p + "set_lanczos_steps").argtypes = [_vp, C.c_int64]
        getattr(L, p + "compute").argtypes = [_vp]
        getattr(L, p + "compute_structure_factor_z").argtypes = [_vp, C.c_int]
        getattr(L, p + "sizes").argtypes = [_vp, _lp]
        getattr(L, p + "get").argtypes = [_vp, _dp, _dp, _dp, _dp, _dp]
        getattr(L, p + "spectrum").argtypes = [_vp, _dp, C.c_int64, C.c_double, _dp]
        getattr(L, p + "moment").argtypes = [_vp, C.c_int, _dp]
        for kind in ("dynamics", "momentum_dynamics", "evolution", "time_correlation", "entanglement"):
            p = f"eigenex_spin_{kind}_solver_"
            getattr(L, p + "create").argtypes = []
            getattr(L, p + "create").restype = _vp
            getattr(L, p + "destroy").argtypes = [_vp]
            getattr(L, p + "destroy").restype = None
            getattr(L, p + "log_line").argtypes = [_vp, C.c_int64]
            getattr(L, p + "log_line").restype = C.c_char_p
        for kind in ("dynamics", "evolution", "time_correlation"):
            p = f"eigenex_spin_{kind}_solver_"
            getattr(L, p + "set_model").argtypes = [_vp, _vp, C.c_int, C.c_int, _ip32, _ip32, _dp, _dp, _dp, _dp, C.c_int]
        for kind in ("evolution", "time_correlation"):
            p = f"eigenex_spin_{kind}_solver_"
            getattr(L, p + "set_state").argtypes = [_vp, _dp, C.c_int64, C.c_int]
            getattr(L, p + "set_product_state").argtypes = [_vp, C.c_uint32]
            getattr(L, p + "set_krylov_dimension").argtypes = [_vp, C.c_int64]
            getattr(L, p + "set_tolerance").argtypes = [_vp, C.c_double]
            getattr(L, p + "evolve").argtypes = [_vp, C.c_double, _lp]
            getattr(L, p + "status").argtypes = [_vp, _dp, _lp]
            getattr(L, p + "fetch").argtypes = [_vp, _dp]
        p = "eigenex_spin_dynamics_solver_"
        getattr(L, p + "set_state").argtypes = [_vp, _dp, C.c_int64]
        getattr(L, p + "set_state_energy").argtypes = [_vp, C.c_double]
        getattr(L, p + "set_site_operator").argtypes = [_vp, C.c_int, _dp, C.c_int]
        getattr(L, p + "set_lanczos_steps").argtypes = [_vp, C.c_int64]
        getattr(L, p + "compute").argtypes = [_vp]
        getattr(L, p + "compute_structure_factor_z").argtypes = [_vp, C.c_double]
        getattr(L, p + "compute_structure_factor_z_single_run").argtypes = [_vp, C.c_double]
        getattr(L, p + "set_state_z").argtypes = [_vp, _dp, C.c_int64]
        getattr(L, p + "set_site_operator_z").argtypes = [_vp, C.c_int, _dp, _dp, C.c_int]
        getattr(L, p + "sizes").argtypes = [_vp, _lp]
        getattr(L, p + "get").argtypes = [_vp, _dp, _dp, _dp, _dp, _dp]
        getattr(L, p + "spectrum").argtypes = [_vp, _dp, C.c_int64, C.c_double, _dp]
        getattr(L, p + "moment").argtypes = [_vp, C.c_int, _dp]
        getattr(L, p + "static_structure_factor_z").argtypes = [_vp, C.c_double, _dp]
        p = "eigenex_spin_evolution_solver_"
        getattr(L, p + "scalar").argtypes = [_vp, C.c_int, _dp]
        getattr(L, p + "measure").argtypes = [_vp, C.c_int, _lp]
        getattr(L, p + "entanglement").argtypes = [_vp, C.c_uint32, _ip32, C.c_int, C.c_int, _lp]
        p = "eigenex_spin_time_correlation_solver_"
        getattr(L, p + "set_eigenstate").argtypes = [_vp, C.c_double]
        getattr(L, p + "set_source_operator").argtypes = [_vp, C.c_int, _dp, C.c_int]
        getattr(L, p + "add_measured_operator").argtypes = [_vp, _dp, C.c_int]
        getattr(L, p + "clear_measured_operators").argtypes = [_vp]
        getattr(L, p + "set_measured_sites").argtypes = [_vp]
        getattr(L, p + "set_momentum_z").argtypes = [_vp, C.c_double]
        getattr(L, p + "values").argtypes = [_vp, _lp]
        getattr(L, p + "operator_bounds").argtypes = [_vp, C.c_int64, _dp]
        p = "eigenex_spin_entanglement_solver_"
        getattr(L, p + "set_device_operator").argtypes = [_vp, _vp, _vp]
        getattr(L, p + "set_state").argtypes = [_vp, _dp, C.c_int64]
        getattr(L, p + "set_subsystem").argtypes = [_vp, _ip32, C.c_int]
        getattr(L, p + "set_subsystem_mask").argtypes = [_vp, C.c_uint32]
        getattr(L, p + "compute").argtypes = [_vp]
        getattr(L, p + "sizes").argtypes = [_vp, _lp]
        getattr(L, p + "block").argtypes = [_vp, C.c_int64, C.POINTER(C.c_int), _lp, _dp]
        getattr(L, p + "set_state_z").argtypes = [_vp, _dp, C.c_int64]
        getattr(L, p + "block_z").argtypes = [_vp, C.c_int64, C.POINTER(C.c_int), _dp]
        getattr(L, p + "get").argtypes = [_vp, _dp, _dp]
        getattr(L, p + "renyi").argtypes = [_vp, C.c_double, _dp]
        getattr(L, p + "schmidt_rank").argtypes = [_vp, C.c_double, _lp]
        for kind in FAMILIES:
            p = f"eigenex_{kind}_solver_"
            getattr(L, p + "create").restype = _vp
            getattr(L, p + "destroy").argtypes = [_vp]
            getattr(L, p + "destroy").restype = None
            getattr(L, p + "set_device_operator").argtypes = [_vp, _vp, _vp]
            getattr(L, p + "set_host_operator").argtypes = [_vp, _vp, capi.MATVEC_FN, _vp, C.c_int64]
            getattr(L, p + "set").argtypes = [_vp, C.c_char_p, C.c_double, C.c_double]
            getattr(L, p + "set_indices_for_convergence").argtypes = [_vp, _lp, C.c_int]
            getattr(L, p + "set_initial_vector").argtypes = [_vp, _dp, C.c_int64]
            getattr(L, p + "set_orthogonalizing_vectors").argtypes = [_vp, _dp, C.c_int64, C.c_int]
            getattr(L, p + "compute").argtypes = [_vp]
            getattr(L, p + "continue").argtypes = [_vp]
            getattr(L, p + "sizes").argtypes = [_vp, _lp]
            getattr(L, p + "log_line").argtypes = [_vp, C.c_int64]
            getattr(L, p + "log_line").restype = C.c_char_p
        for kind in ("lanczos", "zlanczos"):
            p = f"eigenex_{kind}_solver_"
            getattr(L, p + "get").argtypes = [_vp, _dp, _dp, _dp, _dp]
            getattr(L, p + "lanczosvector").argtypes = [_vp, C.c_int64, _dp]
            getattr(L, p + "convergence_log").argtypes = [_vp, C.c_int64, _dp, C.c_int64]
            getattr(L, p + "convergence_log").restype = C.c_int64
            getattr(L, p + "exp_with_lanczos").argtypes = [_vp, C.c_double, C.c_double, _dp]
            getattr(L, p + "function_of").argtypes = [_vp, C.c_int, C.c_double, C.c_double, _dp]
        L.eigenex_solver_exp_eigens.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int64, C.c_int64, _dp, _dp, C.c_int64, _dp, _dp]
        L.eigenex_solver_exp_taylor.argtypes = [C.c_int, _vp, _vp, capi.MATVEC_FN, _vp, C.c_int64, C.c_double, C.c_double, C.c_double,
                                                _dp, C.c_int64, _dp, C.c_double, C.c_int64, C.c_int]
        for kind in ("arnoldi", "zarnoldi"):
            getattr(L, f"eigenex_{kind}_solver_get").argtypes = [_vp, _dp, _dp, _dp, _dp]
            getattr(L, f"eigenex_{kind}_solver_convergence_log").argtypes = [_vp, C.c_int64, _dp, C.c_int64]
            getattr(L, f"eigenex_{kind}_solver_convergence_log").restype = C.c_int64
        _LIB = L
    return _LIB


def _chk(rc):
    if rc != 0:
        raise capi.EigenexError(lib().eigenex_solver_last_error().decode(errors="replace"))


def _d(a):
    return a.ctypes.data_as(_dp)


def default_start_vector(n: int) -> np.ndarray:
    out = np.empty(n)
    _chk(lib().eigenex_solver_default_start_vector(n, _d(out)))
    return out


def random_vector(seed: int, n: int, dtype=np.float64) -> np.ndarray:
    """LanczosBase<S>::makeRandomVector(std::mt19937(seed), n)"""
    if np.dtype(dtype).kind == "c":
        out = np.empty(n, np.complex128)
        _chk(lib().eigenex_solver_random_vector_z(seed, n, _d(out)))
        return out
    out = np.empty(n)
    _chk(lib().eigenex_solver_random_vector(seed, n, _d(out)))
    return out


def stl_normal(seed: int, n: int) -> np.ndarray:
    """n draws of std::normal_distribution<double>(0, 1) from std::mt19937(seed), in order (the host's <random>)"""
    out = np.empty(n)
    _chk(lib().eigenex_solver_stl_normal(seed, n, _d(out)))
    return out


def random_csr(n: int, per: int, seed: int):
    """SURVEY 8d RandomCSR from std::mt19937_64(seed), row by row (columns, then values): rowptr, col (int32), val"""
    rowptr, col, val = np.empty(n + 1, np.int32), np.empty(n * per, np.int32), np.empty(n * per)
    ip = C.POINTER(C.c_int32)
    _chk(lib().eigenex_solver_random_csr(n, per, seed, rowptr.ctypes.data_as(ip), col.ctypes.data_as(ip), _d(val)))
    return rowptr, col, val


def tridiagonal_eigen(diag, sub, vectors=True):
    diag = np.ascontiguousarray(diag, np.float64)
    n = diag.size
    sub = np.ascontiguousarray(np.concatenate([np.asarray(sub, np.float64), np.zeros(1)]))
    vals = np.empty(n)
    vecs = np.empty((n, n)) if vectors else None
    _chk(lib().eigenex_solver_tridiagonal_eigen(n, _d(diag), _d(sub), _d(vals), _d(vecs) if vectors else None))
    return vals, (vecs.T.copy() if vectors else None)  # column-major -> [row, col]


def hessenberg_eigen(H, vectors=True):
    H = np.asfortranarray(H, np.complex128)
    n = H.shape[0]
    vals = np.empty(n, np.complex128)
    vecs = np.empty((n, n), np.complex128, order="F") if vectors else None
    _chk(lib().eigenex_solver_hessenberg_eigen(n, _d(H), _d(vals), _d(vecs) if vectors else None))
    return vals, vecs


def hessenberg_values_real(H):
    """eigenvalues of a real upper-Hessenberg matrix (double-shift QR in real arithmetic)"""
    H = np.asfortranarray(H, np.float64)
    n = H.shape[0]
    vals = np.empty(n, np.complex128)
    _chk(lib().eigenex_solver_hessenberg_values_real(n, _d(H), _d(vals)))
    return vals


def symmetric_eigen(A):
    A = np.asfortranarray(A, np.float64)
    n = A.shape[0]
    vals = np.empty(n)
    vecs = np.empty((n, n), order="F")
    _chk(lib().eigenex_solver_symmetric_eigen(n, _d(A), _d(vals), _d(vecs)))
    return vals, vecs


def krylov_schur_basis(H, keep: int, residue: float):
    """small_eigen::krylov_schur_basis on the projected matrix H (m x m, real or complex; Hessenberg or with a full leading
    block): the restart basis of a Krylov-Schur cycle.  Returns keep (grown by one if a real matrix's conjugate pair would
    have been split), Q (m x keep, orthonormal), B ((keep+1) x keep: Q^H H Q over the row residue * Q[m-1, :]) and all m
    Ritz values, |theta| descending."""
    cplx = bool(np.iscomplexobj(H))
    dt = np.complex128 if cplx else np.float64
    H = np.asfortranarray(H, dt)
    m = H.shape[0]
    Q = np.zeros((m, keep + 1), dt, order="F")
    B = np.zeros((keep + 2) * (keep + 1), dt)
    theta = np.zeros(m, np.complex128)
    k = C.c_int(0)
    _chk(lib().eigenex_solver_krylov_schur_basis(int(cplx), _d(H), m, m, int(keep), float(residue), C.byref(k), _d(Q), _d(B), _d(theta)))
    k = k.value
    return k, Q[:, :k].copy(), B[: (k + 1) * k].reshape((k + 1, k), order="F").copy(), theta


def chebyshev_delta(tau: float, center: float, halfwidth: float, degree: int) -> np.ndarray:
    """chebyshevDeltaCoefficients (filtered_lanczos.hpp): mu[degree + 1] of the Jackson-damped delta peak at tau, p(tau) = 1"""
    mu = np.zeros(int(degree) + 1)
    _chk(lib().eigenex_solver_chebyshev_delta(float(tau), float(center), float(halfwidth), int(degree), _d(mu)))
    return mu


def triplets_to_csr(n, rows, cols, vals):
    """COO -> CSR with the semantics of the reference's TripletsMatrix::shrink (sort, add duplicates, drop zeros)."""
    rows = np.ascontiguousarray(rows, np.int64)
    cols = np.ascontiguousarray(cols, np.int64)
    cplx = np.iscomplexobj(vals)
    vals = np.ascontiguousarray(vals, np.complex128 if cplx else np.float64)
    rowptr = np.zeros(n + 1, np.int32)
    col = np.zeros(max(rows.size, 1), np.int32)
    val = np.zeros(max(rows.size, 1), vals.dtype)
    nnz = C.c_int64()
    _chk(lib().eigenex_solver_triplets_to_csr(n, rows.size, rows.ctypes.data_as(_lp), cols.ctypes.data_as(_lp), _d(vals),
                                              1 if cplx else 0, rowptr.ctypes.data_as(C.POINTER(C.c_int32)),
                                              col.ctypes.data_as(C.POINTER(C.c_int32)), _d(val), C.byref(nnz)))
    return rowptr, col[: nnz.value].copy(), val[: nnz.value].copy()


def blocks_to_csr(row_sizes, col_sizes, blocks):
    """BlockSparseMatrix<double>::toCsr: blocks = {(qr, qc): 2-D array}; duplicates of a block index are added."""
    rs = np.ascontiguousarray(row_sizes, np.int64)
    cs = np.ascontiguousarray(col_sizes, np.int64)
    keys = list(blocks.keys()) if isinstance(blocks, dict) else [k for k, _ in blocks]
    mats = list(blocks.values()) if isinstance(blocks, dict) else [m for _, m in blocks]
    qr = np.array([k[0] for k in keys], np.int64)
    qc = np.array([k[1] for k in keys], np.int64)
    # the C side sizes every block from the partition, so a mismatch here would be an out-of-bounds read
    for (r, c), m in zip(keys, mats):
        if not (0 <= r < rs.size and 0 <= c < cs.size):
            raise ValueError(f"block index ({r}, {c}) out of range")
        if np.shape(m) != (rs[r], cs[c]):
            raise ValueError(f"block ({r}, {c}) has shape {np.shape(m)}, the partition says {(int(rs[r]), int(cs[c]))}")
    vals = np.concatenate([np.asfortranarray(m, np.float64).ravel(order="F") for m in mats]) if mats else np.zeros(0)
    n = int(rs.sum())
    rowptr = np.zeros(n + 1, np.int32)
    col = np.zeros(max(vals.size, 1), np.int32)
    val = np.zeros(max(vals.size, 1))
    nnz = C.c_int64()
    i32 = C.POINTER(C.c_int32)
    _chk(lib().eigenex_solver_blocks_to_csr(rs.size, rs.ctypes.data_as(_lp), cs.size, cs.ctypes.data_as(_lp), len(keys),
                                            qr.ctypes.data_as(_lp), qc.ctypes.data_as(_lp), _d(vals), rowptr.ctypes.data_as(i32),
                                            col.ctypes.data_as(i32), _d(val), C.byref(nnz)))
    return rowptr, col[: nnz.value].copy(), val[: nnz.value].copy()


def exp_with_eigens(x, eivals, eivecs, max_expand, vin):
    """LanczosExponentialSolver::solveWithEigens on explicit host eigenpairs (vector arithmetic on the GPU)."""
    X = np.asfortranarray(eivecs)
    cplx = np.iscomplexobj(X) or np.iscomplexobj(vin) or complex(x).imag != 0.0
    dt = np.complex128 if cplx else np.float64
    X = np.asfortranarray(X, dt)
    v = np.ascontiguousarray(vin, dt)
    ev = np.ascontiguousarray(eivals, np.float64)
    out = np.zeros(v.size, dt)
    z = complex(x)
    _chk(lib().eigenex_solver_exp_eigens(int(cplx), z.real, z.imag, X.shape[0], X.shape[1], _d(ev), _d(X), int(max_expand), _d(v), _d(out)))
    return out


def exp_taylor(x, operator, radius, vin, ctx=None, height=None, error=1.0e-14, max_expansion=-1, auto_division=False, dtype=None):
    """LanczosExponentialSolver::solveWithTaylor{No,Auto}Division.  operator: a capi.Csr (device) or a callable
    x -> A x of `height` rows (host callback); vin / result: the rows this process owns."""
    dt = np.dtype(dtype if dtype is not None else (np.complex128 if (np.iscomplexobj(vin) or complex(x).imag != 0.0) else np.float64))
    cplx = dt.kind == "c"
    v = np.ascontiguousarray(vin, dt)
    out = np.zeros(v.size, dt)
    z = complex(x)
    keep = None
    if isinstance(operator, capi.Csr):
        assert bool(getattr(operator, "is_complex", False)) == cplx, "scalar type of operator and vector differ"
        c, csr, cb, h = operator.ctx, operator.h, capi.MATVEC_FN(0), 0
    else:
        n, es = int(height), (2 if cplx else 1)

        def tramp(pin, pout, _user):
            a = np.ctypeslib.as_array(pin, shape=(n * es,)).view(dt)
            b = np.ctypeslib.as_array(pout, shape=(n * es,)).view(dt)
            b[:] = operator(a)

        cb = keep = capi.MATVEC_FN(tramp)
        c = ctx if ctx is not None else capi.Context()
        csr, h = None, n
    _chk(lib().eigenex_solver_exp_taylor(int(cplx), c.h, csr, cb, None, h, z.real, z.imag, float(radius), _d(v), v.size, _d(out),
                                         float(error), int(max_expansion), int(bool(auto_division))))
    del keep
    return out


def gershgorin_range(n, rows, cols, vals):
    rows = np.ascontiguousarray(rows, np.int64)
    cols = np.ascontiguousarray(cols, np.int64)
    cplx = np.iscomplexobj(vals)
    vals = np.ascontiguousarray(vals, np.complex128 if cplx else np.float64)
    out = np.zeros(2)
    _chk(lib().eigenex_solver_gershgorin_range(n, rows.size, rows.ctypes.data_as(_lp), cols.ctypes.data_as(_lp), _d(vals),
                                               1 if cplx else 0, _d(out)))
    return out[0], out[1]


def jackson_factors(M: int) -> np.ndarray:
    """g_0..g_{M-1} of the Jackson kernel (jacksonFactor, filtered_lanczos.hpp)"""
    g = np.zeros(M)
    _chk(lib().eigenex_solver_jackson_factors(M, _d(g)))
    return g


def kpm_density(mu, center, halfwidth, E) -> np.ndarray:
    """kpmDensity (spectral_density.hpp) of normalised moments mu at the energies E"""
    mu, E = np.ascontiguousarray(mu, np.float64), np.ascontiguousarray(np.atleast_1d(E), np.float64)
    out = np.zeros(E.size)
    _chk(lib().eigenex_solver_kpm_density(_d(mu), mu.size, center, halfwidth, _d(E), E.size, _d(out)))
    return out


def kpm_count(mu, center, halfwidth, a, b, N) -> float:
    mu = np.ascontiguousarray(mu, np.float64)
    out = C.c_double()
    _chk(lib().eigenex_solver_kpm_count(_d(mu), mu.size, center, halfwidth, a, b, N, C.byref(out)))
    return out.value


def kpm_window(mu, center, halfwidth, tau, count, N) -> float:
    mu = np.ascontiguousarray(mu, np.float64)
    out = C.c_double()
    _chk(lib().eigenex_solver_kpm_window(_d(mu), mu.size, center, halfwidth, tau, count, N, C.byref(out)))
    return out.value


class _SolverBase:
    _base = ""

    def __init__(self, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.is_complex = self.dtype.kind == "c"
        self._kind = ("z" if self.is_complex else "") + self._base
        self._L = lib()
        self.h = _vp(getattr(self._L, f"eigenex_{self._kind}_solver_create")())
        if not self.h:
            raise capi.EigenexError("solver create failed")
        self._keep = []

    def _f(self, name):
        return getattr(self._L, f"eigenex_{self._kind}_solver_{name}")

    def setDeviceOperator(self, csr: capi.Csr):
        assert bool(getattr(csr, "is_complex", False)) == self.is_complex, "scalar type of solver and operator differ"
        self._keep.append(csr)
        _chk(self._f("set_device_operator")(self.h, csr.ctx.h, csr.h))
        return self

    def setMatrixMultiplication(self, fn, height: int, ctx: capi.Context | None = None):
        """fn(x: ndarray) -> ndarray, the reference's MatMulFunction (called on the host)."""
        n, es, dt = height, (2 if self.is_complex else 1), self.dtype

        def tramp(pin, pout, _user):
            x = np.ctypeslib.as_array(pin, shape=(n * es,)).view(dt)
            y = np.ctypeslib.as_array(pout, shape=(n * es,)).view(dt)
            y[:] = fn(x)

        cb = capi.MATVEC_FN(tramp)
        self._keep += [cb, ctx]
        _chk(self._f("set_host_operator")(self.h, ctx.h if ctx else None, cb, None, height))
        return self

    def set(self, **kw):
        for k, v in kw.items():
            if k == "indicesForConvergence":
                a = np.ascontiguousarray(v, np.int64)
                _chk(self._f("set_indices_for_convergence")(self.h, a.ctypes.data_as(_lp), a.size))
            elif k == "initialVector":
                a = np.ascontiguousarray(v, self.dtype)
                _chk(self._f("set_initial_vector")(self.h, _d(a), a.size))
            elif k == "orthogonalizingVectors":
                a = np.ascontiguousarray(np.stack(v), self.dtype) if len(v) else np.zeros((0, 1), self.dtype)
                _chk(self._f("set_orthogonalizing_vectors")(self.h, _d(a), a.shape[1], a.shape[0]))
            else:
                z = complex(v)
                _chk(self._f("set")(self.h, k.encode(), z.real, z.imag))
        return self

    def compute(self):
        _chk(self._f("compute")(self.h))
        return self

    def continueToCompute(self):
        _chk(self._f("continue")(self.h))
        return self

    def log(self):
        n = self._sizes()["nlog"]
        return [self._f("log_line")(self.h, i).decode() for i in range(n)]

    def close(self):
        if self.h:
            self._f("destroy")(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LanczosEigenSolver(_SolverBase):
    """LanczosEigenSolver<double> (dtype float64) or LanczosEigenSolver<std::complex<double>> (complex128)."""

    _base = "lanczos"
    _names = ("iterations", "nvec", "nalpha", "nbeta", "neig", "vec_rows", "vec_cols", "nlog", "info", "hasWARN", "hasERROR")

    def _sizes(self):
        out = np.zeros(len(self._names), np.int64)
        _chk(self._f("sizes")(self.h, out.ctypes.data_as(_lp)))
        return dict(zip(self._names, (int(x) for x in out)))

    def results(self):
        s = self._sizes()
        alpha, beta, ev = np.zeros(s["nalpha"]), np.zeros(s["nbeta"]), np.zeros(s["neig"])
        X = np.zeros((s["vec_rows"], s["vec_cols"]), self.dtype, order="F")
        _chk(self._f("get")(self.h, _d(alpha), _d(beta), _d(ev), _d(X) if X.size else None))
        s.update(alpha=alpha, beta=beta, eigenvalues=ev, eigenvectors=X, info_name=INFO[s["info"]])
        return s

    def lanczosvector(self, k: int, n_rows: int):
        out = np.empty(n_rows, self.dtype)
        _chk(self._f("lanczosvector")(self.h, k, _d(out)))
        return out

    def expWithLanczos(self, x, n_rows: int):
        """LanczosExponentialSolver::solveWithLanczos(x, *this, out): runs compute(), returns exp(xA)|initialVector>
        (the rows this process owns: n_rows of them)."""
        out = np.zeros(n_rows, self.dtype)
        z = complex(x)
        _chk(self._f("exp_with_lanczos")(self.h, z.real, z.imag, _d(out)))
        return out

    def functionOf(self, kind: int, a, n_rows: int):
        """LanczosFunctionSolver::solve(f, *this) on an already computed solver; f by kind: 0 exp(a t), 1 1/(t - a), 2 t^2 + a."""
        out = np.zeros(n_rows, self.dtype)
        z = complex(a)
        _chk(self._f("function_of")(self.h, kind, z.real, z.imag, _d(out)))
        return out

    def convergenceLog(self, index: int):
        buf = np.zeros(1 << 16)
        n = self._f("convergence_log")(self.h, index, _d(buf), buf.size)
        return buf[:n].copy()


class ArnoldiEigenSolver(_SolverBase):
    """ArnoldiEigenSolver<double> or ArnoldiEigenSolver<std::complex<double>>."""

    _base = "arnoldi"
    _names = ("iterations", "nvec", "hess_rows", "neig", "vec_rows", "vec_cols", "nlog", "info", "hasWARN", "hasERROR")

    def _sizes(self):
        out = np.zeros(len(self._names), np.int64)
        _chk(self._f("sizes")(self.h, out.ctypes.data_as(_lp)))
        return dict(zip(self._names, (int(x) for x in out)))

    def convergenceLog(self, index: int):
        buf = np.zeros(1 << 16, np.complex128)
        n = self._f("convergence_log")(self.h, index, _d(buf), buf.size)
        return buf[:n].copy()

    def results(self):
        s = self._sizes()
        m = s["hess_rows"]
        H = np.zeros((m, m), self.dtype, order="F")
        ev = np.zeros(s["neig"], np.complex128)
        X = np.zeros((s["vec_rows"], s["vec_cols"]), np.complex128, order="F")
        res = C.c_double()
        _chk(self._f("get")(self.h, _d(H) if H.size else None, _d(ev), _d(X) if X.size else None, C.byref(res)))
        s.update(hessenberg=H, eigenvalues=ev, eigenvectors=X, residue=res.value, info_name=INFO[s["info"]])
        return s


class ThickRestartLanczosEigenSolver(_SolverBase):
    """ThickRestartLanczosEigenSolver<S> (thick_restart_lanczos.hpp): lowest eigenpairs with bounded memory."""

    _base = "trlanczos"
    _names = ("neig", "vec_rows", "vec_cols", "restarts", "operatorApplications", "nlog", "info")

    def _sizes(self):
        out = np.zeros(len(self._names), np.int64)
        _chk(self._f("sizes")(self.h, out.ctypes.data_as(_lp)))
        return dict(zip(self._names, (int(x) for x in out)))

    def results(self):
        s = self._sizes()
        ev, res = np.zeros(s["neig"]), np.zeros(s["neig"])
        X = np.zeros((s["vec_rows"], s["vec_cols"]), self.dtype, order="F")
        _chk(self._f("get")(self.h, _d(ev), _d(res), _d(X) if X.size else None))
        s.update(eigenvalues=ev, residuals=res, eigenvectors=X, info_name=INFO[s["info"]])
        return s


class FilteredLanczosEigenSolver(ThickRestartLanczosEigenSolver):
    """FilteredLanczosEigenSolver<S> (filtered_lanczos.hpp): the eigenpairs of a Hermitian device operator nearest
    `target`, by thick-restart Lanczos on a Chebyshev delta filter of the operator.  Settings of the thick-restart solver
    plus target, filterDegree and spectralRange=(lo, hi) (required).  residuals are the true ||A x - lambda x||."""

    _base = "flanczos"

    def set(self, **kw):
        if "spectralRange" in kw:
            lo, hi = kw.pop("spectralRange")
            _chk(self._f("set")(self.h, b"spectralRange", float(lo), float(hi)))
        return super().set(**kw)


class KrylovSchurEigenSolver(_SolverBase):
    """KrylovSchurEigenSolver<S> (krylov_schur.hpp): eigenvalues of largest magnitude of a general operator from a basis of
    fixed size (thick-restart Arnoldi).  Eigenvalues and eigenvectors are complex for either scalar type."""

    _base = "kschur"
    _names = ("neig", "vec_rows", "vec_cols", "restarts", "operatorApplications", "nlog", "info")

    def _sizes(self):
        out = np.zeros(len(self._names), np.int64)
        _chk(self._f("sizes")(self.h, out.ctypes.data_as(_lp)))
        return dict(zip(self._names, (int(x) for x in out)))

    def results(self):
        s = self._sizes()
        ev, res = np.zeros(s["neig"], np.complex128), np.zeros(s["neig"])
        X = np.zeros((s["vec_rows"], s["vec_cols"]), np.complex128, order="F")
        _chk(self._f("get")(self.h, _d(ev), _d(res), _d(X) if X.size else None))
        s.update(eigenvalues=ev, residuals=res, eigenvectors=X, info_name=INFO[s["info"]])
        return s


class SpectralDensitySolver(_SolverBase):
    """SpectralDensitySolver<S> (spectral_density.hpp): Chebyshev moments of a Hermitian device operator by the kernel
    polynomial method, and from them the Jackson-damped density of states, eigenvalue counts of energy windows and the
    window that holds a wanted number of levels.  Settings: spectralRange=(lo, hi) (required), moments, randomVectors, seed,
    initialVector (the local density of that vector instead; None returns to random vectors)."""

    _base = "density"
    _names = ("nmoments", "nvectors", "operatorApplications", "nlog", "info")

    def set(self, **kw):
        for k, v in kw.items():
            if k == "spectralRange":
                _chk(self._f("set")(self.h, b"spectralRange", float(v[0]), float(v[1])))
            elif k == "seed":
                _chk(self._f("set_seed")(self.h, int(v)))
            elif k == "initialVector":
                if v is None:
                    _chk(self._f("set_initial_vector")(self.h, None, 0))
                else:
                    a = np.ascontiguousarray(v, self.dtype)
                    _chk(self._f("set_initial_vector")(self.h, _d(a), a.size))
            else:
                _chk(self._f("set")(self.h, k.encode(), float(v), 0.0))
        return self

    def _sizes(self):
        out = np.zeros(len(self._names), np.int64)
        _chk(self._f("sizes")(self.h, out.ctypes.data_as(_lp)))
        return dict(zip(self._names, (int(x) for x in out)))

    def results(self):
        s = self._sizes()
        M, R = s["nmoments"], s["nvectors"]
        mean, se, each, rng = np.zeros(M), np.zeros(M), np.zeros((R, M)), np.zeros(2)
        _chk(self._f("get")(self.h, _d(mean), _d(se), _d(each) if each.size else None, _d(rng)))
        s.update(moments=mean, momentsStandardError=se, momentsOfEachVector=each, center=rng[0], halfwidth=rng[1], info_name=INFO[s["info"]])
        return s

    def density(self, E):
        E = np.ascontiguousarray(np.atleast_1d(E), np.float64)
        out = np.zeros(E.size)
        _chk(self._f("density")(self.h, _d(E), E.size, _d(out)))
        return out

    def eigenvalueCount(self, a, b):
        c = C.c_double()
        _chk(self._f("eigenvalue_count")(self.h, a, b, C.byref(c), None))
        return c.value

    def eigenvalueCountStandardError(self, a, b):
        e = C.c_double()
        _chk(self._f("eigenvalue_count")(self.h, a, b, None, C.byref(e)))
        return e.value

    def energyWindow(self, tau, count):
        d = C.c_double()
        _chk(self._f("energy_window")(self.h, tau, count, C.byref(d)))
        return d.value


class ThermalLanczosSolver(_SolverBase):
    """ThermalLanczosSolver<S> (thermal_lanczos.hpp): the finite-temperature Lanczos method on one Hermitian device operator --
    log Z, E, C, S, F from R runs of M steps, and thermal averages of spin observables (real states of matrix-free spin operators)
    through eigenex_spin_measure_columns.  Settings: lanczosSteps, randomVectors, seed, firstStream; setSampleVectors for explicit
    start vectors; setSpinObservables / setAllSitesAndPairs for the observables (they return the ComputationInfo's name)."""

    _base = "thermal"
    _names = ("dimension", "samples", "operatorApplications", "nlog", "info", "ndiag", "nflip", "sites")
    QUANTITIES = ("logPartitionFunction", "energy", "specificHeat", "entropy", "freeEnergy", "observable")

    def __init__(self, dtype=np.float64):
        super().__init__(dtype)
        self._seed = [0, 0]

    def set(self, **kw):
        for k, v in kw.items():
            if k in ("seed", "firstStream"):
                self._seed[k == "firstStream"] = int(v)
                _chk(self._f("set_seed")(self.h, *self._seed))
            else:
                _chk(self._f("set")(self.h, k.encode(), float(v), 0.0))
        return self

    def setSampleVectors(self, vectors):
        """vectors: (R, N), one start vector per row; None returns to random sign vectors"""
        if vectors is None:
            _chk(self._f("set_sample_vectors")(self.h, None, 0, 0))
        else:
            a = np.ascontiguousarray(vectors, self.dtype)
            _chk(self._f("set_sample_vectors")(self.h, _d(a.view(np.float64)), a.shape[1], a.shape[0]))
        return self

    def _observables(self, nd, dp, nf, fp):
        info = C.c_int()
        _chk(self._f("set_spin_observables")(self.h, nd, dp, nf, fp, C.byref(info)))
        return INFO[info.value]

    def setSpinObservables(self, diag_masks, flip_masks):
        u = C.POINTER(C.c_uint32)
        d, f = np.ascontiguousarray(diag_masks, np.uint32).reshape(-1), np.ascontiguousarray(flip_masks, np.uint32).reshape(-1)
        return self._observables(d.size, d.ctypes.data_as(u) if d.size else None, f.size, f.ctypes.data_as(u) if f.size else None)

    def setAllSitesAndPairs(self):
        return self._observables(-1, None, 0, None)

    def _sizes(self):
        out = np.zeros(len(self._names), np.int64)
        _chk(self._f("sizes")(self.h, out.ctypes.data_as(_lp)))
        return dict(zip(self._names, (int(x) for x in out)))

    def results(self):
        s = self._sizes()
        s["info_name"] = INFO[s["info"]]
        return s

    def sample(self, r):
        """(theta, weight) of sample r: the Ritz values of its tridiagonal matrix and their weights in the start vector"""
        n = C.c_int64()
        _chk(self._f("sample")(self.h, r, C.byref(n), None, None))
        th, w = np.zeros(n.value), np.zeros(n.value)
        _chk(self._f("sample")(self.h, r, None, _d(th), _d(w)))
        return th, w

    def _value(self, q, beta, t=0, error=False):
        v = C.c_double()
        _chk(self._f("value")(self.h, q, int(t), float(beta), None if error else C.byref(v), C.byref(v) if error else None))
        return v.value

    def logPartitionFunction(self, beta):
        return self._value(0, beta)

    def energy(self, beta):
        return self._value(1, beta)

    def specificHeat(self, beta):
        return self._value(2, beta)

    def entropy(self, beta):
        return self._value(3, beta)

    def freeEnergy(self, beta):
        return self._value(4, beta)

    def diagonal(self, t, beta):
        s = self._sizes()
        if not 0 <= t < s["ndiag"]:
            raise capi.EigenexError("no such diagonal observable")
        return self._value(5, beta, t)

    def flip(self, t, beta):
        s = self._sizes()
        if not 0 <= t < s["nflip"]:
            raise capi.EigenexError("no such flip observable")
        return self._value(5, beta, s["ndiag"] + t)

    def _correlation(self, kind, i, j, beta):
        v = C.c_double()
        _chk(self._f("correlation")(self.h, kind, int(i), int(j), float(beta), C.byref(v)))
        return v.value

    def correlationZZ(self, i, j, beta):
        return self._correlation(0, i, j, beta)

    def correlationXY(self, i, j, beta):
        return self._correlation(1, i, j, beta)

    def correlationSS(self, i, j, beta):
        return self._correlation(2, i, j, beta)

    def observableIndex(self, which, i, j=None):
        """the index `t` that standardError takes for an observable: which = "diagonal" or "flip" with the list index i, or "ZZ"
        / "XY" with the sites i, j after setAllSitesAndPairs"""
        s = self._sizes()
        if which in ("diagonal", "flip"):
            return i if which == "diagonal" else s["ndiag"] + i
        L = s["sites"]
        if L == 0 or i == j or not (0 <= i < L and 0 <= j < L):
            raise capi.EigenexError("the correlations need setAllSitesAndPairs() and two different sites of the model")
        a, b = min(i, j), max(i, j)
        p = a * L - a * (a + 1) // 2 + (b - a - 1)
        return L + p if which == "ZZ" else s["ndiag"] + p

    def standardError(self, quantity, beta, t=0):
        """the delete-one jackknife error over the samples of quantity (a name of QUANTITIES); t as observableIndex gives it"""
        return self._value(self.QUANTITIES.index(quantity), beta, t, error=True)


class ThermalEnsemble:
    """ThermalEnsemble (thermal_lanczos.hpp): sectors added up with multiplicities; multiplicity 2 stands for a sector and its
    image under spin inversion at +M and -M.  observable(t, beta) is valid for terms invariant under that symmetry."""

    _quantities = ("logPartitionFunction", "energy", "specificHeat", "entropy", "susceptibility", "observable")

    def __init__(self, sites=0):
        self._L = lib()
        self.h = _vp(self._L.eigenex_thermal_ensemble_create(int(sites)))
        if not self.h:
            raise capi.EigenexError("ensemble create failed")

    def add(self, solver: ThermalLanczosSolver, multiplicity=1.0, magnetisation=0.0):
        _chk(solver._f("add_to_ensemble")(solver.h, self.h, float(multiplicity), float(magnetisation)))
        return self

    def _value(self, q, beta, t=0):
        v = C.c_double()
        _chk(self._L.eigenex_thermal_ensemble_value(self.h, q, int(t), float(beta), C.byref(v)))
        return v.value

    def logPartitionFunction(self, beta):
        return self._value(0, beta)

    def energy(self, beta):
        return self._value(1, beta)

    def specificHeat(self, beta):
        return self._value(2, beta)

    def entropy(self, beta):
        return self._value(3, beta)

    def susceptibility(self, beta):
        return self._value(4, beta)

    def observable(self, t, beta):
        return self._value(5, beta, t)

    def close(self):
        if self.h:
            self._L.eigenex_thermal_ensemble_destroy(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SpinSolverBase:
    """What the spin front-ends share: the handle of `_prefix`, the model (where the class takes one), the log and the end."""

    _prefix = ""

    def __init__(self):
        self._L = lib()
        self.h = _vp(self._f("create")())
        if not self.h:
            raise capi.EigenexError("solver create failed")
        self._keep = []

    def _f(self, name):
        return getattr(self._L, self._prefix + name)

    def setModel(self, ctx: capi.Context, n_sites, bonds, hz=None, hx=None, n_up=None):
        i32 = C.POINTER(C.c_int32)
        si = np.ascontiguousarray([b[0] for b in bonds], np.int32)
        sj = np.ascontiguousarray([b[1] for b in bonds], np.int32)
        jz = np.ascontiguousarray([b[2] for b in bonds], np.float64)
        jxy = np.ascontiguousarray([b[3] for b in bonds], np.float64)
        fz = None if hz is None else np.ascontiguousarray(hz, np.float64)
        fx = None if hx is None else np.ascontiguousarray(hx, np.float64)
        self._keep.append(ctx)
        self._sites = int(n_sites)
        _chk(self._f("set_model")(self.h, ctx.h, int(n_sites), si.size, si.ctypes.data_as(i32), sj.ctypes.data_as(i32), _d(jz), _d(jxy),
                                  None if fz is None else _d(fz), None if fx is None else _d(fx), -1 if n_up is None else int(n_up)))
        return self

    def _nlog(self):
        return self._sizes()["nlog"]

    def log(self):
        return [self._f("log_line")(self.h, i).decode() for i in range(self._nlog())]

    def close(self):
        if self.h:
            self._f("destroy")(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SpinEvolvingSolverBase(_SpinSolverBase):
    """... of the two that evolve a state: the state, the step control, evolve() and the status arrays of `_status_sizes`."""

    _status_sizes = (0, 0)

    def setState(self, v):
        cplx = np.iscomplexobj(v)
        a = np.ascontiguousarray(v, np.complex128 if cplx else np.float64)
        _chk(self._f("set_state")(self.h, _d(a.view(np.float64)), a.size, int(cplx)))
        return self

    def setProductState(self, bits):
        _chk(self._f("set_product_state")(self.h, int(bits)))
        return self

    def setKrylovDimension(self, m):
        _chk(self._f("set_krylov_dimension")(self.h, int(m)))
        return self

    def setTolerance(self, tol):
        _chk(self._f("set_tolerance")(self.h, float(tol)))
        return self

    def evolve(self, dt):
        n = C.c_int64()
        _chk(self._f("evolve")(self.h, float(dt), C.byref(n)))
        return n.value

    def _status(self):
        sc, cnt = np.zeros(self._status_sizes[0]), np.zeros(self._status_sizes[1], np.int64)
        _chk(self._f("status")(self.h, _d(sc), cnt.ctypes.data_as(_lp)))
        return sc, cnt

    def _nlog(self):
        return int(self._status()[1][0])

    def info(self):
        return INFO[int(self._status()[1][1])]


class SpinDynamicsSolver(_SpinSolverBase):
    """SpinDynamicsSolver (spin_dynamics.hpp): dynamical spin correlations of a state by the Lanczos continued fraction.  The
    model is (n_sites, bonds, hz, hx) with bonds = [(i, j, Jz, Jxy), ...]; n_up = None: the full space."""

    _names = ("npoles", "nalpha", "nbeta", "nlog", "info")
    _prefix = "eigenex_spin_dynamics_solver_"

    def setState(self, v):
        """a real state, or a complex one (then the run is a complex one)"""
        if np.iscomplexobj(v):
            a = np.ascontiguousarray(v, np.complex128)
            _chk(self._f("set_state_z")(self.h, _d(a.view(np.float64)), a.size))
            return self
        a = np.ascontiguousarray(v, np.float64)
        _chk(self._f("set_state")(self.h, _d(a), a.size))
        return self

    def setStateEnergy(self, E0):
        _chk(self._f("set_state_energy")(self.h, float(E0)))
        return self

    def setSiteOperator(self, kind, coef):
        """real coefficients, or complex ones (then the run is a complex one)"""
        if np.iscomplexobj(coef):
            c = np.asarray(coef).reshape(-1)
            cr, ci = np.ascontiguousarray(c.real, np.float64), np.ascontiguousarray(c.imag, np.float64)
            _chk(self._f("set_site_operator_z")(self.h, int(kind), _d(cr), _d(ci), cr.size))
            return self
        a = np.ascontiguousarray(coef, np.float64)
        _chk(self._f("set_site_operator")(self.h, int(kind), _d(a), a.size))
        return self

    def setLanczosSteps(self, m):
        _chk(self._f("set_lanczos_steps")(self.h, int(m)))
        return self

    def compute(self):
        _chk(self._f("compute")(self.h))
        return self

    def computeStructureFactorZ(self, q):
        _chk(self._f("compute_structure_factor_z")(self.h, float(q)))
        return self

    def computeStructureFactorZSingleRun(self, q):
        """Szz(q, w) from one complex run with c_r = L^{-1/2} e^{iqr}"""
        _chk(self._f("compute_structure_factor_z_single_run")(self.h, float(q)))
        return self

    def _sizes(self):
        out = np.zeros(len(self._names), np.int64)
        _chk(self._f("sizes")(self.h, out.ctypes.data_as(_lp)))
        return dict(zip(self._names, (int(x) for x in out)))

    def results(self):
        s = self._sizes()
        poles, weights, alpha, beta, sc = np.zeros(s["npoles"]), np.zeros(s["npoles"]), np.zeros(s["nalpha"]), np.zeros(s["nbeta"]), np.zeros(3)
        _chk(self._f("get")(self.h, _d(poles), _d(weights), _d(alpha), _d(beta), _d(sc)))
        s.update(poles=poles, weights=weights, lanczosAlpha=alpha, lanczosBeta=beta, totalWeight=sc[0], stateEnergy=sc[1],
                 stateNormSquared=sc[2], info_name=INFO[s["info"]])
        return s

    def spectrum(self, omega, eta):
        w = np.ascontiguousarray(np.atleast_1d(omega), np.float64)
        out = np.zeros(w.size)
        _chk(self._f("spectrum")(self.h, _d(w), w.size, float(eta), _d(out)))
        return out

    def moment(self, k):
        m = C.c_double()
        _chk(self._f("moment")(self.h, int(k), C.byref(m)))
        return m.value

    def staticStructureFactorZ(self, q):
        """SpinCorrelationSolver::structureFactorZ(q) of the same model and state"""
        v = C.c_double()
        _chk(self._f("static_structure_factor_z")(self.h, float(q), C.byref(v)))
        return v.value


class SpinMomentumDynamicsSolver(SpinDynamicsSolver):
    """SpinMomentumDynamicsSolver (spin_momentum_dynamics.hpp): dynamical spin correlations of a state of one momentum sector, the
    continued fraction run in the momentum sector the site operator leads to (rings of up to 48 sites).  The model is
    (n_sites, bonds, hz) with bonds = [(i, j, Jz, Jxy), ...], the state lives in the sector (n_up, momentum, cell)."""

    _names = ("npoles", "nalpha", "nbeta", "nlog", "info", "destinationSitesUp", "destinationMomentum", "destinationDimension", "complexRun")
    _prefix = "eigenex_spin_momentum_dynamics_solver_"

    def setModel(self, ctx: capi.Context, n_sites, bonds, n_up, momentum, hz=None, cell=1):
        i32 = C.POINTER(C.c_int32)
        si = np.ascontiguousarray([b[0] for b in bonds], np.int32)
        sj = np.ascontiguousarray([b[1] for b in bonds], np.int32)
        jz = np.ascontiguousarray([b[2] for b in bonds], np.float64)
        jxy = np.ascontiguousarray([b[3] for b in bonds], np.float64)
        fz = None if hz is None else np.ascontiguousarray(hz, np.float64)
        self._keep.append(ctx)
        self._sites = int(n_sites)
        _chk(self._f("set_model")(self.h, ctx.h, int(n_sites), si.size, si.ctypes.data_as(i32), sj.ctypes.data_as(i32), _d(jz), _d(jxy),
                                  None if fz is None else _d(fz), int(n_up), int(momentum), int(cell)))
        return self

    def setState(self, v):
        """a real or a complex state over the rows of the momentum sector"""
        cplx = np.iscomplexobj(v)
        a = np.ascontiguousarray(v, np.complex128 if cplx else np.float64)
        _chk(self._f("set_state")(self.h, _d(a.view(np.float64)), a.size, int(cplx)))
        return self

    def setSiteOperator(self, kind, cell_coef, p):
        """one real or complex coefficient per site of the cell, and the momentum index p of the operator"""
        c = np.asarray(cell_coef).reshape(-1)
        cr, ci = np.ascontiguousarray(c.real, np.float64), np.ascontiguousarray(c.imag, np.float64)
        _chk(self._f("set_site_operator")(self.h, int(kind), _d(cr), _d(ci), cr.size, int(p)))
        return self

    def computeStructureFactorZ(self, q_index):
        """Szz(q, w) at q = 2 pi q_index / n_sites"""
        _chk(self._f("compute_structure_factor_z")(self.h, int(q_index)))
        return self

    def computeStructureFactorZSingleRun(self, q):
        raise AttributeError("SpinMomentumDynamicsSolver runs one fraction per call: computeStructureFactorZ(q_index)")

    def staticStructureFactorZ(self, q):
        raise AttributeError("SpinMomentumDynamicsSolver: the static value is SpinMomentumCorrelationSolver's, or totalWeight")


class SpinTimeEvolutionSolver(_SpinEvolvingSolverBase):
    """SpinTimeEvolutionSolver (spin_evolution.hpp): |psi(t)> = exp(-i H t)|psi_0> of a spin-1/2 model by Krylov propagation on
    the device, with an a-posteriori error bound per call.  The model is given as for SpinDynamicsSolver."""

    _prefix = "eigenex_spin_evolution_solver_"
    _status_sizes = (5, 4)

    def time(self):
        return self._status()[0][0]

    def errorBound(self):
        return self._status()[0][1]

    def totalErrorBound(self):
        return self._status()[0][2]

    def initialNorm(self):
        return self._status()[0][3]

    def operatorApplications(self):
        return int(self._status()[0][4])

    def _scalar(self, what):
        out = np.zeros(2)
        _chk(self._f("scalar")(self.h, what, _d(out)))
        return out

    def normSquared(self):
        return float(self._scalar(0)[0])

    def energy(self):
        return float(self._scalar(1)[0])

    def overlapWithInitial(self):
        z = self._scalar(2)
        return complex(z[0], z[1])

    def _vector(self, what):
        n = C.c_int64()
        _chk(self._f("measure")(self.h, what, C.byref(n)))
        out = np.zeros(n.value)
        _chk(self._f("fetch")(self.h, _d(out)))
        return out

    def magnetisation(self):
        return self._vector(0)

    def correlationsZZ(self):
        return self._vector(1).reshape(self._sites, self._sites)

    def correlationsXY(self):
        return self._vector(2).reshape(self._sites, self._sites)

    def state(self):
        return self._vector(3).view(np.complex128)

    def _entanglement(self, subsystem, what):
        """subsystem: a site mask (int) or a list of sites"""
        n = C.c_int64()
        if isinstance(subsystem, (int, np.integer)):
            _chk(self._f("entanglement")(self.h, int(subsystem), None, 0, what, C.byref(n)))
        else:
            a = np.ascontiguousarray(subsystem, np.int32).reshape(-1)
            keep = a if a.size else np.zeros(1, np.int32)  # an empty list is still a list: a non-NULL pointer
            _chk(self._f("entanglement")(self.h, 0, keep.ctypes.data_as(C.POINTER(C.c_int32)), a.size, what, C.byref(n)))
        out = np.zeros(n.value)
        _chk(self._f("fetch")(self.h, _d(out)))
        return out

    def entanglementEntropy(self, subsystem):
        """the von Neumann entropy of the subsystem (a site mask or a list of sites) of psi(t), formed on the device"""
        return float(self._entanglement(subsystem, 0)[0])

    def entanglementRenyi2(self, subsystem):
        return float(self._entanglement(subsystem, 1)[0])

    def entanglementSpectrum(self, subsystem):
        return self._entanglement(subsystem, 2)


class SpinTimeCorrelationSolver(_SpinEvolvingSolverBase):
    """SpinTimeCorrelationSolver (spin_time_correlation.hpp): C_n(t) = <A_n psi(t) | exp(-iHt) B psi_0> of a spin-1/2 model by
    Krylov propagation of two vectors on the device.  The model is given as for SpinDynamicsSolver; coefficients are real or
    complex, one per site."""

    _prefix = "eigenex_spin_time_correlation_solver_"
    _status_sizes = (6, 3)

    def setEigenstate(self, E0):
        _chk(self._f("set_eigenstate")(self.h, float(E0)))
        return self

    @staticmethod
    def _coef(coef):
        return np.ascontiguousarray(np.asarray(coef).reshape(-1), np.complex128)

    def setSourceOperator(self, kind, coef):
        c = self._coef(coef)
        _chk(self._f("set_source_operator")(self.h, int(kind), _d(c.view(np.float64)), c.size))
        return self

    def addMeasuredOperator(self, coef):
        c = self._coef(coef)
        _chk(self._f("add_measured_operator")(self.h, _d(c.view(np.float64)), c.size))
        return self

    def clearMeasuredOperators(self):
        _chk(self._f("clear_measured_operators")(self.h))
        return self

    def setMeasuredSites(self):
        _chk(self._f("set_measured_sites")(self.h))
        return self

    def setMomentumZ(self, q):
        _chk(self._f("set_momentum_z")(self.h, float(q)))
        return self

    def values(self):
        n = C.c_int64()
        _chk(self._f("values")(self.h, C.byref(n)))
        out = np.zeros(n.value, np.complex128)
        _chk(self._f("fetch")(self.h, _d(out.view(np.float64))))
        return out

    def time(self):
        return self._status()[0][0]

    def sourceNormSquared(self):
        return self._status()[0][1]

    def errorBound(self, n=None):
        """the bound on |delta C_n| of measured operator n, or the largest over all of them"""
        if n is None:
            return self._status()[0][2]
        out = np.zeros(2)
        _chk(self._f("operator_bounds")(self.h, int(n), _d(out)))
        return out[0]

    def operatorNormBound(self, n):
        out = np.zeros(2)
        _chk(self._f("operator_bounds")(self.h, int(n), _d(out)))
        return out[1]

    def stateErrorBound(self):
        return self._status()[0][3]

    def sourceErrorBound(self):
        return self._status()[0][4]

    def operatorApplications(self):
        return int(self._status()[0][5])


class SpinEntanglementSolver(_SpinSolverBase):
    """SpinEntanglementSolver (spin_entanglement.hpp): the reduced density matrix of a subsystem of a state of a matrix-free
    spin-1/2 operator (capi.Csr.spin_half, capi.Csr.spin_half_sector), formed on the device, and what follows from it: the
    entanglement spectrum, the von Neumann and Renyi entropies and the Schmidt rank."""

    _names = ("nblocks", "neigenvalues", "nlog", "info")
    _prefix = "eigenex_spin_entanglement_solver_"

    def setDeviceOperator(self, csr: capi.Csr):
        self._keep.append(csr)
        _chk(self._f("set_device_operator")(self.h, csr.ctx.h, csr.h))
        return self

    def setState(self, v):
        """a real state, or a complex one (then the operator must be one for complex states: complex_states=True)"""
        if np.iscomplexobj(v):
            a = np.ascontiguousarray(v, np.complex128)
            _chk(self._f("set_state_z")(self.h, _d(a.view(np.float64)), a.size))
        else:
            a = np.ascontiguousarray(v, np.float64)
            _chk(self._f("set_state")(self.h, _d(a), a.size))
        return self

    def setSubsystem(self, sites):
        a = np.ascontiguousarray(sites, np.int32).reshape(-1)
        _chk(self._f("set_subsystem")(self.h, a.ctypes.data_as(C.POINTER(C.c_int32)), a.size))
        return self

    def setSubsystemMask(self, mask):
        _chk(self._f("set_subsystem_mask")(self.h, int(mask)))
        return self

    def compute(self):
        _chk(self._f("compute")(self.h))
        return self

    def _sizes(self):
        out = np.zeros(len(self._names), np.int64)
        _chk(self._f("sizes")(self.h, out.ctypes.data_as(_lp)))
        return dict(zip(self._names, (int(x) for x in out)))

    def results(self):
        """blocks = [(sites up inside the subsystem, unit-trace block of rho_A as ndarray(d, d)), ...], spectrum (descending),
        normSquared, entropy, renyi2, info"""
        s = self._sizes()
        spectrum, sc, blocks = np.zeros(s["neigenvalues"]), np.zeros(3), []
        _chk(self._f("get")(self.h, _d(spectrum), _d(sc)))
        for n in range(s["nblocks"]):
            up, dim, cplx = C.c_int(), C.c_int64(), C.c_int()
            _chk(self._f("block")(self.h, n, C.byref(up), C.byref(dim), None))
            _chk(self._f("block_z")(self.h, n, C.byref(cplx), None))
            if cplx.value:  # a complex state: complex128 blocks
                rho = np.zeros(2 * dim.value * dim.value)
                _chk(self._f("block_z")(self.h, n, None, _d(rho)))
                rho = rho.view(np.complex128)
            else:
                rho = np.zeros(dim.value * dim.value)
                _chk(self._f("block")(self.h, n, None, None, _d(rho)))
            blocks.append((up.value, rho.reshape(dim.value, dim.value).T.copy()))
        s.update(blocks=blocks, spectrum=spectrum, normSquared=sc[0], entropy=sc[1], renyi2=sc[2], info_name=INFO[s["info"]])
        return s

    def renyi(self, alpha):
        v = C.c_double()
        _chk(self._f("renyi")(self.h, float(alpha), C.byref(v)))
        return v.value

    def schmidtRank(self, tol):
        r = C.c_int64()
        _chk(self._f("schmidt_rank")(self.h, float(tol), C.byref(r)))
        return r.value
