"""ctypes binding of include/eigenex_hip.h (the C ABI of libeigenex_hip.so).

This is plumbing for tests/ and bench.py; the product's host side is the
header-only C++ in cmpt-eigenex_amd/include/cmpt/eigen_ex/.  Nothing here
computes: every function forwards to the HIP library and raises EigenexError
when the library reports a failure (there is no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libeigenex_hip.so")

ORTHO_BATCHED = 0
ORTHO_SEQUENTIAL = 1
ORTHO_BATCHED_TWICE = 2
ORTHO_BATCHED_ADAPTIVE = 3
VEC_V = -1
VEC_W = -2
VEC_START = -3
K_SPMV, K_DOTS, K_UPDATE, K_SMALL, K_COMM, K_RITZ = range(6)
SPIN_SITE_Z, SPIN_SITE_PLUS, SPIN_SITE_MINUS = range(3)


def VEC_COL(c: int) -> int:
    return int(c)


def VEC_ORTHO(q: int) -> int:
    return -16 - int(q)


class EigenexError(RuntimeError):
    pass


class State(C.Structure):
    _fields_ = [("nvec", C.c_int32), ("iterations", C.c_int32), ("nalpha", C.c_int32), ("nbeta", C.c_int32),
                ("stopped", C.c_int32), ("calls_true", C.c_int32), ("residue", C.c_double)]


MATVEC_FN = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)
_vp = C.c_void_p
_up = C.POINTER(C.c_uint32)

# name -> (restype, argtypes): every symbol include/eigenex_hip.h declares
SIGNATURES = {
    "eigenex_version": (C.c_int, []),
    "eigenex_last_error": (C.c_char_p, []),
    "eigenex_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "eigenex_partition": (C.c_int, [C.c_int64, C.c_int, C.c_int, _lp, _lp]),
    "eigenex_halo_plan": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int64, _ip, _lp, _ip, _lp]),
    "eigenex_rccl_unique_id": (C.c_int, [_vp]),
    "eigenex_context_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    "eigenex_context_create_loopback": (C.c_int, [C.c_int, C.c_int, C.POINTER(_vp)]),
    "eigenex_context_destroy": (C.c_int, [_vp]),
    "eigenex_context_selftest": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "eigenex_context_sync": (C.c_int, [_vp]),
    "eigenex_context_info": (C.c_int, [_vp] + [C.POINTER(C.c_int)] * 4),
    "eigenex_context_comm_info": (C.c_int, [_vp] + [C.POINTER(C.c_int)] * 3),
    "eigenex_context_trace": (C.c_int, [_vp, C.c_int]),
    "eigenex_context_set_halo_overlap": (C.c_int, [_vp, C.c_int]),
    "eigenex_context_trace_get": (C.c_int, [_vp, _ip, _ip, C.c_int, C.POINTER(C.c_int)]),
    "eigenex_debug_allocations": (C.c_int, [_lp, _lp, _lp]),
    "eigenex_debug_fail_allocation": (C.c_int, [C.c_int64]),
    "eigenex_plan_create": (C.c_int, [C.c_int64, C.c_int, C.c_int, _ip, _ip, C.POINTER(_vp)]),
    "eigenex_plan_destroy": (C.c_int, [_vp]),
    "eigenex_plan_tiles": (C.c_int, [_vp, _ip, C.POINTER(C.c_int64), _ip, C.POINTER(C.c_int64)]),
    "eigenex_plan_sizes": (C.c_int, [_vp] + [C.POINTER(C.c_int64)] * 4 + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_int64)]),
    "eigenex_plan_local_columns": (C.c_int, [_vp, _ip]),
    "eigenex_plan_halo_columns": (C.c_int, [_vp, _ip]),
    "eigenex_plan_recv_segments": (C.c_int, [_vp, _ip, _lp, _lp]),
    "eigenex_plan_add_request": (C.c_int, [_vp, C.c_int, _ip, C.c_int64]),
    "eigenex_plan_send_segments": (C.c_int, [_vp, _ip, _lp, _lp, _lp]),
    "eigenex_plan_send_rows": (C.c_int, [_vp, _ip]),
    "eigenex_lanczos_collectives": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                              _ip, _ip, C.c_int, C.POINTER(C.c_int)]),
    "eigenex_context_stream": (_vp, [_vp]),
    "eigenex_profile_enable": (C.c_int, [_vp, C.c_int]),
    "eigenex_profile_reset": (C.c_int, [_vp]),
    "eigenex_profile_get": (C.c_int, [_vp, C.c_int, _lp, _dp, _dp]),
    "eigenex_csr_upload": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, _ip, _ip, _dp, C.POINTER(_vp)]),
    "eigenex_csr_upload_z": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, _ip, _ip, _dp, C.POINTER(_vp)]),
    "eigenex_csr_upload64": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64), _ip, _dp, C.POINTER(_vp)]),
    "eigenex_csr_laplacian3d": (C.c_int, [_vp, C.c_int64, C.POINTER(_vp)]),
    "eigenex_csr_destroy": (C.c_int, [_vp]),
    "eigenex_csr_upload_ex": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, _ip, _ip, _dp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "eigenex_csr_column_blocks": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "eigenex_csr_layout": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "eigenex_csr_encoding": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "eigenex_csr_upload_device": (C.c_int, [_vp, C.c_int64, _vp, _vp, _vp, C.c_int, C.POINTER(_vp)]),
    "eigenex_block_upload": (C.c_int, [_vp, C.c_int64, C.c_int, _lp, C.c_int, _lp, C.c_int64, _lp, _lp, C.POINTER(C.c_void_p), C.POINTER(_vp)]),
    "eigenex_block_upload_z": (C.c_int, [_vp, C.c_int64, C.c_int, _lp, C.c_int, _lp, C.c_int64, _lp, _lp, C.POINTER(C.c_void_p), C.POINTER(_vp)]),
    "eigenex_csr_info": (C.c_int, [_vp, _lp, _lp, _lp, _lp]),
    "eigenex_spin_upload": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, C.POINTER(_vp)]),
    "eigenex_spin_csr": (C.c_int, [C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, C.c_int64, C.c_int64, _lp, _ip, _dp, _lp]),
    "eigenex_spin_sector_dim": (C.c_int, [C.c_int, C.c_int, _lp]),
    "eigenex_spin_sector_states": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_uint32)]),
    "eigenex_spin_sector_csr": (C.c_int, [C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, C.c_int64, C.c_int64, _lp, _ip, _dp, _lp]),
    "eigenex_spin_sector_upload": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, C.POINTER(_vp)]),
    "eigenex_spin_upload_z": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, C.POINTER(_vp)]),
    "eigenex_spin_sector_upload_z": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, C.POINTER(_vp)]),
    "eigenex_spin_momentum_dim": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _lp]),
    "eigenex_spin_momentum_states": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
    "eigenex_spin_momentum_csr": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, C.c_int64, C.c_int64, _lp, _ip, _dp, _lp]),
    "eigenex_spin_momentum_upload": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, C.POINTER(_vp)]),
    "eigenex_spin_momentum_upload_z": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, C.POINTER(_vp)]),
    "eigenex_spin_momentum_geometry": (C.c_int, [_vp] + [C.POINTER(C.c_int)] * 4),
    "eigenex_spin_momentum_expand": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _dp]),
    "eigenex_spin_momentum_expand_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp]),
    "eigenex_spin_momentum64_dim": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _lp]),
    "eigenex_spin_momentum64_states": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)]),
    "eigenex_spin_momentum64_csr": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, C.c_int64, C.c_int64, _lp, _ip, _dp, _lp]),
    "eigenex_spin_momentum64_upload": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, C.POINTER(_vp)]),
    "eigenex_spin_momentum64_upload_z": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, C.POINTER(_vp)]),
    "eigenex_spin_momentum_measure": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_uint64), _dp, _dp]),
    "eigenex_spin_momentum_measure_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.POINTER(C.c_uint64), _dp, _dp]),
    "eigenex_spin_momentum_site_apply": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _dp, _dp]),
    "eigenex_spin_momentum_site_apply_z": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp]),
    "eigenex_spin_momentum_site_apply_host": (C.c_int, [C.c_int] * 7 + [_dp] * 5),
    "eigenex_spin_measure": (C.c_int, [_vp, C.c_int, C.c_int, _up, C.c_int, _up, _dp, _dp, _dp]),
    "eigenex_spin_measure_host": (C.c_int, [C.c_int, C.c_int, _dp, C.c_int, _up, C.c_int, _up, _dp, _dp, _dp]),
    "eigenex_spin_measure_host_z": (C.c_int, [C.c_int, C.c_int, _dp, C.c_int, _up, C.c_int, _up, _dp, _dp, _dp]),
    "eigenex_spin_measure_columns": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _up, C.c_int, _up, _dp, _dp]),
    "eigenex_spin_measure_columns_host": (C.c_int, [C.c_int, C.c_int, _dp, _dp, C.c_int64, C.c_int, C.c_int, _up, C.c_int, _up, _dp, _dp]),
    "eigenex_spin_geometry": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "eigenex_spin_site_apply": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, _dp, _dp]),
    "eigenex_spin_site_apply_host": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp]),
    "eigenex_spin_site_apply_z": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, _dp, _dp, _dp]),
    "eigenex_spin_site_apply_host_z": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "eigenex_spin_rdm_layout": (C.c_int, [C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int), _lp, _lp]),
    "eigenex_spin_rdm": (C.c_int, [_vp, C.c_int, C.c_uint32, _dp, C.c_int64]),
    "eigenex_spin_rdm_host": (C.c_int, [C.c_int, C.c_int, _dp, C.c_uint32, _dp, C.c_int64]),
    "eigenex_spin_rdm_z": (C.c_int, [_vp, C.c_int, C.c_uint32, _dp, C.c_int64]),
    "eigenex_spin_rdm_host_z": (C.c_int, [C.c_int, C.c_int, _dp, C.c_uint32, _dp, C.c_int64]),
    "eigenex_basis_create": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.POINTER(_vp)]),
    "eigenex_basis_create_ex": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "eigenex_basis_is_complex": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "eigenex_basis_configure_z": (C.c_int, [_vp, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int]),
    "eigenex_basis_destroy": (C.c_int, [_vp]),
    "eigenex_basis_set_host_operator": (C.c_int, [_vp, MATVEC_FN, _vp]),
    "eigenex_basis_configure": (C.c_int, [_vp, C.c_double, C.c_double, C.c_int64, C.c_int]),
    "eigenex_basis_clear": (C.c_int, [_vp]),
    "eigenex_vec_upload": (C.c_int, [_vp, C.c_int, _dp]),
    "eigenex_vec_download": (C.c_int, [_vp, C.c_int, _dp]),
    "eigenex_vec_copy": (C.c_int, [_vp, C.c_int, C.c_int]),
    "eigenex_basis_reserve": (C.c_int, [_vp, C.c_int]),
    "eigenex_basis_capacity": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "eigenex_basis_tune": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    "eigenex_ritz_vectors_complex": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int64]),
    "eigenex_krylov_combine": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int64]),
    "eigenex_krylov_combine_to": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_int]),
    "eigenex_apply": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, _dp]),
    "eigenex_basis_set_filter": (C.c_int, [_vp, C.c_int, _dp, C.c_double, C.c_double]),
    "eigenex_filter_apply": (C.c_int, [_vp, C.c_int, C.c_int]),
    "eigenex_kpm_moments": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_double, _dp]),
    "eigenex_kpm_trace_moments": (C.c_int, [_vp, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_double, C.c_double, _dp]),
    "eigenex_vec_random_signs": (C.c_int, [_vp, C.c_int, C.c_uint64, C.c_uint64]),
    "eigenex_dots": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp]),
    "eigenex_update": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp]),
    "eigenex_axpy2": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int]),
    "eigenex_scale": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double]),
    "eigenex_lanczos_enqueue": (C.c_int, [_vp, C.c_int]),
    "eigenex_basis_set_alpha_fusion": (C.c_int, [_vp, C.c_int]),
    "eigenex_basis_clone": (C.c_int, [_vp, C.POINTER(_vp)]),
    "eigenex_basis_graph_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "eigenex_basis_repairs": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "eigenex_basis_close_pending": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "eigenex_arnoldi_enqueue": (C.c_int, [_vp, C.c_int]),
    "eigenex_lanczos_restart": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double]),
    "eigenex_arnoldi_restart": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, C.c_int]),
    "eigenex_lanczos_state": (C.c_int, [_vp, C.POINTER(State), _dp, _dp]),
    "eigenex_arnoldi_state": (C.c_int, [_vp, C.POINTER(State), _dp, C.c_int]),
    "eigenex_ritz_vectors": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int64]),
}

_LIB = None


def _preload_torch_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / librccl.so.1 (ROCm 7.0 here) under the same SONAMEs as
    the system ROCm this library is linked against.  Whichever copy is loaded first serves both: torch first is
    fine (this library then runs on torch's runtime; that is how bench.py and the tests run), this library first makes
    torch mix runtimes and abort at exit ("double free or corruption").  So when torch is installed it is imported
    before the library is loaded.  EIGENEX_NO_TORCH_PRELOAD=1 skips this for processes that never import torch."""
    if "torch" in sys.modules or os.environ.get("EIGENEX_NO_TORCH_PRELOAD"):
        return
    import importlib.util

    if importlib.util.find_spec("torch") is not None:
        try:
            import torch  # noqa: F401
        except Exception:  # a broken torch install must not keep the library from loading
            pass


def _hip_runtimes_mapped():
    """distinct libamdhip64 / librccl files mapped into this process (from /proc/self/maps)"""
    found = {"libamdhip64": set(), "librccl": set()}
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(None, 1)[-1]
                base = os.path.basename(path)
                for k in found:
                    if base.startswith(k + ".so"):
                        found[k].add(os.path.realpath(path))
    except OSError:
        pass
    return found


def _refuse_mixed_runtimes():
    """Two copies of the HIP (or RCCL) runtime in one process -- the system one this library links against and the
    one a PyTorch-ROCm wheel bundles under the same SONAME -- end in an abort at interpreter exit ("double free or
    corruption") long after the cause.  That can only happen when something loaded one copy by path before the other
    was resolved by name; refuse right here, where the order can still be fixed."""
    for name, paths in _hip_runtimes_mapped().items():
        if len(paths) > 1:
            raise EigenexError(
                f"two copies of {name} are loaded in this process ({', '.join(sorted(paths))}): import torch BEFORE anything "
                "loads the system ROCm runtime (cmpt_eigenex_amd.capi does so by itself unless EIGENEX_NO_TORCH_PRELOAD is set), "
                "or do not import torch in this process at all")


def lib():
    """Load libeigenex_hip.so (built in-tree by cmpt_eigenex_amd.build).  Fails loudly if missing."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise EigenexError(
                f"{LIB_PATH} is missing: build it with `python -m cmpt_eigenex_amd.build` "
                "(there is no CPU fallback for the Krylov hot path)")
        _preload_torch_runtime()
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        _refuse_mixed_runtimes()
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def _chk(rc: int):
    if rc != 0:
        raise EigenexError(f"eigenex error {rc}: {lib().eigenex_last_error().decode(errors='replace')}")


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().eigenex_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def partition(n_global: int, nshards: int, shard: int):
    b, e = C.c_int64(), C.c_int64()
    _chk(lib().eigenex_partition(n_global, nshards, shard, C.byref(b), C.byref(e)))
    return b.value, e.value


def halo_plan(n_global: int, nshards: int, shard: int, col_global: np.ndarray):
    col = np.ascontiguousarray(col_global, np.int32)
    nh = C.c_int64()
    _chk(lib().eigenex_halo_plan(n_global, nshards, shard, col.size, _i(col), C.byref(nh), None, None))
    cols = np.empty(nh.value, np.int32)
    per = np.zeros(nshards, np.int64)
    _chk(lib().eigenex_halo_plan(n_global, nshards, shard, col.size, _i(col), C.byref(nh), _i(cols),
                                 per.ctypes.data_as(_lp)))
    return cols, per


COLL_ALLREDUCE, COLL_HALO = 1, 2


def lanczos_collectives(call_index: int, last_in_batch: bool, alpha_pending: bool, interval=1, n_ortho=0, ortho_mode=ORTHO_BATCHED,
                        alpha_fusion=True, is_complex=False):
    """[(op, count), ...] of one Lanczos step call between shards, and the alpha-fusion state after it"""
    pend = C.c_int(int(alpha_pending))
    n = C.c_int()
    ops, cnt = np.zeros(4096, np.int32), np.zeros(4096, np.int32)
    _chk(lib().eigenex_lanczos_collectives(call_index, int(last_in_batch), C.byref(pend), interval, n_ortho, ortho_mode, int(alpha_fusion),
                                           int(is_complex), _i(ops), _i(cnt), ops.size, C.byref(n)))
    return [(int(ops[i]), int(cnt[i])) for i in range(n.value)], bool(pend.value)


def _spin_model(n_sites, bonds, hz, hx):
    """ctypes arguments of the spin-1/2 model (include/eigenex_hip.h: eigenex_spin_upload): bonds = [(i, j, Jz, Jxy), ...],
    hz / hx = n_sites fields or None.  Returns (keep-alive arrays, argument tuple)."""
    bonds = list(bonds)
    si = np.ascontiguousarray([b[0] for b in bonds], np.int32)
    sj = np.ascontiguousarray([b[1] for b in bonds], np.int32)
    jz = np.ascontiguousarray([b[2] for b in bonds], np.float64)
    jxy = np.ascontiguousarray([b[3] for b in bonds], np.float64)
    fields = []
    for h in (hz, hx):
        if h is not None:
            h = np.ascontiguousarray(h, np.float64)
            if h.shape != (n_sites,):
                raise ValueError("a site field needs n_sites entries")
        fields.append(h)
    keep = (si, sj, jz, jxy, *fields)
    return keep, (int(n_sites), len(bonds), _i(si), _i(sj), _d(jz), _d(jxy), *[_d(h) if h is not None else None for h in fields])


def spin_csr(n_sites: int, bonds, hz=None, hx=None, row_begin: int = 0, n_rows: int | None = None):
    """eigenex_spin_csr: rows [row_begin, row_begin + n_rows) of the spin-1/2 Hamiltonian as CSR (host code, no GPU needed), in
    the stored order the matrix-free kernel adds them in.  Returns rowptr (int64, starting at 0), col (int32, global), val."""
    keep, args = _spin_model(n_sites, bonds, hz, hx)
    if n_rows is None:
        n_rows = (1 << n_sites) - row_begin if 2 <= n_sites <= 30 else 0  # (the library refuses any other n_sites)
    rowptr = np.zeros(max(int(n_rows), 0) + 1, np.int64)
    nnz = C.c_int64()
    _chk(lib().eigenex_spin_csr(*args, row_begin, n_rows, rowptr.ctypes.data_as(_lp), None, None, C.byref(nnz)))
    col, val = np.zeros(nnz.value, np.int32), np.zeros(nnz.value, np.float64)
    _chk(lib().eigenex_spin_csr(*args, row_begin, n_rows, rowptr.ctypes.data_as(_lp), _i(col), _d(val), C.byref(nnz)))
    return rowptr, col, val


def spin_sector_dim(n_sites: int, n_up: int) -> int:
    """eigenex_spin_sector_dim: C(n_sites, n_up), the number of states of n_sites sites (2..32) with n_up sites up"""
    dim = C.c_int64()
    _chk(lib().eigenex_spin_sector_dim(int(n_sites), int(n_up), C.byref(dim)))
    return dim.value


def spin_sector_states(n_sites: int, n_up: int, first: int = 0, count: int | None = None):
    """eigenex_spin_sector_states: the states (uint32, ascending) of ranks first .. first + count - 1 of the sector; x_full[states]
    = x_sector scatters a sector vector into the full space"""
    if count is None:
        count = spin_sector_dim(n_sites, n_up) - first
    states = np.zeros(max(int(count), 0), np.uint32)
    _chk(lib().eigenex_spin_sector_states(int(n_sites), int(n_up), int(first), int(count), states.ctypes.data_as(C.POINTER(C.c_uint32))))
    return states


def _sector_args(args, n_up):
    """the model arguments of _spin_model with n_up behind n_sites"""
    return (args[0], int(n_up), *args[1:])


def spin_sector_csr(n_sites: int, n_up: int, bonds, hz=None, hx=None, row_begin: int = 0, n_rows: int | None = None):
    """eigenex_spin_sector_csr: rows [row_begin, row_begin + n_rows) (ranks) of the spin-1/2 Hamiltonian in the sector of n_up
    sites up, as CSR (host code, no GPU needed), in the stored order of spin_csr.  Returns rowptr (int64), col (int32, ranks), val."""
    keep, args = _spin_model(n_sites, bonds, hz, hx)
    args = _sector_args(args, n_up)
    if n_rows is None:
        n_rows = spin_sector_dim(n_sites, n_up) - row_begin
    rowptr = np.zeros(max(int(n_rows), 0) + 1, np.int64)
    nnz = C.c_int64()
    _chk(lib().eigenex_spin_sector_csr(*args, row_begin, n_rows, rowptr.ctypes.data_as(_lp), None, None, C.byref(nnz)))
    col, val = np.zeros(nnz.value, np.int32), np.zeros(nnz.value, np.float64)
    _chk(lib().eigenex_spin_sector_csr(*args, row_begin, n_rows, rowptr.ctypes.data_as(_lp), _i(col), _d(val), C.byref(nnz)))
    return rowptr, col, val


def _momentum_args(args, n_up, cell, momentum):
    """the model arguments of _spin_model(hx=None) as the momentum entry points take them: (n_sites, n_up, cell, momentum,
    n_bonds, site_i, site_j, jz, jxy, hz) -- there is no hx argument"""
    return (args[0], int(n_up), int(cell), int(momentum), *args[1:-1])


# the host entry points of a momentum sector exist once per state word: (symbol suffix, dtype of a state)
_WORD32, _WORD64 = ("", np.uint32), ("64", np.uint64)


def _momentum_entry(word, name):
    return getattr(lib(), "eigenex_spin_momentum%s_%s" % (word[0], name))


def _momentum_dim(word, n_sites, n_up, momentum, cell):
    dim = C.c_int64()
    _chk(_momentum_entry(word, "dim")(int(n_sites), int(n_up), int(cell), int(momentum), C.byref(dim)))
    return dim.value


def _momentum_states(word, n_sites, n_up, momentum, cell, first, count):
    if count is None:
        count = _momentum_dim(word, n_sites, n_up, momentum, cell) - first
    states, periods = np.zeros(max(int(count), 0), word[1]), np.zeros(max(int(count), 0), np.uint8)
    _chk(_momentum_entry(word, "states")(int(n_sites), int(n_up), int(cell), int(momentum), int(first), int(count),
                                         states.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(word[1]))),
                                         periods.ctypes.data_as(C.POINTER(C.c_uint8))))
    return states, periods


def _momentum_csr(word, n_sites, n_up, momentum, bonds, hz, cell, row_begin, n_rows):
    keep, args = _spin_model(n_sites, bonds, hz, None)
    args = _momentum_args(args, n_up, cell, momentum)
    csr = _momentum_entry(word, "csr")
    nnz = C.c_int64()
    if n_rows is None:
        one = np.zeros(1, np.int64)
        _chk(csr(*args, 0, 0, one.ctypes.data_as(_lp), None, None, C.byref(nnz)))  # the model's own refusal first
        n_rows = _momentum_dim(word, n_sites, n_up, momentum, cell) - row_begin
    rowptr = np.zeros(max(int(n_rows), 0) + 1, np.int64)
    _chk(csr(*args, row_begin, n_rows, rowptr.ctypes.data_as(_lp), None, None, C.byref(nnz)))
    col, val = np.zeros(nnz.value, np.int32), np.zeros(nnz.value, np.complex128)
    _chk(csr(*args, row_begin, n_rows, rowptr.ctypes.data_as(_lp), _i(col), _d(val.view(np.float64)), C.byref(nnz)))
    return rowptr, col, val


def spin_momentum_dim(n_sites: int, n_up: int, momentum: int, cell: int = 1) -> int:
    """eigenex_spin_momentum_dim: the number of rows of the momentum sector (n_sites, n_up, cell, momentum)"""
    return _momentum_dim(_WORD32, n_sites, n_up, momentum, cell)


def spin_momentum_states(n_sites: int, n_up: int, momentum: int, cell: int = 1, first: int = 0, count: int | None = None):
    """eigenex_spin_momentum_states: (representatives (uint32, ascending), their periods (uint8)) of rows first .. first + count - 1"""
    return _momentum_states(_WORD32, n_sites, n_up, momentum, cell, first, count)


def spin_momentum_csr(n_sites: int, n_up: int, momentum: int, bonds, hz=None, cell: int = 1, row_begin: int = 0, n_rows: int | None = None):
    """eigenex_spin_momentum_csr: rows [row_begin, row_begin + n_rows) of the spin-1/2 Hamiltonian in a momentum sector as CSR
    (host code, no GPU needed), in the stored order the matrix-free kernel adds them in.  Returns rowptr (int64), col (int32),
    val (complex128; all imaginary parts are exactly 0 at a real momentum)."""
    return _momentum_csr(_WORD32, n_sites, n_up, momentum, bonds, hz, cell, row_begin, n_rows)


def spin_momentum_expand_host(n_sites: int, n_up: int, momentum: int, x, cell: int = 1):
    """eigenex_spin_momentum_expand_host: the Sz-sector vector of the momentum vector x (float64: a real momentum only; complex128
    else), the definition the device call is held against"""
    is_complex = np.iscomplexobj(x)
    x = np.ascontiguousarray(x, np.complex128 if is_complex else np.float64).reshape(-1)
    if x.size != spin_momentum_dim(n_sites, n_up, momentum, cell):  # the library cannot see the length
        raise ValueError("x needs one entry per row of the momentum sector")
    y = np.zeros(spin_sector_dim(n_sites, n_up), x.dtype)
    _chk(lib().eigenex_spin_momentum_expand_host(int(n_sites), int(n_up), int(cell), int(momentum), int(is_complex), _d(x.view(np.float64)),
                                                 _d(y.view(np.float64))))
    return y


def spin_momentum64_dim(n_sites: int, n_up: int, momentum: int, cell: int = 1) -> int:
    """eigenex_spin_momentum64_dim: the number of rows of the momentum sector (n_sites up to 48, n_up, cell, momentum)"""
    return _momentum_dim(_WORD64, n_sites, n_up, momentum, cell)


def spin_momentum64_states(n_sites: int, n_up: int, momentum: int, cell: int = 1, first: int = 0, count: int | None = None):
    """eigenex_spin_momentum64_states: (representatives (uint64, ascending), their periods (uint8)) of rows first .. first + count - 1"""
    return _momentum_states(_WORD64, n_sites, n_up, momentum, cell, first, count)


def spin_momentum64_csr(n_sites: int, n_up: int, momentum: int, bonds, hz=None, cell: int = 1, row_begin: int = 0, n_rows: int | None = None):
    """eigenex_spin_momentum64_csr: spin_momentum_csr for rings of up to 48 sites and 128 bonds (64-bit states).  Returns rowptr
    (int64), col (int32), val (complex128; all imaginary parts are exactly 0 at a real momentum)."""
    return _momentum_csr(_WORD64, n_sites, n_up, momentum, bonds, hz, cell, row_begin, n_rows)


def _mask_list64(masks):
    """a list of 64-bit site masks as (keep-alive array, count, pointer or None)"""
    m = np.ascontiguousarray(masks, np.uint64).reshape(-1)
    return m, int(m.size), (m.ctypes.data_as(C.POINTER(C.c_uint64)) if m.size else None)


def spin_momentum_measure_host(n_sites: int, n_up: int, momentum: int, x, masks, cell: int = 1):
    """eigenex_spin_momentum_measure_host: (diag, norm2), the raw sums of the diagonal correlations of the momentum vector x (float64
    or complex128, one entry per row of the sector; n_sites up to 48) over 64-bit site masks: <D_t> = diag[t] / (N norm2) with
    N = n_sites / cell.  The definition the device call is held against."""
    is_complex = np.iscomplexobj(x)
    x = np.ascontiguousarray(x, np.complex128 if is_complex else np.float64).reshape(-1)
    keep, n, ptr = _mask_list64(masks)
    if x.size != spin_momentum64_dim(n_sites, n_up, momentum, cell):  # the library cannot see the length
        raise ValueError("x needs one entry per row of the momentum sector")
    diag, norm2 = np.zeros(n, np.float64), C.c_double()
    _chk(lib().eigenex_spin_momentum_measure_host(int(n_sites), int(n_up), int(cell), int(momentum), int(is_complex), _d(x.view(np.float64)), n, ptr,
                                                  _d(diag) if n else None, C.byref(norm2)))
    return diag, norm2.value


def _cell_coefficients(cell_coef, imaginary="auto"):
    """cell coefficients as (re, im or None): 48 doubles each, so that the library never reads past what the caller handed over"""
    coef = np.asarray(cell_coef).reshape(-1)
    with_im = np.iscomplexobj(coef) if imaginary == "auto" else bool(imaginary)
    cr, ci = np.zeros(max(48, coef.size)), np.zeros(max(48, coef.size))
    cr[:coef.size], ci[:coef.size] = coef.real, coef.imag
    return cr, (ci if with_im else None)


def spin_momentum_site_apply_host(n_sites: int, n_up: int, momentum: int, kind: int, cell_coef, p: int, x, cell: int = 1, imaginary="auto",
                                  in_place: bool = False):
    """eigenex_spin_momentum_site_apply_host: (y, norm2) of the sum of site operators (kind, cell_coef, p) applied to the vector x of
    the momentum sector (n_sites, n_up, cell, momentum), n_sites up to 48; y lives in the sector (n_up', (momentum - p) mod N).  x
    float64: the real form (real momenta and coefficients only); complex128 else.  The definition the device call is held against.
    in_place hands x over as y (Z with p = 0 only)."""
    is_complex = np.iscomplexobj(x)
    x = np.ascontiguousarray(x, np.complex128 if is_complex else np.float64).reshape(-1)
    cr, ci = _cell_coefficients(cell_coef, imaginary)
    n_trans = n_sites // cell if cell > 0 and n_sites % cell == 0 else 0
    dst = None
    if n_trans and int(kind) in (0, 1, 2):
        try:  # the library cannot see the lengths; where the sectors do not exist, its own refusal is what the caller gets
            if x.size != spin_momentum64_dim(n_sites, n_up, momentum, cell):
                raise ValueError("x needs one entry per row of the source sector")
            dst = spin_momentum64_dim(n_sites, n_up + (0, 1, -1)[int(kind)], (momentum - p) % n_trans, cell)
        except EigenexError:
            dst = None
    y = x if in_place else np.zeros(dst if dst is not None else 1, x.dtype)
    norm2 = C.c_double()
    _chk(lib().eigenex_spin_momentum_site_apply_host(int(n_sites), int(n_up), int(cell), int(momentum), int(kind), int(p), int(is_complex), _d(cr),
                                                     _d(ci) if ci is not None else None, _d(x.view(np.float64)), _d(y.view(np.float64)),
                                                     C.byref(norm2)))
    return y, norm2.value


def _mask_list(masks):
    """a list of 32-bit site masks as (keep-alive array, count, pointer or None)"""
    m = np.ascontiguousarray(masks, np.uint32).reshape(-1)
    return m, int(m.size), (m.ctypes.data_as(_up) if m.size else None)


def _spin_measure_host(entry, dtype, n_sites, n_up, x, diag_masks, flip_masks):
    """spin_measure_host and spin_measure_host_z: x as dtype, handed over as doubles"""
    x = np.ascontiguousarray(x, dtype)
    dm, nd, dp = _mask_list(diag_masks)
    fm, nf, fp = _mask_list(flip_masks)
    diag, flip, norm2 = np.zeros(nd), np.zeros(nf), C.c_double()
    _chk(entry(int(n_sites), -1 if n_up is None else int(n_up), _d(x.view(np.float64)), nd, dp, nf, fp, _d(diag) if nd else None,
               _d(flip) if nf else None, C.byref(norm2)))
    return diag, flip, norm2.value


def spin_measure_host(n_sites: int, n_up, x, diag_masks, flip_masks):
    """eigenex_spin_measure_host: the raw sums (diag, flip, norm2) of the masks over the real vector x, in host code (no GPU).
    n_up = None: the full space (x has 2^n_sites entries), else the sector of n_up sites up (C(n_sites, n_up) entries)."""
    return _spin_measure_host(lib().eigenex_spin_measure_host, np.float64, n_sites, n_up, x, diag_masks, flip_masks)


def spin_measure_host_z(n_sites: int, n_up, x, diag_masks, flip_masks):
    """eigenex_spin_measure_host_z: the Hermitian raw sums (diag, flip, norm2) of the masks over the complex vector x, in host code
    (no GPU); n_up as for spin_measure_host."""
    return _spin_measure_host(lib().eigenex_spin_measure_host_z, np.complex128, n_sites, n_up, x, diag_masks, flip_masks)


def spin_measure_columns_host(n_sites: int, n_up, x, columns, diag_masks, flip_masks):
    """eigenex_spin_measure_columns_host: the raw sums (diag[n_diag, count], flip[n_flip, count]) = <V_j| A_t |x> of the masks, in
    host code (no GPU).  columns[j] is column V_j, a (count, rows) array; n_up as for spin_measure_host."""
    x = np.ascontiguousarray(x, np.float64)
    v = np.ascontiguousarray(columns, np.float64)
    if v.ndim != 2 or x.ndim != 1 or v.shape[1] != x.size:
        raise ValueError("columns must be a (count, rows) array with the rows of x")
    count = int(v.shape[0])
    dm, nd, dp = _mask_list(diag_masks)
    fm, nf, fp = _mask_list(flip_masks)
    diag, flip = np.zeros((nd, count)), np.zeros((nf, count))
    _chk(lib().eigenex_spin_measure_columns_host(int(n_sites), -1 if n_up is None else int(n_up), _d(x), _d(v), int(v.shape[1]), count, nd, dp, nf, fp,
                                                 _d(diag) if diag.size else None, _d(flip) if flip.size else None))
    return diag, flip


def spin_rdm_layout(n_sites: int, n_up, mask_a: int):
    """eigenex_spin_rdm_layout: (k_first, dims, offsets) of the reduced density matrix of the subsystem mask_a -- block n has k_first
    + n up sites inside the subsystem (one block, k_first = 0, in the full space: n_up = None), dims[n] rows and starts at offsets[n]
    of the packed output, whose length is offsets[-1].  Host code, no GPU."""
    nb, kf = C.c_int(), C.c_int()
    dims, offs = np.zeros(33, np.int64), np.zeros(34, np.int64)
    _chk(lib().eigenex_spin_rdm_layout(int(n_sites), -1 if n_up is None else int(n_up), int(mask_a), C.byref(nb), C.byref(kf),
                                       dims.ctypes.data_as(_lp), offs.ctypes.data_as(_lp)))
    return kf.value, [int(d) for d in dims[: nb.value]], [int(o) for o in offs[: nb.value + 1]]


def _rdm_blocks(k_first, dims, offsets, out, dtype):
    """the packed column-major blocks (doubles; of a complex dtype interleaved pairs) as [(k, ndarray(d, d), dtype), ...] (copies)"""
    z = out.view(dtype)
    return [(k_first + n, z[offsets[n] : offsets[n + 1]].reshape(d, d).T.copy()) for n, d in enumerate(dims)]


def _spin_rdm_host(name, dtype, n_sites, n_up, x, mask_a):
    """spin_rdm_host and spin_rdm_host_z: x as dtype, x and the result handed over as doubles"""
    x = np.ascontiguousarray(x, dtype)
    kf, dims, offs = spin_rdm_layout(n_sites, n_up, mask_a)
    if x.size != (1 << int(n_sites) if n_up is None else spin_sector_dim(n_sites, n_up)):  # the library cannot see the length
        raise EigenexError(name + ": x must have one entry per row of the geometry")
    out = np.zeros(offs[-1], dtype).view(np.float64)
    _chk(getattr(lib(), "eigenex_" + name)(int(n_sites), -1 if n_up is None else int(n_up), _d(x.view(np.float64)), int(mask_a), _d(out), out.size))
    return _rdm_blocks(kf, dims, offs, out, dtype)


def spin_rdm_host(n_sites: int, n_up, x, mask_a: int):
    """eigenex_spin_rdm_host: the raw, unnormalised reduced density matrix of the subsystem mask_a of the real vector x as a list
    of (k, ndarray(d_k, d_k)), in host code (no GPU).  n_up = None: the full space (one block, k = 0)."""
    return _spin_rdm_host("spin_rdm_host", np.float64, n_sites, n_up, x, mask_a)


def spin_rdm_host_z(n_sites: int, n_up, x, mask_a: int):
    """eigenex_spin_rdm_host_z: the raw, unnormalised reduced density matrix M M^H of the subsystem mask_a of the complex vector
    x as a list of (k, ndarray(d_k, d_k), complex128), in host code (no GPU).  n_up = None: the full space (one block, k = 0)."""
    return _spin_rdm_host("spin_rdm_host_z", np.complex128, n_sites, n_up, x, mask_a)


def spin_site_apply_host(n_sites: int, n_up, kind: int, coef, x):
    """eigenex_spin_site_apply_host: (y, norm2) of y = O x for the sum of site operators (kind, coef), in host code (no GPU).
    n_up = None: the full space; else x lives on the sector of n_up sites up and y on the sector the kind leads to (Z: the same,
    PLUS: n_up + 1, MINUS: n_up - 1)."""
    x = np.ascontiguousarray(x, np.float64)
    coef = np.ascontiguousarray(coef, np.float64)
    if coef.size < int(n_sites):  # the library reads n_sites entries
        raise EigenexError("spin_site_apply_host: coef has fewer entries than n_sites")
    if n_up is None:
        rows = 1 << max(int(n_sites), 0) if int(n_sites) <= 30 else 0
    else:
        up = int(n_up) + (1 if kind == SPIN_SITE_PLUS else -1 if kind == SPIN_SITE_MINUS else 0)
        rows = spin_sector_dim(n_sites, up) if 2 <= int(n_sites) <= 32 and 0 <= up <= int(n_sites) else 0
    y, norm2 = np.zeros(rows), C.c_double()
    _chk(lib().eigenex_spin_site_apply_host(int(n_sites), -1 if n_up is None else int(n_up), int(kind), _d(coef), _d(x), _d(y), C.byref(norm2)))
    return y, norm2.value


def spin_site_apply_host_z(n_sites: int, n_up, kind: int, coef, x, imaginary="auto"):
    """eigenex_spin_site_apply_host_z: (y, norm2) of y = O x for a complex vector x and real or complex coefficients, in host code
    (no GPU); geometry as for spin_site_apply_host.  imaginary: "auto" hands the imaginary parts over when coef is a complex
    array and NULL otherwise, True always hands them over (zeros for a real coef), False never."""
    x = np.ascontiguousarray(x, np.complex128)
    coef = np.asarray(coef)
    if coef.size < int(n_sites):  # the library reads n_sites entries
        raise EigenexError("spin_site_apply_host_z: coef has fewer entries than n_sites")
    with_im = np.iscomplexobj(coef) if imaginary == "auto" else bool(imaginary)
    cr, ci = np.ascontiguousarray(coef.real, np.float64), np.ascontiguousarray(coef.imag, np.float64)
    if n_up is None:
        rows = 1 << max(int(n_sites), 0) if int(n_sites) <= 30 else 0
    else:
        up = int(n_up) + (1 if kind == SPIN_SITE_PLUS else -1 if kind == SPIN_SITE_MINUS else 0)
        rows = spin_sector_dim(n_sites, up) if 2 <= int(n_sites) <= 32 and 0 <= up <= int(n_sites) else 0
    y, norm2 = np.zeros(rows, np.complex128), C.c_double()
    _chk(lib().eigenex_spin_site_apply_host_z(int(n_sites), -1 if n_up is None else int(n_up), int(kind), _d(cr), _d(ci) if with_im else None,
                                              _d(x.view(np.float64)), _d(y.view(np.float64)), C.byref(norm2)))
    return y, norm2.value


class ShardPlan:
    """eigenex_plan_*: the host-side plan of one CSR row shard (no GPU).  rowptr relative to the shard's first row,
    col with GLOBAL column indices."""

    def __init__(self, n_global: int, nshards: int, shard: int, rowptr, col_global):
        self.h = _vp()
        rp = np.ascontiguousarray(rowptr, np.int32)
        cl = np.ascontiguousarray(col_global, np.int32)
        _chk(lib().eigenex_plan_create(n_global, nshards, shard, _i(rp), _i(cl), C.byref(self.h)))

    def sizes(self):
        a = [C.c_int64() for _ in range(4)]
        b = [C.c_int() for _ in range(2)]
        c = C.c_int64()
        _chk(lib().eigenex_plan_sizes(self.h, *[C.byref(x) for x in a], *[C.byref(x) for x in b], C.byref(c)))
        return dict(n_local=a[0].value, n_pad=a[1].value, nnz=a[2].value, n_halo=a[3].value, n_recv=b[0].value, n_send=b[1].value,
                    n_send_rows=c.value)

    def local_columns(self):
        out = np.zeros(max(self.sizes()["nnz"], 1), np.int32)
        _chk(lib().eigenex_plan_local_columns(self.h, _i(out)))
        return out[: self.sizes()["nnz"]]

    def tiles(self):
        """(interior, boundary): the 256-row tiles that read no halo column / at least one (eigenex_plan_tiles)"""
        ni, nb = C.c_int64(), C.c_int64()
        _chk(lib().eigenex_plan_tiles(self.h, None, C.byref(ni), None, C.byref(nb)))
        ti, tb = np.zeros(max(ni.value, 1), np.int32), np.zeros(max(nb.value, 1), np.int32)
        _chk(lib().eigenex_plan_tiles(self.h, _i(ti), C.byref(ni), _i(tb), C.byref(nb)))
        return ti[:ni.value], tb[:nb.value]

    def halo_columns(self):
        out = np.zeros(max(self.sizes()["n_halo"], 1), np.int32)
        _chk(lib().eigenex_plan_halo_columns(self.h, _i(out)))
        return out[: self.sizes()["n_halo"]]

    def recv_segments(self):
        n = self.sizes()["n_recv"]
        peer, off, cnt = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        _chk(lib().eigenex_plan_recv_segments(self.h, _i(peer), off.ctypes.data_as(_lp), cnt.ctypes.data_as(_lp)))
        return [(int(peer[i]), int(off[i]), int(cnt[i])) for i in range(n)]

    def add_request(self, from_shard: int, rows_global):
        r = np.ascontiguousarray(rows_global, np.int32)
        _chk(lib().eigenex_plan_add_request(self.h, from_shard, _i(r), r.size))

    def send_segments(self):
        n = self.sizes()["n_send"]
        peer = np.zeros(max(n, 1), np.int32)
        off, cnt, cs = (np.zeros(max(n, 1), np.int64) for _ in range(3))
        _chk(lib().eigenex_plan_send_segments(self.h, _i(peer), *[x.ctypes.data_as(_lp) for x in (off, cnt, cs)]))
        return [(int(peer[i]), int(off[i]), int(cnt[i]), int(cs[i])) for i in range(n)]

    def send_rows(self):
        n = self.sizes()["n_send_rows"]
        out = np.zeros(max(n, 1), np.int32)
        _chk(lib().eigenex_plan_send_rows(self.h, _i(out)))
        return out[:n]

    def close(self):
        if self.h:
            lib().eigenex_plan_destroy(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rccl_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    _chk(lib().eigenex_rccl_unique_id(buf))
    return buf.raw


class Context:
    def __init__(self, device=0, rank=0, world_size=1, rccl_id: bytes | None = None, loopback_shards: int = 0):
        self.h = _vp()
        if loopback_shards:
            _chk(lib().eigenex_context_create_loopback(device, loopback_shards, C.byref(self.h)))
        else:
            idbuf = C.create_string_buffer(rccl_id, 128) if rccl_id else None
            _chk(lib().eigenex_context_create(device, rank, world_size, idbuf, C.byref(self.h)))

    def info(self):
        v = [C.c_int() for _ in range(4)]
        _chk(lib().eigenex_context_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("rank", "world_size", "nshards_total", "nshards_local"), (x.value for x in v)))

    def trace(self, on=True):
        _chk(lib().eigenex_context_trace(self.h, int(on)))

    def set_halo_overlap(self, on=True) -> bool:
        """neighbour exchange beside the interior rows (True) or in front of the operator (False); returns what is in force"""
        rc = lib().eigenex_context_set_halo_overlap(self.h, int(on))
        if rc < 0:
            _chk(rc)
        return rc == 1

    def trace_get(self):
        n = C.c_int()
        _chk(lib().eigenex_context_trace_get(self.h, None, None, 0, C.byref(n)))
        ops, cnt = np.zeros(max(n.value, 1), np.int32), np.zeros(max(n.value, 1), np.int32)
        _chk(lib().eigenex_context_trace_get(self.h, _i(ops), _i(cnt), ops.size, C.byref(n)))
        return [(int(ops[i]), int(cnt[i])) for i in range(n.value)]

    def comm_info(self):
        """(ranks, rank, device) as the RCCL communicator reports them; ranks = 0 without a communicator"""
        v = [C.c_int() for _ in range(3)]
        _chk(lib().eigenex_context_comm_info(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def sync(self):
        _chk(lib().eigenex_context_sync(self.h))

    def rccl_selftest(self) -> bool:
        ok = C.c_int(0)
        _chk(lib().eigenex_context_selftest(self.h, C.byref(ok)))
        return bool(ok.value)

    def profile_enable(self, on=True):
        _chk(lib().eigenex_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        _chk(lib().eigenex_profile_reset(self.h))

    def profile_get(self, kind: int):
        n, ms, by = C.c_int64(), C.c_double(), C.c_double()
        _chk(lib().eigenex_profile_get(self.h, kind, C.byref(n), C.byref(ms), C.byref(by)))
        return n.value, ms.value, by.value

    def close(self):
        if self.h:
            lib().eigenex_context_destroy(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Csr:
    def __init__(self, ctx: Context, handle):
        self.ctx, self.h = ctx, handle

    @classmethod
    def upload(cls, ctx: Context, n_global: int, rowptr, col, val, row_begin: int = 0, column_blocks: int | None = None):
        """val real (float64) or complex (complex128: uploaded as interleaved pairs, eigenex_csr_upload_z).
        column_blocks: None = the plain entry points (automatic choice), else eigenex_csr_upload_ex's argument."""
        rp = np.ascontiguousarray(rowptr, np.int32)
        cl = np.ascontiguousarray(col, np.int32)
        h = _vp()
        cplx = bool(np.iscomplexobj(val))
        vl = np.ascontiguousarray(val, np.complex128 if cplx else np.float64)
        vp = _d(vl.view(np.float64))
        if column_blocks is not None:
            _chk(lib().eigenex_csr_upload_ex(ctx.h, n_global, row_begin, rp.size - 1, _i(rp), _i(cl), vp, int(cplx), int(column_blocks), C.byref(h)))
        elif cplx:
            _chk(lib().eigenex_csr_upload_z(ctx.h, n_global, row_begin, rp.size - 1, _i(rp), _i(cl), vp, C.byref(h)))
        else:
            _chk(lib().eigenex_csr_upload(ctx.h, n_global, row_begin, rp.size - 1, _i(rp), _i(cl), vp, C.byref(h)))
        obj = cls(ctx, h)
        obj.is_complex = bool(np.iscomplexobj(val))
        return obj

    @classmethod
    def upload64(cls, ctx: Context, n_global: int, rowptr, col, val, row_begin: int = 0):
        """eigenex_csr_upload64: real CSR with 64-bit row pointers (shards of >= 2^31 stored entries are kept as plain CSR with
        64-bit row pointers on the device, smaller ones exactly as `upload` stores them)."""
        rp = np.ascontiguousarray(rowptr, np.int64)
        cl = np.ascontiguousarray(col, np.int32)
        vl = np.ascontiguousarray(val, np.float64)
        h = _vp()
        _chk(lib().eigenex_csr_upload64(ctx.h, n_global, row_begin, rp.size - 1, rp.ctypes.data_as(C.POINTER(C.c_int64)), _i(cl), _d(vl), C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_device(cls, ctx: Context, n: int, rowptr_ptr: int, col_ptr: int, val_ptr: int, is_complex: bool = False):
        """eigenex_csr_upload_device: CSR arrays already on this GPU, given as raw device addresses
        (e.g. torch tensors' .data_ptr(): int32 rowptr[n+1], int32 col[nnz], float64/complex128 val[nnz])."""
        h = _vp()
        _chk(lib().eigenex_csr_upload_device(ctx.h, n, _vp(rowptr_ptr), _vp(col_ptr), _vp(val_ptr), int(is_complex), C.byref(h)))
        obj = cls(ctx, h)
        obj.is_complex = bool(is_complex)
        return obj

    @classmethod
    def upload_blocks(cls, ctx: Context, row_sizes, col_sizes, blocks):
        """eigenex_block_upload[_z]: blocks = {(qr, qc): 2-D array of shape (row_sizes[qr], col_sizes[qc])}, all real
        (float64) or, if any is complex, all uploaded as complex128."""
        rs = np.ascontiguousarray(row_sizes, np.int64)
        cs = np.ascontiguousarray(col_sizes, np.int64)
        keys = list(blocks.keys())
        cplx = any(np.iscomplexobj(blocks[k]) for k in keys)
        dt = np.complex128 if cplx else np.float64
        mats = []
        for (r, c) in keys:
            m = np.asfortranarray(blocks[(r, c)], dt)
            if not (0 <= r < rs.size and 0 <= c < cs.size) or m.shape != (rs[r], cs[c]):
                raise ValueError(f"block ({r}, {c}): shape {m.shape} does not match the partition")
            mats.append(m)
        qr = np.array([k[0] for k in keys], np.int64)
        qc = np.array([k[1] for k in keys], np.int64)
        ptrs = (C.c_void_p * max(len(mats), 1))(*[m.ctypes.data for m in mats])
        h = _vp()
        fn = lib().eigenex_block_upload_z if cplx else lib().eigenex_block_upload
        _chk(fn(ctx.h, int(rs.sum()), rs.size, rs.ctypes.data_as(_lp), cs.size, cs.ctypes.data_as(_lp),
                len(mats), qr.ctypes.data_as(_lp), qc.ctypes.data_as(_lp), ptrs, C.byref(h)))
        obj = cls(ctx, h)
        obj.is_complex = cplx
        return obj

    @classmethod
    def upload_blocks_raw(cls, ctx: Context, row_sizes, col_sizes, qr, qc, values, offsets):
        """eigenex_block_upload for many blocks without a Python object per block: block k is the column-major
        array starting at values[offsets[k]] (values: one contiguous float64 array)."""
        rs = np.ascontiguousarray(row_sizes, np.int64)
        cs = np.ascontiguousarray(col_sizes, np.int64)
        qr = np.ascontiguousarray(qr, np.int64)
        qc = np.ascontiguousarray(qc, np.int64)
        values = np.ascontiguousarray(values, np.float64)
        offsets = np.ascontiguousarray(offsets, np.int64)
        sizes = rs[qr] * cs[qc]
        if qr.size and (offsets.min() < 0 or (offsets + sizes).max() > values.size):
            raise ValueError("a block reaches outside the value array")
        ptrs = (values.ctypes.data + 8 * offsets).astype(np.uint64)
        h = _vp()
        _chk(lib().eigenex_block_upload(ctx.h, int(rs.sum()), rs.size, rs.ctypes.data_as(_lp), cs.size, cs.ctypes.data_as(_lp),
                                        qr.size, qr.ctypes.data_as(_lp), qc.ctypes.data_as(_lp),
                                        C.cast(ptrs.ctypes.data, C.POINTER(C.c_void_p)), C.byref(h)))
        obj = cls(ctx, h)
        obj.is_complex = False
        return obj

    @classmethod
    def spin_half(cls, ctx: Context, n_sites: int, bonds, hz=None, hx=None, complex_states=False):
        """eigenex_spin_upload: the spin-1/2 Hamiltonian on n_sites sites, applied matrix-free (nothing is stored).
        bonds = [(i, j, Jz, Jxy), ...]; hz, hx = n_sites fields or None.  complex_states: eigenex_spin_upload_z, the same
        Hamiltonian as a handle for complex states."""
        keep, args = _spin_model(n_sites, bonds, hz, hx)
        h = _vp()
        _chk((lib().eigenex_spin_upload_z if complex_states else lib().eigenex_spin_upload)(ctx.h, *args, C.byref(h)))
        obj = cls(ctx, h)
        obj.is_complex = bool(complex_states)
        return obj

    @classmethod
    def spin_half_sector(cls, ctx: Context, n_sites: int, n_up: int, bonds, hz=None, hx=None, complex_states=False):
        """eigenex_spin_sector_upload: the same Hamiltonian in the sector of n_up sites up (n_sites up to 32, C(n_sites, n_up)
        rows), applied matrix-free.  The model must conserve Sz: hx is None or all zeros.  complex_states:
        eigenex_spin_sector_upload_z."""
        keep, args = _spin_model(n_sites, bonds, hz, hx)
        h = _vp()
        _chk((lib().eigenex_spin_sector_upload_z if complex_states else lib().eigenex_spin_sector_upload)(ctx.h, *_sector_args(args, n_up), C.byref(h)))
        obj = cls(ctx, h)
        obj.is_complex = bool(complex_states)
        return obj

    @classmethod
    def spin_half_momentum(cls, ctx: Context, n_sites: int, n_up: int, momentum: int, bonds, hz=None, cell: int = 1, complex_states=False):
        """eigenex_spin_momentum_upload: the same Hamiltonian in the momentum sector `momentum` (0 .. n_sites/cell - 1) of the
        sector of n_up sites up, applied matrix-free.  The model must be invariant under the translation by `cell` sites.  Real
        states take a real momentum only (0 or half the number of translations); complex_states:
        eigenex_spin_momentum_upload_z, any momentum.  Every argument is checked before ctx is looked at."""
        keep, args = _spin_model(n_sites, bonds, hz, None)
        h = _vp()
        entry = lib().eigenex_spin_momentum_upload_z if complex_states else lib().eigenex_spin_momentum_upload
        _chk(entry(ctx.h if ctx is not None else None, *_momentum_args(args, n_up, cell, momentum), C.byref(h)))
        obj = cls(ctx, h)
        obj.is_complex = bool(complex_states)
        return obj

    @classmethod
    def spin_half_momentum64(cls, ctx: Context, n_sites: int, n_up: int, momentum: int, bonds, hz=None, cell: int = 1, complex_states=False):
        """eigenex_spin_momentum64_upload: spin_half_momentum for rings of up to 48 sites and 128 bonds, with 64-bit states
        (complex_states: eigenex_spin_momentum64_upload_z).  Every argument is checked before ctx is looked at."""
        keep, args = _spin_model(n_sites, bonds, hz, None)
        h = _vp()
        entry = lib().eigenex_spin_momentum64_upload_z if complex_states else lib().eigenex_spin_momentum64_upload
        _chk(entry(ctx.h if ctx is not None else None, *_momentum_args(args, n_up, cell, momentum), C.byref(h)))
        obj = cls(ctx, h)
        obj.is_complex = bool(complex_states)
        return obj

    @classmethod
    def laplacian3d(cls, ctx: Context, n: int):
        h = _vp()
        _chk(lib().eigenex_csr_laplacian3d(ctx.h, n, C.byref(h)))
        return cls(ctx, h)

    def layout(self) -> str:
        v = C.c_int()
        _chk(lib().eigenex_csr_layout(self.h, C.byref(v)))
        return ("csr", "column_blocked", "sorted_tiles", "dense_blocks", "split_tiles", "matrix_free_spin", "matrix_free_spin_sector",
                "matrix_free_spin_momentum", "matrix_free_spin_momentum64")[v.value]

    def spin_momentum_geometry(self):
        """eigenex_spin_momentum_geometry: (n_sites, n_up, cell, momentum) of a momentum-sector operator"""
        out = [C.c_int() for _ in range(4)]
        _chk(lib().eigenex_spin_momentum_geometry(self.h, *[C.byref(v) for v in out]))
        return tuple(v.value for v in out)

    def spin_geometry(self):
        """eigenex_spin_geometry: (n_sites, n_up) of a matrix-free spin operator, n_up = None for the full space"""
        ns, nu = C.c_int(), C.c_int()
        _chk(lib().eigenex_spin_geometry(self.h, C.byref(ns), C.byref(nu)))
        return ns.value, (None if nu.value < 0 else nu.value)

    def encoding(self) -> str:
        """"plain" or "row_codes" (include/eigenex_hip.h: eigenex_csr_encoding)"""
        v = C.c_int()
        _chk(lib().eigenex_csr_encoding(self.h, C.byref(v)))
        return ("plain", "row_codes")[v.value]

    def column_blocks(self) -> int:
        k = C.c_int()
        _chk(lib().eigenex_csr_column_blocks(self.h, C.byref(k)))
        return k.value

    def info(self):
        v = [C.c_int64() for _ in range(4)]
        _chk(lib().eigenex_csr_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("n_global", "n_local", "nnz_local", "n_halo_local"), (x.value for x in v)))

    def close(self):
        if self.h:
            lib().eigenex_csr_destroy(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Basis:
    """Krylov state on the device (basis slab, work vectors, coefficient arrays).
    dtype float64 or complex128 (taken from the CSR operator when one is given)."""

    def __init__(self, ctx: Context, csr: Csr | None, n_global: int, capacity: int, n_ortho: int = 0, dtype=None):
        self.ctx, self.csr, self.n_global, self.capacity, self.n_ortho = ctx, csr, n_global, capacity, n_ortho
        if dtype is None:
            dtype = np.complex128 if (csr is not None and getattr(csr, "is_complex", False)) else np.float64
        self.dtype = np.dtype(dtype)
        self.is_complex = self.dtype.kind == "c"
        self.h = _vp()
        _chk(lib().eigenex_basis_create_ex(ctx.h, csr.h if csr else None, n_global, capacity, n_ortho,
                                           1 if self.is_complex else 0, C.byref(self.h)))
        info = ctx.info()
        if info["nshards_local"] == info["nshards_total"]:
            self.n_rows = n_global
        else:
            b, e = partition(n_global, info["world_size"], info["rank"])
            self.n_rows = e - b
        self._cb = None

    def _vec(self, x):
        x = np.ascontiguousarray(x, self.dtype)
        return x, _d(x.view(np.float64))

    def configure(self, shift=0.0, threshold=1e-12, interval=1, ortho_mode=ORTHO_BATCHED):
        sh = complex(shift)
        _chk(lib().eigenex_basis_configure_z(self.h, sh.real, sh.imag, threshold, interval, ortho_mode))

    def set_host_operator(self, fn):
        """fn(x: ndarray) -> ndarray  (the reference's MatMulFunction, lanczos.hpp:116)."""
        n, es, dt = self.n_rows, (2 if self.is_complex else 1), self.dtype

        def tramp(pin, pout, _user):
            x = np.ctypeslib.as_array(pin, shape=(n * es,)).view(dt)
            y = np.ctypeslib.as_array(pout, shape=(n * es,)).view(dt)
            y[:] = fn(x)

        self._cb = MATVEC_FN(tramp)
        _chk(lib().eigenex_basis_set_host_operator(self.h, self._cb, None))

    def tune(self, vec_blocks_per_cu=2, spmv_blocks_per_cu=4, flags=0):
        _chk(lib().eigenex_basis_tune(self.h, vec_blocks_per_cu, spmv_blocks_per_cu, flags))

    def graph_info(self):
        n, t, lim = C.c_int(), C.c_int64(), C.c_int64()
        _chk(lib().eigenex_basis_graph_info(self.h, C.byref(n), C.byref(t), C.byref(lim)))
        return dict(graphs=n.value, nodes=t.value, node_limit=lim.value)

    def repairs(self) -> int:
        """one-sweep Lanczos steps since the last clear whose pending vector the guard re-orthogonalised with the two-sweep pass"""
        n = C.c_int()
        _chk(lib().eigenex_basis_repairs(self.h, C.byref(n)))
        return n.value

    def close_pending(self) -> bool:
        """the last batch of one-sweep Lanczos steps has left its newest column to be written by the next call that needs it"""
        n = C.c_int()
        _chk(lib().eigenex_basis_close_pending(self.h, C.byref(n)))
        return bool(n.value)

    def set_alpha_fusion(self, on: bool):
        _chk(lib().eigenex_basis_set_alpha_fusion(self.h, int(bool(on))))

    def clear(self):
        _chk(lib().eigenex_basis_clear(self.h))

    def upload(self, ref: int, x):
        x, p = self._vec(x)
        assert x.size == self.n_rows
        _chk(lib().eigenex_vec_upload(self.h, ref, p))

    def copy(self, dst_ref: int, src_ref: int):
        _chk(lib().eigenex_vec_copy(self.h, dst_ref, src_ref))

    def clone(self):
        """eigenex_basis_clone: a deep copy of this state on the device (same context and operator)"""
        other = Basis.__new__(Basis)
        other.__dict__.update(self.__dict__)
        other.h, other._cb = _vp(), None
        _chk(lib().eigenex_basis_clone(self.h, C.byref(other.h)))
        return other

    def reserve(self, capacity: int):
        _chk(lib().eigenex_basis_reserve(self.h, capacity))
        self.capacity = max(self.capacity, capacity)

    def download(self, ref: int):
        x = np.empty(self.n_rows, self.dtype)
        _chk(lib().eigenex_vec_download(self.h, ref, _d(x.view(np.float64))))
        return x

    # -- primitives
    def apply(self, x_ref, y_ref, shift=0.0, want_dot=False):
        d = np.zeros(1, self.dtype)
        _chk(lib().eigenex_apply(self.h, x_ref, y_ref, shift, _d(d.view(np.float64)) if want_dot else None))
        return d[0] if want_dot else None

    def spin_measure(self, x_ref, diag_masks, flip_masks):
        """eigenex_spin_measure: the raw sums (diag, flip, norm2) of the site masks over the vector x_ref, in one sweep on the
        device; the operator of this state must be a matrix-free spin operator.  No vector and no coefficient changes."""
        dm, nd, dp = _mask_list(diag_masks)
        fm, nf, fp = _mask_list(flip_masks)
        diag, flip, norm2 = np.zeros(nd), np.zeros(nf), C.c_double()
        _chk(lib().eigenex_spin_measure(self.h, x_ref, nd, dp, nf, fp, _d(diag) if nd else None, _d(flip) if nf else None, C.byref(norm2)))
        return diag, flip, norm2.value

    def spin_measure_columns(self, x_ref, first, count, diag_masks, flip_masks):
        """eigenex_spin_measure_columns: (diag[n_diag, count], flip[n_flip, count]) = <V_j| A_t |x_ref> against the basis columns
        first .. first + count - 1, the basis streaming past once per 16 terms; real states of matrix-free spin operators.  A pending
        newest column is closed first if the call reads it; nothing else of the state changes."""
        dm, nd, dp = _mask_list(diag_masks)
        fm, nf, fp = _mask_list(flip_masks)
        count = int(count)
        diag, flip = np.zeros((nd, max(count, 0))), np.zeros((nf, max(count, 0)))
        _chk(lib().eigenex_spin_measure_columns(self.h, x_ref, int(first), count, nd, dp, nf, fp, _d(diag) if diag.size else None,
                                                _d(flip) if flip.size else None))
        return diag, flip

    def _spin_rdm(self, entry, dtype, x_ref, mask_a):
        """spin_rdm and spin_rdm_z: the result is handed over as doubles and returned as blocks of dtype"""
        ns, nu = C.c_int(), C.c_int()
        if self.csr is None or lib().eigenex_spin_geometry(self.csr.h, C.byref(ns), C.byref(nu)) != 0:
            _chk(entry(self.h, x_ref, int(mask_a), None, 0))  # the library says what is wrong with the state
        try:
            kf, dims, offs = spin_rdm_layout(ns.value, None if nu.value < 0 else nu.value, mask_a)
        except EigenexError:
            _chk(entry(self.h, x_ref, int(mask_a), None, 0))  # the same refusal under the entry point's own name
            raise
        out = np.zeros(offs[-1], dtype).view(np.float64)
        _chk(entry(self.h, x_ref, int(mask_a), _d(out), out.size))
        return _rdm_blocks(kf, dims, offs, out, dtype)

    def spin_rdm(self, x_ref, mask_a):
        """eigenex_spin_rdm: the raw, unnormalised reduced density matrix of the subsystem mask_a of the vector x_ref, formed on
        the device, as a list of (k, ndarray(d_k, d_k)); the operator of this state must be a matrix-free spin operator.  No
        vector and no coefficient changes."""
        return self._spin_rdm(lib().eigenex_spin_rdm, np.float64, x_ref, mask_a)

    def spin_rdm_z(self, x_ref, mask_a):
        """eigenex_spin_rdm_z: the raw, unnormalised reduced density matrix M M^H of the subsystem mask_a of the complex vector
        x_ref, formed on the device, as a list of (k, ndarray(d_k, d_k), complex128); the state must be a complex one on a
        matrix-free spin operator for complex states.  No vector and no coefficient changes."""
        return self._spin_rdm(lib().eigenex_spin_rdm_z, np.complex128, x_ref, mask_a)

    def spin_site_apply(self, x_ref, dst, y_ref, kind, coef):
        """eigenex_spin_site_apply: vector y_ref of the state dst = (sum of site operators kind, coef) applied to vector x_ref of
        this state, on the device; returns norm2 = |y|^2.  Both states need matrix-free spin operators of one context whose
        geometries fit the kind; dst may be this state.  No coefficient, counter or recorded step batch changes."""
        coef = np.ascontiguousarray(coef, np.float64).reshape(-1)
        buf = np.zeros(max(32, coef.size))  # the library reads n_sites <= 32 entries, whatever the caller handed over
        buf[:coef.size] = coef
        norm2 = C.c_double()
        _chk(lib().eigenex_spin_site_apply(self.h, x_ref, dst.h, y_ref, int(kind), _d(buf), C.byref(norm2)))
        return norm2.value

    def spin_momentum_expand(self, x_ref, dst, y_ref):
        """eigenex_spin_momentum_expand: vector y_ref of the state dst, on a sector operator of the same (n_sites, n_up), scalar
        type and context, = the momentum vector x_ref of this state written out in the Sz sector; returns norm2 = |y|^2.  No
        coefficient, counter or recorded step batch changes."""
        norm2 = C.c_double()
        _chk(lib().eigenex_spin_momentum_expand(self.h, x_ref, dst.h, y_ref, C.byref(norm2)))
        return norm2.value

    def spin_momentum_measure(self, x_ref, masks):
        """eigenex_spin_momentum_measure: (diag, norm2), the raw sums of the diagonal correlations of vector x_ref of this state,
        on a momentum-sector operator of either word size, over 64-bit site masks; <D_t> = diag[t] / (N norm2).  No coefficient,
        counter or recorded step batch changes."""
        keep, n, ptr = _mask_list64(masks)
        diag, norm2 = np.zeros(n, np.float64), C.c_double()
        _chk(lib().eigenex_spin_momentum_measure(self.h, x_ref, n, ptr, _d(diag) if n else None, C.byref(norm2)))
        return diag, norm2.value

    def spin_momentum_site_apply(self, x_ref, dst, y_ref, kind, cell_coef, p=0, imaginary="auto"):
        """eigenex_spin_momentum_site_apply (real states) or eigenex_spin_momentum_site_apply_z (complex states, by this state's
        is_complex): vector y_ref of the state dst, on the momentum sector (n_up', (m - p) mod N) of the same ring, cell and
        word, = (sum of site operators kind with the cell coefficients cell_coef and the momentum index p) applied to vector x_ref
        of this state; returns norm2 = |y|^2.  dst may be this state for Z with p = 0 only.  No coefficient, counter or recorded
        step batch changes."""
        cr, ci = _cell_coefficients(cell_coef, imaginary)
        norm2 = C.c_double()
        if self.is_complex:
            _chk(lib().eigenex_spin_momentum_site_apply_z(self.h, x_ref, dst.h, y_ref, int(kind), int(p), _d(cr), _d(ci) if ci is not None else None,
                                                          C.byref(norm2)))
        else:
            if ci is not None and np.any(ci != 0.0):
                raise ValueError("real states take real cell coefficients")
            _chk(lib().eigenex_spin_momentum_site_apply(self.h, x_ref, dst.h, y_ref, int(kind), int(p), _d(cr), C.byref(norm2)))
        return norm2.value

    def spin_site_apply_z(self, x_ref, dst, y_ref, kind, coef, imaginary="auto"):
        """eigenex_spin_site_apply_z: spin_site_apply for two complex spin states, with real or complex coefficients; returns
        norm2 = |y|^2.  imaginary: "auto" hands the imaginary parts over when coef is a complex array and NULL otherwise, True
        always hands them over (zeros for a real coef), False never."""
        coef = np.asarray(coef).reshape(-1)
        with_im = np.iscomplexobj(coef) if imaginary == "auto" else bool(imaginary)
        cr, ci = np.zeros(max(32, coef.size)), np.zeros(max(32, coef.size))  # the library reads n_sites <= 32 entries
        cr[:coef.size], ci[:coef.size] = coef.real, coef.imag
        norm2 = C.c_double()
        _chk(lib().eigenex_spin_site_apply_z(self.h, x_ref, dst.h, y_ref, int(kind), _d(cr), _d(ci) if with_im else None, C.byref(norm2)))
        return norm2.value

    def set_filter(self, mu, center=0.0, halfwidth=1.0, degree=None):
        """Chebyshev filter p(A) = sum_k mu[k] T_k((A - center)/halfwidth) for the Lanczos steps and filter_apply; mu = None
        (or degree = 0) removes it.  degree defaults to len(mu) - 1 (given explicitly by the argument tests)."""
        if mu is None:
            _chk(lib().eigenex_basis_set_filter(self.h, 0 if degree is None else degree, None, center, halfwidth))
            return
        mu = np.ascontiguousarray(mu, np.float64)
        _chk(lib().eigenex_basis_set_filter(self.h, mu.size - 1 if degree is None else degree, _d(mu), center, halfwidth))

    def filter_apply(self, x_ref, y_ref):
        """y = p(A) x with the filter of set_filter"""
        _chk(lib().eigenex_filter_apply(self.h, x_ref, y_ref))

    def kpm_moments(self, x_ref, n_moments, center, halfwidth):
        """mu[k] = <x| T_k((A - center)/halfwidth) |x>, k < n_moments; VEC_V then holds the last Chebyshev vector"""
        mu = np.zeros(max(int(n_moments), 0), np.float64)
        _chk(lib().eigenex_kpm_moments(self.h, x_ref, n_moments, center, halfwidth, _d(mu) if mu.size else None))
        return mu

    def kpm_trace_moments(self, n_moments, n_vectors, seed, first_stream, center, halfwidth):
        """the moments of n_vectors random-sign vectors (streams first_stream ..), divided by N: array [n_vectors, n_moments]"""
        mu = np.zeros((max(int(n_vectors), 0), max(int(n_moments), 0)), np.float64)
        _chk(lib().eigenex_kpm_trace_moments(self.h, n_moments, n_vectors, seed, first_stream, center, halfwidth, _d(mu) if mu.size else None))
        return mu

    def random_signs(self, x_ref, seed, stream):
        _chk(lib().eigenex_vec_random_signs(self.h, x_ref, seed, stream))

    def dots(self, w_ref, first, stride, count, n_ortho_used=0):
        h = np.zeros(count + n_ortho_used, self.dtype)
        _chk(lib().eigenex_dots(self.h, w_ref, first, stride, count, n_ortho_used, _d(h.view(np.float64))))
        return h

    def update(self, w_ref, first, stride, count, h, n_ortho_used=0):
        h, p = self._vec(h)
        nrm2 = C.c_double()
        _chk(lib().eigenex_update(self.h, w_ref, first, stride, count, n_ortho_used, p if h.size else None, C.byref(nrm2)))
        return nrm2.value

    def axpy2(self, z_ref, x_ref, a, p_ref, b, q_ref):
        _chk(lib().eigenex_axpy2(self.h, z_ref, x_ref, a, p_ref, b, q_ref))

    def scale(self, dst_ref, src_ref, s):
        _chk(lib().eigenex_scale(self.h, dst_ref, src_ref, s))

    # -- fused steps
    def lanczos_enqueue(self, ncalls: int):
        _chk(lib().eigenex_lanczos_enqueue(self.h, ncalls))

    def lanczos_restart(self, S, coupling_last: float):
        """thick restart: keep the Ritz vectors V_m S (S: m x nkeep, real)"""
        S = np.asfortranarray(S, np.float64)
        _chk(lib().eigenex_lanczos_restart(self.h, S.shape[1], _d(S), S.shape[0], float(coupling_last)))

    def arnoldi_enqueue(self, ncalls: int):
        _chk(lib().eigenex_arnoldi_enqueue(self.h, ncalls))

    def arnoldi_restart(self, Q, B, nkeep: int | None = None, ldq: int | None = None, ldb: int | None = None):
        """Krylov-Schur restart: keep V_m Q (Q: m x nkeep) with the projected matrix B ((nkeep+1) x nkeep), both in the
        basis' scalar type.  nkeep / ldq / ldb default to the arrays' shapes (given explicitly by the argument tests)."""
        Q = np.asfortranarray(Q, self.dtype)
        B = np.asfortranarray(B, self.dtype)
        _chk(lib().eigenex_arnoldi_restart(self.h, Q.shape[1] if nkeep is None else nkeep, _d(Q), Q.shape[0] if ldq is None else ldq, _d(B),
                                           B.shape[0] if ldb is None else ldb))

    def arnoldi_projected(self):
        """state and the (nalpha + 1) x nalpha projected matrix as the device stores it, coupling row included"""
        st = State()
        ldh = self.capacity + 2
        H = np.zeros((self.capacity + 1, ldh), self.dtype)  # row c = column c of H
        _chk(lib().eigenex_arnoldi_state(self.h, C.byref(st), _d(H.view(np.float64)), ldh))
        return st, H[: st.nalpha, : st.nalpha + 1].T.copy()

    def lanczos_state(self):
        st = State()
        a = np.zeros(self.capacity + 2)
        b = np.zeros(self.capacity + 2)
        _chk(lib().eigenex_lanczos_state(self.h, C.byref(st), _d(a), _d(b)))
        return st, a[: st.nalpha].copy(), b[: st.nbeta].copy()

    def arnoldi_state(self):
        st = State()
        ldh = self.capacity + 2
        H = np.zeros((self.capacity + 1, ldh), self.dtype)  # row c = column c of H
        _chk(lib().eigenex_arnoldi_state(self.h, C.byref(st), _d(H.view(np.float64)), ldh))
        m = min(st.nalpha, self.n_global)
        return st, H[:m, :m].T.copy()

    @staticmethod
    def _padded(A, ld, dtype):
        """A (rows x cols) copied into the top of a column-major (ld x cols) array whose other rows are NaN"""
        P = np.full((max(ld, A.shape[0]), A.shape[1]), np.nan, dtype, order="F")
        P[: A.shape[0]] = A
        return P

    def _combine(self, nvec, S, lds, ldx, raw):
        nev = S.shape[1]
        cplx = np.iscomplexobj(S)
        S = self._padded(S, S.shape[0] if lds is None else lds, np.complex128 if cplx else np.float64)
        ldx = self.n_rows if ldx is None else ldx
        # the rows n_rows..ldx of each column are a gap the library must not write: NaN sentinels (X.base holds them)
        X = self._padded(np.zeros((self.n_rows, nev)), ldx, np.complex128 if cplx else self.dtype)
        if nev:
            if cplx:
                Sr, Si = np.asfortranarray(S.real), np.asfortranarray(S.imag)
                if raw:
                    _chk(lib().eigenex_krylov_combine(self.h, nvec, nev, _d(Sr), _d(Si), S.shape[0], X.ctypes.data_as(_dp), ldx))
                else:
                    _chk(lib().eigenex_ritz_vectors_complex(self.h, nvec, nev, _d(Sr), _d(Si), S.shape[0],
                                                            X.ctypes.data_as(_dp), ldx))
            elif raw:
                _chk(lib().eigenex_krylov_combine(self.h, nvec, nev, _d(S), None, S.shape[0], X.ctypes.data_as(_dp), ldx))
            else:
                _chk(lib().eigenex_ritz_vectors(self.h, nvec, nev, _d(S), S.shape[0], X.ctypes.data_as(_dp), ldx))
        return X if ldx == self.n_rows else X[: self.n_rows]

    def ritz_vectors(self, nvec: int, S, lds: int | None = None, ldx: int | None = None):
        """X = V S, normalised and phase-fixed.  Real S: X has the basis dtype; complex S: X is complex.
        lds / ldx: column strides handed to the library (default: S's rows, n_rows).  S is passed with NaN in its rows
        past S.shape[0]; X is returned as the top n_rows of an ldx-row array whose gap rows were filled with NaN."""
        return self._combine(nvec, S, lds, ldx, False)

    def krylov_combine(self, nvec: int, C, ldc: int | None = None, ldx: int | None = None):
        """X = V C as it is (eigenex_krylov_combine: no normalisation, no phase).  Real C: X has the basis dtype;
        complex C: X is complex."""
        return self._combine(nvec, C, ldc, ldx, True)

    def krylov_combine_to(self, nvec: int, coef, dst_ref: int):
        """dst = sum_m coef[m] col(m), left on the device (eigenex_krylov_combine_to); complex coef needs a complex state"""
        c = np.asarray(coef).reshape(-1)
        if np.iscomplexobj(c):
            cr, ci = np.ascontiguousarray(c.real, np.float64), np.ascontiguousarray(c.imag, np.float64)
            _chk(lib().eigenex_krylov_combine_to(self.h, int(nvec), _d(cr), _d(ci), int(dst_ref)))
        else:
            cr = np.ascontiguousarray(c, np.float64)
            _chk(lib().eigenex_krylov_combine_to(self.h, int(nvec), _d(cr), None, int(dst_ref)))

    def close(self):
        if self.h:
            lib().eigenex_basis_destroy(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
