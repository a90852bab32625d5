"""One Lanczos run whose one-sweep batch leaves its newest column pending, followed by eigenex_krylov_combine_to over all columns
-- the child process of tests/test_gpu_krylov_combine_to.py:

    python -m tests.combine_to_case OUT.npz

The library reads EIGENEX_EAGER_CLOSE once per process, so one configuration is one process.  Importable without a GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, NCALLS = 1000, 9


def coefficients(nvec):
    return np.random.default_rng(31).standard_normal(nvec)


def run():
    """(pending before the call, dst = W, dst = V, dst = a free column, the host form's result)"""
    from cmpt_eigenex_amd import capi
    from tests import one_sweep_reference as osr

    ctx = capi.Context()
    A = capi.Csr.upload(ctx, N, *osr.tridiagonal_csr(N), column_blocks=0)
    out = {}
    for name, dst in (("w", capi.VEC_W), ("v", capi.VEC_V), ("col", capi.VEC_COL(NCALLS + 1))):
        b = capi.Basis(ctx, A, N, NCALLS + 3)
        b.upload(capi.VEC_W, np.random.default_rng(5).standard_normal(N))
        b.lanczos_enqueue(4)
        b.lanczos_enqueue(NCALLS - 4)
        out["pending_" + name] = np.array(b.close_pending())
        b.krylov_combine_to(NCALLS, coefficients(NCALLS), dst)
        out["after_" + name] = np.array(b.close_pending())
        out[name] = b.download(dst)
        out["host_" + name] = b.krylov_combine(NCALLS, coefficients(NCALLS).reshape(-1, 1))[:, 0]
        b.close()
    A.close()
    ctx.close()
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **run())
