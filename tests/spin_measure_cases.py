"""A fixed Lanczos run on the matrix-free sector operator of the 12-site Heisenberg ring, (12,6), optionally interrupted by a
spin measurement between its two batches -- shared by tests/test_gpu_spin_measure.py and its child process:

    python -m tests.spin_measure_cases OUT.npz

The library reads EIGENEX_NO_GRAPHS once per process, so the run without recorded step batches is a process of its own.
Importable without a GPU: nothing touches the device before run()."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

L, N_UP, ROWS, STEPS = 12, 6, 924, 20


def run(capi, interrupt: bool):
    """alpha, beta, the basis columns and W after STEPS step calls from a fixed start vector; interrupt: two batches of
    STEPS / 2 with a measurement of column 3 (every site, every pair) in between, else one batch.  Also the measurement."""
    import spin_measure_reference as mr
    import spin_reference as sr

    ctx = capi.Context()
    S = capi.Csr.spin_half_sector(ctx, L, N_UP, sr.chain(L, periodic=True))
    b = capi.Basis(ctx, S, ROWS, STEPS + 2)
    b.upload(capi.VEC_W, np.random.RandomState(5).standard_normal(ROWS))
    measured = None
    if interrupt:
        b.lanczos_enqueue(STEPS // 2)
        measured = b.spin_measure(capi.VEC_COL(3), mr.site_masks(L) + mr.pair_masks(L), mr.pair_masks(L))
        b.lanczos_enqueue(STEPS - STEPS // 2)
    else:
        b.lanczos_enqueue(STEPS)
    st, alpha, beta = b.lanczos_state()
    out = dict(alpha=alpha, beta=beta, state=np.array([st.nvec, st.iterations, st.nalpha, st.nbeta, st.stopped, st.calls_true]),
               V=np.stack([b.download(capi.VEC_COL(c)) for c in range(st.nvec)]), W=b.download(capi.VEC_W), v=b.download(capi.VEC_V))
    if measured is not None:
        out.update(diag=measured[0], flip=measured[1], norm2=np.array([measured[2]]))
    for h in (b, S, ctx):
        h.close()
    return out


if __name__ == "__main__":
    from cmpt_eigenex_amd import capi as _capi

    np.savez(sys.argv[1], **run(_capi, True))
