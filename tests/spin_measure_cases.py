"""A fixed Lanczos run on the matrix-free sector operator of the 12-site Heisenberg ring, (12,6), optionally interrupted by a
spin measurement between its two batches -- shared by tests/test_gpu_spin_measure.py and its child process:

    python -m tests.spin_measure_cases OUT.npz

The library reads EIGENEX_NO_GRAPHS once per process, so the run without recorded step batches is a process of its own.
Also the shapes, term lists and the measurement whose bits tests/golden/spin_measure_bits_parent.npz records
(scripts/record_spin_measure_bits.py writes it, test_measurement_bits_equal_the_parent_build reads it).
Importable without a GPU: nothing touches the device before run() or measure_bits()."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

L, N_UP, ROWS, STEPS = 12, 6, 924, 20

# (n_sites, n_up or None, one workgroup per CU): two tiles; one partial tile; 496 rows with bit 31; 512 tiles on a grid of one
# workgroup per CU, so the tile loop goes round -- the only shape whose partial sums depend on the device's CU count
BITS_SHAPES = [(9, None, False), (10, 5, False), (32, 2, False), (17, None, True)]


def bits_key(n_sites, n_up):
    return "%d_%s" % (n_sites, "full" if n_up is None else n_up)


def bits_lists(n_sites, n_up):
    """every site, the pairs with the top site, a low and a middle pair, the pairs with site 0, the string, the all-sites mask and
    a duplicate: at least 17 terms on either list at every shape of BITS_SHAPES, so both span two chunks or more"""
    import spin_measure_reference as mr

    full_d, _ = mr.term_lists(n_sites, n_up)
    top = [(1 << i) | (1 << (n_sites - 1)) for i in range(n_sites - 1)] + [0b11, (1 << (n_sites // 2 - 1)) | (1 << (n_sites // 2))]
    low = [1 | (1 << i) for i in range(2, n_sites - 1)]
    diag = mr.site_masks(n_sites) + top + [int(m) for m in full_d[-3:]]
    flip = top + [top[0]] + low + (mr.site_masks(n_sites) if n_up is None else [])
    assert len(diag) >= 17 and len(flip) >= 17
    return np.array(diag, np.uint32), np.array(flip, np.uint32)


def measure_bits(capi, n_sites, n_up, one_workgroup_per_cu):
    """{"norm2", "diag", "flip"}: the raw bytes (uint8) of one eigenex_spin_measure of spin_measure_reference.vector"""
    import spin_measure_reference as mr
    import spin_reference as sr

    bonds = sr.chain(n_sites, 1.0, 0.7, periodic=True)
    ctx = capi.Context()
    S = capi.Csr.spin_half(ctx, n_sites, bonds) if n_up is None else capi.Csr.spin_half_sector(ctx, n_sites, n_up, bonds)
    b = capi.Basis(ctx, S, mr.rows(n_sites, n_up), 2)
    if one_workgroup_per_cu:
        b.tune(2, 1, 0)
    b.upload(capi.VEC_COL(1), mr.vector(n_sites, n_up))
    diag, flip, norm2 = b.spin_measure(capi.VEC_COL(1), *bits_lists(n_sites, n_up))
    for h in (b, S, ctx):
        h.close()
    return {k: np.frombuffer(np.ascontiguousarray(v, np.float64).tobytes(), np.uint8) for k, v in (("norm2", norm2), ("diag", diag), ("flip", flip))}


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
