"""Fixed one-sweep Lanczos runs through the C ABI, written to one .npz -- the child process of
tests/test_gpu_sweep_parked_stores.py.

    python -m tests.sweep_parked_cases OUT.npz

The library reads EIGENEX_SWEEP_DIRECT_STORES, EIGENEX_SWEEP_SLOT_SHIFT and EIGENEX_NO_GRAPHS once per process, so one
configuration is one process.  Per case the file holds alpha, beta, the state fields with the repair counter, every basis column
and W under "<case>/<key>"; the columns and W of the large cases as SHA-256 digests of their bytes.  Importable without a GPU.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TILE = 2048
CALLS = 12  # steps k = 0..11: no, one and two full groups of four streamed columns with 0-3 left over (a step streams k - 1 columns)
DIGEST_ABOVE = 100000  # rows


def shape_rows(G):
    """rows of the tile-shape cases on a grid of G workgroups (one per CU)"""
    return {"n1": 1, "n2047": TILE - 1, "n2048": TILE, "n2049": TILE + 1,
            "second_partial_tile": TILE * G + 5,         # one workgroup has a second tile, of five rows
            "three_tiles": 3 * TILE * G - 2047}          # three tiles per workgroup; the last tile has one row


BATCHES = {"ones": [1] * CALLS, "three_and_rest": [3, CALLS - 3]}
LONG_N, LONG_CAP = 4096, 1023  # the longest basis a one-sweep step takes: k = 1022 needs 81,904 of the 81,920 bytes of LDS


def start(n):
    return np.random.default_rng(40 + n).standard_normal(n)


def chain_linear_diagonal(n):
    """tridiagonal, -1 beside a diagonal that rises linearly: n distinct eigenvalues"""
    i = np.arange(n)
    rows = np.concatenate([i[1:], i, i[:-1]])
    cols = np.concatenate([i[:-1], i, i[1:]])
    vals = np.concatenate([np.full(n - 1, -1.0), 0.25 * i, np.full(n - 1, -1.0)])
    order = np.lexsort((cols, rows))
    rowptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr, cols[order].astype(np.int32), vals[order]


def _keep(x, n):
    x = np.ascontiguousarray(x)
    return x if n <= DIGEST_ABOVE else np.frombuffer(hashlib.sha256(x.tobytes()).digest(), np.uint8)


def record(capi, b, n, key, out):
    st, alpha, beta = b.lanczos_state()
    out[key + "alpha"], out[key + "beta"] = alpha, beta
    out[key + "state"] = np.array([st.nvec, st.iterations, st.nalpha, st.nbeta, st.stopped, b.repairs()], np.int64)
    out[key + "V"] = np.stack([_keep(b.download(capi.VEC_COL(c)), n) for c in range(max(st.nvec, 1))])
    out[key + "W"] = _keep(b.download(capi.VEC_W), n)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    import torch

    import one_sweep_reference as osr
    from cmpt_eigenex_amd import capi

    G = int(torch.cuda.get_device_properties(0).multi_processor_count)
    ctx = capi.Context()
    out = {"G": np.array([G])}
    rows = shape_rows(G)
    for name, n in rows.items():
        A = capi.Csr.upload(ctx, n, *osr.tridiagonal_csr(n), column_blocks=0)
        scheds = {"": [CALLS]}
        if name == "second_partial_tile":
            scheds.update({"/" + k: v for k, v in BATCHES.items()})
        for sched, batches in scheds.items():
            b = capi.Basis(ctx, A, n, CALLS + 1)
            b.tune(1, 4, 0)
            b.upload(capi.VEC_W, start(n))
            newest = []
            for i, k in enumerate(batches):
                b.lanczos_enqueue(k)
                if i + 1 < len(batches):  # something reads the batch's newest column: its closing pass runs between the batches
                    st = b.lanczos_state()[0]
                    if st.nvec > 0:
                        newest.append(_keep(b.download(capi.VEC_COL(st.nvec - 1)), n))
            key = "%s%s/" % (name, sched)
            record(capi, b, n, key, out)
            if newest:
                out[key + "newest"] = np.stack(newest)
            b.close()
        A.close()
    A = capi.Csr.upload(ctx, LONG_N, *chain_linear_diagonal(LONG_N), column_blocks=0)
    b = capi.Basis(ctx, A, LONG_N, LONG_CAP)
    b.upload(capi.VEC_W, start(LONG_N))
    b.lanczos_enqueue(LONG_CAP)
    record(capi, b, LONG_N, "long/", out)
    b.close()
    A.close()
    ctx.close()
    tmp = argv[0] + ".part.npz"
    np.savez(tmp, **out)
    os.replace(tmp, argv[0])
    print("%d arrays -> %s" % (len(out), argv[0]))


if __name__ == "__main__":
    main()
