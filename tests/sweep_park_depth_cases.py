"""Fixed one-sweep Lanczos runs through the C ABI, written to one .npz -- the child process of
tests/test_gpu_sweep_park_depth.py.

    python -m tests.sweep_park_depth_cases OUT.npz

The library reads EIGENEX_SWEEP_DIRECT_STORES, EIGENEX_SWEEP_PARK_TILES, EIGENEX_SWEEP_SLOT_SHIFT and EIGENEX_NO_GRAPHS once
per process, so one configuration is one process.  Per case the file holds what tests/sweep_parked_cases.py records: alpha, beta,
the state fields with the repair counter, every basis column and W under "<case>/<key>", the columns and W of the large cases as
SHA-256 digests of their bytes.  Importable without a GPU.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tests.sweep_parked_cases import BATCHES, CALLS, TILE, _keep, record, start  # noqa: E402

CUT_CASES = ("two_tiles", "three_tiles")  # the batch cuts run with the queue never full and with a release at a full queue
# launch_sweep parks two tiles while 2 * 32768 + 48 (k + 1) + 32 <= 81920 bytes, that is up to k = 339, and one tile from k = 340:
# a basis of 345 columns takes steps k = 0..344, five of them behind the change
LONG_N, LONG_CAP, LAST_K_AT_DEPTH_2 = 4096, 345, 339


def shape_rows(G):
    """rows of the tile-shape cases on a grid of G workgroups (one per CU)"""
    return {"n1": 1, "n2047": TILE - 1, "n2048": TILE, "n2049": TILE + 1,
            "two_tiles": TILE * G + 5,           # one workgroup has a second tile, of five rows: the queue is never full
            "three_tiles": 2 * TILE * G + 5,     # one workgroup has a third tile: its first release is at a tile end, queue full
            "five_tiles": 5 * TILE * G - 2047}   # five tiles per workgroup, the last one of one row: the queue wraps twice


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    import torch

    import one_sweep_reference as osr
    from cmpt_eigenex_amd import capi

    G = int(torch.cuda.get_device_properties(0).multi_processor_count)
    ctx = capi.Context()
    out = {"G": np.array([G])}
    for name, n in shape_rows(G).items():
        A = capi.Csr.upload(ctx, n, *osr.tridiagonal_csr(n), column_blocks=0)
        scheds = {"": [CALLS]}
        if name in CUT_CASES:
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
    A = capi.Csr.upload(ctx, LONG_N, *osr.tridiagonal_csr(LONG_N), column_blocks=0)
    b = capi.Basis(ctx, A, LONG_N, LONG_CAP)
    b.tune(1, 4, 0)
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
