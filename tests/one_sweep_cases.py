"""Fixed Lanczos runs of the one-sweep step through the C ABI, written to one .npz -- the child process of
tests/test_gpu_one_sweep.py.

    python -m tests.one_sweep_cases OUT.npz

The library reads its switches (EIGENEX_NO_INLINE_FIN, EIGENEX_NO_GRAPHS, EIGENEX_TWO_SWEEPS) once per process, so one
configuration is one process.  Per case and batch schedule the file holds alpha, beta, every basis column, W, the state fields
and the repair counter under "<case>/<schedule>/<key>".  Importable without a GPU.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = {  # name -> (operator, calls)
    "lap16": (("lap", 16), 41),    # row codes, inline finalisers where they are on
    "tri4097": (("tri", 4097), 13),  # plain CSR, three tiles, the last one of one row
}


def schedules(ncalls):
    mixed, pat, i = [], (1, 1, 5, 2, 7, 1, 4, 6), 0
    while sum(mixed) < ncalls:
        mixed.append(min(pat[i % len(pat)], ncalls - sum(mixed)))
        i += 1
    pairs = [2] * (ncalls // 2) + ([1] if ncalls % 2 else [])
    return {"whole": [ncalls], "mixed": mixed, "pairs": pairs}


def start(n):
    return np.random.default_rng(20 + n).standard_normal(n)


def run_case(ctx, name, out):
    import one_sweep_reference as osr
    from cmpt_eigenex_amd import capi

    (kind, size), ncalls = CASES[name]
    if kind == "lap":
        n = size ** 3
        A = capi.Csr.laplacian3d(ctx, size)
    else:
        n = size
        A = capi.Csr.upload(ctx, n, *osr.tridiagonal_csr(n), column_blocks=0)
    for sched, batches in schedules(ncalls).items():
        b = capi.Basis(ctx, A, n, ncalls + 1)
        b.upload(capi.VEC_W, start(n))
        for k in batches:
            b.lanczos_enqueue(k)
        st, alpha, beta = b.lanczos_state()
        key = "%s/%s/" % (name, sched)
        out[key + "alpha"], out[key + "beta"] = alpha, beta
        out[key + "state"] = np.array([st.nvec, st.iterations, st.nalpha, st.nbeta, st.stopped, st.calls_true, b.repairs()], np.int64)
        out[key + "V"] = np.stack([b.download(capi.VEC_COL(c)) for c in range(st.nvec)])
        out[key + "W"] = b.download(capi.VEC_W)
        b.close()
    A.close()


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    from cmpt_eigenex_amd import capi

    ctx = capi.Context()
    out = {}
    for name in CASES:
        run_case(ctx, name, out)
    ctx.close()
    tmp = argv[0] + ".part.npz"
    np.savez(tmp, **out)
    os.replace(tmp, argv[0])
    print("%d cases -> %s" % (len(CASES), argv[0]))


if __name__ == "__main__":
    main()
