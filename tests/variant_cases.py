"""Fixed, seeded Krylov runs through the C ABI, written to one .npz -- the child process of tests/test_gpu_variants.py.

    python -m tests.variant_cases OUT.npz [--only PATTERN ...]

The library reads its switches (EIGENEX_NO_INLINE_FIN, EIGENEX_NO_GRAPHS, EIGENEX_DOTS_RED4) once into a `static`, so one
configuration is one process: the parent starts this module once per configuration and compares the files bit for bit.
Everything a case observes is stored under "<case>/<key>": alpha / beta or H, the state fields, the residue, the basis
columns (SHA-256 per column plus a few full columns on the large operators), Ritz vectors, the operator's layout and the
number of recorded step graphs.  Operators, start vectors and deflation vectors come from the functions below, which the
parent calls again for its oracle comparisons; they use numpy's seeded generators and elementwise arithmetic only (no
LAPACK), so every process builds the same bits.

Importable without a GPU: nothing touches the device before main().
"""
from __future__ import annotations

import argparse
import fnmatch
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STATE_FIELDS = ("nvec", "iterations", "nalpha", "nbeta", "stopped", "calls_true")
SCHEDULES = ("whole", "single", "mixed")
BIG_N = 250_000  # from this many rows on, columns are stored as SHA-256 digests plus a few full columns


def schedule(kind: str, m: int) -> list[int]:
    """batch sizes of one run of m calls: one batch (recorded as a graph from kMinGraphCalls = 4 calls on), one call per
    batch (never recorded; every call is the last of its batch), or a mix of both around the graph threshold"""
    if kind == "whole":
        return [m]
    if kind == "single":
        return [1] * m
    out, pat, i = [], (3, 1, 7, 2, 5, 1, 4, 6), 0
    while sum(out) < m:
        out.append(min(pat[i % len(pat)], m - sum(out)))
        i += 1
    return out


# --------------------------------------------------------------------------- operators (host arrays)
def laplacian(n: int):
    from oracle import cref

    return cref.laplacian3d(n)


def random_csr(seed: int, n: int, per: int, symmetric: bool = False, cplx: bool = False):
    """per entries per row at uniform random columns (sorted, duplicates summed); symmetric: (B + B^T) / 2"""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    col = np.sort(rng.integers(0, n, (n, per)), axis=1).ravel()
    row = np.repeat(np.arange(n), per)
    val = rng.uniform(-1, 1, n * per)
    if cplx:
        val = val + 1j * rng.uniform(-1, 1, n * per)
    B = sp.csr_matrix((val, (row, col)), shape=(n, n))
    if symmetric:
        B = (B + (B.conj().T if cplx else B.T)) * 0.5
    B = sp.csr_matrix(B)
    B.sum_duplicates()
    B.sort_indices()
    return B.indptr.astype(np.int32), B.indices.astype(np.int32), B.data.copy()


def block_diagonal(seed: int, n: int, small: int):
    """a dense symmetric small x small block followed by a symmetric random sparse block: a start vector that lives in the
    first `small` rows spans an invariant subspace of dimension `small`, so Lanczos breaks down at that step"""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    D = rng.uniform(-1, 1, (small, small))
    D = (D + D.T) * 0.5 + np.diag(np.arange(1, small + 1, dtype=np.float64))
    rp, cl, vl = random_csr(seed + 1, n - small, 6, symmetric=True)
    R = sp.csr_matrix((vl, cl, rp), shape=(n - small, n - small))
    A = sp.csr_matrix(sp.block_diag([sp.csr_matrix(D), R]))
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def scattered(seed: int, n: int, per: int):
    """per entries per row at uniform random columns, no duplicates needed: the automatic layout's split-tile case"""
    rng = np.random.default_rng(seed)
    col = np.sort(rng.integers(0, n, (n, per)), axis=1).astype(np.int32).ravel()
    rowptr = (per * np.arange(n + 1)).astype(np.int32)
    return rowptr, col, rng.uniform(-1, 1, n * per)


def cosine_rows(n: int, first: int, count: int):
    """rows first .. first+count-1 of the orthonormal DCT-II basis of R^n (deflation vectors without a factorisation)"""
    i = np.arange(n) + 0.5
    Q = np.empty((count, n))
    for r in range(count):
        j = first + r
        Q[r] = np.cos(np.pi * j * i / n) * (np.sqrt(1.0 / n) if j == 0 else np.sqrt(2.0 / n))
    return Q


def start_vector(seed: int, n: int, cplx: bool = False, support: int | None = None):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    if cplx:
        x = x + 1j * rng.standard_normal(n)
    if support is not None:
        x[support:] = 0.0
    return x


# --------------------------------------------------------------------------- the case matrix
def _solver_cases():
    """base cases: name -> dict(kind, op, m (calls), cap, n, shift, nq, mode, cplx, layout, ...)"""
    c = {}
    # Lanczos: InlineFin in k_dots / k_spmv (short-row form), batched and adaptive, shift, two deflation vectors; complex control
    c["lz_lap24_b"] = dict(kind="lanczos", op=("lap", 24), m=60, shift=0.75, nq=2, mode=0, layout="csr")
    c["lz_lap24_a"] = dict(kind="lanczos", op=("lap", 24), m=60, shift=0.75, nq=2, mode=3, layout="csr")
    c["lz_lap24_z"] = dict(kind="lanczos", op=("lapz", 24), m=60, shift=0.75, nq=2, mode=0, cplx=True, layout="csr")
    # LONG_ROWS instantiation (>= 16 entries per row), plain CSR asked for
    c["lz_long"] = dict(kind="lanczos", op=("sym", 101, 4000, 12), m=40, layout="csr")
    # 64-bit row pointers (launch_spmv64) on a small operator
    c["lz_wide"] = dict(kind="lanczos", op=("lap", 24), m=40, wide=True, layout="csr")
    # more than 256 workgroups in the vector and operator kernels: the strided part of every fused sum
    c["lz_big"] = dict(kind="lanczos", op=("lap", 85), m=30, layout="csr")
    # breakdown (beta <= threshold) inside a batch: the start vector lives in a 5-dimensional invariant subspace
    c["lz_breakdown"] = dict(kind="lanczos", op=("blockdiag", 103, 3000, 5), m=12, support=5, layout="csr")
    # full Krylov space (n <= capacity) reached inside a batch
    c["lz_full"] = dict(kind="lanczos", op=("sym", 104, 40, 5), m=50, layout="csr")
    # Arnoldi: InlineArnoldiBegin (batched) and the whole adaptive set (InlineDecide, InlineReduce, deferred tail)
    c["ar_rand_b"] = dict(kind="arnoldi", op=("rand", 201, 3000, 9), m=40, shift=0.3, nq=2, mode=0, layout="csr")
    c["ar_rand_a"] = dict(kind="arnoldi", op=("rand", 201, 3000, 9), m=40, shift=0.3, nq=2, mode=3, layout="csr")
    c["ar_rand_z"] = dict(kind="arnoldi", op=("randz", 202, 3000, 9), m=40, nq=2, mode=3, cplx=True, layout="csr")
    c["ar_big"] = dict(kind="arnoldi", op=("lap", 85), m=30, mode=3, layout="csr")
    # full Krylov space (n_global reached) inside a batch; the deferred tail is switched off by k + 1 < n_global
    c["ar_full"] = dict(kind="arnoldi", op=("rand", 205, 40, 5), m=50, mode=3, layout="csr")
    # capacity reached by the last batch (k + 1 < cap switches the deferred tail off on the last step)
    c["ar_cap"] = dict(kind="arnoldi", op=("rand", 206, 2500, 7), m=33, cap=33, mode=3, layout="csr")
    # second Gram-Schmidt pass needed on some steps and not on others (test_arnoldi_orthogonality_when_ritz_values_converge)
    c["ar_dgks"] = dict(kind="arnoldi", op=("lap", 16), m=150, mode=3, layout="csr")
    # split tiles chosen automatically: k_spmv_split with InlineArnoldiBegin, 1024-thread workgroups
    c["ar_split"] = dict(kind="arnoldi", op=("scattered", 207, 600_000, 24), m=20, mode=3, layout="split_tiles", auto=True)
    # more than kInlineReduceMaxCoef = 4096 coefficients: the non-inline branch of the adaptive scheme with inline on
    c["ar_defl"] = dict(kind="arnoldi", op=("rand", 208, 8192, 7), m=10, nq=4095, mode=3, layout="csr")
    for v in c.values():
        v.setdefault("shift", 0.0)
        v.setdefault("nq", 0)
        v.setdefault("mode", 0)
        v.setdefault("cplx", False)
        v.setdefault("cap", v["m"] + 2)
    return c


SOLVER_CASES = _solver_cases()
PRIM_CASES = {}
for _n in (2047, 2048, 2049, 600_000):
    for _cplx in (False, True):
        for _ncols in ((1, 64) if _n >= BIG_N else (1, 37, 3000)):
            PRIM_CASES["prim-%d-%s-%d" % (_n, "z" if _cplx else "d", _ncols)] = dict(n=_n, cplx=_cplx, ncols=_ncols)


def all_case_names():
    names = ["%s-%s" % (b, s) for b in SOLVER_CASES for s in SCHEDULES]
    return names + list(PRIM_CASES)


def operator(spec):
    """host CSR (rowptr int32, col int32, val) of an operator spec"""
    kind = spec[0]
    if kind == "lap":
        return laplacian(spec[1])
    if kind == "lapz":  # the Laplacian as a complex operator with a Hermitian imaginary part on the off-diagonal
        rp, cl, vl = laplacian(spec[1])
        row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
        vz = vl.astype(np.complex128) + 0.25j * np.sign(cl - row)
        return rp, cl, vz
    if kind == "sym":
        return random_csr(spec[1], spec[2], spec[3], symmetric=True)
    if kind == "rand":
        return random_csr(spec[1], spec[2], spec[3])
    if kind == "randz":
        return random_csr(spec[1], spec[2], spec[3], cplx=True)
    if kind == "blockdiag":
        return block_diagonal(spec[1], spec[2], spec[3])
    if kind == "scattered":
        return scattered(spec[1], spec[2], spec[3])
    raise ValueError(spec)


def case_inputs(base: str):
    """(rowptr, col, val, init, Q) of a solver case"""
    cs = SOLVER_CASES[base]
    rp, cl, vl = operator(cs["op"])
    n = rp.size - 1
    init = start_vector(hash_seed(base), n, cs["cplx"], cs.get("support"))
    Q = cosine_rows(n, 1, cs["nq"]) if cs["nq"] else np.zeros((0, n))
    return rp, cl, vl, init, Q


def hash_seed(name: str) -> int:
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def prim_inputs(name: str):
    """(M: ncols x n, w) of a primitive case"""
    pc = PRIM_CASES[name]
    rng = np.random.default_rng(hash_seed(name))
    n, k = pc["n"], pc["ncols"]
    M = rng.standard_normal((k, n))
    w = rng.standard_normal(n)
    if pc["cplx"]:
        M = M + 1j * rng.standard_normal((k, n))
        w = w + 1j * rng.standard_normal(n)
    return M, w


# --------------------------------------------------------------------------- running (GPU)
def _columns(out, key, b, ncols, n):
    cols = [b.download(b_col(c)) for c in range(ncols)]
    if n < BIG_N:
        out[key + "V"] = np.stack(cols) if cols else np.zeros((0, n), b.dtype)
        return
    out[key + "Vsha"] = np.array([hashlib.sha256(c.tobytes()).hexdigest() for c in cols])
    keep = sorted({0, ncols // 2, ncols - 1}) if ncols else []
    for c in keep:
        out[key + "V%d" % c] = cols[c]


def b_col(c):
    from cmpt_eigenex_amd import capi

    return capi.VEC_COL(c)


def run_solver(ctx, name: str, out: dict):
    from cmpt_eigenex_amd import capi

    base, sched = name.rsplit("-", 1)
    cs = SOLVER_CASES[base]
    rp, cl, vl, init, Q = case_inputs(base)
    n = rp.size - 1
    if cs["op"][0] == "lap":
        if cs.get("wide"):  # read per call by eigenex_csr_laplacian3d: only this operator gets the 64-bit row pointers
            os.environ["EIGENEX_FORCE_WIDE_ROWPTR"] = "1"
        try:
            A = capi.Csr.laplacian3d(ctx, cs["op"][1])
        finally:
            os.environ.pop("EIGENEX_FORCE_WIDE_ROWPTR", None)
    else:
        A = capi.Csr.upload(ctx, n, rp, cl, vl, column_blocks=None if cs.get("auto") else 0)
    key = name + "/"
    out[key + "layout"] = np.array(A.layout())
    b = capi.Basis(ctx, A, n, cs["cap"], cs["nq"])
    b.configure(cs["shift"], 1e-12, 1, cs["mode"])
    for q in range(cs["nq"]):
        b.upload(capi.VEC_ORTHO(q), Q[q])
    lanczos = cs["kind"] == "lanczos"

    def run_all(suffix):
        b.upload(capi.VEC_W, init)
        for k in schedule(sched, cs["m"]):
            (b.lanczos_enqueue if lanczos else b.arnoldi_enqueue)(k)
        if lanczos:
            st, a, bt = b.lanczos_state()
            out[key + "alpha" + suffix], out[key + "beta" + suffix] = a, bt
        else:
            st, H = b.arnoldi_state()
            out[key + "H" + suffix] = H
        out[key + "state" + suffix] = np.array([getattr(st, f) for f in STATE_FIELDS], np.int64)
        out[key + "residue" + suffix] = np.array([st.residue])
        return st

    st = run_all("")
    out[key + "graphs"] = np.array(b.graph_info()["graphs"])
    nvec = min(st.nvec, cs["cap"])
    _columns(out, key, b, nvec, n)
    # Ritz vectors X = V S: Lanczos with the eigenvectors of the tridiagonal matrix, Arnoldi with fixed coefficients
    if nvec:
        if lanczos:
            a, bt = out[key + "alpha"], out[key + "beta"]
            k = min(a.size, nvec)
            T = np.diag(a[:k]) + np.diag(bt[: k - 1], 1) + np.diag(bt[: k - 1], -1)
            S = np.linalg.eigh(T)[1][:, [0, k - 1]] if k > 1 else np.ones((1, 1))
        else:
            k = nvec
            S = np.random.default_rng(hash_seed(base) + 1).standard_normal((k, 3))  # the same for every schedule
        X = b.ritz_vectors(k, S)
        if n < BIG_N:
            out[key + "ritz"] = X
        else:
            out[key + "ritzsha"] = np.array([hashlib.sha256(np.ascontiguousarray(X[:, e]).tobytes()).hexdigest() for e in range(X.shape[1])])
    if sched == "whole":  # the same batch again: replayed from the recorded graph where one was recorded
        b.clear()
        run_all("_again")
    b.close()
    A.close()


def run_prim(ctx, name: str, out: dict):
    from cmpt_eigenex_amd import capi

    pc = PRIM_CASES[name]
    M, w = prim_inputs(name)
    n, k = pc["n"], pc["ncols"]
    b = capi.Basis(ctx, None, n, k, 0, dtype=np.complex128 if pc["cplx"] else np.float64)
    for c in range(k):
        b.upload(capi.VEC_COL(c), M[c])
    b.upload(capi.VEC_W, w)
    h = b.dots(capi.VEC_W, 0, 1, k)
    b.upload(capi.VEC_V, w)
    nrm2 = b.update(capi.VEC_V, 0, 1, k, h)
    key = name + "/"
    out[key + "h"] = h
    out[key + "nrm2"] = np.array([nrm2])
    wn = b.download(capi.VEC_V)
    if n < BIG_N:
        out[key + "w"] = wn
    else:
        out[key + "wsha"] = np.array(hashlib.sha256(wn.tobytes()).hexdigest())
    b.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out")
    ap.add_argument("--only", nargs="*", default=None, help="fnmatch patterns of case names (default: every case)")
    args = ap.parse_args(argv)
    from cmpt_eigenex_amd import capi

    names = all_case_names()
    if args.only:
        names = [x for x in names if any(fnmatch.fnmatchcase(x, p) for p in args.only)]
    if not names:
        raise SystemExit("no case matches --only")
    ctx = capi.Context()
    out = {}
    for name in names:
        (run_prim if name in PRIM_CASES else run_solver)(ctx, name, out)
    ctx.close()
    out["_cases"] = np.array(names)
    tmp = args.out + ".part.npz"
    np.savez(tmp, **out)
    os.replace(tmp, args.out)
    print("%d cases -> %s" % (len(names), args.out))


if __name__ == "__main__":
    main()
