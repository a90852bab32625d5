"""The cases of tests/test_gpu_general_step_passes.py: Krylov steps whose Gram-Schmidt passes run over a general column set
(library.hip: enq_orthogonalize; kernels.hip: k_dots / k_update over first / stride / count basis columns followed by nq
orthogonalizing vectors).  Operators, start vectors and orthogonalizing vectors come from seeds; importable without a GPU: nothing
touches the device before upload().  tests/test_general_step_reference_host.py runs the fp64 recurrences of
tests/krylov_local_reference.py over every case on the CPU, without and with every fault that applies to it.

Operators (rows(name)): variant_cases.random_csr with 6 draws per row,
  sym / herm     real symmetric, complex Hermitian: the Lanczos cases
  gen / zgen     real and complex general: the Arnoldi cases
  gap, zgap      a diagonal of uniform(0, 1) levels with three separated levels 2, 2.5 and 3 on top and a symmetric random coupling of
                 0.02: Lanczos converges to the top levels within 20 steps, so that a partial re-orthogonalisation (interval 2, 3, 5)
                 has coefficients far above rounding from then on.  24 calls.
  warm, zwarm    the operator of the adaptive Arnoldi cases: gen / zgen plus a diagonal that is 4 on a tenth of the rows and 0 elsewhere,
                 with a start vector that lives mostly on those rows; the share of hu that lies inside the basis changes from step to
                 step, so that |r_1|^2 / |hu|^2 falls on both sides of 0.5.  10 calls.
Sizes: 2500 rows real (one full and one ragged 2048-row tile of k_dots / k_update), 1400 entries complex (2800 doubles), 7000 rows
(3600 complex entries) on three loopback shards, so that every shard has more than one tile.

Orthogonalizing vectors: "orth" the Q factor of a seeded normal matrix (host QR); "skew" unit vectors with pairwise overlaps of
0.3, sqrt(0.7) e_i + sqrt(0.3) e_c of an orthonormal e.  They are not invariant under the operator, so that their coefficients
are O(0.01 .. 1) on every step that uses them and the columns lose orthogonality to them on every step that does not.

Chunk cases: nq orthonormal vectors just below the budget of one dots launch (kDotsMaxAcc = 2048 accumulators: 2048 real or 1024
complex vectors, half of that for the two-source k_dots of the fused alpha), so that the set crosses it during the run.  With
interval 3 the orthogonalizing vectors are used at k = 2, 5, 8, 11, 14 beside 1 .. 5 columns: 2044 + 4 = 2048 at k = 11 is the
last set of one launch and 2049 at k = 14 the first chunked one, so that case makes 16 calls instead of 8.

Case fields: kind (lanczos / arnoldi), op, n, shift, mode (name of capi.ORTHO_*), interval, nq, q (orth / skew / None), shards,
fusion (None: the default), layout (plain: column_blocks = 0; auto), calls, split (a second schedule of batches that must give
the same bytes, or None), budget (chunk cases), faults (applicable_faults)."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import krylov_local_reference as kl  # noqa: E402
import variant_cases as vc  # noqa: E402

MODES = {"ORTHO_BATCHED": kl.BATCHED, "ORTHO_SEQUENTIAL": kl.SEQUENTIAL, "ORTHO_BATCHED_TWICE": kl.TWICE, "ORTHO_BATCHED_ADAPTIVE": kl.ADAPTIVE}
CALLS, CALLS_GAP, CALLS_ADAPTIVE, CALLS_STRIDED_CHUNK = 8, 24, 10, 16
SPLIT = (1, 3, 4)
DOTS_BUDGET = 2048  # library.hip: kDotsMaxAcc
SHIFT_SYM, SHIFT_HERM, SHIFT_GEN, SHIFT_Z = -0.7, -0.3, -0.37, 0.3 - 0.2j
_ROWS, _Q = {}, {}


def _seed(what):
    return vc.hash_seed(f"general_step_cases/{what}")


def _with_diagonal(rows, d):
    import scipy.sparse as sp

    rowptr, col, val = rows
    n = rowptr.size - 1
    A = sp.csr_matrix((val, col, rowptr), shape=(n, n)) + sp.diags(d.astype(val.dtype))
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def warm_rows(n):
    """the rows that carry the diagonal of 4 and most of the start vector of warm / zwarm"""
    return np.arange(n) % 10 == 3


def rows(op, n):
    key = (op, n)
    if key not in _ROWS:
        s = _seed(f"{op}/{n}")
        if op == "sym":
            out = vc.random_csr(s, n, 6, symmetric=True)
        elif op == "herm":
            out = vc.random_csr(s, n, 6, symmetric=True, cplx=True)
        elif op == "gen":
            out = vc.random_csr(s, n, 6)
        elif op == "zgen":
            out = vc.random_csr(s, n, 6, cplx=True)
        elif op in ("gap", "zgap"):
            rp, cl, vl = vc.random_csr(s, n, 6, symmetric=True, cplx=op == "zgap")
            d = np.random.default_rng(s + 1).uniform(0.0, 1.0, n)
            d[[n // 7, n // 2, n - 5]] = (2.0, 2.5, 3.0)
            out = _with_diagonal((rp, cl, 0.02 * vl), d)
        elif op in ("warm", "zwarm"):
            out = _with_diagonal(vc.random_csr(s, n, 6, cplx=op == "zwarm"), (5.5 if op == "zwarm" else 4.0) * warm_rows(n))
        else:
            raise ValueError(op)
        _ROWS[key] = out
    return _ROWS[key]


def is_complex(op):
    return op in ("herm", "zgen", "zwarm", "zgap")


def start(op, n):
    x = vc.start_vector(_seed(f"start/{op}/{n}"), n, is_complex(op))
    if op in ("warm", "zwarm"):
        x = np.where(warm_rows(n), x, 0.05 * x)
    return x


def ortho_vectors(op, n, nq, q):
    """nq orthogonalizing vectors as rows: orthonormal, or unit vectors with pairwise overlaps of 0.3"""
    key = (op, n, nq, q)
    if key not in _Q:
        if nq == 0:
            out = np.zeros((0, n), np.complex128 if is_complex(op) else np.float64)
        else:
            rng = np.random.default_rng(_seed(f"q/{op}/{n}/{nq}/{q}"))
            G = rng.standard_normal((n, nq + 1))
            if is_complex(op):
                G = G + 1j * rng.standard_normal((n, nq + 1))
            E = np.linalg.qr(G)[0].T
            out = E[:nq] if q == "orth" else np.sqrt(0.7) * E[:nq] + np.sqrt(0.3) * E[nq]
            out = np.ascontiguousarray(out)
        _Q[key] = out
    return _Q[key]


def applicable_faults(c):
    """the faults of krylov_local_reference.FAULTS that change what this case computes far beyond rounding.  A fault in the choice
    of basis columns shows in a Lanczos case only where the columns' coefficients are far above rounding: a partial
    re-orthogonalisation (interval >= 2) that is disturbed by orthogonalizing vectors or by the converged levels of `gap`; the
    Arnoldi coefficients are the entries of H."""
    lanczos, mode, nq, interval = c["kind"] == "lanczos", c["mode"], c["nq"], c["interval"]
    disturbed = nq > 0 or c["op"] in ("gap", "zgap")
    if c.get("budget"):  # the chunk cases: the fault that is theirs alone and two of the others (a reference run costs seconds here)
        return ("swap_budget", "q_no_step") + (("first_plus_one",) if interval >= 2 else ())
    f = []
    if (not lanczos) or (interval >= 2 and disturbed):
        f.append("first_plus_one")
    if (not lanczos) or (interval >= 3 and disturbed):  # (interval 2: the newest selected column is k or k - 1, which the recurrence removes)
        f.append("drop_newest")
    if nq > 0:
        f.append("start_not_deflated")
        if not lanczos or interval >= 1:
            f.append("q_no_step")
        if lanczos and interval != 1:
            f.append("q_every_step")
        if is_complex(c["op"]):
            f.append("no_conj_q")
    if c["q"] == "skew":  # an order, a second pass or a decision shows beyond rounding only on a set that is not orthonormal
        if mode == "ORTHO_SEQUENTIAL":
            f += ["q_reversed", "q_first_flip"]
        if mode == "ORTHO_BATCHED_TWICE":
            f.append("skip_second")
        if mode == "ORTHO_BATCHED_ADAPTIVE" and not lanczos:
            f += ["eta_quarter", "always_second", "never_second"]
    return tuple(f)


def _case(name, kind, op, n, mode, interval=1, nq=0, q=None, shards=1, fusion=None, layout="plain", calls=CALLS, budget=None):
    shift = {"sym": SHIFT_SYM, "gap": SHIFT_SYM, "herm": SHIFT_HERM, "zgap": SHIFT_HERM, "gen": SHIFT_GEN, "warm": SHIFT_GEN, "zgen": SHIFT_Z, "zwarm": SHIFT_Z}[op]
    split = SPLIT[:2] + (calls - sum(SPLIT[:2]),)  # (1, 3, 4) of eight calls: a batch of one, a batch below the graph threshold, a captured one
    # between shards a fused alpha is closed by a launch of its own at the end of a batch (library.hip: fuses_alpha; never in the
    # sequential scheme): the same bytes are promised only without fusion
    if budget or (shards > 1 and fusion is not False and kind == "lanczos" and mode != "SEQUENTIAL"):
        split = None
    c = dict(name=name, kind=kind, op=op, n=n, shift=shift, mode="ORTHO_" + mode, interval=interval, nq=nq, q=q if nq else None, shards=shards,
             fusion=fusion, layout=layout, calls=calls, split=split, budget=budget)
    c["faults"] = applicable_faults(c)
    return c


N, NZ, N3, NZ3 = 2500, 1400, 7000, 3600
CASES = [
    # Lanczos, real symmetric, one shard
    _case("l-b-1-2-orth", "lanczos", "sym", N, "BATCHED", 1, 2, "orth"),
    _case("l-b-3-2-skew-auto", "lanczos", "sym", N, "BATCHED", 3, 2, "skew", layout="auto"),
    _case("l-b-5-3-orth", "lanczos", "sym", N, "BATCHED", 5, 3, "orth"),
    _case("l-b-0-2-skew", "lanczos", "sym", N, "BATCHED", 0, 2, "skew"),
    _case("l-t-3-2-orth", "lanczos", "sym", N, "BATCHED_TWICE", 3, 2, "orth", layout="auto"),
    _case("l-t-1-2-skew", "lanczos", "sym", N, "BATCHED_TWICE", 1, 2, "skew"),
    _case("l-s-3-2-skew", "lanczos", "sym", N, "SEQUENTIAL", 3, 2, "skew"),
    _case("l-s-5-3-orth", "lanczos", "sym", N, "SEQUENTIAL", 5, 3, "orth", layout="auto"),
    _case("l-a-3-2-skew", "lanczos", "sym", N, "BATCHED_ADAPTIVE", 3, 2, "skew"),
    _case("gap-b-2", "lanczos", "gap", N, "BATCHED", 2, 0, calls=CALLS_GAP),
    _case("gap-t-3", "lanczos", "gap", N, "BATCHED_TWICE", 3, 0, calls=CALLS_GAP),
    _case("gap-s-5", "lanczos", "gap", N, "SEQUENTIAL", 5, 0, calls=CALLS_GAP),
    # Lanczos, complex Hermitian, one shard
    _case("lz-b-3-2-skew", "lanczos", "herm", NZ, "BATCHED", 3, 2, "skew"),
    _case("zgap-b-2", "lanczos", "zgap", NZ, "BATCHED", 2, 0, calls=CALLS_GAP),
    _case("lz-t-1-2-skew", "lanczos", "herm", NZ, "BATCHED_TWICE", 1, 2, "skew"),
    _case("lz-t-5-3-orth", "lanczos", "herm", NZ, "BATCHED_TWICE", 5, 3, "orth"),
    _case("lz-s-3-2-skew", "lanczos", "herm", NZ, "SEQUENTIAL", 3, 2, "skew"),
    _case("lz-a-3-2-skew", "lanczos", "herm", NZ, "BATCHED_ADAPTIVE", 3, 2, "skew"),
    _case("lz-b-0-2-orth", "lanczos", "herm", NZ, "BATCHED", 0, 2, "orth"),
    # Lanczos on three loopback shards: the fused alpha rides on the dots' all-reduce, or not
    _case("l3-b-3-2-skew-fused", "lanczos", "sym", N3, "BATCHED", 3, 2, "skew", shards=3, fusion=True),
    _case("l3-b-3-2-skew-unfused", "lanczos", "sym", N3, "BATCHED", 3, 2, "skew", shards=3, fusion=False),
    _case("l3-t-1-2-skew-fused", "lanczos", "sym", N3, "BATCHED_TWICE", 1, 2, "skew", shards=3, fusion=True),
    _case("l3-t-1-2-skew-unfused", "lanczos", "sym", N3, "BATCHED_TWICE", 1, 2, "skew", shards=3, fusion=False),
    _case("l3-s-5-3-orth", "lanczos", "sym", N3, "SEQUENTIAL", 5, 3, "orth", shards=3),
    _case("lz3-b-3-2-skew-fused", "lanczos", "herm", NZ3, "BATCHED", 3, 2, "skew", shards=3, fusion=True),
    _case("lz3-t-5-3-orth-unfused", "lanczos", "herm", NZ3, "BATCHED_TWICE", 5, 3, "orth", shards=3, fusion=False),
    # Arnoldi, real general
    _case("a-b-0", "arnoldi", "gen", N, "BATCHED"),
    _case("a-b-2-skew-auto", "arnoldi", "gen", N, "BATCHED", nq=2, q="skew", layout="auto"),
    _case("a-s-2-skew", "arnoldi", "gen", N, "SEQUENTIAL", nq=2, q="skew"),
    _case("a-t-2-orth", "arnoldi", "gen", N, "BATCHED_TWICE", nq=2, q="orth"),
    _case("a-t-2-skew", "arnoldi", "gen", N, "BATCHED_TWICE", nq=2, q="skew", layout="auto"),
    _case("a-a-2-skew", "arnoldi", "warm", N, "BATCHED_ADAPTIVE", nq=2, q="skew", calls=CALLS_ADAPTIVE),
    _case("a-a-0-auto", "arnoldi", "warm", N, "BATCHED_ADAPTIVE", layout="auto", calls=CALLS_ADAPTIVE),
    # Arnoldi, complex
    _case("az-b-2-skew", "arnoldi", "zgen", NZ, "BATCHED", nq=2, q="skew"),
    _case("az-s-2-skew", "arnoldi", "zgen", NZ, "SEQUENTIAL", nq=2, q="skew"),
    _case("az-t-0", "arnoldi", "zgen", NZ, "BATCHED_TWICE"),
    _case("az-t-2-skew", "arnoldi", "zgen", NZ, "BATCHED_TWICE", nq=2, q="skew"),
    _case("az-a-2-skew", "arnoldi", "zwarm", NZ, "BATCHED_ADAPTIVE", nq=2, q="skew", calls=CALLS_ADAPTIVE),
    # Arnoldi on three loopback shards
    _case("a3-b-2-skew", "arnoldi", "gen", N3, "BATCHED", nq=2, q="skew", shards=3),
    _case("a3-a-2-skew", "arnoldi", "warm", N3, "BATCHED_ADAPTIVE", nq=2, q="skew", shards=3, calls=CALLS_ADAPTIVE),
    _case("az3-s-2-skew", "arnoldi", "zgen", NZ3, "SEQUENTIAL", nq=2, q="skew", shards=3),
    # sets beyond the budget of one dots launch
    _case("chunk-l-1-2044", "lanczos", "sym", N, "BATCHED", 1, 2044, "orth", budget=DOTS_BUDGET),
    _case("chunk-l-3-2044", "lanczos", "sym", N, "BATCHED", 3, 2044, "orth", calls=CALLS_STRIDED_CHUNK, budget=DOTS_BUDGET),
    _case("chunk-l3-1-1020-fused", "lanczos", "sym", N3, "BATCHED", 1, 1020, "orth", shards=3, fusion=True, budget=DOTS_BUDGET // 2),
    _case("chunk-lz-1-1020", "lanczos", "herm", NZ, "BATCHED", 1, 1020, "orth", budget=DOTS_BUDGET // 2),
    _case("chunk-lz3-1-508-fused", "lanczos", "herm", NZ3, "BATCHED", 1, 508, "orth", shards=3, fusion=True, budget=DOTS_BUDGET // 4),
    _case("chunk-az-a-1020", "arnoldi", "zwarm", NZ, "BATCHED_ADAPTIVE", nq=1020, q="orth", budget=DOTS_BUDGET // 2),
    _case("chunk-az-a-2045", "arnoldi", "zwarm", 2100, "BATCHED_ADAPTIVE", nq=2045, q="orth", budget=DOTS_BUDGET // 2),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def inputs(c):
    """(rows, x0, Q) of a case, built once per operator / vector set"""
    return rows(c["op"], c["n"]), start(c["op"], c["n"]), ortho_vectors(c["op"], c["n"], c["nq"], c["q"])


def reference(c, fault=None, calls=None):
    """the fp64 recurrence of a case and its report: (report, state dict)"""
    r, x0, Q = inputs(c)
    apply, mode, calls = kl.csr_matmul(r), MODES[c["mode"]], calls or c["calls"]
    orthonormal = c["q"] in (None, "orth")
    if c["kind"] == "lanczos":
        a, b, V = kl.lanczos_general_fp64(apply, x0, calls - 1, c["shift"], c["interval"], Q, mode, fault, c["budget"])
        return kl.check_lanczos_general(r, c["shift"], V, Q, a, b, c["interval"], mode, x0, orthonormal), dict(alpha=a, beta=b, U=V)
    V, H, residue, w = kl.arnoldi_general_fp64(apply, x0, calls, c["shift"], Q, mode, fault, c["budget"])
    return kl.check_arnoldi_general(r, c["shift"], V, Q, H, residue, w, mode, x0, orthonormal), dict(U=V, H=H, residue=residue, w=w)


def check(c, got):
    """the local check of a downloaded state (tests/krylov_pass_runs.py: lanczos, arnoldi)"""
    r, x0, Q = inputs(c)
    mode, orthonormal = MODES[c["mode"]], c["q"] in (None, "orth")
    if c["kind"] == "lanczos":
        return kl.check_lanczos_general(r, c["shift"], got["U"], Q, got["alpha"], got["beta"], c["interval"], mode, x0, orthonormal)
    return kl.check_arnoldi_general(r, c["shift"], got["U"], Q, got["H"], got["residue"], got["w"], mode, x0, orthonormal)


def upload(capi, ctx, c):
    r = rows(c["op"], c["n"])
    return capi.Csr.upload(ctx, c["n"], *r, column_blocks=0 if c["layout"] == "plain" else None)
