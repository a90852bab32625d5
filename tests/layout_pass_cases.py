"""The operators of tests/test_gpu_layout_krylov_passes.py: every stored layout that library.hip's launch_operator chooses between,
as host rows (rowptr, col, val) for the local check of tests/krylov_local_reference.py and as a way to put them on the device.
tests/test_layout_pass_cases_host.py runs the fp64 recurrences over every one of them on the CPU.

Importable without a GPU: nothing touches the device before upload().  numpy's seeded generators and elementwise arithmetic only
(scipy.sparse adds A and A^T: no LAPACK), so every process builds the same bits.

Every operator comes as a family: rows(family, "sym") is symmetric (Hermitian for a complex family) and serves the Lanczos
schemes, rows(family, "gen") is general and serves the Arnoldi schemes.

ragged(n, top)  rows of 0 .. top-1 entries at ascending random columns, about 2 % of the rows empty, the first and the last among
                them, twelve rows of 60 to 200 entries.  No entry sits in the column of an empty row, so that A + A^T keeps the
                empty rows: there y = shift x scale, and u_out is still to be written.  "sym" is A + A^T of a ragged(n, top_sym).
  r5000, r9001      one input slice, 20 and 36 tiles of 256 rows: plain CSR, three column-blocked passes, split tiles (256-row
                    tiles at 9,001, 512-row tiles at 5,000: split_layout.hpp, split_geometry) and 64-bit row pointers
  band9001          r9001 with every column within 200 rows of its row (a band that symmetrising keeps): on three shards of about
                    twelve 256-row tiles only the tiles at a shard's ends read halo columns, so that the interior and the
                    boundary tile list both exist (a uniformly random column makes every tile a boundary tile)
  z5000, z9001      the same with complex values: one pass (k_spmv_z), three passes, split tiles
  s40000_4, s40000_2, s70001_1   column-sorted row tiles, k_spmv_sorted<4>, <2> and <1>.  A (tile, slice) segment holds at most
                    kSortCap - 4 = 8188 entries (library.hip, build_sorted_layout_t) and the largest of 4096-, 2048- and 1024-row
                    tiles that fits is taken; a segment of a T-row tile holds about T * mean / K entries over K slices of 32768
                    columns.  40,000 rows, K = 2: a mean of 3 entries per row puts 6144 into a 4096-row tile's segment (<4>); a
                    mean of 6 puts 12288 there and 6144 into a 2048-row tile's (<2>).  70,001 rows, K = 3: a mean of 18 puts
                    12288 into a 2048-row tile's segment and 6144 into a 1024-row tile's (<1>).  The symmetrised operators have
                    the same means (top_sym is chosen for it).  sorted_tile_rows() restates the rule; the host suite asserts
                    4096, 2048, 1024.  70,001 rows are also 274 plain tiles of 256 rows: more than one per CU under tune(2, 1, 0).
long4000        16 entries per row or more on average (kSpmvLongRows): variant_cases.random_csr, 24 per row.
lap18           the 18^3 Laplacian, stored as row codes by Csr.laplacian3d; symmetric, it serves both kinds of scheme.
blocks, zblocks dense blocks in the manner of test_block_operator_kernel_bit_exact_vs_flattened_csr: ragged sectors with empty
                ones, a sector of 700 rows, a sector row without a block, a block of 4500 columns (three chunks of kBlockStage =
                2048 staged input elements) and a first sector of 5 rows that is coupled to nothing (the breakdown case; its diagonal 2, 4, .., 10 keeps
                the last beta before the stop near 1, so that one Gram-Schmidt pass leaves an orthogonal fifth column).  The
                same partition on both axes, so that "sym" can be symmetric.  zblocks is a third of the size: a complex entry
                takes two doubles of every buffer.
bd3000, bd40000 variant_cases.block_diagonal: a dense 5 x 5 block, then a sparse symmetric one; a start vector on the first five
                rows breaks down after five columns.  40,000 rows at about 12 entries per row are eligible for the column-sorted
                tiles (K = 2, 6144 entries in a 1024-row tile's segment).  zbd3000: the same with a Hermitian imaginary part.
                bdlong3000: 24 entries per row in the sparse block, the breakdown case of the long-rows kernel variant.
chain3000       a tridiagonal operator of five values, cut behind row 4: the breakdown case that row codes can store when it goes
                up through Csr.upload (encoded on the host; lap18 is encoded on the device), also run through the step schemes.
                As plain CSR on three shards it has interior and boundary tiles on every shard: the breakdown case of that
                branch, with the start vector on the first shard alone.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import variant_cases as vc  # noqa: E402

SORT_CAP = 8192          # kernels.hpp: kSortCap
SORT_SLICE = 32768       # 256 KB of operator input
SUPPORT = 5              # rows that carry the breakdown start vector


# ---- ragged rows -------------------------------------------------------------------------------------------------------------------
def ragged(n, top, seed, cplx=False, band=None):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, top, n)
    empty = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, n // 50)]))
    live = np.setdiff1d(np.arange(n), empty)
    counts[live[rng.integers(0, live.size, 12)]] = rng.integers(60, 201, 12)
    counts[empty] = 0
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=rowptr[1:])
    nnz = int(rowptr[-1])
    row = np.repeat(np.arange(n), counts)
    if band is None:
        col = live[rng.integers(0, live.size, nnz)]
    else:  # the nearest rows with entries at or above row + offset, |offset| <= band
        col = live[np.searchsorted(live, row + rng.integers(-band, band + 1, nnz)).clip(0, live.size - 1)]
    col = col[np.lexsort((col, row))]  # ascending within a row; duplicates stay separate stored entries
    val = rng.uniform(-1, 1, nnz)
    if cplx:
        val = val + 1j * rng.uniform(-1, 1, nnz)
    return rowptr.astype(np.int32), col.astype(np.int32), val


def symmetrised(rows):
    """A + A^T (A + A^H for complex values), duplicates summed, columns ascending"""
    import scipy.sparse as sp

    rowptr, col, val = rows
    n = rowptr.size - 1
    A = sp.csr_matrix((val, col, rowptr), shape=(n, n))
    S = sp.csr_matrix(A + (A.conj().T if np.iscomplexobj(val) else A.T))
    S.sum_duplicates()
    S.sort_indices()
    return S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.copy()


def sorted_tile_rows(rows):
    """the tile height that build_sorted_layout takes on one shard: the largest of 4096, 2048, 1024 rows at which every (tile,
    slice) segment holds at most kSortCap - 4 entries; None if there is none, or not 2 .. 64 slices"""
    rowptr, col, _ = rows
    n = rowptr.size - 1
    K = -(-n // SORT_SLICE)
    if K < 2 or K > 64:
        return None
    W = -(-n // K)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    for T in (4096, 2048, 1024):
        seg = np.bincount((row // T) * K + col // W)
        if seg.max() <= SORT_CAP - 4:
            return T
    return None


# ---- dense blocks ------------------------------------------------------------------------------------------------------------------
def block_operator(cplx, symmetric):
    """(sizes, blocks): sector 0 (5 rows) has its diagonal block alone; the sector of 9 rows has no block in its row (and, in the
    symmetric operator, none in its column); the sector of 4500 has no diagonal block and is coupled to the sector of 40 by a
    40 x 4500 block and back; the others are coupled with probability 0.45"""
    rng = np.random.default_rng(177 if cplx else 77)
    sizes = [SUPPORT, 3, 0, 17, 700, 1, 40, 9, 0, 64, 4500] if cplx else [SUPPORT, 3, 0, 17, 700, 1, 40, 300, 9, 0, 64, 256, 5, 4500]
    bare, wide, partner = sizes.index(9), sizes.index(4500), sizes.index(40)

    def block(r, c):
        B = rng.uniform(-1, 1, (sizes[r], sizes[c]))
        return B + 1j * rng.uniform(-1, 1, B.shape) if cplx else B

    def dagger(B):
        return B.conj().T.copy()

    blocks = {(0, 0): (lambda D: (D + dagger(D)) / 2 + np.diag(2.0 * np.arange(1.0, SUPPORT + 1)))(block(0, 0))}
    for r in range(1, len(sizes)):
        for c in range(1, len(sizes)):
            if sizes[r] * sizes[c] == 0 or r == bare or (symmetric and (c == bare or c < r)):
                continue
            if wide in (r, c):
                if {r, c} != {wide, partner}:
                    continue
            elif r != c and rng.random() >= 0.45:
                continue
            B = block(r, c)
            if symmetric and r == c:
                B = (B + dagger(B)) / 2
            blocks[(r, c)] = B
            if symmetric and r != c:
                blocks[(c, r)] = dagger(B)
    return sizes, blocks


def flatten_blocks(sizes, blocks):
    """rows of the block matrix in stored order: block by block (ascending block column), columns ascending -- what
    solver.blocks_to_csr and tests/test_gpu_more.py's _flatten_blocks write, without a Python loop over the entries"""
    off = np.concatenate([[0], np.cumsum(sizes)])
    cplx = any(np.iscomplexobj(B) for B in blocks.values())
    rowptr, col, val = [np.zeros(1, np.int64)], [], []
    for r in range(len(sizes)):
        keys = sorted(k for k in blocks if k[0] == r)
        width = sum(sizes[c] for _, c in keys)
        if sizes[r] == 0:
            continue
        rowptr.append(rowptr[-1][-1] + width * np.arange(1, sizes[r] + 1))
        if keys:
            cols = np.concatenate([np.arange(off[c], off[c + 1]) for _, c in keys])
            col.append(np.tile(cols, sizes[r]))
            val.append(np.concatenate([blocks[k] for k in keys], axis=1).ravel())
    dt = np.complex128 if cplx else np.float64
    return (np.concatenate(rowptr).astype(np.int32), np.concatenate(col).astype(np.int32) if col else np.zeros(0, np.int32),
            np.concatenate(val).astype(dt) if val else np.zeros(0, dt))


# ---- the families ------------------------------------------------------------------------------------------------------------------
# ragged families: (n, top of "gen", top of "sym", complex, band or None)
RAGGED = {
    "band9001": (9001, 12, 7, False, 200),
    "r5000": (5000, 12, 7, False), "r9001": (9001, 12, 7, False), "z5000": (5000, 12, 7, True), "z9001": (9001, 12, 7, True),
    "s40000_4": (40000, 7, 4, False), "s40000_2": (40000, 13, 7, False), "s70001_1": (70001, 37, 19, False),
}
SORTED_TILE_ROWS = {"s40000_4": 4096, "s40000_2": 2048, "s70001_1": 1024, "bd40000": 1024}
BREAKDOWN = ("bd3000", "bdlong3000", "bd40000", "zbd3000", "chain3000", "blocks", "zblocks")  # families whose first SUPPORT rows are coupled to nothing else
FAMILIES = tuple(RAGGED) + ("long4000", "lap18", "blocks", "zblocks", "bd3000", "bdlong3000", "bd40000", "zbd3000", "chain3000")
_ROWS, _BLOCKS = {}, {}


def _seed(family, kind):
    return vc.hash_seed(f"layout_pass_cases/{family}/{kind}")


def blocks_of(family, kind):
    key = (family, kind)
    if key not in _BLOCKS:
        _BLOCKS[key] = block_operator(family == "zblocks", kind == "sym")
    return _BLOCKS[key]


def _hermitian_twist(rows):
    """the same pattern with an antisymmetric imaginary part: Hermitian where the input is symmetric"""
    rowptr, col, val = rows
    row = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    return rowptr, col, val * (1.0 + 0.25j * np.sign(col - row))


def _chain(n):
    i = np.arange(n)
    lower, upper = (i > 0) & (i != SUPPORT), (i < n - 1) & (i != SUPPORT - 1)
    counts = 1 + lower.astype(np.int64) + upper
    rowptr = np.concatenate([[0], np.cumsum(counts)])
    col, val = np.empty(rowptr[-1], np.int64), np.empty(rowptr[-1])
    p = rowptr[:-1].copy()
    for keep, d, v in ((lower, -1, np.full(n, -1.0)), (np.ones(n, bool), 0, 2.0 + 0.25 * (i % 4)), (upper, 1, np.full(n, -1.0))):
        col[p[keep]], val[p[keep]] = i[keep] + d, v[keep]
        p[keep] += 1
    return rowptr.astype(np.int32), col.astype(np.int32), val


def _block_diagonal_long(seed, n):
    """variant_cases.block_diagonal with 12 draws per row in the sparse block instead of 6: about 24 entries per row"""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    D = rng.uniform(-1, 1, (SUPPORT, SUPPORT))
    D = (D + D.T) * 0.5 + np.diag(np.arange(1, SUPPORT + 1, dtype=np.float64))
    rp, cl, vl = vc.random_csr(seed + 1, n - SUPPORT, 12, symmetric=True)
    A = sp.csr_matrix(sp.block_diag([sp.csr_matrix(D), sp.csr_matrix((vl, cl, rp), shape=(n - SUPPORT, n - SUPPORT))]))
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def rows(family, kind):
    """(rowptr, col, val) of a family, kind "sym" or "gen"; built once"""
    key = (family, kind)
    if key in _ROWS:
        return _ROWS[key]
    if family in RAGGED:
        n, top_gen, top_sym, cplx, band = (RAGGED[family] + (None,))[:5]
        if kind == "sym":
            out = symmetrised(ragged(n, top_sym, _seed(family, kind), cplx, band))
        else:
            out = ragged(n, top_gen, _seed(family, kind), cplx, band)
    elif family == "long4000":
        out = vc.random_csr(101, 4000, 12, symmetric=True) if kind == "sym" else vc.random_csr(102, 4000, 20)
    elif family == "lap18":
        out = vc.laplacian(18)
    elif family in ("blocks", "zblocks"):
        out = flatten_blocks(*blocks_of(family, kind))
    elif family in ("bd3000", "bd40000", "zbd3000"):  # symmetric only, like bdlong3000 and chain3000: the breakdown cases run every scheme on it
        out = vc.block_diagonal(103 if family != "bd40000" else 105, 40000 if family == "bd40000" else 3000, SUPPORT)
        if family == "zbd3000":
            out = _hermitian_twist(out)
    elif family == "bdlong3000":
        out = _block_diagonal_long(107, 3000)
    elif family == "chain3000":
        out = _chain(3000)
    else:
        raise ValueError(family)
    _ROWS[key] = out
    return out


def is_complex(family):
    return family in ("z5000", "z9001", "zblocks", "zbd3000")


def start(family, seed=7, support=None):
    n = rows(family, "sym")[0].size - 1
    return vc.start_vector(vc.hash_seed(f"layout_pass_cases/start/{family}/{seed}"), n, is_complex(family), support)


# ---- layouts: how a family goes up, and what the handle must then report ------------------------------------------------------------
# name -> (upload kind, column_blocks argument, layout(), encoding(), column_blocks(), bit-identical to plain CSR in every scheme)
# ("wide" reports what plain CSR reports: the handle has no accessor for the width of its row pointers, so that EIGENEX_FORCE_WIDE_ROWPTR
# took effect rests on eigenex_csr_upload64 reading it, as in test_upload_with_64_bit_row_pointers)
LAYOUTS = {
    "csr": ("upload", 0, "csr", "plain", 1, False),
    "wide": ("upload64", None, "csr", "plain", 1, True),
    "codes": ("laplacian", None, "csr", "row_codes", 1, True),
    "codes_up": ("upload", None, "csr", "row_codes", 1, True),
    "cb3": ("upload", 3, "column_blocked", "plain", 3, True),
    "sorted": ("upload", -2, "sorted_tiles", "plain", 1, False),
    "split": ("upload", -3, "split_tiles", "plain", 1, False),
    "dense": ("blocks", None, "dense_blocks", "plain", 1, False),
}
# (family, layout) of the step cases
STEP_CASES = [(f, lay) for f in ("r5000", "r9001") for lay in ("csr", "wide", "cb3", "split")]
STEP_CASES += [(f, lay) for f in ("z5000", "z9001") for lay in ("csr", "cb3", "split")]
STEP_CASES += [("long4000", "csr"), ("lap18", "codes"), ("s40000_4", "sorted"), ("s40000_2", "sorted"), ("s70001_1", "sorted"),
               ("blocks", "dense"), ("zblocks", "dense"), ("chain3000", "codes_up")]
SHARD_CASES = [("band9001", "csr"), ("r9001", "csr"), ("s70001_1", "sorted"), ("r9001", "split"), ("blocks", "dense")]
TILE_LOOP_CASES = [("s70001_1", "csr"), ("s70001_1", "cb3"), ("s70001_1", "sorted")]
BREAKDOWN_CASES = [("bd3000", "csr"), ("bdlong3000", "csr"), ("bd3000", "wide"), ("bd3000", "cb3"), ("bd3000", "split"), ("bd40000", "sorted"), ("chain3000", "codes_up"),
                   ("zbd3000", "csr"), ("zbd3000", "cb3"), ("zbd3000", "split"), ("blocks", "dense"), ("zblocks", "dense")]


SHARD_BREAKDOWN_CASES = [("chain3000", "csr")]  # three shards of 1,000 rows: the start vector lives on the first shard alone


def upload(capi, ctx, family, kind, layout):
    """the handle of a family in a layout; "plain" is the plain-CSR handle every case is compared with (column_blocks = 0)"""
    r = rows(family, kind)
    n = r[0].size - 1
    how, cb = ("upload", 0) if layout == "plain" else LAYOUTS[layout][:2]
    if how == "upload":
        return capi.Csr.upload(ctx, n, *r, column_blocks=cb)
    if how == "laplacian":
        assert family == "lap18"
        return capi.Csr.laplacian3d(ctx, 18)
    if how == "blocks":
        sizes, blocks = blocks_of(family, kind)
        return capi.Csr.upload_blocks(ctx, sizes, sizes, blocks)
    if how == "upload64":  # read per call by eigenex_csr_upload64: only this operator gets the 64-bit row pointers on the device
        os.environ["EIGENEX_FORCE_WIDE_ROWPTR"] = "1"
        try:
            A = capi.Csr.upload64(ctx, n, r[0].astype(np.int64), r[1], r[2])
        finally:
            os.environ.pop("EIGENEX_FORCE_WIDE_ROWPTR", None)
        A.is_complex = False
        return A
    raise ValueError(layout)
