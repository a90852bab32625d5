"""The operators of tests/layout_pass_cases.py on the host: what makes the assertion of tests/test_gpu_layout_krylov_passes.py fair.
No GPU; the library is used for solver.blocks_to_csr alone (host code).

For every family, "sym" and "gen", and every shift the device cases use, the fp64 recurrences run for 8 calls and pass the local
check of tests/krylov_local_reference.py, orthogonality included: kl.lanczos_fp64 (on "sym"), kl.arnoldi_fp64 with one and with
two passes (on both), one_sweep_reference.one_sweep (on the real "sym").  An input on which a recurrence comes near the bound
would be replaced, not tolerated: every ratio must stay below 0.1.

Also: the properties the families are built for (empty rows, row lengths, the tile height of the column-sorted layout, symmetry,
the isolated first rows of the breakdown families) and the agreement of flatten_blocks with the two other writers of block rows.

Measured ratios: profiles/layout_krylov_passes.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import krylov_local_reference as kl  # noqa: E402
import layout_pass_cases as lc  # noqa: E402
import one_sweep_reference as osr  # noqa: E402
from krylov_pass_runs import CALLS, SHIFT_Z, SHIFTS  # noqa: E402

ROOM = 0.1  # a reference recurrence that uses more than a tenth of the bound means another input


def _dense(rows):
    rowptr, col, val = rows
    n = rowptr.size - 1
    D = np.zeros((n, n), val.dtype)
    np.add.at(D, (np.repeat(np.arange(n), np.diff(rowptr)), col), val)
    return D


def _recurrences(family, kind):
    rows = lc.rows(family, kind)
    n = rows[0].size - 1
    cplx = lc.is_complex(family)
    apply = kl.csr_matmul(rows)
    x = lc.start(family)
    worst, worst_ortho = 0.0, 0.0
    for shift in SHIFTS + ((SHIFT_Z,) if cplx else ()):
        reports = []
        if kind == "sym" and shift != SHIFT_Z:
            a, b, V = kl.lanczos_fp64(apply, x, CALLS - 1, shift)
            reports.append(("lanczos", kl.check_lanczos(rows, shift, V, a, b)))
            if not cplx:
                a, b, V, _, _ = osr.one_sweep(apply, x, CALLS - 1, shift)
                reports.append(("one_sweep", kl.check_lanczos(rows, shift, V, a, b)))
        for passes in (1, 2):
            V, H, residue, w = kl.arnoldi_fp64(apply, x, CALLS, shift, passes)
            reports.append((f"arnoldi{passes}", kl.check_arnoldi(rows, shift, V, H, residue, w)))
        for name, rep in reports:
            print(rep.line(f"{family} {kind} n={n} shift={shift} {name}"))
            assert rep.ok(), rep.line(name)
            worst, worst_ortho = max(worst, rep.ratio()), max(worst_ortho, rep["ortho"] / rep["ortho_bound"])
    print(f"HOST RATIO {family} {kind} n={n} nnz={rows[0][-1]}: coefficients {worst:.3e} orthogonality {worst_ortho:.3e}")
    assert worst <= ROOM and worst_ortho <= ROOM


@pytest.mark.parametrize("kind", ["sym", "gen"])
@pytest.mark.parametrize("family", [f for f in lc.FAMILIES if f not in ("bd3000", "bdlong3000", "bd40000", "zbd3000")])
def test_fp64_recurrences_pass_with_room(family, kind):
    _recurrences(family, kind)


@pytest.mark.parametrize("family", lc.BREAKDOWN)
def test_fp64_recurrences_break_down_after_the_isolated_rows(family):
    """a start vector on the first five rows: five columns, then a residue at rounding level; the steps before the stop pass"""
    rows = lc.rows(family, "sym")
    rowptr, col, _ = rows
    assert col[: rowptr[lc.SUPPORT]].max() < lc.SUPPORT and col[rowptr[lc.SUPPORT]:].min() >= lc.SUPPORT
    apply = kl.csr_matmul(rows)
    x = lc.start(family, support=lc.SUPPORT)
    assert np.count_nonzero(x) == lc.SUPPORT
    a, b, V = kl.lanczos_fp64(apply, x, CALLS - 1)
    assert V.shape[0] == lc.SUPPORT and b.size == lc.SUPPORT and b[-1] <= 1e-12
    reports = [("lanczos", kl.check_lanczos(rows, 0.0, V, a, b))]
    if not lc.is_complex(family):
        a, b, V, _, _ = osr.one_sweep(apply, x, CALLS - 1)
        assert V.shape[0] == lc.SUPPORT and b[-1] <= 1e-12
        reports.append(("one_sweep", kl.check_lanczos(rows, 0.0, V, a, b)))
    for passes in (1, 2):
        V, H, residue, w = kl.arnoldi_fp64(apply, x, CALLS, 0.0, passes)
        assert V.shape[0] == lc.SUPPORT and residue <= 1e-12
        reports.append((f"arnoldi{passes}", kl.check_arnoldi(rows, 0.0, V, H, residue, w)))
    worst, worst_ortho = 0.0, 0.0
    for name, rep in reports:
        print(rep.line(f"{family} breakdown {name}"))
        assert rep.ok(), rep.line(name)
        worst, worst_ortho = max(worst, rep.ratio()), max(worst_ortho, rep["ortho"] / rep["ortho_bound"])
    print(f"HOST RATIO breakdown {family} n={rowptr.size - 1}: coefficients {worst:.3e} orthogonality {worst_ortho:.3e}")
    assert worst <= ROOM and worst_ortho <= ROOM  # orthogonality too: one Gram-Schmidt pass must leave an orthogonal last column


@pytest.mark.parametrize("family", list(lc.RAGGED))
def test_ragged_rows_are_what_the_layouts_need(family):
    n, cplx = lc.RAGGED[family][0], lc.RAGGED[family][3]
    for kind in ("sym", "gen"):
        rowptr, col, val = lc.rows(family, kind)
        length = np.diff(rowptr)
        assert rowptr.size == n + 1 and np.iscomplexobj(val) == cplx
        assert length[0] == 0 and length[-1] == 0 and 0.015 * n <= np.count_nonzero(length == 0) <= 0.2 * n
        assert np.count_nonzero(length >= 60) >= 8 and length.max() <= 400
        row = np.repeat(np.arange(n), length)
        assert np.all((np.diff(col) >= 0) | (np.diff(row) > 0))  # ascending within every row
        if kind == "sym":
            D = None if n > 10000 else _dense((rowptr, col, val))
            assert D is None or np.array_equal(D, D.conj().T)
        assert lc.sorted_tile_rows((rowptr, col, val)) == lc.SORTED_TILE_ROWS.get(family), (family, kind)
    assert lc.sorted_tile_rows(lc.rows("bd40000", "sym")) == lc.SORTED_TILE_ROWS["bd40000"]


def test_the_band_leaves_interior_and_boundary_tiles_on_three_shards():
    """eigenex_plan_tiles (host code) on the shards the loopback context makes: both lists exist on every shard of band9001, and
    of chain3000 (the sharded breakdown case), and uniformly random columns (r9001) leave no interior tile"""
    from cmpt_eigenex_amd import capi

    for family, interior in (("band9001", True), ("chain3000", True), ("r9001", False)):
        for kind in ("sym", "gen"):
            rowptr, col, _ = lc.rows(family, kind)
            n = rowptr.size - 1
            for shard in range(3):
                b, e = capi.partition(n, 3, shard)
                plan = capi.ShardPlan(n, 3, shard, rowptr[b:e + 1] - rowptr[b], col[rowptr[b]:rowptr[e]])
                ti, tb = plan.tiles()
                plan.close()
                assert tb.size > 0 and (ti.size > 0) == interior, (family, kind, shard, ti.size, tb.size)
                assert ti.size + tb.size == -(-(e - b) // 256)


def test_the_other_families_are_what_the_layouts_need():
    for kind in ("sym", "gen"):
        for family in ("long4000", "bdlong3000"):
            rowptr, _, _ = lc.rows(family, kind)
            assert rowptr[-1] >= 16 * (rowptr.size - 1)  # has_long_rows
    for family in ("blocks", "zblocks"):
        sizes, blocks = lc.blocks_of(family, "sym")
        assert 0 in sizes and max(sizes) > 2 * 2048 and 700 in sizes
        bare = sizes.index(9)
        assert not any(bare in k for k in blocks) and [k for k in blocks if 0 in k] == [(0, 0)]
        assert any(B.shape[1] > 2 * 2048 for B in blocks.values())
        D = _dense(lc.rows(family, "sym"))
        assert np.array_equal(D, D.conj().T) and np.iscomplexobj(D) == (family == "zblocks")
        sizes, blocks = lc.blocks_of(family, "gen")
        assert not any(k[0] == sizes.index(9) for k in blocks)
    D = _dense(lc.rows("zbd3000", "sym"))
    assert np.array_equal(D, D.conj().T) and np.abs(D.imag).max() > 0
    D = _dense(lc.rows("chain3000", "sym"))
    assert np.array_equal(D, D.T) and np.unique(lc.rows("chain3000", "sym")[2]).size == 5


def test_flatten_blocks_equals_the_other_two_writers():
    import test_gpu_more as tm
    from cmpt_eigenex_amd import solver

    for kind in ("sym", "gen"):
        sizes, blocks = lc.blocks_of("blocks", kind)
        for got, want in zip(lc.rows("blocks", kind), solver.blocks_to_csr(sizes, sizes, blocks)):
            assert got.dtype == want.dtype and np.array_equal(got, want)
    rng = np.random.default_rng(3)
    sizes = [2, 0, 5, 3, 1]
    blocks = {(r, c): rng.standard_normal((sizes[r], sizes[c])) + 1j * rng.standard_normal((sizes[r], sizes[c]))
              for r, c in ((0, 0), (0, 3), (2, 2), (2, 0), (3, 4), (3, 2), (0, 2))}
    for got, want in zip(lc.flatten_blocks(sizes, blocks), tm._flatten_blocks(sizes, sizes, blocks, np.complex128)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
