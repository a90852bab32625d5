"""The Chebyshev filter and moments kernels (k_spmv_cheb, k_spmv_rows_cheb, k_cheb_combine, k_spmv_moments, k_spmv_rows_moments,
k_cheb_moments) at the shapes the inputs of tests/test_gpu_filter.py and tests/test_gpu_density.py do not reach: whole vector
tiles of 2048 doubles, several tiles per workgroup (fewer workgroups than tiles after eigenex_basis_tune), the XCD-sliced tile
order, long rows, 64-bit row pointers, 16-byte row-code records, rows and a whole 256-row tile without entries, retuned grids.

References and bounds are the ones of those two modules: the float64 restatement (density_reference.device_matmul,
chebyshev_vectors) for t_d bit for bit, long double for the filter output (error <= 4 x the restatement's own + 4 eps sum|mu|
|x|_inf), _check_moments for the moments; everything else is exact equality between two forms of the same computation.

Which test launches which kernel body (LONG, OFF, NT are the template arguments of k_spmv_cheb / k_spmv_moments):
  <false, int32, false>   test_several_tiles_per_workgroup[chain], test_rows_without_entries[narrow, no_row_codes]
  <false, int32, true>    test_wide_row_pointers_change_nothing (tune(flags=2) on the chain)
  <true,  int32, false>   test_long_rows[flags=0]
  <true,  int32, true>    test_long_rows[flags=2]
  <false, int64, false>   test_wide_row_pointers_change_nothing[chain], test_rows_without_entries[wide]
  <false, int64, true>    test_wide_row_pointers_change_nothing[chain] (tune(flags=2))
  <true,  int64, false>   test_wide_row_pointers_change_nothing[band]
  <true,  int64, true>    test_wide_row_pointers_change_nothing[band] (tune(flags=2))
  k_spmv_rows_cheb<8> / k_spmv_rows_moments<8>     test_several_tiles_per_workgroup[stencil3]
  k_spmv_rows_cheb<16> / k_spmv_rows_moments<16>   test_sixteen_byte_row_codes
  cheb_tile<true|false>, moments_tile<true|false>  test_whole_vector_tiles_and_a_tail, test_several_vector_tiles_per_workgroup
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_reference as dr  # noqa: E402
import filter_reference as fr  # noqa: E402
import test_gpu_density as td  # noqa: E402  (_check_moments, _counted_moments)
import test_gpu_filter as tf  # noqa: E402  (its inputs, _set_filter_form, _run_steps)

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
DEGREES = (1, 2, 3, 6)
N_MOMENTS = (1, 2, 3, 4, 5, 12, 13)
TILE_DOUBLES = 2048  # kTileRows of the streaming kernels
TILE_ROWS = 256  # kSpmvRows of the operator kernels
PALETTE = np.array([2.5, -1.0, 0.5, -0.25, 0.125])


@pytest.fixture(scope="module")
def capi():
    from cmpt_eigenex_amd import capi as c

    assert c.device_count() >= 1
    return c


@pytest.fixture(scope="module")
def cus(capi):
    """compute units of the device: the persistent grids are min(tiles, CUs x blocks per CU)"""
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _context(capi, shards):
    return capi.Context(loopback_shards=shards) if shards > 1 else capi.Context()


# ---- inputs: built once per module ----------------------------------------------------------------------------------
def _csr(rows, cols, vals, n):
    import scipy.sparse as sp

    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


def _palette_stencil(n, offsets, always, seed):
    """symmetric matrix with the diagonals `offsets` (>= 0; 0 is the main diagonal), values drawn from PALETTE; an entry of an
    offset not in `always` is stored with probability 0.8 (with its mirror image), one of `always` always: as _few_value_stencil
    of test_gpu_row_codes.py, whose docstring says why the outermost pair must be complete"""
    rng = np.random.RandomState(seed)
    rows, cols, vals = [], [], []
    for d in offsets:
        r = np.arange(n - d)
        if d not in always:
            r = r[rng.rand(n - d) < 0.8]
        v = PALETTE[rng.randint(0, PALETTE.size, r.size)]
        rows.append(r), cols.append(r + d), vals.append(v)
        if d:
            rows.append(r + d), cols.append(r), vals.append(v)
    return _csr(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), n)


def _band(n=700, half=12, seed=9):
    """B + B^T of an upper band of random normal values: about 2 half entries per row, columns ascending, no few-value palette"""
    rng = np.random.RandomState(seed)
    rows, cols, vals = [], [], []
    for d in range(half + 1):
        r = np.arange(n - d)
        v = rng.standard_normal(n - d)
        rows.append(r), cols.append(r + d), vals.append(2 * v if d == 0 else v)
        if d:
            rows.append(r + d), cols.append(r), vals.append(v)
    return _csr(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), n)


GONE = np.concatenate([[0, 7], np.arange(256, 512), [999]])  # rows and columns removed from the chain of 1000: one whole tile, three more


def _chain_with_gaps():
    import scipy.sparse as sp

    keep = np.ones(1000)
    keep[GONE] = 0.0
    A = (sp.diags(keep) @ fr.anderson_chain(1000) @ sp.diags(keep)).tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    assert np.all(np.diff(A.indptr)[GONE] == 0) and abs(A - A.T).nnz == 0
    return A


_INPUTS = {}


def _input(name):
    if name not in _INPUTS:
        kind, _, size = name.partition(":")
        if kind == "chain":
            A = fr.anderson_chain(int(size))
        elif kind == "ztridiagonal":
            A = fr.hermitian_tridiagonal(int(size))
        elif kind == "stencil3":
            A = _palette_stencil(int(size), (0, 1), (0, 1), 21)
        elif kind == "stencil11":
            A = _palette_stencil(3001, (0, 1, 2, 40, 41, 80), (80,), 23)
        elif kind == "band":
            A = _band()
        elif kind == "gaps":
            A = _chain_with_gaps()
        elif kind == "laplacian12":
            A = tf._input("laplacian12")
        else:
            raise KeyError(name)
        _INPUTS[name] = A
    return _INPUTS[name]


def _upload(capi, ctx, name, column_blocks=None):
    A = _input(name)
    if name == "laplacian12":
        return capi.Csr.laplacian3d(ctx, 12)
    return capi.Csr.upload(ctx, A.shape[0], A.indptr, A.indices, A.data, column_blocks=column_blocks)


# ---- references: computed once per (input, degree) and left unchanged --------------------------------------------------
_FREFS, _MREFS = {}, {}


def _start_vector(A):
    n = A.shape[0]
    rng = np.random.RandomState(17)
    return rng.standard_normal(n) + (1j * rng.standard_normal(n) if np.iscomplexobj(A.data) else 0.0)


def _filter_reference(name, degree):
    """x, mu, center, halfwidth, p(A) x in long double, the float64 restatement's own error against it (as
    test_gpu_filter._reference, with the matmul that takes rows without entries)"""
    key = (name, degree)
    if key not in _FREFS:
        A = _input(name)
        x = _start_vector(A)
        mu, c, h = tf._filter_of(A, degree)
        ld = np.clongdouble if np.iscomplexobj(A.data) else np.longdouble
        y64 = fr.apply_filter(fr.csr_rowsum_matmul_any_rows(A.indptr, A.indices, A.data, A.data.dtype), x, mu, c, h)
        yld = fr.apply_filter(fr.csr_rowsum_matmul_any_rows(A.indptr, A.indices, A.data, ld), x.astype(ld), mu, c, h)
        _FREFS[key] = (x, mu, c, h, yld, float(np.abs(y64.astype(ld) - yld).max()))
    return _FREFS[key]


def _moments_reference(name, n_moments=N_MOMENTS):
    """x, (center, halfwidth), the float64 restatement's t_0 .. t_d"""
    d = dr.applications(max(n_moments))
    if name not in _MREFS or len(_MREFS[name][3]) <= d:
        A = _input(name)
        x = _start_vector(A)
        c, h = dr.widened(*fr.gershgorin(A))
        _MREFS[name] = (x, c, h, dr.chebyshev_vectors(dr.device_matmul(A), x, c, h, d))
    return _MREFS[name]


# ---- the checks ------------------------------------------------------------------------------------------------------
def _counted_filter(capi, ctx, b, x):
    """y = p(A) x, the launches booked as operator work for it and their bytes"""
    b.upload(capi.VEC_COL(0), x)
    ctx.profile_enable(True)
    ctx.profile_reset()
    b.filter_apply(capi.VEC_COL(0), capi.VEC_V)
    launches, _, nbytes = ctx.profile_get(capi.K_SPMV)
    ctx.profile_enable(False)
    return b.download(capi.VEC_V), launches, nbytes


def _check_filter(capi, monkeypatch, ctx, b, name, label, shards, epilogue, degrees=DEGREES):
    """For every degree: the launches of the form (one per degree and shard where the operator kernel takes the step in its
    epilogue, else two), the output within the bound of test_filter_apply_against_long_double, the input left alone, and where
    there is an epilogue the same bits from the composed form (EIGENEX_NO_FUSED_FILTER).  Returns {degree: (y, bytes booked)}
    of the first form."""
    out = {}
    for degree in degrees:
        x, mu, c, h, yld, err64 = _filter_reference(name, degree)
        got = {}
        for form in ("fused", "composed") if epilogue else ("fused",):
            tf._set_filter_form(monkeypatch, b, form, mu, c, h)
            y, launches, nbytes = _counted_filter(capi, ctx, b, x)
            assert launches == (degree if epilogue and form == "fused" else 2 * degree) * shards
            np.testing.assert_array_equal(b.download(capi.VEC_COL(0)), x)
            got[form] = (y, nbytes)
        if epilogue:
            np.testing.assert_array_equal(got["fused"][0], got["composed"][0])
        y = got["fused"][0]
        err = float(np.abs(y.astype(yld.dtype) - yld).max())
        bound = 4 * err64 + 4 * EPS * np.abs(mu).sum() * np.abs(x).max()
        print(f"{label} degree={degree}: device error {err:.3e}, float64 restatement {err64:.3e}, bound {bound:.3e}")
        assert err <= bound
        out[degree] = got["fused"]
    monkeypatch.delenv("EIGENEX_NO_FUSED_FILTER", raising=False)
    return out


def _check_moments(capi, monkeypatch, ctx, b, name, label, shards, epilogue, n_moments=N_MOMENTS):
    """For every moment count: the launches of the form, t_d the restatement's bit for bit, every moment within
    test_gpu_density._check_moments -- in the fused and (where there is an epilogue) the streaming form.  Returns
    {n_moments: (mu, t_d)} of the first form."""
    x, c, h, ts = _moments_reference(name)
    b.upload(capi.VEC_COL(0), x)
    out = {}
    for nm in n_moments:
        d = dr.applications(nm)
        for form in ("fused", "streaming") if epilogue else ("fused",):
            if form == "streaming":
                monkeypatch.setenv("EIGENEX_NO_FUSED_FILTER", "1")
            else:
                monkeypatch.delenv("EIGENEX_NO_FUSED_FILTER", raising=False)
            mu, t_d, launches, _ = td._counted_moments(capi, ctx, b, nm, c, h)
            assert launches == (d if epilogue and form == "fused" else 2 * d) * shards
            np.testing.assert_array_equal(t_d, ts[d])
            td._check_moments(f"{label} {form}", mu, name, ts, nm)
            out.setdefault(nm, (mu, t_d))
    monkeypatch.delenv("EIGENEX_NO_FUSED_FILTER", raising=False)
    np.testing.assert_array_equal(b.download(capi.VEC_COL(0)), x)
    return out


# ---- (a) whole vector tiles and a ragged tail: k_cheb_combine, k_cheb_moments ------------------------------------------
@pytest.mark.parametrize("shards", [1, 2, 3])
@pytest.mark.parametrize("case", ["column_blocked", "plain", "complex"])
def test_whole_vector_tiles_and_a_tail(capi, monkeypatch, case, shards):
    """2 x 2048 + 38 doubles: two tiles take cheb_tile<true> / moments_tile<true>, the last one the ragged form, in one launch
    (one shard; two shards: one whole tile and a tail each).  The chain in two column blocks and the complex tridiagonal
    matrix have no epilogue (two launches per degree); the plain chain runs fused and under EIGENEX_NO_FUSED_FILTER."""
    n_doubles = 2 * TILE_DOUBLES + 38
    name = f"ztridiagonal:{n_doubles // 2}" if case == "complex" else f"chain:{n_doubles}"
    ctx = _context(capi, shards)
    A = _upload(capi, ctx, name, column_blocks=2 if case == "column_blocked" else None)
    assert A.layout() == ("column_blocked" if case == "column_blocked" else "csr") and A.encoding() == "plain"
    n = _input(name).shape[0]
    assert n * (2 if case == "complex" else 1) == n_doubles
    b = capi.Basis(ctx, A, n, 3)
    label = f"{case} shards={shards}"
    _check_filter(capi, monkeypatch, ctx, b, name, label, shards, epilogue=case == "plain")
    _check_moments(capi, monkeypatch, ctx, b, name, label, shards, epilogue=case == "plain")
    b.close()
    A.close()
    ctx.close()


@pytest.mark.parametrize("form", ["fused", "composed"])
def test_odd_length_stays_inside_its_column(capi, monkeypatch, form):
    """4135 rows: the last 16-byte access of the ragged tile straddles n.  The filter writes into basis column 0; column 1,
    next to it in memory, keeps its pattern bit for bit, and so does column 2 that holds the input"""
    name = "chain:4135"
    ctx = capi.Context()
    A = _upload(capi, ctx, name)
    n = _input(name).shape[0]
    b = capi.Basis(ctx, A, n, 3)
    pattern = np.ldexp(1.0 + np.arange(n) / 8192.0, (np.arange(n) % 7) - 3) * np.where(np.arange(n) % 2, -1.0, 1.0)
    for degree in DEGREES:
        x, mu, c, h, yld, err64 = _filter_reference(name, degree)
        tf._set_filter_form(monkeypatch, b, form, mu, c, h)
        b.upload(capi.VEC_COL(1), pattern)
        b.upload(capi.VEC_COL(2), x)
        b.filter_apply(capi.VEC_COL(2), capi.VEC_COL(0))
        np.testing.assert_array_equal(b.download(capi.VEC_COL(1)).view(np.uint64), pattern.view(np.uint64))
        np.testing.assert_array_equal(b.download(capi.VEC_COL(2)), x)
        err = float(np.abs(b.download(capi.VEC_COL(0)).astype(np.longdouble) - yld).max())
        assert err <= 4 * err64 + 4 * EPS * np.abs(mu).sum() * np.abs(x).max()
    x, c, h, ts = _moments_reference(name)
    if form == "composed":
        monkeypatch.setenv("EIGENEX_NO_FUSED_FILTER", "1")
    b.upload(capi.VEC_COL(0), x)
    for nm in N_MOMENTS:
        mu = b.kpm_moments(capi.VEC_COL(0), nm, c, h)
        np.testing.assert_array_equal(b.download(capi.VEC_V), ts[dr.applications(nm)])
        td._check_moments(f"{name} {form}", mu, name, ts, nm)
        np.testing.assert_array_equal(b.download(capi.VEC_COL(1)).view(np.uint64), pattern.view(np.uint64))
    b.close()
    A.close()
    ctx.close()


# ---- (b) several tiles per workgroup, operator kernels -----------------------------------------------------------------
def _rows_for_tiles_per_workgroup(cus, lists=1):
    """rows of (2 CUs + 1) whole tiles and a last one of 37: more than 2 tiles per workgroup of a grid of CUs.  lists > 1: that
    many times 2 CUs + 3 tiles, so that each of `lists` shards has as many behind its two boundary tiles"""
    return lists * (2 * cus + (3 if lists > 1 else 1)) * TILE_ROWS + 37


@pytest.mark.parametrize("shards,lists", [(1, 1), (3, 1), (3, 3)])
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("kind", ["chain", "stencil3"])
def test_several_tiles_per_workgroup(capi, monkeypatch, cus, kind, flags, shards, lists):
    """After tune(2, 1, flags) the operator grid is one workgroup per CU.  (2 CUs + 1) x 256 + 37 rows: some workgroups go round
    their tile loop three times, the others twice, the dots are carried from tile to tile, the prefetch of the next tile's rows
    runs in front of an epilogue, and the last tile has 37 rows.  flags = 1: the XCD-sliced tile order.  Three shards at this
    length have fewer tiles each than the grid has workgroups and test the interior / boundary tile lists side by side; at three
    times the length (lists = 3) every shard's interior list again has more than two tiles per workgroup."""
    n = _rows_for_tiles_per_workgroup(cus, lists)
    assert cus % 8 == 0  # else the XCD-sliced order is not taken and flags = 1 does nothing
    rows_per_shard = [e - s for s, e in (capi.partition(n, shards, k) for k in range(shards))]
    if shards == lists:
        assert min(-(-r // TILE_ROWS) for r in rows_per_shard) - (2 if shards > 1 else 0) > 2 * cus  # (less the two boundary tiles)
    name = f"{kind}:{n}"
    ctx = _context(capi, shards)
    A = _upload(capi, ctx, name)
    assert A.layout() == "csr" and A.encoding() == ("row_codes" if kind == "stencil3" else "plain")
    b = capi.Basis(ctx, A, n, 3)
    b.tune(2, 1, flags)
    label = f"{kind} n={n} flags={flags} shards={shards}"
    _check_filter(capi, monkeypatch, ctx, b, name, label, shards, epilogue=True)
    _check_moments(capi, monkeypatch, ctx, b, name, label, shards, epilogue=True)
    b.close()
    A.close()
    ctx.close()


# ---- (c) several tiles per workgroup, streaming kernels ----------------------------------------------------------------
@pytest.mark.parametrize("case", ["real", "complex"])
def test_several_vector_tiles_per_workgroup(capi, monkeypatch, cus, case):
    """After tune(1, 4, 0) the vector grid is one workgroup per CU.  (2 CUs + 1) x 2048 + 38 doubles: k_cheb_combine and
    k_cheb_moments go round their tile loop two and three times, whole tiles first and the ragged one last (real: the chain
    under EIGENEX_NO_FUSED_FILTER, compared with the fused form as well; complex: the tridiagonal matrix of half as many rows)"""
    n_doubles = (2 * cus + 1) * TILE_DOUBLES + 38
    assert -(-n_doubles // TILE_DOUBLES) > 2 * cus
    name = f"ztridiagonal:{n_doubles // 2}" if case == "complex" else f"chain:{n_doubles}"
    ctx = capi.Context()
    A = _upload(capi, ctx, name)
    n = _input(name).shape[0]
    assert n * (2 if case == "complex" else 1) == n_doubles and A.layout() == "csr" and A.encoding() == "plain"
    b = capi.Basis(ctx, A, n, 3)
    b.tune(1, 4, 0)
    _check_filter(capi, monkeypatch, ctx, b, name, case, 1, epilogue=case == "real", degrees=(1, 3))
    _check_moments(capi, monkeypatch, ctx, b, name, case, 1, epilogue=case == "real", n_moments=(3, 6))
    b.close()
    A.close()
    ctx.close()


# ---- (d) long rows -------------------------------------------------------------------------------------------------------
def _assert_long_rows_on_every_shard(capi, A, shards):
    for k in range(shards):
        r0, r1 = capi.partition(A.shape[0], shards, k)
        assert A.indptr[r1] - A.indptr[r0] >= 16 * (r1 - r0)  # has_long_rows is decided per shard


@pytest.mark.parametrize("shards", [1, 2, 3])
@pytest.mark.parametrize("flags", [0, 2])
def test_long_rows(capi, monkeypatch, flags, shards):
    """The band matrix: about 24 entries per row, so the LONG instances of the fused kernels; a tile of 256 rows holds about 6000
    entries, three chunks of 2048, and rows cross the chunk boundaries.  The long-rows loop adds in stored order: t_d bit for bit"""
    name = "band"
    Asp = _input(name)
    assert np.diff(Asp.indptr).max() == 25 and Asp.indptr[256] > 2 * 2048
    _assert_long_rows_on_every_shard(capi, Asp, shards)
    ctx = _context(capi, shards)
    A = _upload(capi, ctx, name)
    assert A.layout() == "csr" and A.encoding() == "plain"
    b = capi.Basis(ctx, A, Asp.shape[0], 3)
    b.tune(flags=flags)
    label = f"band flags={flags} shards={shards}"
    _check_filter(capi, monkeypatch, ctx, b, name, label, shards, epilogue=True)
    _check_moments(capi, monkeypatch, ctx, b, name, label, shards, epilogue=True)
    b.close()
    A.close()
    ctx.close()


# ---- (e) 64-bit row pointers ---------------------------------------------------------------------------------------------
def _upload_wide_or_not(capi, monkeypatch, ctx, name, wide):
    if wide:
        monkeypatch.setenv("EIGENEX_FORCE_WIDE_ROWPTR", "1")  # read per upload
    else:
        monkeypatch.delenv("EIGENEX_FORCE_WIDE_ROWPTR", raising=False)
    A = _upload(capi, ctx, name)
    monkeypatch.delenv("EIGENEX_FORCE_WIDE_ROWPTR", raising=False)
    return A


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("name", ["chain:1000", "band"])
def test_wide_row_pointers_change_nothing(capi, monkeypatch, name, shards):
    """The same operator with 64-bit and with 32-bit row pointers, default and non-temporal cache policy: one kernel body and one
    grid, so the filter output, t_d and every moment agree bit for bit, with one launch per degree in all four"""
    n = _input(name).shape[0]
    if name == "band":
        _assert_long_rows_on_every_shard(capi, _input(name), shards)
    out = {}
    for wide in (False, True):
        ctx = _context(capi, shards)
        A = _upload_wide_or_not(capi, monkeypatch, ctx, name, wide)
        assert A.layout() == "csr" and A.encoding() == "plain"
        b = capi.Basis(ctx, A, n, 3)
        for flags in (0, 2):
            b.tune(flags=flags)
            label = f"{name} wide={wide} flags={flags} shards={shards}"
            ys = _check_filter(capi, monkeypatch, ctx, b, name, label, shards, epilogue=True)
            ms = _check_moments(capi, monkeypatch, ctx, b, name, label, shards, epilogue=True)
            out[(wide, flags)] = ([ys[d][0] for d in DEGREES], [ms[nm][0] for nm in N_MOMENTS], [ms[nm][1] for nm in N_MOMENTS])
        b.close()
        A.close()
        ctx.close()
    for key in ((False, 2), (True, 0), (True, 2)):
        for got, want in zip(out[key], out[(False, 0)]):
            for u, v in zip(got, want):
                np.testing.assert_array_equal(u, v)


# ---- (f) 16-byte row-code records ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [1, 2])
def test_sixteen_byte_row_codes(capi, monkeypatch, shards):
    """11 offsets {0, +-1, +-2, +-40, +-41, +-80} (16 with the halo offsets of a second shard), five values: records of 16 bytes,
    k_spmv_rows_cheb<16> / k_spmv_rows_moments<16>.  That the 16-byte form is in use is read from the bytes the profile books
    per fused degree: the operator's share is record bytes x 3072 (the rows rounded up to whole tiles; 2 x 1536 on two shards)
    + 8 x palette entries per shard.  The same stencil as plain CSR (EIGENEX_NO_ROW_CODES): the same bits"""
    name = "stencil11"
    Asp = _input(name)
    n = Asp.shape[0]
    offsets = np.unique(Asp.indices - np.repeat(np.arange(n), np.diff(Asp.indptr)))
    np.testing.assert_array_equal(offsets, [-80, -41, -40, -2, -1, 0, 1, 2, 40, 41, 80])
    assert np.unique(Asp.data).size == 5 and abs(Asp - Asp.T).nnz == 0
    out = {}
    for coded in (True, False):
        ctx = _context(capi, shards)
        if coded:
            monkeypatch.delenv("EIGENEX_NO_ROW_CODES", raising=False)
        else:
            monkeypatch.setenv("EIGENEX_NO_ROW_CODES", "1")  # read per upload
        A = _upload(capi, ctx, name)
        monkeypatch.delenv("EIGENEX_NO_ROW_CODES", raising=False)
        assert A.layout() == "csr" and A.encoding() == ("row_codes" if coded else "plain")
        b = capi.Basis(ctx, A, n, 3)
        label = f"{name} coded={coded} shards={shards}"
        ys = _check_filter(capi, monkeypatch, ctx, b, name, label, shards, epilogue=True)
        ms = _check_moments(capi, monkeypatch, ctx, b, name, label, shards, epilogue=True)
        if coded:
            for degree in DEGREES:  # enq_filter books 24 n bytes of vectors in the first degree and 40 n in every later one
                operator_bytes = ys[degree][1] - (24.0 + 40.0 * (degree - 1)) * n
                assert operator_bytes == degree * (16 * 3072 + 8 * PALETTE.size * shards)
        out[coded] = ([ys[d][0] for d in DEGREES], [ms[nm][1] for nm in N_MOMENTS], [ms[nm][0] for nm in N_MOMENTS])
        b.close()
        A.close()
        ctx.close()
    for k, (got, want) in enumerate(zip(out[True], out[False])):
        if k < 2 or shards == 1:  # filter output and t_d; the moments on one shard
            for u, v in zip(got, want):
                np.testing.assert_array_equal(u, v)


# ---- (g) rows without entries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("form", ["narrow", "no_row_codes", "wide"])
def test_rows_without_entries(capi, monkeypatch, form, shards):
    """The chain of 1000 rows without rows and columns 256 .. 511 (a whole tile whose [p0, p1) is empty) and 0, 7, 999.  The
    epilogue still takes the step there: t_{k+1} = c (0 - center t_k) - t_{k-1}, a scalar recurrence per row, asserted exactly.
    Of two shards the first keeps 254 sites and the hopping, 255 distinct values: it just fits the palette of 255 and is row-coded
    (records without any slot for its empty rows), so the plain 32-bit kernels get that sharding under EIGENEX_NO_ROW_CODES"""
    name = "gaps"
    Asp = _input(name)
    n = Asp.shape[0]
    wide = form == "wide"
    ctx = _context(capi, shards)
    if form == "no_row_codes":
        monkeypatch.setenv("EIGENEX_NO_ROW_CODES", "1")  # read per upload
    A = _upload_wide_or_not(capi, monkeypatch, ctx, name, wide)
    monkeypatch.delenv("EIGENEX_NO_ROW_CODES", raising=False)
    values = [np.unique(Asp.data[Asp.indptr[r0]:Asp.indptr[r1]]).size for r0, r1 in (capi.partition(n, shards, k) for k in range(shards))]
    assert values == ([742] if shards == 1 else [255, 488])
    coded = form == "narrow" and min(values) <= 255  # kRowCodeMaxValues
    assert A.layout() == "csr" and A.encoding() == ("row_codes" if coded else "plain")
    b = capi.Basis(ctx, A, n, 3)
    label = f"gaps {form} shards={shards}"
    _check_filter(capi, monkeypatch, ctx, b, name, label, shards, epilogue=True)
    ms = _check_moments(capi, monkeypatch, ctx, b, name, label, shards, epilogue=True)
    x, c, h, _ = _moments_reference(name)
    assert c != 0.0
    c1, c2, shift = np.float64(1.0 / h), np.float64(2.0 / h), np.float64(-c)
    t = [x[GONE]]
    for k in range(dr.applications(max(N_MOMENTS))):
        a = 0.0 + shift * t[-1]
        t.append(c1 * a if k == 0 else c2 * a - t[-2])
    for nm in N_MOMENTS:
        np.testing.assert_array_equal(ms[nm][1][GONE], t[dr.applications(nm)])
    b.close()
    A.close()
    ctx.close()


# ---- (h) retuned grids -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["chain1000x3", "laplacian12x2", "tilesx1", "tilesx3"])
def test_retuned_operator_grids(capi, monkeypatch, cus, case):
    """eigenex_basis_tune(2, s, 0), s = 1, 4, 16, changes how many partial dots k_reduce sums behind the fused moments kernels
    (between shards: two launches, interior and boundary, their partials side by side).  t_d does not depend on the grid: bit
    for bit across s and against the restatement; every moment within the bound; a repeated run gives the same bits.  The two
    small inputs have fewer tiles than any of the grids has workgroups (the grid is then the number of tiles, whatever s); the
    chain of 3 x (2 CUs + 1) tiles has 1, 4 and 6 CUs' worth of workgroups on one shard and 1 and 2 per shard on three"""
    nm = 13
    d = dr.applications(nm)
    name, shards = {"chain1000x3": ("chain:1000", 3), "laplacian12x2": ("laplacian12", 2),
                    "tilesx1": (f"chain:{_rows_for_tiles_per_workgroup(cus, 3)}", 1),
                    "tilesx3": (f"chain:{_rows_for_tiles_per_workgroup(cus, 3)}", 3)}[case]
    n = _input(name).shape[0]
    x, c, h, ts = _moments_reference(name)
    ctx = _context(capi, shards)
    A = _upload(capi, ctx, name)
    assert A.encoding() == ("row_codes" if name == "laplacian12" else "plain")
    b = capi.Basis(ctx, A, n, 3)
    b.upload(capi.VEC_COL(0), x)
    for s in (1, 4, 16):
        b.tune(2, s, 0)
        mu, t_d, launches, _ = td._counted_moments(capi, ctx, b, nm, c, h)
        mu2, t_d2, _, _ = td._counted_moments(capi, ctx, b, nm, c, h)
        assert launches == d * shards
        np.testing.assert_array_equal(mu, mu2)
        np.testing.assert_array_equal(t_d, t_d2)
        np.testing.assert_array_equal(t_d, ts[d])
        td._check_moments(f"{case} blocks per CU = {s}", mu, name, ts, nm)
    b.close()
    A.close()
    ctx.close()


# ---- (i) filtered Lanczos steps on the new instances ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["band", "wide_chain", "stencil11", "tiles"])
def test_filtered_lanczos_steps_fused_and_composed(capi, monkeypatch, cus, case):
    """8 filtered Lanczos steps of degree 6: here the fused kernel also applies the device scale to its input and writes the
    basis column u.  alpha and beta of the fused and the composed form agree bit for bit"""
    name = {"band": "band", "wide_chain": "chain:1000", "stencil11": "stencil11", "tiles": f"chain:{_rows_for_tiles_per_workgroup(cus)}"}[case]
    n = _input(name).shape[0]
    ctx = capi.Context()
    A = _upload_wide_or_not(capi, monkeypatch, ctx, name, case == "wide_chain")
    assert A.layout() == "csr" and A.encoding() == ("row_codes" if case == "stencil11" else "plain")
    b = capi.Basis(ctx, A, n, 9)
    if case == "tiles":
        b.tune(2, 1, 1)
    x, mu, c, h, _, _ = _filter_reference(name, 6)
    out = {}
    for form in ("fused", "composed"):
        tf._set_filter_form(monkeypatch, b, form, mu, c, h)
        st, alpha, beta = tf._run_steps(capi, b, x, 8)
        assert st.nvec == 8 and st.stopped == 0
        out[form] = (np.array(alpha), np.array(beta), np.stack([b.download(capi.VEC_COL(k)) for k in range(8)]))
    for u, v in zip(out["fused"], out["composed"]):
        np.testing.assert_array_equal(u, v)
    assert np.all(np.isfinite(out["fused"][0])) and np.all(out["fused"][1] > 0)
    b.close()
    A.close()
    ctx.close()
