"""The observables of one vector against basis columns on the device (eigenex_spin_measure_columns, kernels.hip:
k_spin_measure_columns and k_spin_measure_columns_reduce) against the long double restatement of
tests/spin_measure_columns_reference.py, within |out - ref| <= n eps sum_s |term_s| -- the rounding of an n-term sum in any
grouping, so it holds for every launch grid.  Shapes: those of tests/test_gpu_spin_measure.py -- full space L = 3, 6, 8, 9 and 17
with one workgroup per CU (512 tiles: the tile loop goes round); sectors (4,2), (6,0), (6,6), (10,5), (11,5), (31,2), (32,2), (32,31)
and (20,10) with one workgroup per CU (722 tiles); the two large shapes take the short term lists that still span three chunks
of 16 terms.  The columns are uploaded test vectors, so every case is launches of the one kernel pair.  Column counts 1, 3, 4, 5 and
9 around the kernel's chunk of 4, first = 0 and 3.  Then: every chunk boundary of the term lists at (32,2), the independence of a
sum from what shares its call, the cross-check against eigenex_spin_site_apply + eigenex_dots, a Lanczos run that does not notice
a call between its batches -- the pending column of the one-sweep step included -- and the refusals."""
import os
import sys
from math import comb

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_measure_columns_reference as cr  # noqa: E402
import spin_measure_reference as mr  # noqa: E402
import spin_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu
LD = np.longdouble
SHAPES = [(3, None), (6, None), (8, None), (9, None), (17, None), (4, 2), (6, 0), (6, 6), (10, 5), (11, 5), (31, 2), (32, 2), (32, 31), (20, 10)]
LARGE = ((17, None), (20, 10))
J = 4  # csrc/spin_measure_columns.hpp: kSpinMeasureColumns
RANGES = [(0, 1), (0, J - 1), (0, J), (3, J + 1), (3, 2 * J + 1), (0, 1 + 2 * J + 3)]  # (first, count); the last one is every column


@pytest.fixture(scope="module")
def capi():
    from cmpt_eigenex_amd import capi as c

    assert c.device_count() >= 1
    return c


def _operator(capi, ctx, L, n_up, bonds=None, **kw):
    bonds = sr.chain(L, 1.0, 0.7, periodic=True) if bonds is None else bonds
    return capi.Csr.spin_half(ctx, L, bonds, **kw) if n_up is None else capi.Csr.spin_half_sector(ctx, L, n_up, bonds, **kw)


def _short_lists(L, n_up):
    """tests/test_gpu_spin_measure.py: every site, the pairs with the top site, a low and a middle pair, the string, the all-sites
    mask, a duplicate: three chunks"""
    full_d, _ = mr.term_lists(L, n_up)
    top = [(1 << i) | (1 << (L - 1)) for i in range(L - 1)] + [0b11, (1 << (L // 2 - 1)) | (1 << (L // 2))]
    diag = mr.site_masks(L) + top + [int(m) for m in full_d[-3:]]
    flip = top + [top[0]] + (mr.site_masks(L) if n_up is None else [])
    return np.array(diag, np.uint32), np.array(flip, np.uint32)


def _state(capi, ctx, S, V, x=None):
    """a state whose columns are the rows of V; x, if given, in the work vector W"""
    b = capi.Basis(ctx, S, V.shape[1], V.shape[0])
    for j in range(V.shape[0]):
        b.upload(capi.VEC_COL(j), V[j])
    if x is not None:
        b.upload(capi.VEC_W, x)
    return b


@pytest.mark.parametrize("L,n_up", SHAPES)
def test_device_sums_equal_the_restatement_within_the_bound(capi, L, n_up):
    large = (L, n_up) in LARGE
    ranges = [(0, J + 1)] if large else RANGES
    ncol = max(f + c for f, c in ranges)
    diag_masks, flip_masks = _short_lists(L, n_up) if large else mr.term_lists(L, n_up)
    x, V = mr.vector(L, n_up), cr.columns(L, n_up, ncol)
    ref = cr.measure(L, n_up, x, V, diag_masks, flip_masks)
    ctx = capi.Context()
    S = _operator(capi, ctx, L, n_up)
    b = _state(capi, ctx, S, V, x)
    if large:
        b.tune(2, 1, 0)  # 256 workgroups: the tile loop goes round
    for first, count in ranges:
        got = b.spin_measure_columns(capi.VEC_W, first, count, diag_masks, flip_masks)
        cr.check(f"device ({L},{n_up}) columns {first}..{first + count - 1}", L, n_up, got, tuple(r[:, first : first + count] for r in ref))
        if not large:  # the duplicates are the same bits as their originals
            assert got[0][-1].tobytes() == got[0][L].tobytes() and got[1][len(mr.pairs(L))].tobytes() == got[1][0].tobytes()
    assert b.download(capi.VEC_W).tobytes() == x.tobytes() and b.download(capi.VEC_COL(ncol - 1)).tobytes() == V[ncol - 1].tobytes()
    for h in (b, S, ctx):
        h.close()


def test_term_counts_across_every_chunk_boundary(capi):
    """(32,2), 496 rows, five columns.  Each list takes 0, 1, 15, 16, 17 and 33 terms independently of the other, cut from one pool of
    33 masks each whose reference is computed once."""
    L, n_up = 32, 2
    pm = mr.pair_masks(L)
    pool_d = np.array(pm[:1] + mr.site_masks(L), np.uint32)
    pool_f = np.array(pm[:33], np.uint32)
    x, V = mr.vector(L, n_up), cr.columns(L, n_up, J + 1)
    ref = cr.measure(L, n_up, x, V, pool_d, pool_f)
    ctx = capi.Context()
    S = _operator(capi, ctx, L, n_up)
    b = _state(capi, ctx, S, V, x)
    fixed = set()
    for cd in (0, 1, 15, 16, 17, 33):
        for cf in (0, 1, 15, 16, 17, 33):
            got = b.spin_measure_columns(capi.VEC_W, 0, J + 1, pool_d[:cd], pool_f[:cf])
            assert got[0].shape == (cd, J + 1) and got[1].shape == (cf, J + 1)
            cr.check(f"(32,2) counts {cd}, {cf}", L, n_up, got, (ref[0][:cd], ref[1][:cf], ref[2][:cd], ref[3][:cf]))
            if cd:
                fixed.add(("diag", got[0][0].tobytes()))
            if cf:
                fixed.add(("flip", got[1][0].tobytes()))
    assert len(fixed) == 2  # term 0 of either pool: the same bits in every call
    for h in (b, S, ctx):
        h.close()


@pytest.mark.parametrize("L,n_up", [(9, None), (11, 5)])
def test_a_sum_does_not_depend_on_what_shares_its_call(capi, L, n_up):
    diag_masks, flip_masks = mr.term_lists(L, n_up)
    x, V = mr.vector(L, n_up), cr.columns(L, n_up, 12)
    ctx = capi.Context()
    S = _operator(capi, ctx, L, n_up)
    b = _state(capi, ctx, S, V)
    b.upload(capi.VEC_V, x)
    full = b.spin_measure_columns(capi.VEC_V, 0, 12, diag_masks, flip_masks)
    again = b.spin_measure_columns(capi.VEC_V, 0, 12, diag_masks, flip_masks)
    assert full[0].tobytes() == again[0].tobytes() and full[1].tobytes() == again[1].tobytes()
    td, tf = L + 17, 18  # a pair in the second chunk of either list
    for j in (0, 3, 4, 6, 11):
        alone = b.spin_measure_columns(capi.VEC_V, j, 1, diag_masks[td : td + 1], flip_masks[tf : tf + 1])
        assert alone[0][0, 0] == full[0][td, j] and alone[1][0, 0] == full[1][tf, j], j
    for first, count in ((1, 7), (5, 3), (6, 6), (2, 9)):  # column 6 in another place of another chunk
        part = b.spin_measure_columns(capi.VEC_V, first, count, diag_masks[3:40], flip_masks[5:30])
        assert part[0].tobytes() == full[0][3:40, first : first + count].tobytes()
        assert part[1].tobytes() == full[1][5:30, first : first + count].tobytes()
    # the duplicates, every column
    assert full[0][-1].tobytes() == full[0][L].tobytes() and full[1][len(mr.pairs(L))].tobytes() == full[1][0].tobytes()
    # the vector may be a basis column, inside the range or not; with the column itself the diagonal sums are the measurement's
    xc = b.spin_measure_columns(capi.VEC_COL(2), 0, 4, diag_masks, flip_masks)
    cr.check(f"({L},{n_up}) x = column 2", L, n_up, xc, cr.measure(L, n_up, V[2], V[:4], diag_masks, flip_masks))
    one = b.spin_measure(capi.VEC_COL(2), diag_masks, flip_masks)
    mr.check(f"({L},{n_up}) <x| A |x>", L, n_up, V[2], diag_masks, flip_masks, (xc[0][:, 2], xc[1][:, 2], one[2]))
    for h in (b, S, ctx):
        h.close()


@pytest.mark.parametrize("L,n_up", [(9, None), (10, 5)])
def test_cross_check_against_site_apply_and_dots(capi, L, n_up):
    """diag{i} / 2 = <V_j| Sz_i |x>: eigenex_spin_site_apply(Z, e_i) forms Sz_i x exactly (a sign and a halving per row) and eigenex_dots
    sums it against the same columns.  Each side is within n eps sum |terms| of the true value: the two bounds added."""
    n = mr.rows(L, n_up)
    x, V = mr.vector(L, n_up, seed=41 + L), cr.columns(L, n_up, 6)
    ctx = capi.Context()
    S = _operator(capi, ctx, L, n_up)
    b = _state(capi, ctx, S, V)
    b.upload(capi.VEC_V, x)
    diag, _ = b.spin_measure_columns(capi.VEC_V, 0, 6, mr.site_masks(L), [])
    mag = np.abs(V).astype(LD) @ np.abs(x).astype(LD)  # sum_s |V_j(s) x_s|, of diag; half of it for either side of diag / 2
    worst = 0.0
    for i in range(L):
        b.spin_site_apply(capi.VEC_V, b, capi.VEC_W, capi.SPIN_SITE_Z, np.eye(L)[i])
        dots = b.dots(capi.VEC_W, 0, 1, 6)
        err, bound = np.abs(diag[i].astype(LD) / 2 - dots.astype(LD)), 2 * n * mr.EPS * mag / 2
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (i, err, bound)
    print(f"({L},{n_up}) diag / 2 against site_apply + dots: largest difference / bound = {worst:.3e}")
    for h in (b, S, ctx):
        h.close()


STEPS, HALF = 20, 10


def _lanczos(capi, ranges):
    """20 step calls at (12,6) from a fixed start vector, in two batches of 10, with one call per (first, count) of `ranges` in
    between; alpha, beta, the counters, every column, both work vectors, whether a column was pending before and after the calls,
    and what they returned"""
    L, n_up, n = 12, 6, 924
    ctx = capi.Context()
    S = capi.Csr.spin_half_sector(ctx, L, n_up, sr.chain(L, periodic=True))
    b = capi.Basis(ctx, S, n, STEPS + 2)
    b.upload(capi.VEC_W, np.random.RandomState(5).standard_normal(n))
    b.lanczos_enqueue(HALF)
    pending, measured = [b.close_pending()], []
    for first, count in ranges:
        measured.append(b.spin_measure_columns(capi.VEC_COL(0), first, count, mr.site_masks(L) + mr.pair_masks(L), mr.pair_masks(L)))
        pending.append(b.close_pending())
    b.lanczos_enqueue(STEPS - HALF)
    st, alpha, beta = b.lanczos_state()
    out = dict(alpha=alpha, beta=beta, state=np.array([st.nvec, st.iterations, st.nalpha, st.nbeta, st.stopped, st.calls_true, b.repairs()]),
               V=np.stack([b.download(capi.VEC_COL(c)) for c in range(st.nvec)]), W=b.download(capi.VEC_W), v=b.download(capi.VEC_V))
    for h in (b, S, ctx):
        h.close()
    return out, pending, measured


def test_a_lanczos_run_does_not_notice_a_call_between_its_batches(capi):
    """The one-sweep step is on (the default of a real state on a device operator): the first batch leaves column 9 pending.  A
    call on columns 0..8 leaves it pending, a call whose range holds column 9 closes it first; either way alpha, beta, the
    counters, every column and both work vectors are the bytes of the run without a call, and columns 0..8 give the same bits
    in both calls.  What the closing call returned is then held against the restatement on the finished run's columns."""
    L = 12
    plain, p0, _ = _lanczos(capi, [])
    short, p1, m1 = _lanczos(capi, [(0, HALF - 1)])
    closing, p2, m2 = _lanczos(capi, [(0, HALF - 1), (0, HALF), (HALF - 1, 1)])
    assert p0 == [True], "the one-sweep step did not leave its newest column pending: this test does not test what it says"
    assert p1 == [True, True] and p2 == [True, True, False, False]
    assert plain["state"].tolist()[0] == STEPS and plain["V"].shape == (STEPS, 924)
    for key in ("alpha", "beta", "state", "V", "W", "v"):
        assert plain[key].tobytes() == short[key].tobytes(), key
        assert plain[key].tobytes() == closing[key].tobytes(), key + " (closing)"
    for k in (0, 1):
        assert m1[0][k].tobytes() == m2[0][k].tobytes() == m2[1][k][:, : HALF - 1].tobytes()
        assert m2[1][k][:, HALF - 1].tobytes() == m2[2][k][:, 0].tobytes()
    # against the closed columns of the finished run, on the host
    V = plain["V"]
    ref = cr.measure(L, 6, V[0], V[:HALF], mr.site_masks(L) + mr.pair_masks(L), mr.pair_masks(L))
    cr.check("(12,6) Lanczos columns 0..9", L, 6, m2[1], ref)


def test_refusals(capi):
    ctx = capi.Context()
    L, n_up, n = 6, 3, 20
    served = "eigenex_spin_upload and eigenex_spin_sector_upload"
    rowptr, col, val = capi.spin_sector_csr(L, n_up, sr.chain(L))
    A = capi.Csr.upload(ctx, n, rowptr, col, val, column_blocks=0)
    ba = capi.Basis(ctx, A, n, 2)
    with pytest.raises(capi.EigenexError, match="stored operator.*" + served):
        ba.spin_measure_columns(capi.VEC_COL(0), 0, 1, [1], [3])
    assert capi.lib().eigenex_spin_measure_columns(ba.h, 0, 0, 1, 0, None, 0, None, None, None) == -4  # EIGENEX_ERR_STATE
    bh = capi.Basis(ctx, None, n, 2)
    bh.set_host_operator(lambda v: v)
    with pytest.raises(capi.EigenexError, match="host callback.*" + served):
        bh.spin_measure_columns(capi.VEC_COL(0), 0, 1, [1], [3])
    M = capi.Csr.spin_half_momentum(ctx, L, n_up, 0, sr.chain(L, periodic=True))
    bm = capi.Basis(ctx, M, capi.spin_momentum_dim(L, n_up, 0), 2)
    with pytest.raises(capi.EigenexError, match="momentum-sector operator.*" + served):
        bm.spin_measure_columns(capi.VEC_COL(0), 0, 1, [1], [3])
    Z = _operator(capi, ctx, L, n_up, complex_states=True)
    bz = capi.Basis(ctx, Z, n, 2)
    with pytest.raises(capi.EigenexError, match="real states only.*" + served):
        bz.spin_measure_columns(capi.VEC_COL(0), 0, 1, [1], [3])
    S = _operator(capi, ctx, L, n_up)
    V = np.arange(1.0, 3 * n + 1).reshape(3, n)
    bs = _state(capi, ctx, S, V)
    for word, d, f in (("zero", [0], []), ("zero", [], [3, 0]), ("outside", [1 << 6], []), ("one or two", [], [7]), ("conserve total Sz", [], [4]),
                       ("n_diag", [1] * 1025, []), ("n_flip", [], [3] * 1025)):
        with pytest.raises(capi.EigenexError, match=word) as e:
            bs.spin_measure_columns(capi.VEC_COL(0), 0, 3, d, f)
        assert str(e.value).count("eigenex_spin_measure_columns: ") == 1
    for word, first, count in (("count must be at least 1", 0, 0), ("count must be at least 1", 1, -1), ("first must not be negative", -1, 2),
                               ("exceeds the number of columns", 0, 4), ("exceeds the number of columns", 3, 1), ("exceeds the number of columns", 2, 2 ** 31 - 1)):
        with pytest.raises(capi.EigenexError, match=word):
            bs.spin_measure_columns(capi.VEC_COL(0), first, count, [1], [3])
    up = np.array([3], np.uint32).ctypes.data_as(capi._up)
    assert capi.lib().eigenex_spin_measure_columns(bs.h, 0, 0, 3, 1, None, 0, None, None, None) == -1  # EIGENEX_ERR_ARG: a NULL list with a count
    assert capi.lib().eigenex_spin_measure_columns(bs.h, 0, 0, 3, 1, up, 0, None, None, None) == -1  # no output for a non-empty list
    with pytest.raises(capi.EigenexError, match="bad vector reference"):
        bs.spin_measure_columns(capi.VEC_COL(3), 0, 3, [1], [3])
    # empty lists are valid; integers are exact; nothing above changed a vector
    assert capi.lib().eigenex_spin_measure_columns(bs.h, 0, 0, 3, 0, None, 0, None, None, None) == 0
    d, f = bs.spin_measure_columns(capi.VEC_COL(0), 0, 3, [(1 << L) - 1], [])
    assert d.tolist() == [[-float(V[j] @ V[0]) for j in range(3)]] and f.shape == (0, 3)  # three of six sites down on every row
    for j in range(3):
        assert bs.download(capi.VEC_COL(j)).tobytes() == V[j].tobytes()
    for h in (bs, bz, bm, bh, ba, S, Z, M, A, ctx):
        h.close()
