"""The spin measurement on the device (eigenex_spin_measure, kernels.hip: k_spin_measure and k_spin_measure_reduce) against the
long double restatement of tests/spin_measure_reference.py, within |out - ref| <= n eps sum_s |term_s| -- the rounding of an
n-term sum in any grouping, so it holds for every launch grid.  Shapes, full space: L = 3 (8 rows), 6 (a ragged tile), 8 (one
tile), 9 (a top-bit pair crosses tiles), 17 with one workgroup per CU (512 tiles: the tile loop goes round); sectors: (4,2),
(6,0) and (6,6) (one row), (10,5), (11,5) (pairs across the split of the rank tables), (31,2), (32,2), (32,31) (bits 30 and 31),
(20,10) with one workgroup per CU (722 tiles).  The two large shapes take a shorter term list that still spans three chunks of
16 terms.  Then: every chunk boundary of the term lists at (32,2), determinism, the cross-check against eigenex_apply on
single-bond operators, a Lanczos run that does not notice a measurement between its batches, the ground state of the 12-ring
end to end, the refusals, and the C++ class."""
import json
import os
import subprocess
import sys
from math import comb

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_measure_reference as mr  # noqa: E402
import spin_reference as sr  # noqa: E402
from tests import spin_measure_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
SHAPES = [(3, None), (6, None), (8, None), (9, None), (17, None), (4, 2), (6, 0), (6, 6), (10, 5), (11, 5), (31, 2), (32, 2), (32, 31), (20, 10)]
LARGE = ((17, None), (20, 10))
E0_HEIS12 = -5.387390917445  # the periodic 12-site Heisenberg ring


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


def _operator(capi, ctx, L, n_up, bonds=None):
    bonds = sr.chain(L, 1.0, 0.7, periodic=True) if bonds is None else bonds
    return capi.Csr.spin_half(ctx, L, bonds) if n_up is None else capi.Csr.spin_half_sector(ctx, L, n_up, bonds)


def _short_lists(L, n_up):
    """every site, the pairs with the top site, a low and a middle pair, the string, the all-sites mask, a duplicate: 36 and 36
    (19 in a sector) terms at L = 17, three chunks"""
    full_d, full_f = mr.term_lists(L, n_up)
    top = [(1 << i) | (1 << (L - 1)) for i in range(L - 1)] + [0b11, (1 << (L // 2 - 1)) | (1 << (L // 2))]
    diag = mr.site_masks(L) + top + [int(m) for m in full_d[-3:]]
    flip = top + [top[0]] + (mr.site_masks(L) if n_up is None else [])
    return np.array(diag, np.uint32), np.array(flip, np.uint32)


@pytest.mark.parametrize("L,n_up", SHAPES)
def test_device_sums_equal_the_restatement_within_the_bound(mods, L, n_up):
    capi, _ = mods
    ctx = capi.Context()
    S = _operator(capi, ctx, L, n_up)
    n = mr.rows(L, n_up)
    assert S.spin_geometry() == (L, n_up) and S.info()["n_global"] == n
    b = capi.Basis(ctx, S, n, 2)
    if (L, n_up) in LARGE:
        b.tune(2, 1, 0)  # 256 workgroups: the tile loop goes round
    diag_masks, flip_masks = _short_lists(L, n_up) if (L, n_up) in LARGE else mr.term_lists(L, n_up)
    x = mr.vector(L, n_up)
    b.upload(capi.VEC_COL(1), x)
    got = b.spin_measure(capi.VEC_COL(1), diag_masks, flip_masks)
    mr.check(f"device ({L},{n_up})", L, n_up, x, diag_masks, flip_masks, got)
    assert b.download(capi.VEC_COL(1)).tobytes() == x.tobytes()
    # against the host definition too: the same sums in another grouping, so twice the bound at most (the test above is the
    # one that decides); and the duplicates are the same bits as their originals
    host = capi.spin_measure_host(L, n_up, x, diag_masks, flip_masks)
    assert abs(got[2] - host[2]) <= 2 * n * mr.EPS * host[2]
    if (L, n_up) not in LARGE:
        assert got[0][-1] == got[0][L] and got[1][len(mr.pairs(L))] == got[1][0]
    for h in (b, S, ctx):
        h.close()


@pytest.mark.parametrize("L,n_up,per_cu", cases.BITS_SHAPES)
def test_measurement_bits_equal_the_parent_build(mods, L, n_up, per_cu):
    """norm2, diag and flip of one measurement are the bytes tests/golden/spin_measure_bits_parent.npz holds, recorded by
    scripts/record_spin_measure_bits.py from the build before the kernels took their row walk from csrc/spin_rows.hpp: the
    bound of the test above would not notice an fma that became a multiply and an add.  (9, full), (10,5) and (32,2) have at
    most one tile per workgroup, so their partial sums, and with them the fixture, are the same on every device.  (17, full) runs
    512 tiles on one workgroup per CU: which tiles a workgroup adds up depends on the CU count, so that shape holds only on a
    device with as many CUs as the recording one, which the test asserts first."""
    capi, _ = mods
    with np.load(os.path.join(ROOT, "tests", "golden", "spin_measure_bits_parent.npz")) as z:
        golden = {k: z[k] for k in z.files}
    if per_cu:
        import torch

        cus, cus_rec = int(torch.cuda.get_device_properties(0).multi_processor_count), int(golden["cus"])
        assert cus == cus_rec, f"this device has {cus} CUs, the fixture was recorded on {cus_rec}: the grid fixes the partial sums of this shape"
    got = cases.measure_bits(capi, L, n_up, per_cu)
    diag_masks, flip_masks = cases.bits_lists(L, n_up)
    assert got["diag"].size == 8 * diag_masks.size and got["flip"].size == 8 * flip_masks.size and got["norm2"].size == 8
    for k in ("norm2", "diag", "flip"):
        assert got[k].tobytes() == golden[cases.bits_key(L, n_up) + "/" + k].tobytes(), (L, n_up, k)


COUNTS = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 496 + 32]


def test_term_counts_across_every_chunk_boundary(mods):
    """(32,2), 496 rows.  Both lists take each count in turn, cut from one pool of 528 masks each whose reference is computed once.
    Term 0 of the pools is in every non-empty call, first or last in the list, with different neighbours: its result is the same
    bits every time.  Two identical calls give identical bytes."""
    capi, _ = mods
    L, n_up = 32, 2
    n = comb(L, n_up)
    pm = mr.pair_masks(L)
    pool_d = np.array(pm[:1] + mr.site_masks(L) + pm[1:], np.uint32)
    pool_f = np.array(pm + pm[:32], np.uint32)  # duplicates are allowed
    assert pool_d.size == pool_f.size == 528
    x = mr.vector(L, n_up)
    ref = mr.measure(L, n_up, x, pool_d, pool_f)
    ctx = capi.Context()
    S = _operator(capi, ctx, L, n_up)
    b = capi.Basis(ctx, S, n, 1)
    b.upload(capi.VEC_COL(0), x)
    fixed = set()
    for cd in COUNTS:
        for cf in (COUNTS if cd in (0, 16, 528) else (0, 17, cd)):
            got = b.spin_measure(capi.VEC_COL(0), pool_d[:cd], pool_f[:cf])
            assert got[0].size == cd and got[1].size == cf
            sub = (ref[0][:cd], ref[1][:cf], ref[2], ref[3][:cd], ref[4][:cf], ref[5])
            mr.check(f"(32,2) counts {cd}, {cf}", L, n_up, x, pool_d[:cd], pool_f[:cf], got, ref=sub)
            fixed.add(("norm2", float(got[2]).hex()))
            if cd:
                fixed.add(("diag", float(got[0][0]).hex()))
            if cf:
                fixed.add(("flip", float(got[1][0]).hex()))
            if cd > 1 and cf > 1:  # the fixed terms last instead of first
                rev = b.spin_measure(capi.VEC_COL(0), pool_d[:cd][::-1].copy(), pool_f[:cf][::-1].copy())
                assert rev[0].tobytes() == got[0][::-1].tobytes() and rev[1].tobytes() == got[1][::-1].tobytes() and rev[2] == got[2]
    assert len(fixed) == 3, fixed
    one = b.spin_measure(capi.VEC_COL(0), pool_d, pool_f)
    two = b.spin_measure(capi.VEC_COL(0), pool_d, pool_f)
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes() and one[2] == two[2]
    # the maximum of 1024 terms per list
    big = b.spin_measure(capi.VEC_COL(0), np.resize(pool_d, 1024), np.resize(pool_f, 1024))
    assert big[0][:528].tobytes() == one[0].tobytes() and big[0][528:].tobytes() == one[0][:496].tobytes() and big[1][528:].tobytes() == one[1][:496].tobytes()
    assert b.download(capi.VEC_COL(0)).tobytes() == x.tobytes()
    for h in (b, S, ctx):
        h.close()


@pytest.mark.parametrize("L,n_up", [(9, None), (10, 5)])
def test_cross_check_against_apply_on_single_bond_operators(mods, L, n_up):
    """flip{i,j} / 2 = x . H x for H = one bond with Jxy = 1, Jz = 0, and diag{i,j} / 4 for Jz = 1, Jxy = 0.  H x is exact there (one
    product with 1/2 or 1/4 per row), so the dot of eigenex_apply carries the rounding of its n-term sum alone: each side within
    n eps sum |terms| of the true value, the two bounds added."""
    capi, _ = mods
    n = mr.rows(L, n_up)
    x = mr.vector(L, n_up, seed=31 + L)
    ctx = capi.Context()
    S = _operator(capi, ctx, L, n_up)
    b = capi.Basis(ctx, S, n, 1)
    b.upload(capi.VEC_COL(0), x)
    five = [(0, 1), (0, L - 1), (L // 2 - 1, L // 2), (2, L - 2), (L - 2, L - 1)]
    masks = [(1 << i) | (1 << j) for (i, j) in five]
    diag, flip, norm2 = b.spin_measure(capi.VEC_COL(0), masks, masks)
    ref = mr.measure(L, n_up, x, masks, masks)
    for k, (i, j) in enumerate(five):
        for which, (jz, jxy), mine, mag in (("zz", (1.0, 0.0), diag[k] / 4, ref[3][k] / 4), ("xy", (0.0, 1.0), flip[k] / 2, ref[4][k] / 2)):
            B = _operator(capi, ctx, L, n_up, [(i, j, jz, jxy)])
            bb = capi.Basis(ctx, B, n, 1)
            bb.upload(capi.VEC_COL(0), x)
            dot = bb.apply(capi.VEC_COL(0), capi.VEC_V, 0.0, want_dot=True)
            bound = 2 * n * mr.EPS * mag
            print(f"({L},{n_up}) pair ({i},{j}) {which}: measure {mine!r}, apply {dot!r}, difference {abs(mine - dot):.3e}, bound {float(bound):.3e}")
            assert abs(LD(mine) - LD(dot)) <= bound
            bb.close()
            B.close()
    for h in (b, S, ctx):
        h.close()


def test_a_lanczos_run_does_not_notice_a_measurement(mods, tmp_path):
    """20 step calls at (12,6): in one batch; in two batches of 10 with a measurement of column 3 in between; the latter with
    EIGENEX_NO_GRAPHS=1 in a child process.  alpha, beta, the counters, every column and both work vectors are identical bytes,
    and the measurement itself is the same bits with and without recorded step batches."""
    capi, _ = mods
    whole, cut = cases.run(capi, False), cases.run(capi, True)
    out = str(tmp_path / "no_graphs.npz")
    env = dict(os.environ, EIGENEX_NO_GRAPHS="1")
    r = subprocess.run([sys.executable, "-m", "tests.spin_measure_cases", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    with np.load(out) as z:
        child = {k: z[k] for k in z.files}
    assert whole["state"].tolist()[0] == cases.STEPS and whole["V"].shape == (cases.STEPS, cases.ROWS)
    for key in ("alpha", "beta", "state", "V", "W", "v"):
        assert whole[key].tobytes() == cut[key].tobytes(), key
        assert whole[key].tobytes() == child[key].tobytes(), key + " (no graphs)"
    for key in ("diag", "flip", "norm2"):
        assert cut[key].tobytes() == child[key].tobytes(), key
    # column 3 is a unit vector of the sector Sz = 0
    assert abs(cut["norm2"][0] - 1.0) < 1e-12 and abs(cut["diag"][: cases.L].sum()) < 1e-12


def test_ground_state_of_the_ring_end_to_end(mods):
    """LanczosEigenSolver on the sector (12,6) of the Heisenberg ring (120 steps: the ground vector is converged far below the
    margin), the vector uploaded and measured: <S^2> = 0 and every nearest-neighbour <S_i.S_j> = E0 / 12, within 1e-6."""
    capi, solver = mods
    L, n_up, n = 12, 6, 924
    ctx = capi.Context()
    S = _operator(capi, ctx, L, n_up, sr.chain(L, periodic=True))
    es = solver.LanczosEigenSolver()
    es.setDeviceOperator(S).set(minIterations=120, maxIterations=120, maxEigenvalues=1, initialVector=solver.random_vector(1, n))
    es.compute()
    r = es.results()
    E0, x = r["eigenvalues"][0], np.ascontiguousarray(r["eigenvectors"][:, 0])
    assert abs(E0 - E0_HEIS12) < 1e-9
    b = capi.Basis(ctx, S, n, 1)
    b.upload(capi.VEC_COL(0), x)
    d, f, n2 = b.spin_measure(capi.VEC_COL(0), mr.site_masks(L) + mr.pair_masks(L), mr.pair_masks(L))
    sz, zz, xy, dot = mr.correlations(L, d[:L], d[L:], f, n2)
    s2 = mr.total_spin_squared(dot)
    nn = np.array([dot[i, (i + 1) % L] for i in range(L)], LD)
    print(f"E0 = {E0:.13f}, <S^2> = {float(s2):.3e}, nearest-neighbour <S.S> in [{float(nn.min()):.12f}, {float(nn.max()):.12f}], E0/12 = {E0 / 12:.12f}")
    assert abs(s2) < 1e-6
    assert np.abs(nn - E0 / 12).max() < 1e-6 and float(nn.max() - nn.min()) < 1e-6
    assert np.abs(sz).max() < 1e-6  # a singlet has no magnetisation anywhere
    for h in (b, es, S, ctx):
        h.close()


def test_refusals(mods):
    capi, _ = mods
    ctx = capi.Context()
    L, n_up, n = 6, 3, 20
    rowptr, col, val = capi.spin_sector_csr(L, n_up, sr.chain(L))
    A = capi.Csr.upload(ctx, n, rowptr, col, val, column_blocks=0)
    ba = capi.Basis(ctx, A, n, 1)
    ba.upload(capi.VEC_COL(0), np.ones(n))
    with pytest.raises(capi.EigenexError, match="not a matrix-free spin operator"):
        ba.spin_measure(capi.VEC_COL(0), [1], [3])
    assert capi.lib().eigenex_spin_measure(ba.h, 0, 0, None, 0, None, None, None, None) == -4  # EIGENEX_ERR_STATE
    with pytest.raises(capi.EigenexError, match="not a matrix-free spin operator"):
        A.spin_geometry()
    bh = capi.Basis(ctx, None, n, 1)
    bh.set_host_operator(lambda v: v)
    with pytest.raises(capi.EigenexError, match="host callback"):
        bh.spin_measure(capi.VEC_COL(0), [1], [3])
    assert capi.lib().eigenex_spin_measure(bh.h, 0, 0, None, 0, None, None, None, None) == -4
    S = _operator(capi, ctx, L, n_up)
    F = _operator(capi, ctx, L, None)
    bs, bf = capi.Basis(ctx, S, n, 2), capi.Basis(ctx, F, 1 << L, 2)
    x = np.arange(1.0, n + 1)
    bs.upload(capi.VEC_COL(0), x)
    bf.upload(capi.VEC_COL(0), np.ones(1 << L))
    for word, d, f in (("zero", [0], []), ("zero", [], [3, 0]), ("outside", [1 << 6], []), ("outside", [], [(1 << 6) | 1]), ("one or two", [], [7]),
                       ("conserve total Sz", [], [4]), ("n_diag", [1] * 1025, []), ("n_flip", [], [3] * 1025)):
        with pytest.raises(capi.EigenexError, match=word) as e:
            bs.spin_measure(capi.VEC_COL(0), d, f)
        assert str(e.value).count("eigenex_spin_measure: ") == 1
    up = np.array([3], np.uint32).ctypes.data_as(capi._up)
    assert capi.lib().eigenex_spin_measure(bs.h, 0, 1, None, 0, None, None, None, None) == -1  # EIGENEX_ERR_ARG: a NULL list with a count
    assert capi.lib().eigenex_spin_measure(bs.h, 0, 1, up, 0, None, None, None, None) == -1  # no output for a non-empty list
    with pytest.raises(capi.EigenexError, match="bad vector reference"):
        bs.spin_measure(capi.VEC_COL(2), [1], [3])
    # a one-bit flip is a measurement in the full space; every output may be absent; nothing above changed the vector
    assert bf.spin_measure(capi.VEC_COL(0), [], [4])[1][0] == float(1 << L)
    assert capi.lib().eigenex_spin_measure(bs.h, 0, 0, None, 0, None, None, None, None) == 0
    assert bs.spin_measure(capi.VEC_COL(0), [], [])[2] == float(x @ x)  # integers: exact
    bs.upload(capi.VEC_W, x)  # any vector reference will do
    assert bs.spin_measure(capi.VEC_W, [3], [3]) == bs.spin_measure(capi.VEC_COL(0), [3], [3])
    assert bs.download(capi.VEC_COL(0)).tobytes() == x.tobytes()
    for h in (bs, bf, ba, bh, S, F, A, ctx):
        h.close()


def test_cpp_program_spin_correlations(tmp_path):
    """tests/cpp/spin_correlations_amd.cpp: SpinCorrelationSolver in a C++11 user program, built with -Wall -Wextra.  The
    eigenvectors come from a Lanczos solver converged to 1e-13 in the eigenvalue: <S^2> is exact to second order in the vector's
    error, the single bonds to first order (about 1e-6), hence the two margins."""
    exe = str(tmp_path / "spin_correlations_amd")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "spin_correlations_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    o = json.loads(subprocess.check_output([exe, "12"]).decode())
    print(o)
    assert o["sites"] == 12 and [s["n_up"] for s in o["sectors"]] == [6, 5] and [s["rows"] for s in o["sectors"]] == [924, 792]
    for s, s2 in zip(o["sectors"], (0.0, 2.0)):
        assert s["info"] == 1 and s["sites_seen"] == 12 and s["n_up_seen"] == s["n_up"] and s["symmetric"] == 1
        assert abs(s["s2"] - s2) < 1e-6
        assert abs(s["norm2"] - 9.0) < 1e-9  # the state went in scaled by 3
        assert s["diagonal_error"] == 0.0
        assert abs(s["sum_sz"] - (s["n_up"] - 6)) < 1e-12
        assert abs(s["sf0"] - s["sf0_expected"]) < 1e-12 and s["sf0_expected"] == (s["n_up"] - 6) ** 2 / 12
    assert abs(o["sectors"][0]["energy"] - E0_HEIS12) < 1e-9 and o["sectors"][0]["bond_spread"] < 1e-5
    assert o["sectors"][0]["sf_pi"] > 0.5  # antiferromagnetic correlations: the singlet's structure factor peaks at pi, where it is about 0.9
    assert o["sectors"][1]["energy"] > o["sectors"][0]["energy"] + 1e-3
    assert (o["refused_csr"], o["refused_zero"], o["refused_length"], o["refused_no_operator"], o["no_result_throws"]) == (1, 1, 1, 1, 1)
    assert o["uniform_info"] == 1 and abs(o["uniform_sum_sz"]) < 1e-12
