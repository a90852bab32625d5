"""GPU tests of the row-coded operator encoding (csrc/row_codes.hpp, kernels.hip: k_spmv_rows): every result of a row-coded
operator equals the one of the same operator held as plain CSR (EIGENEX_NO_ROW_CODES, read per upload) bit for bit -- one
application (y, the partial dot), fused Lanczos steps (alpha, beta, the basis columns u), Arnoldi, thick restart,
exp(xH)v -- on one shard and on 2, 3 and 8 loopback shards with and without halo overlap; the device generator ends in the
same results as a host upload; encoding() reports what the uploads chose."""
import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1, "no GPU visible: the HIP path must fail loudly, not fall back"
    return capi, solver


def _pair(monkeypatch, make):
    """(row-coded, plain) copies of one operator: make() called without and with EIGENEX_NO_ROW_CODES."""
    monkeypatch.delenv("EIGENEX_NO_ROW_CODES", raising=False)
    coded = make()
    monkeypatch.setenv("EIGENEX_NO_ROW_CODES", "1")
    plain = make()
    monkeypatch.delenv("EIGENEX_NO_ROW_CODES", raising=False)
    assert coded.encoding() == "row_codes" and plain.encoding() == "plain"
    assert coded.layout() == "csr" and plain.layout() == "csr"
    return coded, plain


def _few_value_stencil(n, seed):
    """Offsets -37 .. 37 with explicit zeros, +0.0 and -0.0 among 5 values, rows that skip inner offsets; the outer offsets
    +-37 are always stored, so that every halo column of a loopback shard is read and the halo offsets stay constant (a
    halo column that no row reads has no slot, and the ones behind it move: more offsets than a record can name).  Every
    row stores its columns ascending."""
    rng = np.random.default_rng(seed)
    offs = np.array([-37, -5, -1, 0, 1, 2, 5, 37])
    pal = np.array([2.5, -1.0, 0.0, -0.0, 0.125])
    rowptr, col, val = [0], [], []
    for r in range(n):
        for d in offs:
            c = r + d
            if 0 <= c < n and (abs(d) == 37 or rng.random() < 0.8):
                col.append(c)
                val.append(pal[rng.integers(0, pal.size)])
        rowptr.append(len(col))
    return np.array(rowptr, np.int32), np.array(col, np.int32), np.array(val, np.float64)


def _apply(capi, ctx, A, N, x, shift):
    b = capi.Basis(ctx, A, N, 4)
    b.upload(capi.VEC_W, x)
    dot = b.apply(capi.VEC_W, capi.VEC_V, shift, want_dot=True)
    y = b.download(capi.VEC_V)
    b.close()
    return y, dot


@pytest.mark.parametrize("shards,overlap", [(1, False), (2, False), (2, True), (3, True), (8, False), (8, True)])
def test_apply_bitwise_against_plain(mods, monkeypatch, shards, overlap):
    capi, _ = mods
    ctx = capi.Context(loopback_shards=shards) if shards > 1 else capi.Context()
    if shards > 1:
        ctx.set_halo_overlap(overlap)
    rng = np.random.default_rng(shards)
    for rowptr, col, val in (cref.laplacian3d(11), _few_value_stencil(3001, shards)):
        N = rowptr.size - 1
        coded, plain = _pair(monkeypatch, lambda: capi.Csr.upload(ctx, N, rowptr, col, val))
        x = rng.standard_normal(N)
        for shift in (0.0, -0.75):
            yc, dc = _apply(capi, ctx, coded, N, x, shift)
            yp, dp = _apply(capi, ctx, plain, N, x, shift)
            np.testing.assert_array_equal(yc.view(np.uint64), yp.view(np.uint64))
            assert np.float64(dc).tobytes() == np.float64(dp).tobytes()
            if shift == 0.0:
                np.testing.assert_array_equal(yc, cref.csr_spmv(rowptr, col, val, x))
        coded.close(), plain.close()
    ctx.close()


@pytest.mark.parametrize("shards", [1, 2, 3, 8])
def test_lanczos_steps_bitwise_against_plain(mods, monkeypatch, shards):
    """fused Lanczos steps: alpha, beta and every basis column (the operator kernel's u output) equal bit for bit"""
    capi, solver = mods
    n, m = 12, 30
    N = n ** 3
    ctx = capi.Context(loopback_shards=shards) if shards > 1 else capi.Context()
    coded, plain = _pair(monkeypatch, lambda: capi.Csr.laplacian3d(ctx, n))
    init = solver.default_start_vector(N)
    out = []
    for A in (coded, plain):
        b = capi.Basis(ctx, A, N, m + 2)
        b.upload(capi.VEC_W, init)
        b.lanczos_enqueue(m + 1)
        st, alpha, beta = b.lanczos_state()
        V = np.stack([b.download(capi.VEC_COL(c)) for c in range(m + 1)])
        out.append((np.array(alpha), np.array(beta), V))
        b.close()
    for a, p in zip(out[0], out[1]):
        np.testing.assert_array_equal(a.view(np.uint64), p.view(np.uint64))
    coded.close(), plain.close()
    ctx.close()


def test_lanczos_128_bitwise_against_plain(mods, monkeypatch):
    """config 2 (128^3, device generator, m = 50): alpha, beta and the Ritz values bit for bit"""
    capi, solver = mods
    n, m = 128, 50
    N = n ** 3
    ctx = capi.Context()
    coded, plain = _pair(monkeypatch, lambda: capi.Csr.laplacian3d(ctx, n))
    init = solver.default_start_vector(N)
    res = []
    for A in (coded, plain):
        es = solver.LanczosEigenSolver()
        es.setDeviceOperator(A).set(minIterations=m, maxIterations=m, maxEigenvalues=5, initialVector=init)
        es.compute()
        r = es.results()
        res.append((np.array(r["alpha"]), np.array(r["beta"]), np.array(r["eigenvalues"])))
        es.close()
    for a, p in zip(res[0], res[1]):
        np.testing.assert_array_equal(a.view(np.uint64), p.view(np.uint64))
    coded.close(), plain.close()
    ctx.close()


def test_arnoldi_thick_restart_function_solver_bitwise(mods, monkeypatch):
    capi, solver = mods
    n = 14
    N = n ** 3
    ctx = capi.Context()
    rowptr, col, val = cref.laplacian3d(n)
    coded, plain = _pair(monkeypatch, lambda: capi.Csr.upload(ctx, N, rowptr, col, val))
    init = solver.default_start_vector(N)
    got = []
    for A in (coded, plain):
        r = {}
        es = solver.ArnoldiEigenSolver()
        es.setDeviceOperator(A).set(minIterations=25, maxIterations=25, maxEigenvalues=4, initialVector=init)
        es.compute()
        r["arnoldi"] = np.asarray(es.results()["eigenvalues"])
        es.close()
        es = solver.ThickRestartLanczosEigenSolver()
        es.setDeviceOperator(A).set(numberOfEigenvalues=4, maxBasisSize=24, tolerance=1e-8, initialVector=init)
        es.compute()
        tr = es.results()
        r["thick"] = np.asarray(tr["eigenvalues"])
        r["thick_vec"] = np.asarray(tr["eigenvectors"])
        es.close()
        es = solver.LanczosEigenSolver()
        es.setDeviceOperator(A).set(minIterations=20, maxIterations=20, initialVector=init)
        r["exp"] = np.asarray(es.expWithLanczos(0.1, N))
        es.close()
        got.append(r)
    for k in got[0]:
        a, p = np.ascontiguousarray(got[0][k]), np.ascontiguousarray(got[1][k])
        assert a.tobytes() == p.tobytes(), k
    coded.close(), plain.close()
    ctx.close()


@pytest.mark.parametrize("shards", [1, 2, 3])
def test_generator_equals_host_upload(mods, shards):
    capi, _ = mods
    n = 24
    N = n ** 3
    ctx = capi.Context(loopback_shards=shards) if shards > 1 else capi.Context()
    rowptr, col, val = cref.laplacian3d(n)
    G = capi.Csr.laplacian3d(ctx, n)
    H = capi.Csr.upload(ctx, N, rowptr, col, val)
    assert G.encoding() == H.encoding() == "row_codes"
    x = np.random.default_rng(5).standard_normal(N)
    yg, dg = _apply(capi, ctx, G, N, x, 0.25)
    yh, dh = _apply(capi, ctx, H, N, x, 0.25)
    np.testing.assert_array_equal(yg.view(np.uint64), yh.view(np.uint64))
    assert np.float64(dg).tobytes() == np.float64(dh).tobytes()
    G.close(), H.close()
    ctx.close()


def test_encoding_of_the_baseline_configs(mods):
    """configs 2 and 4 (7-point Laplacian 128^3 / 256^3 from the generator, also a 256^3 shard of two) are row-coded; an
    operator with more offsets than a record can name or a column-blocked / complex one stays plain"""
    capi, _ = mods
    ctx = capi.Context()
    for n in (128, 256):
        A = capi.Csr.laplacian3d(ctx, n)
        assert A.encoding() == "row_codes" and A.layout() == "csr"
        A.close()
    ctx.close()
    ctx = capi.Context(loopback_shards=2)
    A = capi.Csr.laplacian3d(ctx, 256)
    assert A.encoding() == "row_codes"
    A.close()
    ctx.close()
    ctx = capi.Context()
    n = 400  # 17 offsets: plain
    rowptr = np.arange(0, 17 * n + 1, 17, dtype=np.int32)
    col = np.array([(r + d) % n for r in range(n) for d in sorted(range(0, 17 * 23, 23), key=lambda d: (r + d) % n)], np.int32)
    A = capi.Csr.upload(ctx, n, rowptr, col, np.ones(col.size))
    assert A.encoding() == "plain"
    A.close()
    rowptr, col, val = cref.laplacian3d(8)
    A = capi.Csr.upload(ctx, 512, rowptr, col, val, column_blocks=2)
    assert A.encoding() == "plain"
    A.close()
    ctx.close()
