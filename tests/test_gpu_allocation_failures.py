"""Error paths of every allocating entry point: each device / pinned-host allocation the library makes goes through one
function with two test hooks (include/eigenex_hip.h: eigenex_debug_allocations, eigenex_debug_fail_allocation).  For each
entry point a clean call first counts the allocations N it makes; then for k = 1..N the k-th allocation is made to fail,
and the call must report EIGENEX_ERR_HIP naming that allocation and hold exactly the buffers it held before (nothing
leaked, nothing freed).  Once everything is closed the library holds no buffer.

A failed eigenex_basis_reserve leaves the state as it was: on 2 loopback shards a failure among shard 1's new arrays
keeps the capacity, and a later reserve and more Arnoldi steps give H, the residue and the basis bit for bit as a run
that never failed (shard 0 must not keep a new H laid out for the new capacity)."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAILED = r"eigenex error -2: .*\.alloc\(.*: out of memory"


@pytest.fixture(scope="module")
def capi():
    from cmpt_eigenex_amd import capi as m

    assert m.device_count() >= 1
    return m


@pytest.fixture(scope="module")
def cref():
    from oracle import cref as m

    return m


@pytest.fixture(autouse=True)
def nothing_left(capi):
    gc.collect()
    assert held(capi) == (0, 0)
    yield
    capi.lib().eigenex_debug_fail_allocation(0)
    gc.collect()
    assert held(capi) == (0, 0)


def counts(capi):
    v = [C.c_int64() for _ in range(3)]
    assert capi.lib().eigenex_debug_allocations(*[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


def held(capi):
    return counts(capi)[:2]


def every_failure(capi, setup, call, teardown=lambda state, out: None):
    """setup() -> state; call(state) -> what the call made; teardown(state, made or None) closes both.  Returns N."""
    L = capi.lib()
    state = setup()
    made0 = counts(capi)[2]
    out = call(state)
    n = counts(capi)[2] - made0
    teardown(state, out)
    assert n > 0
    for k in range(1, n + 1):
        state = setup()
        before = held(capi)
        L.eigenex_debug_fail_allocation(k)
        try:
            with pytest.raises(capi.EigenexError, match=FAILED):
                call(state)
        finally:
            L.eigenex_debug_fail_allocation(0)
        assert held(capi) == before, k
        teardown(state, None)
    return n


def close(*objs):
    for o in objs:
        if o is not None:
            o.close()


def ctx_for(capi, shards):
    return capi.Context(loopback_shards=shards) if shards > 1 else capi.Context()


def random_csr(rng, n, max_per_row):
    counts_ = rng.integers(0, max_per_row + 1, n)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(counts_, out=rowptr[1:])
    col = np.concatenate([np.sort(rng.choice(n, c, replace=False)) for c in counts_]).astype(np.int32)
    return rowptr.astype(np.int32), col, rng.uniform(-1, 1, col.size)


def upload_failures(capi, shards, make):
    ctx = ctx_for(capi, shards)
    every_failure(capi, lambda: None, lambda _: make(ctx), lambda _, A: close(A))
    ctx.close()


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("row_codes", [True, False])
def test_upload(capi, cref, monkeypatch, shards, row_codes):
    if not row_codes:
        monkeypatch.setenv("EIGENEX_NO_ROW_CODES", "1")
    rowptr, col, val = cref.laplacian3d(9)
    upload_failures(capi, shards, lambda ctx: capi.Csr.upload(ctx, 729, rowptr, col, val))


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("column_blocks", [2, -3])
def test_upload_column_blocked_and_split(capi, shards, column_blocks):
    n = 9_001
    rowptr, col, val = random_csr(np.random.default_rng(5), n, 30)

    def make(ctx):
        A = capi.Csr.upload(ctx, n, rowptr, col, val, column_blocks=column_blocks)
        if column_blocks == -3:
            assert A.layout() == "split_tiles"
        return A

    upload_failures(capi, shards, make)


@pytest.mark.parametrize("wide", [False, True])
def test_upload64(capi, cref, monkeypatch, wide):
    if wide:
        monkeypatch.setenv("EIGENEX_FORCE_WIDE_ROWPTR", "1")
    rowptr, col, val = cref.laplacian3d(9)
    upload_failures(capi, 2, lambda ctx: capi.Csr.upload64(ctx, 729, rowptr.astype(np.int64), col, val))


def test_upload_complex_and_from_device(capi):
    import torch

    n = 3000
    rowptr, col, val = random_csr(np.random.default_rng(6), n, 9)
    z = val + 1j * np.random.default_rng(7).uniform(-1, 1, val.size)
    upload_failures(capi, 2, lambda ctx: capi.Csr.upload(ctx, n, rowptr, col, z))
    dev = torch.device("cuda", 0)
    t_rp, t_col, t_val = (torch.from_numpy(a).to(dev) for a in (rowptr, col, val))
    upload_failures(capi, 1, lambda ctx: capi.Csr.from_device(ctx, n, t_rp.data_ptr(), t_col.data_ptr(), t_val.data_ptr()))


@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_upload_blocks(capi, dtype):
    rng = np.random.default_rng(8)
    sizes = [8, 12, 10]
    blocks = {}
    for key in ((0, 0), (0, 1), (1, 1), (2, 0), (2, 2)):
        blocks[key] = rng.standard_normal((sizes[key[0]], sizes[key[1]])).astype(dtype)
    upload_failures(capi, 2, lambda ctx: capi.Csr.upload_blocks(ctx, sizes, sizes, blocks))


@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("wide", [False, True])
def test_laplacian3d(capi, monkeypatch, shards, wide):
    if wide:
        monkeypatch.setenv("EIGENEX_FORCE_WIDE_ROWPTR", "1")

    def make(ctx):
        A = capi.Csr.laplacian3d(ctx, 12)
        assert A.encoding() == ("plain" if wide else "row_codes")
        return A

    upload_failures(capi, shards, make)


@pytest.mark.parametrize("operator", ["device", "host"])
def test_basis(capi, operator):
    ctx = capi.Context()
    A = capi.Csr.laplacian3d(ctx, 10) if operator == "device" else None
    every_failure(capi, lambda: None, lambda _: capi.Basis(ctx, A, 1000, 6, 2), lambda _, b: close(b))
    close(A, ctx)


def arnoldi_state(capi, shards, cap=8, steps=5):
    ctx = ctx_for(capi, shards)
    A = capi.Csr.laplacian3d(ctx, 10)
    b = capi.Basis(ctx, A, 1000, cap)
    b.upload(capi.VEC_W, np.random.default_rng(9).standard_normal(1000))
    b.arnoldi_enqueue(steps)
    return ctx, A, b


def test_clone_and_reserve(capi):
    def clone(state):
        h = C.c_void_p()
        capi._chk(capi.lib().eigenex_basis_clone(state[2].h, C.byref(h)))
        return h

    def drop(state, h):
        if h is not None:
            capi.lib().eigenex_basis_destroy(h)
        close(state[2], state[1], state[0])

    every_failure(capi, lambda: arnoldi_state(capi, 2), clone, drop)
    every_failure(capi, lambda: arnoldi_state(capi, 2), lambda s: s[2].reserve(16), drop)


def test_lanczos_restart(capi):
    m, keep = 10, 4

    def setup():
        ctx = capi.Context(loopback_shards=2)
        A = capi.Csr.laplacian3d(ctx, 10)
        b = capi.Basis(ctx, A, 1000, m + 1 + keep)
        b.upload(capi.VEC_W, np.random.default_rng(10).standard_normal(1000))
        b.lanczos_enqueue(m + 1)
        return ctx, A, b

    S = np.linalg.qr(np.random.default_rng(11).standard_normal((m, keep)))[0]
    every_failure(capi, setup, lambda s: s[2].lanczos_restart(S, 0.5), lambda s, _: close(s[2], s[1], s[0]))


@pytest.mark.parametrize("kind", ["ritz", "ritz_complex", "combine"])
def test_ritz_vectors(capi, kind):
    rng = np.random.default_rng(12)
    S = rng.standard_normal((6, 3))
    if kind == "ritz_complex":
        S = S + 1j * rng.standard_normal((6, 3))
    call = (lambda s: s[2].krylov_combine(6, S)) if kind == "combine" else (lambda s: s[2].ritz_vectors(6, S))

    def setup():
        state = arnoldi_state(capi, 2)
        call(state)  # the Ritz scratch of every shard is allocated on first use and kept by the basis
        return state

    every_failure(capi, setup, call, lambda s, _: close(s[2], s[1], s[0]))


@pytest.mark.parametrize("shards", [1, 2])
def test_failed_reserve_keeps_the_state(capi, shards):
    def run(fail_at):
        ctx, A, b = arnoldi_state(capi, shards)
        if fail_at:
            capi.lib().eigenex_debug_fail_allocation(fail_at)
            try:
                with pytest.raises(capi.EigenexError, match=FAILED):
                    b.reserve(16)
            finally:
                capi.lib().eigenex_debug_fail_allocation(0)
            cap = C.c_int()
            capi._chk(capi.lib().eigenex_basis_capacity(b.h, C.byref(cap)))
            assert cap.value == 8
        b.reserve(16)
        b.arnoldi_enqueue(8)
        st, H = b.arnoldi_state()
        V = np.stack([b.download(capi.VEC_COL(c)) for c in range(st.nvec)])
        out = (st.nvec, st.residue, H, V)
        close(b, A, ctx)
        return out

    ref = run(0)
    assert ref[0] == 13  # 5 + 8 calls: the first one only normalises the start vector
    # six new arrays per shard (V, partials, hbuf, alpha, beta, H): the last shard's first and last
    for fail_at in (6 * shards - 5, 6 * shards):
        got = run(fail_at)
        assert got[:2] == ref[:2]
        np.testing.assert_array_equal(got[2], ref[2])
        np.testing.assert_array_equal(got[3], ref[3])
