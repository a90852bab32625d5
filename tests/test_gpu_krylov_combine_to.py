"""eigenex_krylov_combine_to: a combination of basis columns left on the device.  Plain CSR, n = 1000, real and complex states,
nvec in {1, 7, 9, 17} (one pass of the combination kernel, and across its 8- and 16-column steps): the device result has the bytes
of eigenex_krylov_combine's host result for the same coefficients, in W, in V and in a free column; the columns that are read stay
as they were; a bad destination is refused.  After a one-sweep batch that leaves its newest column pending, the call writes that
column first: the result equals that of a fresh child process running with EIGENEX_EAGER_CLOSE=1."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import one_sweep_reference as osr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1000
NVECS = (1, 7, 9, 17)


@pytest.fixture(scope="module")
def capi():
    from cmpt_eigenex_amd import capi as c

    assert c.device_count() >= 1
    return c


def _state(capi, ctx, A, cplx, cap):
    b = capi.Basis(ctx, A, N, cap)
    rng = np.random.default_rng(100 + int(cplx))
    cols = rng.standard_normal((cap, N)) + (1j * rng.standard_normal((cap, N)) if cplx else 0.0)
    for c in range(cap):
        b.upload(capi.VEC_COL(c), cols[c])
    return b, cols


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("nvec", NVECS)
def test_device_result_has_the_bytes_of_the_host_result(capi, nvec, cplx):
    ctx = capi.Context()
    rowptr, col, val = osr.tridiagonal_csr(N)
    A = capi.Csr.upload(ctx, N, rowptr, col, val.astype(np.complex128) if cplx else val, column_blocks=0)
    cap = nvec + 2
    b, cols = _state(capi, ctx, A, cplx, cap)
    rng = np.random.default_rng(nvec)
    kinds = [rng.standard_normal(nvec)] + ([rng.standard_normal(nvec) + 1j * rng.standard_normal(nvec)] if cplx else [])
    for coef in kinds:
        host = b.krylov_combine(nvec, coef.reshape(-1, 1))[:, 0]
        assert host.dtype == b.dtype
        ref = cols[:nvec].T @ coef
        assert np.abs(host - ref).max() <= 4 * nvec * np.finfo(float).eps * (np.abs(cols[:nvec]).T @ np.abs(coef)).max()
        for dst in (capi.VEC_W, capi.VEC_V, capi.VEC_COL(nvec), capi.VEC_COL(cap - 1)):
            b.krylov_combine_to(nvec, coef, dst)
            assert b.download(dst).tobytes() == host.tobytes(), (nvec, cplx, dst)
        for c in range(nvec):  # what is read is left alone
            assert b.download(capi.VEC_COL(c)).tobytes() == cols[c].astype(b.dtype).tobytes()
        for c in (nvec, cap - 1):  # put the destinations back for the next kind
            b.upload(capi.VEC_COL(c), cols[c])
    for h in (b, A, ctx):
        h.close()


def test_bad_arguments_are_refused(capi):
    ctx = capi.Context()
    A = capi.Csr.upload(ctx, N, *osr.tridiagonal_csr(N), column_blocks=0)
    b, cols = _state(capi, ctx, A, False, 6)
    coef = np.ones(4)
    for dst in (capi.VEC_COL(0), capi.VEC_COL(3), capi.VEC_COL(6), capi.VEC_START, -40):
        with pytest.raises(capi.EigenexError, match="eigenex_krylov_combine_to: dst"):
            b.krylov_combine_to(4, coef, dst)
    for nvec in (0, 7):
        with pytest.raises(capi.EigenexError, match="eigenex_krylov_combine_to"):
            b.krylov_combine_to(nvec, np.ones(8), capi.VEC_W)
    with pytest.raises(capi.EigenexError, match="complex coefficients need a complex state"):
        b.krylov_combine_to(4, coef + 1j, capi.VEC_W)
    for c in range(6):  # nothing was written
        assert b.download(capi.VEC_COL(c)).tobytes() == cols[c].tobytes()
    b.close()
    A.close()
    ctx.close()
    lb = capi.Context(loopback_shards=2)
    A2 = capi.Csr.upload(lb, N, *osr.tridiagonal_csr(N))
    b2 = capi.Basis(lb, A2, N, 6)
    with pytest.raises(capi.EigenexError, match="one shard"):
        b2.krylov_combine_to(4, coef, capi.VEC_W)
    for h in (b2, A2, lb):
        h.close()


def test_pending_close_is_honoured(capi, tmp_path):
    from tests import combine_to_case as case

    mine = case.run()
    out = str(tmp_path / "eager.npz")
    env = dict(os.environ, EIGENEX_EAGER_CLOSE="1")
    env.pop("EIGENEX_TWO_SWEEPS", None)
    subprocess.run([sys.executable, "-m", "tests.combine_to_case", out], cwd=ROOT, env=env, check=True, timeout=300)
    eager = np.load(out)
    for name in ("w", "v", "col"):
        assert bool(mine["pending_" + name]) and not bool(eager["pending_" + name])  # the case is what it claims to be
        assert not bool(mine["after_" + name])
        assert mine[name].tobytes() == eager[name].tobytes() == mine["host_" + name].tobytes() == eager["host_" + name].tobytes()
        assert np.abs(mine[name]).max() > 0
