"""The reduced density matrix of a complex vector on the host: eigenex_spin_rdm_host_z against the long double restatement of
tests/spin_rdm_z_reference.py within the rounding bound of a 2 n_b-term sum, on every shape of tests/test_gpu_spin_rdm.py; the
two properties of the definition (the diagonal's imaginary part is +0.0, (j, i) is the conjugate of (i, j) bit for bit); the real
case against eigenex_spin_rdm_host; a global phase; the refusals; small_eigen::hermitian through a stand-alone C++ program; and
the host code together with a replay of k_spin_rdm<..., SpinZ>'s work table, panels and padding under AddressSanitizer + UBSan in a
stand-alone program.  No GPU."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_evolution_reference as er  # noqa: E402
import spin_rdm_reference as rr  # noqa: E402
import spin_rdm_z_reference as rz  # noqa: E402
from test_gpu_spin_rdm import SHAPES as GPU_SHAPES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
SHAPES = [(L, n_up, mask) for L, n_up, mask, _ in GPU_SHAPES]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g

    g.build()
    from cmpt_eigenex_amd import capi as c

    return c


@pytest.fixture(scope="module")
def references():
    """the restatement of every shape, computed once: (x, rdm_z) by shape"""
    out = {}
    for L, n_up, mask in SHAPES:
        x = er.vector_z(L, n_up)
        out[(L, n_up, mask)] = (x, rz.rdm_z(L, n_up, x, mask))
    return out


@pytest.mark.parametrize("L,n_up,mask", SHAPES)
def test_host_blocks_equal_the_restatement_within_the_bound(capi, references, L, n_up, mask):
    x, ref = references[(L, n_up, mask)]
    got = capi.spin_rdm_host_z(L, n_up, x, mask)
    rz.check_z(f"host_z ({L},{n_up},{mask:#x})", got, ref)  # the bound, Im of the diagonal +0.0, (j, i) = conj((i, j)) bit for bit
    rz.trace_check(got, x, rr.rows(L, n_up))
    kf, dims, _ = capi.spin_rdm_layout(L, n_up, mask)
    assert [k for k, _ in got] == [kf + i for i in range(len(dims))] and [m.shape[0] for _, m in got] == dims


@pytest.mark.parametrize("L,n_up,mask", [s for s in SHAPES if s[0] <= 14])
def test_a_real_vector_gives_the_real_definition(capi, L, n_up, mask):
    """x = a + 0i: every product with an imaginary part is +-0 and leaves its fma chain unchanged, so the real part is the real
    definition's chain, equal as numbers, and the imaginary part is zero everywhere"""
    a = rr.vector(L, n_up)
    real = capi.spin_rdm_host(L, n_up, a, mask)
    cplx = capi.spin_rdm_host_z(L, n_up, a.astype(np.complex128), mask)
    for (k, r), (kz, z) in zip(real, cplx):
        assert k == kz and np.array_equal(z.real, r) and not z.imag.any()


@pytest.mark.parametrize("L,n_up,mask", [(6, None, 0b101010), (10, 5, 0b0001111000), (12, 6, 0b111111100000)])
def test_a_global_phase_stays_within_the_bound(capi, references, L, n_up, mask):
    """rho of exp(i phi) x is rho of x.  The result is within the bound of the rotated vector y's own restatement, and against the
    restatement of x within that bound plus the rounding of y itself: y_s = fl(fl(exp(i phi)) x_s) is within 3 eps |x_s| of
    exp(i phi) x_s (one eps for the rounded phase, sqrt(2) eps and a little for the complex product), so an entry of rho moves by at
    most sum_b (|dy_i| |y_j| + |y_i| |dy_j|) <= 7 eps (A A^T)[i, j] with A = |M| the moduli."""
    x, ref = references[(L, n_up, mask)]
    y = np.exp(0.7j) * x
    got = capi.spin_rdm_host_z(L, n_up, y, mask)
    own = rz.rdm_z(L, n_up, y, mask)
    rz.check_z(f"host_z rotated ({L},{n_up},{mask:#x})", got, own)
    moduli = rr.panels(L, n_up, np.abs(x), mask)
    for (_, g), (_, re_, im_, _, _), (_, _, _, bre, bim), (_, A) in zip(got, ref, own, moduli):
        slack = 7 * rr.EPS * (A @ A.T)
        assert np.all(np.abs(g.real.astype(LD) - re_) <= bre + slack) and np.all(np.abs(g.imag.astype(LD) - im_) <= bim + slack)


def _raw(capi, n_sites, n_up, mask, out_len=None, x=True, out=True):
    dp = C.POINTER(C.c_double)
    xv, o = np.ones(1 << 17), np.full(1 << 17, -7.0)
    rc = capi.lib().eigenex_spin_rdm_host_z(n_sites, n_up, xv.ctypes.data_as(dp) if x else None, mask, o.ctypes.data_as(dp) if out else None,
                                           0 if out_len is None else out_len)
    return rc, capi.lib().eigenex_last_error().decode(), bool(np.all(o == -7.0))


def test_every_refusal_returns_a_code_and_a_message(capi):
    assert _raw(capi, 6, -1, 0b000111, 128)[0] == 0 and _raw(capi, 6, 3, 0b000111, 40)[0] == 0
    cases = [("zero", (6, -1, 0)), ("zero", (6, 3, 0)), ("outside", (6, -1, 1 << 6)), ("outside", (31, 2, 1 << 31)), ("leaves no site out", (6, -1, 63)),
             ("leaves no site out", (6, 3, 63)), ("n_sites", (31, -1, 1)), ("n_sites", (33, 2, 1)), ("n_up", (6, 7, 1)), ("4096", (14, -1, 0x1FFF)),
             ("4096", (16, 8, 0x7FFF))]
    for word, args in cases:
        rc, msg, untouched = _raw(capi, *args)
        assert rc == -1 and word in msg and msg.startswith("eigenex_spin_rdm_host_z: ") and untouched, (word, args, msg)
    for wrong in (64, 127, 129, 0, -1):  # 64 is the real call's length
        rc, msg, untouched = _raw(capi, 6, -1, 0b000111, wrong)
        assert rc == -1 and "out_len" in msg and untouched
    rc, msg, untouched = _raw(capi, 6, -1, 0b000111, 128, x=False)
    assert rc == -1 and "NULL" in msg and untouched
    rc, msg, _ = _raw(capi, 6, -1, 0b000111, 128, out=False)
    assert rc == -1 and "NULL" in msg
    with pytest.raises(capi.EigenexError, match="one entry per row"):
        capi.spin_rdm_host_z(6, 3, np.ones(19, np.complex128), 7)


def test_exports_are_declared_and_present(capi):
    text = open(os.path.join(ROOT, "include", "eigenex_hip.h")).read()
    for name in ("eigenex_spin_rdm_z", "eigenex_spin_rdm_host_z"):
        assert re.search(r"\bint %s\s*\(" % name, text)
        assert hasattr(capi.lib(), name) and name in capi.SIGNATURES
    from cmpt_eigenex_amd import solver

    for name in ("set_state_z", "block_z"):
        assert hasattr(solver.lib(), "eigenex_spin_entanglement_solver_" + name)
    assert hasattr(solver.lib(), "eigenex_spin_evolution_solver_entanglement")
    for name in ("entanglementEntropy", "entanglementSpectrum", "entanglementRenyi2"):
        assert hasattr(solver.SpinTimeEvolutionSolver, name)
    assert hasattr(capi.Basis, "spin_rdm_z")


def test_small_eigen_hermitian(tmp_path):
    """small_eigen::hermitian goes through the real symmetric embedding of order 2n (Householder tridiagonalisation and QL, backward
    stable: a computed eigenpair of the embedding has a residual of at most c (2n) eps ||A|| with a constant c of order 10) and
    normalises an accepted complex vector that kept at least 1 / (4n) of its squared norm, which amplifies by at most 2 sqrt(n);
    over n columns (Frobenius norm: sqrt(n)) that is ||A V - V Lambda||_F <= 10 (2n) (2 sqrt(n)) sqrt(n) eps ||A||_F = 40 n^2 eps
    ||A||_F, and the same for ||V^H V - I||_F (two passes of Gram-Schmidt leave eps-level overlaps, amplified alike).  An eigenvalue
    is off by at most the backward error, 10 (2n) eps ||A||."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "small_eigen_hermitian")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "small_eigen_hermitian.cpp"), "-o", exe])
    rows = {o["name"]: o for o in map(json.loads, subprocess.check_output([exe]).decode().splitlines())}
    assert set(rows) == {"random7", "degenerate_pair7", "degenerate_triple7", "one", "two"}
    eps = float(rr.EPS)
    for name, o in rows.items():
        n = o["n"]
        print(name, o["residual"], o["orthogonality"], 40 * n * n * eps)
        assert o["ok"] == 1 and o["values_alone_equal"] == 1
        assert o["residual"] <= 40 * n * n * eps and o["orthogonality"] <= 40 * n * n * eps
        assert list(o["values"]) == sorted(o["values"])
    for name, want in (("degenerate_pair7", [-1.5, -0.25, 0.5, 0.5, 1.0, 2.0, 3.5]), ("degenerate_triple7", [0.0, 0.0, 0.0, 0.125, 0.25, 0.25, 0.375]),
                       ("one", [0.75]), ("two", [-1.0, 3.0])):
        norm = float(np.linalg.norm(want))
        assert np.abs(np.array(rows[name]["values"]) - np.array(want)).max() <= 20 * len(want) * eps * norm + 40 * len(want) ** 2 * eps * norm


def test_rdm_z_host_code_under_sanitizers(tmp_path):
    """csrc/spin_rdm.hpp (spin_rdm_host_z and the work table) compiled into a stand-alone program with AddressSanitizer + UBSan:
    outputs into exactly-sized arrays, and the work items of k_spin_rdm<..., SpinZ> and k_spin_rdm_reduce<SpinZ> replayed over the shapes of the
    GPU tests on three launch grids -- the kernel's own index functions (csrc/spin_rdm_rows.hpp, compiled into the program) with
    every access bounds-checked -- equal to the host evaluation within twice the bound."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "spin_rdm_z_sanitize")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "spin_rdm_z_sanitize.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, (out.stdout.decode()[-1500:], out.stderr.decode()[-2000:])
    assert b"SPIN RDM Z OK" in out.stdout
