"""The reduced density matrix on the host: eigenex_spin_rdm_host against the long double restatement of
tests/spin_rdm_reference.py within the rounding bound of an n_b-term sum, the layout against math.comb, cross-checks against
eigenex_spin_measure_host on one and two sites, physics with known answers (the singlet, product states, S(A) = S(complement)),
every refusal of the argument check by its message, and the host code (csrc/spin_rdm.hpp) together with a replay of the kernels'
work table, panels and padding under AddressSanitizer + UBSan in a stand-alone program.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
from math import comb, log

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_rdm_reference as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
# (n_sites, n_up or None, mask_a): the host-sized shapes of tests/test_gpu_spin_rdm.py
SHAPES = [
    (3, None, 0b010),
    (6, None, 0b000111),
    (6, None, 0b101010),
    (10, None, 0b0000111111),
    (10, None, 0b1011011101),
    (4, 2, 0b0011),
    (6, 0, 0b000101),
    (6, 6, 0b000101),
    (10, 5, 0b0001111000),
    (11, 5, 0b10100100011),
    (12, 6, 0b111111100000),
    (32, 2, 0xC0000FFF),
    (32, 31, 0x80000005),
    (14, 7, 0x0FFF),
]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g

    g.build()
    from cmpt_eigenex_amd import capi as c

    return c


@pytest.mark.parametrize("L,n_up,mask", SHAPES)
def test_host_blocks_equal_the_restatement_within_the_bound(capi, L, n_up, mask):
    x = rr.vector(L, n_up)
    got = capi.spin_rdm_host(L, n_up, x, mask)
    rr.check(f"host ({L},{n_up},{mask:#x})", got, rr.rdm(L, n_up, x, mask))
    n = rr.rows(L, n_up)
    trace = sum(float(np.trace(m)) for _, m in got)
    assert abs(trace - float(x @ x)) <= 2 * n * rr.EPS * float(x @ x)


@pytest.mark.parametrize("L,n_up,mask", SHAPES + [(28, 14, 0x3FFF), (28, 14, 0xFFFC000), (30, None, 0xFFF), (32, 16, 0x80000001), (24, 12, 0xFFF000)])
def test_layout_against_comb(capi, L, n_up, mask):
    kf, dims, offs = capi.spin_rdm_layout(L, n_up, mask)
    nA = bin(mask).count("1")
    nB = L - nA
    if n_up is None:
        assert (kf, dims) == (0, [2 ** nA])
    else:
        kmin, kmax = max(0, n_up - nB), min(nA, n_up)
        assert kf == kmin and dims == [comb(nA, k) for k in range(kmin, kmax + 1)]
        # every state of the sector lies in exactly one block
        assert sum(comb(nA, k) * comb(nB, n_up - k) for k in range(kmin, kmax + 1)) == comb(L, n_up)
    assert offs[0] == 0 and [offs[i + 1] - offs[i] for i in range(len(dims))] == [d * d for d in dims] and max(dims) <= 4096


@pytest.mark.parametrize("L,n_up", [(6, None), (9, None), (6, 3), (11, 5), (32, 2)])
def test_cross_checks_against_spin_measure_host(capi, L, n_up):
    """One site i: rho[1,1] - rho[0,0] = diag{i} and tr rho = norm2.  Two sites i < j: 2 rho[01,10] = flip{i,j} (the word 01 has
    site i up, 10 site j).  Each side is an n-term sum of the same products in another grouping: within n eps sum |terms| of
    the true value each, the two bounds added; sum |terms| is norm2 for the diagonal, at most norm2 / 2 for one off-diagonal
    entry (|x y| <= (x^2 + y^2) / 2 over disjoint rows)."""
    x = rr.vector(L, n_up, seed=7 + L)
    n = rr.rows(L, n_up)
    sites = [0, L // 2, L - 1]
    pairs = [(0, 1), (0, L - 1), (L // 2 - 1, L // 2)]
    diag, flip, norm2 = capi.spin_measure_host(L, n_up, x, [1 << i for i in sites], [(1 << i) | (1 << j) for i, j in pairs])
    bound = 2 * n * rr.EPS * norm2
    for t, i in enumerate(sites):
        blocks = dict(capi.spin_rdm_host(L, n_up, x, 1 << i))
        if n_up is None:
            down, up = blocks[0][0, 0], blocks[0][1, 1]
        else:  # block k = 0: the site is down, block k = 1: up; both are 1 x 1
            down, up = blocks[0][0, 0], blocks[1][0, 0]
        assert abs(LD(up) - LD(down) - LD(diag[t])) <= bound and abs(LD(up) + LD(down) - LD(norm2)) <= bound
    for t, (i, j) in enumerate(pairs):
        blocks = dict(capi.spin_rdm_host(L, n_up, x, (1 << i) | (1 << j)))
        off = blocks[0][1, 2] if n_up is None else blocks[1][0, 1]  # words 01 and 10: one site up
        assert off == (blocks[0][2, 1] if n_up is None else blocks[1][1, 0])
        assert abs(2 * LD(off) - LD(flip[t])) <= bound


def test_physics_with_known_answers(capi):
    # the two-site singlet inside four sites, (|ud> - |du>)(|ud> - |du>): S = ln 2 for one site of a singlet, 0 for a whole singlet
    pair = np.array([0.0, 1.0, -1.0, 0.0])
    x = np.kron(pair, pair)  # sites (0,1) and (2,3)
    for mask, want in ((0b0001, log(2)), (0b0011, 0.0), (0b0101, 2 * log(2)), (0b0111, log(2))):
        lam = rr.spectrum(capi.spin_rdm_host(4, None, x, mask))
        assert abs(rr.entropy(lam) - want) < 1e-15 * 16, (mask, lam)
    blocks = dict(capi.spin_rdm_host(2, 1, [1.0, -1.0], 1))
    assert blocks[0].tolist() == [[1.0]] and blocks[1].tolist() == [[1.0]]  # exact: the spectrum is (1/2, 1/2), S = ln 2
    assert abs(rr.entropy(rr.spectrum(list(blocks.items()))) - log(2)) < 1e-15
    assert capi.spin_rdm_host(2, None, [0.0, 1.0, -1.0, 0.0], 2)[0][1].tolist() == [[1.0, 0.0], [0.0, 1.0]]
    # a product state: one nonzero block entry, S = 0 and Schmidt rank 1, in the full space and in its sector
    L, s = 7, 0b1011001
    for n_up in (None, 4):
        xs = np.zeros(rr.rows(L, n_up))
        xs[s if n_up is None else int(np.searchsorted(rr.words(L, 4), s))] = -1.5
        for mask in (0b0000111, 0b1010101, 0b1000000):
            got = capi.spin_rdm_host(L, n_up, xs, mask)
            lam = rr.spectrum(got)
            assert sum(int(np.count_nonzero(m)) for _, m in got) == 1 and sum(float(m.sum()) for _, m in got) == 2.25
            assert lam[0] == 1.0 and int((lam > 0).sum()) == 1 and rr.entropy(lam) == 0.0
    # a product of two random vectors over A and B: Schmidt rank 1 whatever the vectors
    a, b = np.random.RandomState(3).standard_normal(8), np.random.RandomState(4).standard_normal(16)
    lam = rr.spectrum(capi.spin_rdm_host(7, None, np.kron(b, a), 0b0000111))  # the low three sites carry a
    assert abs(lam[0] - 1.0) < 1e-14 and np.all(lam[1:] < 1e-14)


def test_entropy_of_a_subsystem_equals_that_of_its_complement(capi):
    """a random vector at (12,6), nA = 5 against nB = 7: the two reduced density matrices share their nonzero spectrum.  The
    tolerance is the derived one of tests/spin_rdm_reference.py for either side (32 eigenvalues from sums of at most C(7,3) = 35
    terms; 126 eigenvalues from sums of at most C(5,2) = 10 terms), added."""
    L, n_up, A = 12, 6, 0b000110010101
    x = rr.vector(L, n_up, seed=99)
    sa = rr.entropy(rr.spectrum(capi.spin_rdm_host(L, n_up, x, A)))
    sb = rr.entropy(rr.spectrum(capi.spin_rdm_host(L, n_up, x, 0xFFF & ~A)))
    tol = rr.entropy_tolerance(32, 35) + rr.entropy_tolerance(126, 10)
    print(f"S(A) = {sa:.15f}, S(B) = {sb:.15f}, difference {abs(sa - sb):.3e}, tolerance {tol:.3e}")
    assert abs(sa - sb) <= tol and sa > 1.0


def _raw(capi, n_sites, n_up, mask, out_len=None, x=True, out=True):
    dp = C.POINTER(C.c_double)
    xv, o = np.ones(1 << 16), np.full(1 << 16, -7.0)
    rc = capi.lib().eigenex_spin_rdm_host(n_sites, n_up, xv.ctypes.data_as(dp) if x else None, mask, o.ctypes.data_as(dp) if out else None,
                                         0 if out_len is None else out_len)
    return rc, capi.lib().eigenex_last_error().decode(), bool(np.all(o == -7.0))


def test_every_refusal_returns_a_code_and_a_message(capi):
    assert _raw(capi, 6, -1, 0b000111, 64)[0] == 0 and _raw(capi, 6, 3, 0b000111, 20)[0] == 0
    cases = [
        ("zero", (6, -1, 0)),
        ("zero", (6, 3, 0)),
        ("outside", (6, -1, 1 << 6)),
        ("outside", (6, 3, (1 << 6) | 1)),
        ("outside", (31, 2, 1 << 31)),
        ("leaves no site out", (6, -1, 63)),
        ("leaves no site out", (6, 3, 63)),
        ("n_sites", (31, -1, 1)),
        ("n_sites", (33, 2, 1)),
        ("n_sites", (1, -1, 1)),
        ("n_up", (6, 7, 1)),
        ("n_up", (6, -2, 1)),
        ("4096", (14, -1, 0x1FFF)),
        ("4096", (16, 8, 0x7FFF)),
        ("4096", (30, 15, 0x3FFFFFF)),
    ]
    for word, args in cases:
        rc, msg, untouched = _raw(capi, *args)
        assert rc == -1 and word in msg and msg.startswith("eigenex_spin_rdm_host: ") and untouched, (word, args, msg)
        with pytest.raises(capi.EigenexError, match=word) as e:
            capi.spin_rdm_layout(args[0], None if args[1] == -1 else args[1], args[2])
        assert str(e.value).count("eigenex_spin_rdm_layout: ") == 1
    for wrong in (63, 65, 0, -1):
        rc, msg, untouched = _raw(capi, 6, -1, 0b000111, wrong)
        assert rc == -1 and "out_len" in msg and untouched
    rc, msg, untouched = _raw(capi, 6, -1, 0b000111, 64, x=False)
    assert rc == -1 and "NULL" in msg and untouched
    rc, msg, _ = _raw(capi, 6, -1, 0b000111, 64, out=False)
    assert rc == -1 and "NULL" in msg
    with pytest.raises(capi.EigenexError, match="one entry per row"):
        capi.spin_rdm_host(6, 3, np.ones(19), 7)
    # the limits themselves are allowed: 12 sites in the full space, 14 in a sector, bit 31 of 32 sites; outputs of the layout
    # may be absent
    assert capi.spin_rdm_layout(14, None, 0xFFF)[1] == [4096] and max(capi.spin_rdm_layout(28, 14, 0x3FFF)[1]) == 3432
    assert capi.spin_rdm_layout(32, 2, 1 << 31)[1] == [1, 1]
    assert capi.lib().eigenex_spin_rdm_layout(6, 3, 7, None, None, None, None) == 0


def test_exports_are_declared_and_present(capi):
    text = open(os.path.join(ROOT, "include", "eigenex_hip.h")).read()
    for name in ("eigenex_spin_rdm", "eigenex_spin_rdm_host", "eigenex_spin_rdm_layout"):
        assert re.search(r"\bint %s\s*\(" % name, text)
        assert hasattr(capi.lib(), name) and name in capi.SIGNATURES
    from cmpt_eigenex_amd import solver

    for name in ("create", "destroy", "set_device_operator", "set_state", "set_subsystem", "set_subsystem_mask", "compute", "sizes", "block", "get", "renyi",
                 "schmidt_rank", "log_line"):
        assert hasattr(solver.lib(), "eigenex_spin_entanglement_solver_" + name)
    assert hasattr(solver, "SpinEntanglementSolver")


def test_rdm_host_code_under_sanitizers(tmp_path):
    """csrc/spin_rdm.hpp (argument check, layout, work table, host evaluation) compiled into a stand-alone program with
    AddressSanitizer + UBSan: outputs into exactly-sized arrays, and the work items of k_spin_rdm and k_spin_rdm_reduce replayed
    over the shapes of the GPU tests on three launch grids -- the kernel's own index functions (csrc/spin_rdm_rows.hpp, compiled
    into the program) with every access bounds-checked -- equal to the host evaluation within the bound."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "spin_rdm_sanitize")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "spin_rdm_sanitize.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-1500:], out.stderr.decode()[-2000:])
    assert b"SPIN RDM OK" in out.stdout
