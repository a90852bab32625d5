"""Site operators between momentum sectors on the host (csrc/spin_momentum_site.hpp, eigenex_spin_momentum_site_apply_host): the
expand identity against eigenex_spin_site_apply_host_z, which pins sign, phase and ratio independently of the header's derivation;
the host function against the longdouble restatement tests/spin_momentum_site_reference.py at 32-bit and 64-bit shapes; the
real-coefficient identity, adjointness, the refusals with their messages, and the host code together with the kernel's row walk
under AddressSanitizer + UBSan in a stand-alone program, which also holds the two state words against each other.  No GPU.

Bound of a row (or of an element of the Sz sector) with T terms: (T + 6) eps sum|terms|, the sum taken from the reference -- at
most four roundings per term on either side plus the accumulation."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_momentum_site_reference as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
KINDS = (ref.Z, ref.PLUS, ref.MINUS)
SHAPES32 = [(8, 4, 1), (12, 6, 1), (12, 5, 2), (16, 8, 1)]
SHAPES64 = [(36, 3, 1), (36, 4, 1), (48, 3, 1), (36, 4, 2)]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g

    g.build()
    from cmpt_eigenex_amd import capi as c

    return c


def momenta(L, cell):
    """every (m, p) with m in {0, 1, N/2} and p in {0, 1, N/2, N - 1}"""
    N = L // cell
    return [(m, p) for m in sorted({0, 1, N // 2}) for p in sorted({0, 1, N // 2, N - 1})]


def cases(L, n_up, cell):
    """(m, p, kind, rows of the source, rows of the destination) of every kind whose two sectors exist"""
    for m, p in momenta(L, cell):
        for kind in KINDS:
            up2, m2 = ref.destination(L, n_up, cell, m, kind, p)
            n_src, n_dst = ref.rows(L, n_up, cell, m)[0].size, ref.rows(L, up2, cell, m2)[0].size
            if n_src and n_dst:
                yield m, p, kind, n_src, n_dst


def is_real(L, cell, m, p):
    N = L // cell
    return all(q == 0 or 2 * q == N for q in (m, (m - p) % N))


def vectors(rng, n, real):
    """a random complex vector and, where the real form applies, a real one"""
    out = [rng.standard_normal(n) + 1j * rng.standard_normal(n)]
    if real:
        out.append(rng.standard_normal(n))
    return out


def cell_coefficients(rng, cell, real):
    out = [rng.standard_normal(cell) + 1j * rng.standard_normal(cell)]
    if real:
        out.append(rng.standard_normal(cell))
    return out


def to_double(v):
    return np.asarray(v).astype(np.complex128)


# ---- 1. the expand identity ----
@pytest.mark.parametrize("L,n_up,cell", SHAPES32)
def test_expand_of_the_result_is_the_site_operator_on_the_expanded_vector(capi, L, n_up, cell):
    rng = np.random.default_rng(L * 100 + n_up * 10 + cell)
    seen, worst = set(), 0.0
    for m, p, kind, n_src, n_dst in cases(L, n_up, cell):
        up2, m2 = ref.destination(L, n_up, cell, m, kind, p)
        real = is_real(L, cell, m, p)
        for cc in cell_coefficients(rng, cell, real):
            c = to_double(ref.site_coefficients(L, cell, p, cc))  # the per-site coefficients, rounded to double
            for x in vectors(rng, n_src, real and not np.iscomplexobj(cc)):
                y, _ = capi.spin_momentum_site_apply_host(L, n_up, m, kind, cc, p, x, cell)
                assert y.dtype == x.dtype and y.size == n_dst
                lhs = capi.spin_momentum_expand_host(L, up2, m2, y, cell)
                psi = capi.spin_momentum_expand_host(L, n_up, m, x, cell)
                rhs, _ = capi.spin_site_apply_host_z(L, n_up, kind, c, psi.astype(np.complex128))
                _, terms, moduli = ref.apply_sites_in_sector(L, n_up, kind, c, ref.expand(L, n_up, cell, m, x))
                bound = (terms + 6) * EPS * moduli.astype(np.float64)
                err = np.abs(lhs - rhs)
                assert np.all(err <= bound), (m, p, kind, float((err - bound).max()))
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                seen.add(kind)
    assert seen == set(KINDS)
    print("expand identity, largest error / bound:", worst)


def test_the_eight_site_ring_has_every_period_and_rows_of_one_sector_only(capi):
    """what the shape (8, 4, 1) is there for, and that the reference's rows are the library's; the library then maps a row that
    exists at k = 0 only to zero under Z with p = 0 -> 1"""
    for m in (0, 1, 4):
        states, periods = capi.spin_momentum64_states(8, 4, m)
        assert np.array_equal(states, ref.rows(8, 4, 1, m)[0]) and np.array_equal(periods, ref.rows(8, 4, 1, m)[1])
    y, _ = capi.spin_momentum_site_apply_host(8, 4, 1, ref.Z, [1.0], 1, np.ones(8, np.complex128))  # from k = 1 (8 rows) to k = 0 (10)
    only0 = ~np.isin(ref.rows(8, 4, 1, 0)[0], ref.rows(8, 4, 1, 1)[0])
    assert only0.size == y.size == 10 and only0.sum() == 2 and np.all(y[only0] == 0) and np.any(y[~only0] != 0)
    reps0, per0 = ref.rows(8, 4, 1, 0)
    assert sorted(set(per0.tolist())) == [2, 4, 8]
    assert sorted(set(ref.rows(8, 8, 1, 0)[1].tolist()) | set(per0.tolist())) == [1, 2, 4, 8]
    reps1, _ = ref.rows(8, 4, 1, 1)
    assert set(reps1.tolist()) < set(reps0.tolist())  # rows present at k = 0 and absent at k = 1


# ---- 2. the host function against the reference ----
@pytest.mark.parametrize("L,n_up,cell", SHAPES32 + SHAPES64)
def test_host_function_equals_the_longdouble_reference(capi, L, n_up, cell):
    rng = np.random.default_rng(L * 1000 + n_up * 10 + cell)
    seen = set()
    for m, p, kind, n_src, n_dst in cases(L, n_up, cell):
        real = is_real(L, cell, m, p)
        for cc in cell_coefficients(rng, cell, real):
            for x in vectors(rng, n_src, real and not np.iscomplexobj(cc)):
                y, norm2 = capi.spin_momentum_site_apply_host(L, n_up, m, kind, cc, p, x, cell)
                want, terms, moduli = ref.apply(L, n_up, cell, m, kind, cc, p, x)
                bound = (terms + 6) * EPS * moduli.astype(np.float64)
                err = np.abs(y - to_double(want))
                assert np.all(err <= bound), (m, p, kind, float((err - bound).max()))
                # norm2: n eps norm2 for the sum itself, and 2 |y_b| times the bound of y_b, |y_b| <= moduli_b, for what it sums
                n2 = float(np.sum(np.abs(want) ** 2))
                assert abs(norm2 - n2) <= (n_dst + 2 * (terms.max() + 6)) * EPS * max(n2, float(np.sum(moduli ** 2)))
                seen.add((kind, x.dtype.kind))
    assert {k for k, _ in seen} == set(KINDS) and {t for _, t in seen} == {"c", "f"}


def test_bit_47_is_a_site(capi):
    """(48, 3, 1): site 47 is down in every representative of the destination, so every row of S- flips bit 47 up"""
    L, n_up = 48, 3
    n_src = ref.rows(L, n_up, 1, 0)[0].size
    x = np.random.default_rng(5).standard_normal(n_src)
    y, _ = capi.spin_momentum_site_apply_host(L, n_up, 0, ref.MINUS, [1.0], 0, x)
    want, terms, moduli = ref.apply(L, n_up, 1, 0, ref.MINUS, [1.0], 0, x)
    assert terms.min() == L - (n_up - 1) and not np.any((ref.rows(L, n_up - 1, 1, 0)[0] >> np.uint64(47)) & np.uint64(1))
    assert np.all(np.abs(y - to_double(want).real) <= (terms + 6) * EPS * moduli.astype(np.float64))


# ---- 3. real coefficients ----
@pytest.mark.parametrize("L,n_up,cell", [(8, 4, 1), (12, 5, 2), (36, 3, 1)])
def test_real_coefficients_act_on_each_part(capi, L, n_up, cell):
    rng = np.random.default_rng(77 + L)
    seen = set()
    for m, p, kind, n_src, n_dst in cases(L, n_up, cell):
        if not is_real(L, cell, m, p):
            continue
        cc = rng.standard_normal(cell)
        x = rng.standard_normal(n_src) + 1j * rng.standard_normal(n_src)
        for imaginary in (False, True):  # NULL, and zeros handed over
            y, norm2 = capi.spin_momentum_site_apply_host(L, n_up, m, kind, cc, p, x, cell, imaginary=imaginary)
            yr, _ = capi.spin_momentum_site_apply_host(L, n_up, m, kind, cc, p, np.ascontiguousarray(x.real), cell)
            yi, _ = capi.spin_momentum_site_apply_host(L, n_up, m, kind, cc, p, np.ascontiguousarray(x.imag), cell)
            assert yr.dtype == np.float64 and np.array_equal(y.real, yr) and np.array_equal(y.imag, yi)
        seen.add(kind)
    assert seen == set(KINDS)


def test_z_in_place(capi):
    L, n_up, cell, m = 12, 5, 2, 1
    n = ref.rows(L, n_up, cell, m)[0].size
    rng = np.random.default_rng(3)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    cc = [0.5 - 0.25j, 1.5 + 0.125j]
    y, n2 = capi.spin_momentum_site_apply_host(L, n_up, m, ref.Z, cc, 0, x, cell)
    z = x.copy()
    z2, n2z = capi.spin_momentum_site_apply_host(L, n_up, m, ref.Z, cc, 0, z, cell, in_place=True)
    assert np.shares_memory(z2, z) and np.array_equal(z, y) and n2z == n2 and n2 > 0 and not np.array_equal(y, x)


# ---- 4. adjointness ----
@pytest.mark.parametrize("L,n_up,cell", [(8, 4, 1), (12, 5, 2), (16, 8, 1), (36, 4, 1)])
def test_plus_with_conjugate_coefficients_is_the_adjoint_of_minus(capi, L, n_up, cell):
    """<z, O x> = <O^dagger z, x> = conj<x, O^dagger z>, the inner product conjugate-linear in its first argument (np.vdot):
    O = sum c_i S-_i from (n_up, m) to (n_up - 1, m'), O^dagger = the PLUS kind with conj(cc) and N - p, from (n_up - 1, m') back.
    Error at most n eps sum|z||O x|, n the length of the longer of the two vectors."""
    rng = np.random.default_rng(11 * L + cell)
    N = L // cell
    count = 0
    for m, p in momenta(L, cell):
        up2, m2 = ref.destination(L, n_up, cell, m, ref.MINUS, p)
        n_src, n_dst = ref.rows(L, n_up, cell, m)[0].size, ref.rows(L, up2, cell, m2)[0].size
        if not (n_src and n_dst):
            continue
        cc = rng.standard_normal(cell) + 1j * rng.standard_normal(cell)
        x = rng.standard_normal(n_src) + 1j * rng.standard_normal(n_src)
        z = rng.standard_normal(n_dst) + 1j * rng.standard_normal(n_dst)
        ox, _ = capi.spin_momentum_site_apply_host(L, n_up, m, ref.MINUS, cc, p, x, cell)
        oz, _ = capi.spin_momentum_site_apply_host(L, up2, m2, ref.PLUS, np.conj(cc), (N - p) % N, z, cell)
        assert oz.size == n_src
        lhs, rhs = np.vdot(z, ox), np.conj(np.vdot(x, oz))
        scale = float(np.sum(np.abs(z) * np.abs(ox)))
        print(L, n_up, cell, m, p, "adjointness error / (eps sum|z||Ox|):", abs(lhs - rhs) / (EPS * scale), "n:", max(n_src, n_dst))
        assert abs(lhs - rhs) <= max(n_src, n_dst) * EPS * scale
        assert abs(lhs) > 1e-3 * scale / np.sqrt(n_dst)  # not a comparison of two zeros
        count += 1
    assert count >= 6


# ---- 5. refusals ----
def test_refusals_name_the_entry_point_and_the_reason(capi):
    who = "eigenex_spin_momentum_site_apply_host: "
    L, n_up = 8, 4
    x0 = np.ones(ref.rows(L, n_up, 1, 0)[0].size)
    x1 = np.ones(ref.rows(L, n_up, 1, 1)[0].size, np.complex128)
    call = capi.spin_momentum_site_apply_host

    def refused(what, *args, **kw):
        with pytest.raises(capi.EigenexError, match="eigenex error -1: " + who + what):  # EIGENEX_ERR_ARG
            call(*args, **kw)

    refused("kind must be EIGENEX_SPIN_SITE_Z, _PLUS or _MINUS", L, n_up, 0, 3, [1.0], 0, x0)
    refused("p must be 0..n_sites/cell - 1", L, n_up, 0, ref.Z, [1.0], 8, x0)
    refused("p must be 0..n_sites/cell - 1", L, n_up, 0, ref.Z, [1.0], -1, x0)
    refused("a coefficient is not finite", L, n_up, 0, ref.Z, [np.inf], 0, x0)
    refused("a coefficient is not finite", L, n_up, 0, ref.Z, [1.0 + 1j * np.nan], 0, x0.astype(np.complex128))
    refused("the destination sector lies outside 0..n_sites", L, 8, 0, ref.PLUS, [1.0], 0, np.ones(1))
    refused("the destination sector lies outside 0..n_sites", L, 0, 0, ref.MINUS, [1.0], 0, np.ones(1))
    refused("n_sites must be 2..48", 49, 3, 0, ref.Z, [1.0], 0, np.ones(1))
    refused("n_up must be 0..n_sites", L, 9, 0, ref.Z, [1.0], 0, np.ones(1))
    refused("cell must be at least 1 and divide n_sites", L, n_up, 0, ref.Z, [1.0] * 3, 0, np.ones(1), cell=3)
    refused("momentum must be", L, n_up, 8, ref.Z, [1.0], 0, np.ones(1))
    # a real vector: real momenta on both sides and real coefficients only
    refused("a real vector takes real source and destination momenta", L, n_up, 0, ref.Z, [1.0], 1, x0)
    refused("a real vector takes real source and destination momenta", L, n_up, 0, ref.Z, [1.0 + 1j], 0, x0)
    # a flip, or a Z that changes the sector, reads rows it would have written
    refused("y may be x for EIGENEX_SPIN_SITE_Z with p = 0 only", L, n_up, 1, ref.Z, [1.0], 4, x1, in_place=True)
    refused("y may be x for EIGENEX_SPIN_SITE_Z with p = 0 only", L, n_up, 1, ref.MINUS, [1.0], 0, x1, in_place=True)
    # empty sectors: (6, 0) has one state of period 1, which carries k = 0 only
    with pytest.raises(capi.EigenexError, match=r"eigenex_spin_momentum_site_apply_host \(destination\): the sector is empty"):
        call(6, 1, 1, ref.MINUS, [1.0], 0, np.ones(1, np.complex128))
    with pytest.raises(capi.EigenexError, match=who + "the sector is empty"):
        call(6, 0, 1, ref.PLUS, [1.0], 0, np.ones(1, np.complex128))
    with pytest.raises(ValueError, match="one entry per row of the source sector"):
        call(L, n_up, 0, ref.Z, [1.0], 0, np.ones(3))


# ---- 6. the sanitizer program ----
@pytest.fixture(scope="module")
def sanitize_program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("site_sanitize") / "spin_momentum_site_sanitize")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "spin_momentum_site_sanitize.cpp"),
                           "-o", exe])
    return exe


@pytest.mark.parametrize("word", ["32", "64"])
def test_host_code_and_kernel_walk_under_sanitizers(sanitize_program, word):
    """csrc/spin_momentum_site.hpp (check, table, definition) and the walk of k_spin_momentum_site_apply<E, Word> -- the kernel's own
    functions of csrc/spin_rows.hpp, fallback lookups included -- in a stand-alone program under AddressSanitizer + UBSan: every
    load bounds-checked, every row bitwise equal to the definition, for both elements; 32 sites in the 32-bit run, 33, 36 and 48 in
    the 64-bit run, which also holds the two words against each other, byte for byte, on every ring of at most 32 sites."""
    out = subprocess.run([sanitize_program, word], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-1500:], out.stderr.decode()[-2000:])
    assert b"SPIN MOMENTUM SITE OK" in out.stdout
    if word == "64":
        assert re.search(rb"words agree on (\d+) calls", out.stdout) and int(re.search(rb"words agree on (\d+) calls", out.stdout).group(1)) > 20


# ---- 7. the header ----
def test_exports_are_declared_and_present(capi):
    text = open(os.path.join(ROOT, "include", "eigenex_hip.h")).read()
    for name in ("eigenex_spin_momentum_site_apply", "eigenex_spin_momentum_site_apply_z", "eigenex_spin_momentum_site_apply_host"):
        assert re.search(r"\bint %s\s*\(" % name, text)
        assert hasattr(capi.lib(), name) and name in capi.SIGNATURES
