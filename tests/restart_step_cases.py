"""The cases of tests/test_gpu_restart_steps.py: Lanczos and Arnoldi states that eigenex_lanczos_restart or eigenex_arnoldi_restart
has rewritten, and the steps behind the restart.  Seeded; importable without a GPU: nothing touches the device before a runner is
called.  tests/test_restart_step_reference_host.py runs the fp64 recurrences of tests/krylov_local_reference.py
(thick_restart_fp64, krylov_schur_fp64) over every case on the CPU, without and with every fault that applies to it.

Shared: N = 4133 = 2 * 2048 + 37 rows (two tiles of the vector kernels and a ragged third; a complex state is 8266 doubles), m = 24
as in tests/test_gpu_krylov_schur.py.  The Hermitian operator is variant_cases.random_csr with 6 draws per row, symmetrised (about
twelve entries per row); the general one is that of test_gpu_krylov_schur.primitive_problem (solver.random_csr(N, 8, 6), complex:
plus i times a seeded normal), with its start vector.

Lanczos cases (kind "lanczos"): scheme = the orthogonalisation of the calls behind a restart,
  front     one call ORTHO_BATCHED_TWICE, the others ORTHO_BATCHED (thick_restart_lanczos.hpp)
  batched, seq, adaptive   one scheme throughout
crossed with real / complex, nkeep 7 / 17 (17 crosses the 16-column chunk of k_ritz) and one shard / three loopback shards with the
fused alpha on and off; the edges nkeep = 1 and nkeep = m; three cycles; a shift of -0.37.
Arnoldi cases: real nkeep 7 / 17, complex nkeep 3 / 9 (9 crosses the 8-column pass of k_compress_z), the default scheme and
ORTHO_BATCHED_ADAPTIVE, one and three shards, shift 0 and (complex) 0.3 - 0.2i; three cycles.

What a cycle holds (the fp64 recurrence and the device runner return the same dict, see krylov_local_reference) and what is checked
of it (check_cycle): the combination Y = V C within the bound of tests/ritz_reference.py, the kept relation, and the local step check
from first = nkeep, orthogonality of all columns included.

coupling_last: the device echoes it as beta[nkeep - 1], bit for bit, and that is all that is asserted of it.  With full
re-orthogonalisation the later vectors do not depend on it (the pass removes whatever the recurrence left along column nkeep - 1),
so the local check cannot see it, and no tolerance is invented for it."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import krylov_local_reference as kl  # noqa: E402
import ritz_reference as rr  # noqa: E402
import variant_cases as vc  # noqa: E402

N, M = 4133, 24
SHIFT, SHIFT_Z = -0.37, 0.3 - 0.2j
MODES = {"ORTHO_BATCHED": kl.BATCHED, "ORTHO_SEQUENTIAL": kl.SEQUENTIAL, "ORTHO_BATCHED_TWICE": kl.TWICE, "ORTHO_BATCHED_ADAPTIVE": kl.ADAPTIVE}
SCHEMES = {  # name -> (the first call behind a restart, every other call)
    "front": ("ORTHO_BATCHED_TWICE", "ORTHO_BATCHED"),
    "batched": ("ORTHO_BATCHED", "ORTHO_BATCHED"),
    "seq": ("ORTHO_SEQUENTIAL", "ORTHO_SEQUENTIAL"),
    "adaptive": ("ORTHO_BATCHED_ADAPTIVE", "ORTHO_BATCHED_ADAPTIVE"),
    "default": ("ORTHO_BATCHED", "ORTHO_BATCHED"),  # Arnoldi
}
_INPUTS, _REFS = {}, {}


def _seed(what):
    return vc.hash_seed(f"restart_step_cases/{what}")


def inputs(kind, cplx):
    """(rows, x0) of the Hermitian (lanczos) or the general (arnoldi) operator"""
    key = (kind, bool(cplx))
    if key not in _INPUTS:
        if kind == "lanczos":
            rows = vc.random_csr(_seed(f"herm/{int(cplx)}"), N, 6, symmetric=True, cplx=cplx)
            x0 = vc.start_vector(_seed(f"start/{int(cplx)}"), N, cplx)
        else:
            from cmpt_eigenex_amd import solver  # host code of the library: no GPU

            rowptr, col, val = solver.random_csr(N, 8, 6)
            if cplx:
                val = val + 1j * np.random.default_rng(6).standard_normal(val.size)
            rows, x0 = (rowptr, col, val), solver.random_vector(9, N, np.complex128 if cplx else np.float64)
        for a in (*rows, x0):
            a.setflags(write=False)
        _INPUTS[key] = (rows, x0)
    return _INPUTS[key]


def applicable_faults(c):
    """the faults of kl.RESTART_FAULTS that change what this case holds far beyond rounding"""
    nkeep, lanczos = c["nkeep"], c["kind"] == "lanczos"
    f = ["last_basis_column_dropped"]
    if lanczos:
        f += ["alpha_from_previous", "residual_column_previous"]
        if nkeep < M:  # the operator output is read by the next step only
            f.append("stale_v")
    else:
        f.append("coupling_overwritten")
        if c["cplx"]:
            f.append("coupling_row_conjugated")
    if 2 <= nkeep < M:
        f.append("kept_columns_not_projected")
    if nkeep > (8 if (c["cplx"] and not lanczos) else 16):
        f.append("second_chunk_repeats_first")
    return tuple(f)


def _case(kind, cplx, nkeep, scheme, shards=1, fusion=None, shift=0.0, cycles=1):
    name = f"{'l' if kind == 'lanczos' else 'a'}{'z' if cplx else 'r'}-{scheme}-k{nkeep}-s{shards}{ {None: '', True: 'f', False: 'u'}[fusion]}"
    if shift != 0.0:
        name += "-shift"
    if cycles > 1:
        name += f"-c{cycles}"
    c = dict(name=name, kind=kind, cplx=cplx, nkeep=nkeep, scheme=scheme, shards=shards, fusion=fusion, shift=shift, cycles=cycles)
    c["faults"] = applicable_faults(c)
    return c


SHARDINGS = ((1, None), (3, True), (3, False))
LANCZOS_GRID = [_case("lanczos", cplx, nkeep, scheme, shards, fusion) for scheme in ("front", "batched", "seq", "adaptive") for cplx in (False, True)
                for nkeep in (7, 17) for shards, fusion in SHARDINGS]
LANCZOS_EDGES = [_case("lanczos", cplx, nkeep, "front", shards) for nkeep in (1, M) for cplx, shards in ((False, 1), (True, 3))]
LANCZOS_SHIFT = [_case("lanczos", False, 7, "front", shift=SHIFT), _case("lanczos", True, 7, "front", shift=SHIFT)]
LANCZOS_CYCLES = [_case("lanczos", cplx, 7, "front", shards, cycles=3) for cplx in (False, True) for shards in (1, 3)]
LANCZOS_SPLITS = [_case("lanczos", False, 7, "batched"), _case("lanczos", True, 7, "batched"), _case("lanczos", False, 7, "batched", 3, False)]
ARNOLDI_GRID = [_case("arnoldi", cplx, nkeep, scheme, shards, shift=shift) for cplx, keeps, shifts in ((False, (7, 17), (0.0,)), (True, (3, 9), (0.0, SHIFT_Z)))
                for nkeep in keeps for scheme in ("default", "adaptive") for shards in (1, 3) for shift in shifts]
ARNOLDI_CYCLES = [_case("arnoldi", cplx, nkeep, "adaptive", shards, cycles=3) for cplx, nkeep in ((False, 7), (True, 3)) for shards in (1, 3)]
ARNOLDI_SPLITS = [_case("arnoldi", False, 7, "default"), _case("arnoldi", True, 3, "default")]
CASES = LANCZOS_GRID + LANCZOS_EDGES + LANCZOS_SHIFT + LANCZOS_CYCLES + ARNOLDI_GRID + ARNOLDI_CYCLES
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert all(s["name"] in BY_NAME for s in LANCZOS_SPLITS + ARNOLDI_SPLITS)  # a split case is a grid case run three ways


def reference_key(c):
    """what the fp64 recurrence depends on: not the shards and not the fusion"""
    return c["kind"], c["cplx"], c["nkeep"], c["scheme"], c["shift"], c["cycles"]


REFERENCES = {}  # key -> the first case with it
for _c in CASES:
    REFERENCES.setdefault(reference_key(_c), _c)


def modes(c):
    first, rest = SCHEMES[c["scheme"]]
    return MODES[first], MODES[rest]


def reference(c, fault=None):
    """the cycles of the fp64 recurrence of a case: [0] the unrestarted run, [1 ..] one dict per restart"""
    cycles = 1 if fault else c["cycles"]  # a fault shows behind the first restart
    key = reference_key(c)[:-1] + (cycles, fault)
    if key not in _REFS:
        rows, x0 = inputs(c["kind"], c["cplx"])
        first, rest = modes(c)
        run = kl.thick_restart_fp64 if c["kind"] == "lanczos" else kl.krylov_schur_fp64
        _REFS[key] = run(kl.csr_matmul(rows), x0, M, c["nkeep"], cycles, c["shift"], first, rest, fault)
    return _REFS[key]


def combination_ratio(Y, V, C):
    """the worst |Y - V C| / bound of tests/ritz_reference.py (raw: no normalisation), entry by entry; Y and V as rows"""
    ref = rr.combine(V, C)
    ref = ref.astype(np.complex128 if np.iscomplexobj(ref) else np.float64)
    tol = rr.bound(V, C, ref, raw=True)
    err = np.abs(np.asarray(Y).T - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max())


def check_cycle(c, cy):
    """dict(step: Report from first = nkeep, kept: KeptReport, comb: the combination's worst ratio, ortho: orthogonality / bound,
    worst: the largest of the four ratios) of one restarted cycle, from the reference or from the device"""
    rows, _ = inputs(c["kind"], c["cplx"])
    if c["kind"] == "lanczos":
        k = c["nkeep"]
        comb = combination_ratio(cy["Y"][:k], cy["V"][:M], cy["S"])
        kept = kl.check_kept_lanczos(rows, c["shift"], cy["Y"][:k], cy["Y"][k], cy["theta"], cy["s"], cy["S"])
        step = kl.check_lanczos(rows, c["shift"], cy["U"], cy["alpha"], cy["beta"], first=k)
    else:
        k = cy["k"]
        comb = combination_ratio(cy["Y"], cy["V"], cy["Q"])
        # the kept relation of the stored state after the steps: B_top and the coupling row as the device holds them then
        H = cy["H"]
        kept = kl.check_kept_arnoldi(rows, c["shift"], cy["U"][:k], H[:k, :k], cy["w0"], H[k, :k] / cy["residue0"], cy["Q"])
        step = kl.check_arnoldi(rows, c["shift"], cy["U"], H, cy["residue"], cy["w"], first=k)
    ortho = step["ortho"] / step["ortho_bound"]
    return dict(step=step, kept=kept, comb=comb, ortho=ortho, worst=max(step.ratio(), kept.ratio(), comb, ortho))


def line(name, i, r):
    return (f"{name} cycle {i}: step {r['step'].ratio():.3e} kept {r['kept'].ratio():.3e} combination {r['comb']:.3e} ortho {r['ortho']:.3e}")


# ---- the device runners -------------------------------------------------------------------------------------------------------
def upload(capi, ctx, c):
    rows, _ = inputs(c["kind"], c["cplx"])
    return capi.Csr.upload(ctx, N, *rows)


def batches_behind(c, calls):
    """the batches of the calls behind a restart: (1, the rest) where the first call has a scheme of its own, else one batch"""
    first, rest = SCHEMES[c["scheme"]]
    out = (1, calls - 1) if first != rest else (calls,)
    return tuple(n for n in out if n > 0) if calls > 0 else ()


def enqueue_behind(capi, b, c, batches, enqueue):
    first, rest = SCHEMES[c["scheme"]]
    assert first == rest or not batches or batches[0] == 1
    for i, n in enumerate(batches):
        b.configure(shift=c["shift"], ortho_mode=getattr(capi, first if i == 0 else rest))
        enqueue(n)
    b.configure(shift=c["shift"], ortho_mode=getattr(capi, rest))


def lanczos_restart(capi, b, c, prev, T, batches=None):
    """one thick restart of the state `prev` (krylov_pass_runs.lanczos_state) whose projected matrix the host holds as T, and the
    calls behind it.  Returns (the cycle dict, the state right after the restart, the next T)."""
    from krylov_pass_runs import lanczos_state

    k = c["nkeep"]
    theta_all, S_all = np.linalg.eigh(T)
    theta, S = theta_all[:k], np.ascontiguousarray(S_all[:, :k])
    s = prev["beta"][M - 1] * S[M - 1]
    b.lanczos_restart(S, s[k - 1])
    after = lanczos_state(capi, b)
    enqueue_behind(capi, b, c, batches_behind(c, M - k) if batches is None else batches, b.lanczos_enqueue)
    got = lanczos_state(capi, b)
    cy = dict(V=prev["U"], theta=theta, S=S, s=s, coupling_last=s[k - 1], Y=after["U"], alpha=got["alpha"], beta=got["beta"], U=got["U"], got=got)
    return cy, after, next_T(cy)


def next_T(cy):
    """the projected matrix of a completed cycle, as the front-end builds it: diag(theta), the border s, and the tail from the
    downloaded alpha[nkeep ..] and beta[nkeep ..].  None while calls are missing, or when the whole of T was kept."""
    k = len(cy["theta"])
    if k == M or len(cy["alpha"]) < M + 1:
        return None
    return kl.restart_T(cy["theta"], cy["s"], cy["alpha"], cy["beta"], M)


def arnoldi_restart(capi, solver, b, c, prev, batches=None):
    """one Krylov-Schur restart of the state `prev` (krylov_pass_runs.arnoldi_state) and the calls behind it.  Returns (the cycle
    dict, the state right after the restart)."""
    from krylov_pass_runs import arnoldi_state

    k, Q, B, _ = solver.krylov_schur_basis(prev["H"][:M], c["nkeep"], prev["residue"])
    b.arnoldi_restart(Q, B)
    after = arnoldi_state(capi, b)
    enqueue_behind(capi, b, c, batches_behind(c, M - k) if batches is None else batches, b.arnoldi_enqueue)
    got = arnoldi_state(capi, b)
    cy = dict(V=prev["U"], k=k, Q=Q, B=B, w0=prev["w"], residue0=prev["residue"], Y=after["U"], U=got["U"], H=got["H"], residue=got["residue"], w=got["w"],
              got=got)
    return cy, after


# ---- breakdown behind a restart -----------------------------------------------------------------------------------------------
BREAK_D, BREAK_CALLS, BREAK_KEEP, BREAK_BATCH = 12, 8, 3, 12
BREAK_ROWS = np.array([3, 700, 1501, 2047, 2048, 2900, 3333, 4095, 4096, 4100, 4117, 4132])  # every tile of 2048 rows, both edges of each
BREAK_VALUES = np.array([-2.3, -1.9, -1.2, -0.8, -0.35, 0.1, 0.45, 0.9, 1.3, 1.75, 2.2, 2.6])
SENTINEL = 7.25


def breakdown_inputs():
    """a diagonal operator with twelve distinct values on twelve rows and zero elsewhere, and a start vector supported on those
    rows: the Krylov space has dimension twelve"""
    d = np.zeros(N)
    d[BREAK_ROWS] = BREAK_VALUES
    x = np.zeros(N)
    x[BREAK_ROWS] = np.random.default_rng(_seed("breakdown")).uniform(0.5, 1.5, BREAK_D)
    return (np.arange(N + 1, dtype=np.int32), np.arange(N, dtype=np.int32), d), x
