"""The periodic spin-1/2 Heisenberg ring on L sites in momentum sectors of the sector of n_up sites up, matrix-free
(eigenex_spin_momentum_upload / _z), in one process per run:
  (a) the upload time (host enumeration of the representatives, tables, copies);
  (b) time per application of the real kernel (m = 0) and of the complex kernel (m = 0 and m = 1), beside one application of the
      sector operator (eigenex_spin_sector_upload) of the same (L, n_up);
  (c) Lanczos iterations per second at --m steps on the momentum operators;
  (d) expand (eigenex_spin_momentum_expand) into the sector, where --expand names the sector.
Times per application come from the library's own per-kernel profile (HIP events around every launch of eigenex_apply), after
three warm-up applications; the forms alternate inside every repeat.  Lanczos and expand: host clock around calls that end in a
synchronise.
usage: python scripts/probe_spin_momentum.py [--sectors 24:12 28:14 32:16] [--expand 24:12 28:14] [--m 50] [--applies 20]
                                             [--repeats 3] [--no-sector]"""
import argparse
import sys
import time

sys.path.insert(0, ".")
import numpy as np

from cmpt_eigenex_amd import capi


def pair(text):
    L, k = text.split(":")
    return int(L), int(k)


ap = argparse.ArgumentParser()
ap.add_argument("--sectors", type=pair, nargs="+", default=[(24, 12), (28, 14), (32, 16)])
ap.add_argument("--expand", type=pair, nargs="*", default=[(24, 12), (28, 14)])
ap.add_argument("--m", type=int, default=50)
ap.add_argument("--applies", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--no-sector", action="store_true")
args = ap.parse_args()

ctx = capi.Context()


def ring(L):
    return [(i, (i + 1) % L, 1.0, 1.0) for i in range(L)]


def apply_time(b, count):
    """us per application from the profile of `count` applications"""
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(count):
        b.apply(capi.VEC_COL(0), capi.VEC_V)
    launches, ms, by = ctx.profile_get(capi.K_SPMV)
    ctx.profile_enable(False)
    return ms * 1e3 / count


def lanczos_rate(b, m):
    b.clear()
    b.copy(capi.VEC_W, capi.VEC_START)
    ctx.sync()
    t0 = time.perf_counter()
    b.lanczos_enqueue(m + 1)
    st, alpha, beta = b.lanczos_state()
    ctx.sync()
    dt = time.perf_counter() - t0
    assert st.iterations == m and st.stopped == 0
    return m / dt, alpha


for (L, n_up) in args.sectors:
    tag = f"({L},{n_up})"
    forms = {}
    for name, m, cplx in (("real m=0", 0, False), ("complex m=0", 0, True), ("complex m=1", 1, True)):
        t0 = time.perf_counter()
        op = capi.Csr.spin_half_momentum(ctx, L, n_up, m, ring(L), complex_states=cplx)
        dt = time.perf_counter() - t0
        n = op.info()["n_global"]
        forms[name] = (op, n)
        print(f"{tag} {name:12s}: {n} rows, vector {8 * n * (2 if cplx else 1) / 1e6:.1f} MB, upload {dt:.2f} s", flush=True)
    if not args.no_sector:
        forms["sector"] = (capi.Csr.spin_half_sector(ctx, L, n_up, ring(L)), capi.spin_sector_dim(L, n_up))
    states = {}
    for name, (op, rows) in forms.items():
        b = capi.Basis(ctx, op, rows, 2)
        b.random_signs(capi.VEC_START, 1, 0)
        b.copy(capi.VEC_COL(0), capi.VEC_START)
        apply_time(b, 3)  # first launches
        states[name] = (b, rows)
    for rep in range(args.repeats):
        for name, (b, rows) in states.items():
            us = apply_time(b, args.applies if name != "sector" else max(2, args.applies // 4))
            print(f"{tag} rep {rep} {name:12s} apply: {us:11.1f} us = {us * 1e3 / rows:8.4f} ns/row ({rows} rows)", flush=True)
    if (L, n_up) in args.expand and "sector" in states:
        bd = states["sector"][0]
        for name in ("real m=0",):
            bm = states[name][0]
            bm.spin_momentum_expand(capi.VEC_COL(0), bd, capi.VEC_COL(1))  # first launch
            for rep in range(args.repeats):
                ctx.sync()
                t0 = time.perf_counter()
                norm2 = bm.spin_momentum_expand(capi.VEC_COL(0), bd, capi.VEC_COL(1))
                dt = time.perf_counter() - t0
                print(f"{tag} rep {rep} expand ({name}): {dt * 1e6:11.1f} us by the host clock, allocations and the synchronise included "
                      f"(norm2 / rows = {norm2 / states[name][1]:.15f})", flush=True)
    for b, _ in states.values():
        b.close()
    for name in ("real m=0", "complex m=1"):
        op, n = forms[name]
        b = capi.Basis(ctx, op, n, args.m + 2)
        b.random_signs(capi.VEC_START, 1, 0)
        lanczos_rate(b, args.m)  # first launches
        for rep in range(args.repeats):
            rate, alpha = lanczos_rate(b, args.m)
            print(f"{tag} rep {rep} {name:12s} Lanczos m={args.m}: {rate:9.2f} iterations/s   (alpha_0 = {np.real(alpha[0]):.12g})", flush=True)
        b.close()
    for op, _ in forms.values():
        op.close()
ctx.close()
