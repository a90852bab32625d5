"""The periodic spin-1/2 Heisenberg chain on L sites in the sector of n_up sites up, matrix-free (eigenex_spin_sector_upload),
in one process per run:
  (a) time per application of the sector operator;
  (b) the same for the plain-CSR upload (column_blocks = 0) of the same sector rows (eigenex_spin_sector_csr), where --csr names
      the sector (the CSR of (30,15) is 30 GB);
  (c) the same for the full-space operator (eigenex_spin_upload) at the same L <= 30, also per row;
  (d) Lanczos iterations per second at m = 50 on the sector operator, where a basis of m + 2 columns fits --basis-gb.
Times per application come from the library's own per-kernel profile (HIP events around every launch of eigenex_apply), after
three warm-up applications; the forms alternate inside every repeat.  Lanczos: host clock around eigenex_lanczos_enqueue, which
ends in a synchronise.
usage: python scripts/probe_spin_sector.py [--sectors 24:12 28:14 30:15 32:16] [--csr 24:12 28:14] [--m 50] [--applies 20]
                                           [--repeats 3] [--basis-gb 160] [--no-full-space]"""
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
ap.add_argument("--sectors", type=pair, nargs="+", default=[(24, 12), (28, 14), (30, 15), (32, 16)])
ap.add_argument("--csr", type=pair, nargs="*", default=[(24, 12), (28, 14)])
ap.add_argument("--m", type=int, default=50)
ap.add_argument("--applies", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--basis-gb", type=float, default=160.0)
ap.add_argument("--no-full-space", action="store_true")
args = ap.parse_args()

ctx = capi.Context()


def chain(L):
    return [(i, (i + 1) % L, 1.0, 1.0) for i in range(L)]


def apply_time(b, count):
    """(us per application, booked bytes per application, launches per application) from the profile of `count` applications"""
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(count):
        b.apply(capi.VEC_COL(0), capi.VEC_V)
    launches, ms, by = ctx.profile_get(capi.K_SPMV)
    ctx.profile_enable(False)
    return ms * 1e3 / count, by / count, launches / count


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
    return m / dt, alpha, beta


for (L, n_up) in args.sectors:
    n = capi.spin_sector_dim(L, n_up)
    tag = f"({L},{n_up})"
    print(f"{tag}: {n} rows, vector {8 * n / 1e9:.2f} GB", flush=True)
    forms = {"sector": (capi.Csr.spin_half_sector(ctx, L, n_up, chain(L)), n)}
    if (L, n_up) in args.csr:
        t0 = time.perf_counter()
        rowptr, col, val = capi.spin_sector_csr(L, n_up, chain(L))
        print(f"{tag}: CSR rows generated on the host in {time.perf_counter() - t0:.1f} s, {col.size} entries, {(12 * col.size + 4 * n) / 1e9:.2f} GB", flush=True)
        t0 = time.perf_counter()
        forms["sector-csr"] = (capi.Csr.upload(ctx, n, rowptr, col, val, column_blocks=0), n)
        del rowptr, col, val
        print(f"{tag}: CSR uploaded in {time.perf_counter() - t0:.1f} s: layout {forms['sector-csr'][0].layout()}, encoding {forms['sector-csr'][0].encoding()}", flush=True)
    if L <= 30 and not args.no_full_space:
        forms["full-space"] = (capi.Csr.spin_half(ctx, L, chain(L)), 1 << L)
    states = {}
    for name, (op, rows) in forms.items():
        b = capi.Basis(ctx, op, rows, 2)
        b.random_signs(capi.VEC_START, 1, 0)
        b.copy(capi.VEC_COL(0), capi.VEC_START)
        apply_time(b, 3)  # first launches
        states[name] = (b, rows)
    for rep in range(args.repeats):
        for name, (b, rows) in states.items():
            us, by, launches = apply_time(b, args.applies)
            print(f"{tag} rep {rep} {name:10s} apply: {us:11.1f} us = {us * 1e3 / rows:7.4f} ns/row  ({launches:.0f} launch(es), {rows} rows, booked {by / rows:6.1f} B/row, "
                  f"{by / (us * 1e-6) / 1e12:6.3f} TB/s booked)", flush=True)
    if L <= 24 and "sector-csr" in states:  # the two forms compute the same bits (small sizes: the vectors come to the host)
        ys = {}
        for name in ("sector", "sector-csr"):
            b = states[name][0]
            b.apply(capi.VEC_COL(0), capi.VEC_V)
            ys[name] = b.download(capi.VEC_V)
        same = ys["sector"].tobytes() == ys["sector-csr"].tobytes()
        print(f"{tag}: y bit-identical between sector and sector-csr: {same} (max difference {np.abs(ys['sector'] - ys['sector-csr']).max():.3e})", flush=True)
    for b, _ in states.values():
        b.close()
    for name, (op, _) in forms.items():
        if name != "sector":
            op.close()
    basis_gb = 8.0 * n * (args.m + 6) / 1e9  # m + 2 columns and the state's work vectors
    if basis_gb <= args.basis_gb:
        b = capi.Basis(ctx, forms["sector"][0], n, args.m + 2)
        b.random_signs(capi.VEC_START, 1, 0)
        lanczos_rate(b, args.m)  # first launches
        for rep in range(args.repeats):
            rate, alpha, beta = lanczos_rate(b, args.m)
            print(f"{tag} rep {rep} sector     Lanczos m={args.m}: {rate:9.2f} iterations/s   (alpha_0 = {alpha[0]:.12g}, beta_{args.m - 1} = {beta[-1]:.12g})", flush=True)
        b.close()
    else:
        print(f"{tag}: Lanczos m={args.m} not run: its basis takes {basis_gb:.0f} GB, above --basis-gb {args.basis_gb:.0f}", flush=True)
    forms["sector"][0].close()
ctx.close()
