"""The periodic spin-1/2 Heisenberg chain on L sites, matrix-free (eigenex_spin_upload) against the stored CSR of the same model
(eigenex_csr_upload of eigenex_spin_csr's rows, automatic layout) in one process:
  - time per operator application, from the library's own per-kernel profile (HIP events around every launch of eigenex_apply);
  - Lanczos iterations per second at m = 50 (host clock around eigenex_lanczos_enqueue, which ends in a synchronise).
The two forms alternate inside every repeat.  Sizes above --csr-max are run matrix-free only (the CSR of L = 28 is 50 GB).
usage: python scripts/probe_spin_operator.py [--sites 20 24 26] [--csr-max 26] [--m 50] [--applies 50] [--repeats 3]"""
import argparse
import sys
import time

sys.path.insert(0, ".")
import numpy as np

from cmpt_eigenex_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--sites", type=int, nargs="+", default=[20, 24, 26])
ap.add_argument("--csr-max", type=int, default=26)
ap.add_argument("--m", type=int, default=50)
ap.add_argument("--applies", type=int, default=50)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

ctx = capi.Context()


def chain(L):
    return [(i, (i + 1) % L, 1.0, 1.0) for i in range(L)]


def apply_time(b, count):
    """(us per application, booked bytes per application) from the profile of `count` applications"""
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


for L in args.sites:
    n = 1 << L
    forms = {}
    t0 = time.perf_counter()
    forms["matrix-free"] = capi.Csr.spin_half(ctx, L, chain(L))
    if L <= args.csr_max:
        rowptr, col, val = capi.spin_csr(L, chain(L))
        print(f"L={L}: CSR rows generated on the host in {time.perf_counter() - t0:.1f} s, {col.size} entries, {(12 * col.size + 4 * n) / 1e9:.2f} GB", flush=True)
        t0 = time.perf_counter()
        forms["csr"] = capi.Csr.upload(ctx, n, rowptr, col, val)
        del rowptr, col, val
        print(f"L={L}: CSR uploaded in {time.perf_counter() - t0:.1f} s: layout {forms['csr'].layout()}, encoding {forms['csr'].encoding()}", flush=True)
    states = {}
    for name, op in forms.items():
        b = capi.Basis(ctx, op, n, args.m + 2)
        b.random_signs(capi.VEC_START, 1, 0)
        b.copy(capi.VEC_COL(0), capi.VEC_START)
        apply_time(b, 3)  # first launches
        states[name] = b
    ys = {name: None for name in states}
    for rep in range(args.repeats):
        for name, b in states.items():
            us, by, launches = apply_time(b, args.applies)
            print(f"L={L} rep {rep} {name:12s} apply: {us:10.1f} us  ({launches:.0f} launch(es), booked {by / n:6.1f} B/row, {by / (us * 1e-6) / 1e12:6.3f} TB/s booked)", flush=True)
    if L <= 24 and len(states) == 2:  # the two forms compute the same bits (small sizes: the vectors come to the host)
        for name, b in states.items():
            b.apply(capi.VEC_COL(0), capi.VEC_V)
            ys[name] = b.download(capi.VEC_V)
        same = ys["matrix-free"].tobytes() == ys["csr"].tobytes()
        print(f"L={L}: y bit-identical between the forms: {same} (max difference {np.abs(ys['matrix-free'] - ys['csr']).max():.3e})", flush=True)
    for rep in range(args.repeats):
        for name, b in states.items():
            rate, alpha, beta = lanczos_rate(b, args.m)
            print(f"L={L} rep {rep} {name:12s} Lanczos m={args.m}: {rate:9.2f} iterations/s   (alpha_0 = {alpha[0]:.12g}, beta_{args.m - 1} = {beta[-1]:.12g})", flush=True)
    for b in states.values():
        b.close()
    for op in forms.values():
        op.close()
ctx.close()
