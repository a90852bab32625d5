"""S(q, w) in momentum sectors: the site-operator calls (eigenex_spin_momentum_site_apply(_z); k_spin_momentum_site_apply<E, Word>) and
whole solves of SpinMomentumDynamicsSolver (section (c), further down) on the periodic Heisenberg ring, cell = 1, source sector
(L, n_up) at k = 0, in one process per run.  The calls: for Z and MINUS, at p = N/2 (real states) and p = 1 (complex states),
  (a) the time of one call by the host clock -- the call allocates its scratch, copies its table, launches twice and
      synchronises once, all of which is in the figure;
  (b) beside it one application of the operator kernel on the DESTINATION handle (eigenex_apply, which synchronises too), by the
      same clock, and from the library's own per-kernel profile (HIP events around the launch).
The forms alternate inside every repeat, after warm-up calls.  For the kernels' own times run the script under a kernel trace in a
run of its own (rocprofv3 --kernel-trace --stats -- python scripts/probe_spin_momentum_dynamics.py ...): the rows to read are
k_spin_momentum_site_apply and k_spin_momentum_spmv.
usage: python scripts/probe_spin_momentum_dynamics.py [--sectors 24:12 28:14] [--calls 10] [--repeats 3] [--wide]
                                                       [--solves 28:14 32:16] [--sector 28:14] [--m 100]"""
import argparse
import sys
import time

sys.path.insert(0, ".")
import numpy as np

from cmpt_eigenex_amd import capi

Z, PLUS, MINUS = 0, 1, 2


def pair(text):
    L, k = text.split(":")
    return int(L), int(k)


ap = argparse.ArgumentParser()
ap.add_argument("--sectors", type=pair, nargs="+", default=[(24, 12), (28, 14)])
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--wide", action="store_true", help="64-bit state words")
ap.add_argument("--solves", type=pair, nargs="*", default=[(28, 14), (32, 16)], help="whole solves in the momentum sector")
ap.add_argument("--sector", type=pair, nargs="*", default=[(28, 14)], help="... beside SpinDynamicsSolver on the Sz sector")
ap.add_argument("--m", type=int, default=100)
args = ap.parse_args()

ctx = capi.Context()
make = capi.Csr.spin_half_momentum64 if args.wide else capi.Csr.spin_half_momentum


def ring(L):
    return [(i, (i + 1) % L, 1.0, 1.0) for i in range(L)]


def host_us(f, count):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(count):
        f()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e6 / count


def kernel_us(b, count):
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(count):
        b.apply(capi.VEC_COL(0), capi.VEC_V)
    launches, ms, by = ctx.profile_get(capi.K_SPMV)
    ctx.profile_enable(False)
    return ms * 1e3 / count


for (L, n_up) in args.sectors:
    tag = f"({L},{n_up})"
    for p, cplx in ((L // 2, False), (1, True)):
        src_op = make(ctx, L, n_up, 0, ring(L), complex_states=cplx)
        n_src = src_op.info()["n_global"]
        src = capi.Basis(ctx, src_op, n_src, 1)
        src.random_signs(capi.VEC_START, 1, 0)
        src.copy(capi.VEC_COL(0), capi.VEC_START)
        for kind, name in ((Z, "Z"), (MINUS, "MINUS")):
            up2, m2 = n_up - (kind == MINUS), (0 - p) % L
            t0 = time.perf_counter()
            dst_op = make(ctx, L, up2, m2, ring(L), complex_states=cplx)
            upload = time.perf_counter() - t0
            n_dst = dst_op.info()["n_global"]
            dst = capi.Basis(ctx, dst_op, n_dst, 2)
            cc = [1.0 / np.sqrt(L)]
            call = lambda: src.spin_momentum_site_apply(capi.VEC_COL(0), dst, capi.VEC_W, kind, cc, p)  # noqa: E731
            norm2 = call()
            dst.copy(capi.VEC_COL(0), capi.VEC_W)
            host_us(call, 2), kernel_us(dst, 2)  # first launches
            print(f"{tag} {name} p={p} {'complex' if cplx else 'real'}: {n_src} -> {n_dst} rows, destination upload {upload:.2f} s, "
                  f"norm2 / rows = {norm2 / n_src:.12f}", flush=True)
            for rep in range(args.repeats):
                site = host_us(call, args.calls)
                oper = host_us(lambda: dst.apply(capi.VEC_COL(0), capi.VEC_V), args.calls)
                kern = kernel_us(dst, args.calls)
                print(f"{tag} {name} p={p} rep {rep}: site call {site:10.1f} us, operator call {oper:10.1f} us by the host clock; "
                      f"operator kernel {kern:10.1f} us by events", flush=True)
            dst.close()
            dst_op.close()
        src.close()
        src_op.close()

# (c) whole solves: SpinMomentumDynamicsSolver.computeStructureFactorZ(L/2) (the real run) and (1) (the complex run) at --m steps
# from a state of the sector (L, L/2) at k = 0 -- a random one: the time of a solve does not depend on which state it starts from --
# by the host clock, twice each (the first call also builds the destination operator); with --sector, beside
# SpinDynamicsSolver.computeStructureFactorZ(pi) and computeStructureFactorZSingleRun(pi) on the Sz sector in the same process.
from cmpt_eigenex_amd import solver  # noqa: E402


def timed(label, f):
    for rep in range(2):
        ctx.sync()
        t0 = time.perf_counter()
        f()
        ctx.sync()
        print(f"{label} run {rep}: {time.perf_counter() - t0:8.3f} s", flush=True)


for (L, n_up) in args.solves:
    tag = f"({L},{n_up}) m={args.m}"
    n = capi.spin_momentum64_dim(L, n_up, 0) if args.wide else capi.spin_momentum_dim(L, n_up, 0)
    x = np.random.default_rng(1).standard_normal(n)
    ds = solver.SpinMomentumDynamicsSolver()
    ds.setModel(ctx, L, ring(L), n_up, 0).setState(x).setStateEnergy(0.0).setLanczosSteps(args.m)
    for q in (L // 2, 1):
        timed(f"{tag} momentum computeStructureFactorZ({q})", lambda: ds.computeStructureFactorZ(q))
        r = ds.results()
        print(f"{tag} momentum computeStructureFactorZ({q}): {r['info_name']}, {r['npoles']} poles, destination momentum {r['destinationMomentum']}, "
              f"{r['destinationDimension']} rows, {'complex' if r['complexRun'] else 'real'} run, totalWeight {r['totalWeight']:.12f}", flush=True)
    ds.close()
    if (L, n_up) in args.sector:
        xs = np.random.default_rng(2).standard_normal(capi.spin_sector_dim(L, n_up))
        ss = solver.SpinDynamicsSolver()
        ss.setModel(ctx, L, ring(L), n_up=n_up).setState(xs).setStateEnergy(0.0).setLanczosSteps(args.m)
        timed(f"{tag} Sz sector computeStructureFactorZ(pi)", lambda: ss.computeStructureFactorZ(np.pi))
        timed(f"{tag} Sz sector computeStructureFactorZSingleRun(pi)", lambda: ss.computeStructureFactorZSingleRun(np.pi))
        ss.close()
ctx.close()
