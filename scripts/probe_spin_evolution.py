"""What real-time evolution of a spin state costs on one MI355X, one sector per process:

    python scripts/probe_spin_evolution.py --sector 28:14 --out results.jsonl        (one step; run it under `timeout`)
    python scripts/probe_spin_evolution.py --sector 28:14 --kernels-only                 (under a kernel tracer, in a run of its own)
    python scripts/probe_spin_evolution.py --write-profile results.md --out results.jsonl   (no GPU: the tables from the records)

Periodic XXZ chain (Jz = 0.6, Jxy = 1) in the sector (L, n_up), a random-sign start vector.  Host clock around calls that end in
a synchronise, one warm-up call of each kind first, then the kinds in turn, `--repeats` times; a timed window holds `--batch`
calls of its kind (every call synchronises, so a window is `--batch` times launch + kernel + synchronise) and is reported per
call.  These are CALL times; the kernels' own times come from a kernel trace of `--kernels-only`, which runs 20 calls of each
kind and times nothing:
  apply_z     one application of the complex-state operator (k_spin_spmv<..., SpinZ>): eigenex_apply from W into V on a complex state
  apply_real  one application of the real operator (k_spin_spmv) on a real state of the same sector; two of them are what
              evolving the real and the imaginary part as separate planes would cost per operator application
  measure_z   a one-chunk eigenex_spin_measure (16 site masks, 16 pair masks) of the complex vector, measure_real of the real one
  sub_step    one evolve(dt) of SpinTimeEvolutionSolver at m = 30 with dt small enough for a single sub-step: 31 operator
              applications with full re-orthogonalisation, the host's tridiagonal problem and quadrature, the combination into W
No threshold is asserted anywhere: none of these numbers existed before."""
import argparse
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np


def pair(text):
    L, k = text.split(":")
    return int(L), int(k)


def timed(ctx, fn, batch=1):
    """ms per call over a window of `batch` calls"""
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(batch):
        fn()
    return (time.perf_counter() - t0) * 1e3 / batch


def step(args):
    from cmpt_eigenex_amd import capi, solver

    L, n_up = args.sector
    n = capi.spin_sector_dim(L, n_up)
    bonds = [(i, (i + 1) % L, 0.6, 1.0) for i in range(L)]
    ctx = capi.Context()
    Z = capi.Csr.spin_half_sector(ctx, L, n_up, bonds, complex_states=True)
    R = capi.Csr.spin_half_sector(ctx, L, n_up, bonds)
    bz, br = capi.Basis(ctx, Z, n, 1), capi.Basis(ctx, R, n, 1)
    for b in (bz, br):
        b.random_signs(capi.VEC_W, 1, 0)
    sites = [1 << i for i in range(16)]
    pairs = [(1 << i) | (1 << ((i + 1) % L)) for i in range(16)]
    kinds = {
        "apply_z": lambda: bz.apply(capi.VEC_W, capi.VEC_V),
        "apply_real": lambda: br.apply(capi.VEC_W, capi.VEC_V),
        "measure_z": lambda: bz.spin_measure(capi.VEC_W, sites, pairs),
        "measure_real": lambda: br.spin_measure(capi.VEC_W, sites, pairs),
    }
    times = {k: [] for k in kinds}
    for fn in kinds.values():
        fn()
    if args.kernels_only:
        for fn in kinds.values():
            for _ in range(20):
                fn()
        for h in (bz, br, Z, R, ctx):
            h.close()
        return
    for _ in range(args.repeats):
        for k, fn in kinds.items():
            times[k].append(timed(ctx, fn, args.batch))
    for h in (bz, br):
        h.close()
    te = solver.SpinTimeEvolutionSolver().setModel(ctx, L, bonds, n_up=n_up)
    te.setKrylovDimension(30).setTolerance(1e-10).setProductState(sum(1 << i for i in range(0, L, 2)) if 2 * n_up == L else (1 << n_up) - 1)
    assert te.info() == "Success", te.log()
    sub, steps = [], []
    for i in range(args.repeats + 1):
        t = timed(ctx, lambda: steps.append(te.evolve(args.dt)))
        if i:
            sub.append(t)
    rec = dict(L=L, n_up=n_up, rows=n, dt=args.dt, batch=args.batch, sub_steps=steps, sub_step_ms=sub, error_bound=te.errorBound(), applications=te.operatorApplications(),
               norm2=te.normSquared(), **{k + "_ms": v for k, v in times.items()})
    print(json.dumps(rec), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    for h in (te, Z, R, ctx):
        h.close()


def write_profile(args):
    recs = [json.loads(line) for line in open(args.out) if line.strip()]
    med = lambda v: float(np.median(v))  # noqa: E731
    span = lambda v: f"{med(v):.3f} ({min(v):.3f} – {max(v):.3f})"  # noqa: E731
    lines = ["| `(L, n_up)` | rows | `apply_z` | `apply_real` | `apply_z` / (2 `apply_real`) | bytes of x and y per ms, `apply_z` | `measure_z` | `measure_real` | one `m = 30` sub-step |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        az, ar = r["apply_z_ms"], r["apply_real_ms"]
        lines.append(f"| ({r['L']},{r['n_up']}) | {r['rows']:,} | {span(az)} | {span(ar)} | {med(az) / (2 * med(ar)):.2f} | {32 * r['rows'] / med(az) / 1e6:.0f} MB | "
                     f"{span(r['measure_z_ms'])} | {span(r['measure_real_ms'])} | {span(r['sub_step_ms'])} ({r['sub_steps'][-1]} sub-step, dt = {r['dt']}) |")
    text = "\n".join(lines) + "\n"
    with open(args.write_profile, "w") as f:
        f.write(text)
    print(text)


ap = argparse.ArgumentParser()
ap.add_argument("--sector", type=pair, default=(24, 12))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--batch", type=int, default=100)
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--dt", type=float, default=0.02)
ap.add_argument("--out", default="spin_evolution.jsonl")
ap.add_argument("--write-profile", default=None)
args = ap.parse_args()
write_profile(args) if args.write_profile else step(args)
