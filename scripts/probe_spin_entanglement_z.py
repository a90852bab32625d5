"""The reduced density matrix of one COMPLEX vector of the periodic spin-1/2 Heisenberg chain in the sector (L, n_up) beside that
of a real vector on the real operator of the same shape, one shape per process:

    python scripts/probe_spin_entanglement_z.py --sector 28:14 --cut low2 --out results.jsonl           (call times; under `timeout`)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python scripts/probe_spin_entanglement_z.py --sector 28:14 --cut low2 --kernels-only            (kernel times: a run of its own)
    python scripts/probe_spin_entanglement_z.py --sector 28:14 --cut low2 --kernel-stats DIR --out results.jsonl   (no GPU: reads DIR)
    python scripts/probe_spin_entanglement_z.py --write-profile profiles/spin_entanglement_z.md --resources usage.txt --out results.jsonl   (no GPU)

Cuts: low2, low4 (the lowest sites), high2, high4 (the highest), half (the lowest L / 2 sites).  The complex vector is a + ib with
random signs a, b; the real one is a.  A call-time step records, host clock around calls that end in a synchronise, one warm-up
call of each first and then the two in turn:
  rdm_z     eigenex_spin_rdm_z into a preallocated array (the download of the packed pairs is part of the call)
  rdm       eigenex_spin_rdm of the real vector on the real operator, likewise
  baseline  what a user does without it, once: SpinTimeEvolutionSolver.state()'s route -- download the complex vector, take the
            sector's states, group the rows by their A word (one stable argsort) and multiply M M^H block by block with numpy
The two routes are compared entry by entry.  --kernels-only makes the same calls and nothing else, for the kernel trace; the
kernel time of a call is the sum over the tile kernels (64-row and 16-row) and the reduce kernel of that call, from the trace's
statistics.  --resources takes the compiler's -Rpass-analysis=kernel-resource-usage remarks of csrc/kernels.hip.  No threshold is
asserted anywhere: none of these numbers existed before."""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time
from math import comb

sys.path.insert(0, ".")
import numpy as np

CUTS = ("low2", "high2", "low4", "high4", "half")
SHAPES = ((24, 12), (28, 14))


def pair(text):
    L, k = text.split(":")
    return int(L), int(k)


def mask_of(L, cut):
    nA = {"low2": 2, "high2": 2, "low4": 4, "high4": 4, "half": L // 2}[cut]
    low = (1 << nA) - 1
    return low << (L - nA) if cut.startswith("high") else low


def extract(states, mask):
    """the word of the mask's bits of every state (bit j = the j-th lowest set bit of the mask)"""
    w, j = np.zeros(states.size, np.uint32), 0
    for p in range(32):
        if (mask >> p) & 1:
            w |= ((states >> np.uint32(p)) & np.uint32(1)) << np.uint32(j)
            j += 1
    return w


def numpy_route(capi, b, L, n_up, mask):
    """[(k, rho_k)] from the downloaded complex vector"""
    x = b.download(capi.VEC_COL(0))
    states = capi.spin_sector_states(L, n_up)
    nA = bin(mask).count("1")
    a = extract(states, mask)
    order = np.argsort(a, kind="stable")  # for one A word the rows come in ascending B word: the columns of M
    xs = x[order]
    counts = np.bincount(a, minlength=1 << nA)
    start = np.concatenate([[0], np.cumsum(counts)])
    out = []
    for k in range(max(0, n_up - (L - nA)), min(nA, n_up) + 1):
        words = [w for w in range(1 << nA) if bin(w).count("1") == k]
        M = np.stack([xs[start[w] : start[w + 1]] for w in words])
        out.append((k, M @ M.conj().T))
    return out


def set_up(capi, L, n_up):
    n = capi.spin_sector_dim(L, n_up)
    bonds = [(i, (i + 1) % L, 1.0, 1.0) for i in range(L)]
    ctx = capi.Context()
    R, Z = capi.Csr.spin_half_sector(ctx, L, n_up, bonds), capi.Csr.spin_half_sector(ctx, L, n_up, bonds, complex_states=True)
    br, bz = capi.Basis(ctx, R, n, 1), capi.Basis(ctx, Z, n, 1)
    br.random_signs(capi.VEC_COL(0), 1, 0)
    a = br.download(capi.VEC_COL(0))
    rs = np.random.RandomState(7)
    z = a + 1j * (2.0 * rs.randint(0, 2, n) - 1.0)
    bz.upload(capi.VEC_COL(0), z)
    del a, z
    return ctx, R, Z, br, bz, n


def step(args):
    from cmpt_eigenex_amd import capi

    L, n_up = args.sector
    mask = mask_of(L, args.cut)
    kf, dims, offs = capi.spin_rdm_layout(L, n_up, mask)
    nA = bin(mask).count("1")
    fmas = sum(d * (d + 1) // 2 * comb(L - nA, n_up - (kf + i)) for i, d in enumerate(dims))  # of the real call; the complex one has four times as many
    ctx, R, Z, br, bz, n = set_up(capi, L, n_up)
    out_r, out_z = np.zeros(offs[-1]), np.zeros(2 * offs[-1])
    pr, pz = out_r.ctypes.data_as(capi._dp), out_z.ctypes.data_as(capi._dp)

    def rdm():
        rc = capi.lib().eigenex_spin_rdm(br.h, capi.VEC_COL(0), mask, pr, out_r.size)
        assert rc == 0, capi.lib().eigenex_last_error()

    def rdm_z():
        rc = capi.lib().eigenex_spin_rdm_z(bz.h, capi.VEC_COL(0), mask, pz, out_z.size)
        assert rc == 0, capi.lib().eigenex_last_error()

    rdm()
    rdm_z()
    t_r, t_z = [], []
    for _ in range(args.repeats):
        for fn, into in ((rdm_z, t_z), (rdm, t_r)):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            into.append(time.perf_counter() - t0)
    if args.kernels_only:
        print(json.dumps(dict(L=L, n_up=n_up, cut=args.cut, calls_each=args.repeats + 1)), flush=True)
        for h in (br, bz, R, Z, ctx):
            h.close()
        return
    t0 = time.perf_counter()
    ref = numpy_route(capi, bz, L, n_up, mask)
    t_base = time.perf_counter() - t0
    worst = 0.0
    zz = out_z.view(np.complex128)
    for i, (k, m) in enumerate(ref):
        got = zz[offs[i] : offs[i + 1]].reshape(dims[i], dims[i]).T
        assert k == kf + i and m.shape == got.shape
        worst = max(worst, float(np.abs(got - m).max()))
    rec = dict(kind="calls", L=L, n_up=n_up, cut=args.cut, mask=mask, rows=n, nA=nA, blocks=len(dims), largest_block=max(dims), out_doubles=int(2 * offs[-1]),
               fmas_real=fmas, rdm_z_ms=[t * 1e3 for t in t_z], rdm_ms=[t * 1e3 for t in t_r], baseline_ms=t_base * 1e3, largest_difference=worst,
               trace=float(sum(np.trace(m).real for _, m in ref)))
    print(json.dumps(rec), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    for h in (br, bz, R, Z, ctx):
        h.close()


def short(name):
    """'void eigenex::(anonymous namespace)::k_spin_rdm<true, 64, eigenex::SpinZ>(...)' -> 'k_spin_rdm<SpinZ>': the kernel and the
    element of the vector, SpinZ or double"""
    name = name.strip()
    name = name[5:] if name.startswith("void ") else name
    name = name.replace("eigenex::(anonymous namespace)::", "").replace("eigenex::", "")
    head = name.split("(")[0]
    return re.split(r"[<(]", name)[0].strip() + ("<SpinZ>" if "SpinZ" in head else "<double>")


def kernel_stats(args):
    """the newest *_kernel_stats.csv under the directory: total time of the four kernel names over the calls made"""
    L, n_up = args.sector
    files = sorted(glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    assert files, "no kernel statistics under " + args.kernel_stats
    total, calls = {}, {}
    for r in csv.DictReader(open(files[-1])):
        k = short(r["Name"])
        if k.startswith("k_spin_rdm"):
            total[k] = total.get(k, 0.0) + float(r["TotalDurationNs"])
            calls[k] = calls.get(k, 0) + int(r["Calls"])
    n_calls = calls.get("k_spin_rdm_reduce<SpinZ>", 0)
    assert n_calls > 0 and calls.get("k_spin_rdm_reduce<double>", 0) == n_calls, calls
    rec = dict(kind="kernels", L=L, n_up=n_up, cut=args.cut, calls_each=n_calls,
               tiles_z_ms=total.get("k_spin_rdm<SpinZ>", 0.0) / n_calls * 1e-6, reduce_z_ms=total["k_spin_rdm_reduce<SpinZ>"] / n_calls * 1e-6,
               tiles_ms=total.get("k_spin_rdm<double>", 0.0) / n_calls * 1e-6, reduce_ms=total["k_spin_rdm_reduce<double>"] / n_calls * 1e-6)
    print(json.dumps(rec), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def resources(path):
    """[(kernel, SECTOR, TILE, VGPRs, scratch bytes, spilled VGPRs, LDS bytes, waves/SIMD)] of k_spin_rdm<SECTOR, TILE, E> for
    E = double and SpinZ from the compiler's remarks"""
    rows, cur = [], None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            t = re.match(r"_ZN7eigenex12_GLOBAL__N_1\d+(k_spin_rdm)ILb([01])ELi(\d+)E(d|NS_5SpinZE)EE", m.group(1))
            cur = dict(kernel=t.group(1) + ("<double>" if t.group(4) == "d" else "<SpinZ>"), sector=int(t.group(2)), tile=int(t.group(3))) if t else None
            if cur is not None:
                rows.append(cur)
            continue
        if cur is None:
            continue
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return rows


def write_profile(args):
    recs = [json.loads(line) for line in open(args.out) if line.strip()] if os.path.exists(args.out) else []
    calls = {(r["L"], r["n_up"], r["cut"]): r for r in recs if r.get("kind") == "calls"}
    kern = {(r["L"], r["n_up"], r["cut"]): r for r in recs if r.get("kind") == "kernels"}
    want = [(L, k, cut) for (L, k) in SHAPES for cut in CUTS]
    med = lambda v: float(np.median(v))  # noqa: E731
    lines = ["# Reduced density matrix of a complex state: `eigenex_spin_rdm_z` beside `eigenex_spin_rdm`", ""]
    if args.resources:
        lines += ["## What the compiler made", "",
                  "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `csrc/kernels.hip` (no GPU needed).  No instantiation",
                  "uses scratch.  The waves per SIMD are the compiler's figure (registers and LDS together).", "",
                  "| kernel | `SECTOR` | `TILE` | VGPRs | scratch bytes per lane | spilled VGPRs | LDS bytes per workgroup | waves per SIMD |", "|---|---|---|---|---|---|---|---|"]
        for r in sorted(resources(args.resources), key=lambda r: (r["kernel"], -r["tile"], -r["sector"])):
            lines.append(f"| `{r['kernel']}` | {bool(r['sector'])} | {r['tile']} | {r['vgprs']} | {r['scratch']} | {r['spill']} | {r['lds']:,} | {r['waves']} |")
        lines.append("")
    lines += ["## Kernel and call times", "",
              "`scripts/probe_spin_entanglement_z.py` on one MI355X, one process per shape, periodic Heisenberg chain in the sector `(L, n_up)`: a complex",
              "vector `a + ib` of random signs on the operator for complex states and the real vector `a` on the real operator, in the same process.",
              "Kernel times: `rocprofv3 --kernel-trace --stats` in a run of its own, tile kernels + reduce kernel per call, mean over the calls of that",
              "run.  Call times: host clock around calls that end in a synchronise (the download of the packed result is part of the call), one warm-up",
              "call of each, then the two in turn, with the profiler off; median (min – max) in ms.  Expectation from the code alone: about 2× the real",
              "kernel where the gather dominates (16 instead of 8 bytes per element), up to 4× on the half cut (four fmas instead of one).", "",
              "| `(L, n_up)` | cut | blocks, largest | `k_spin_rdm<SpinZ>` + reduce | `k_spin_rdm<double>` + reduce | kernel ratio | `rdm_z` call | `rdm` call | call ratio | download + numpy | largest difference |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    missing_calls, missing_kern, notes = [], [], []
    for key in want:
        c, k = calls.get(key), kern.get(key)
        if c is None:
            missing_calls.append(key)
        if k is None:
            missing_kern.append(key)
        if c is None and k is None:
            continue
        kz = k["tiles_z_ms"] + k["reduce_z_ms"] if k else None
        kr = k["tiles_ms"] + k["reduce_ms"] if k else None
        cells = [f"({key[0]},{key[1]})", key[2], f"{c['blocks']}, {c['largest_block']}" if c else "",
                 f"{kz:.3f} ({k['tiles_z_ms']:.3f} + {k['reduce_z_ms']:.3f})" if k else "not measured",
                 f"{kr:.3f} ({k['tiles_ms']:.3f} + {k['reduce_ms']:.3f})" if k else "not measured", f"{kz / kr:.2f}" if k else ""]
        if c:
            tz, tr = c["rdm_z_ms"], c["rdm_ms"]
            cells += [f"{med(tz):.2f} ({min(tz):.2f} – {max(tz):.2f})", f"{med(tr):.2f} ({min(tr):.2f} – {max(tr):.2f})", f"{med(tz) / med(tr):.2f}", f"{c['baseline_ms']:.0f}",
                      f"{c['largest_difference']:.1e}"]
            if key[2] == "half":
                spread = (max(tz) - min(tz)) / med(tz) + (max(tr) - min(tr)) / med(tr)
                ratio = kz / kr if k else med(tz) / med(tr)
                notes.append(f"Half cut at ({key[0]},{key[1]}): the {'kernel' if k else 'call'} ratio is {ratio:.2f}; the calls of that shape have a relative spread of {spread:.2f}" +
                             (": above 4× by more than the spread; the 64-row complex kernel holds 3 waves per SIMD where the real one holds 4 (table above)." if ratio > 4 * (1 + spread) else ": not above 4× by more than the spread."))
        else:
            cells += ["not measured"] * 5
        lines.append("| " + " | ".join(cells) + " |")
    name = lambda keys: ", ".join(f"({L},{k}) {cut}" for (L, k, cut) in keys)  # noqa: E731
    gaps = (f"call times of {name(missing_calls)}; " if missing_calls else "") + (f"kernel times of {name(missing_kern)}; " if missing_kern else "")
    lines += [""] + notes + ["", f"Not measured: {gaps}`(30,15)` and `(32,16)`; a full-space operator; "
                                  "any hardware counter of `k_spin_rdm<SpinZ>` (LDS bank conflicts among them: the panel layout is derived from the bank rule, not counted); the spread between processes and machines."]
    with open(args.write_profile, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


ap = argparse.ArgumentParser()
ap.add_argument("--sector", type=pair, default=(24, 12))
ap.add_argument("--cut", choices=CUTS, default="low2")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default="spin_entanglement_z.jsonl")
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--resources", default=None)
ap.add_argument("--write-profile", default=None)
args = ap.parse_args()
if args.write_profile:
    write_profile(args)
elif args.kernel_stats:
    kernel_stats(args)
else:
    step(args)
