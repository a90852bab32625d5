"""The reduced density matrix of one random-sign vector of the periodic spin-1/2 Heisenberg chain in the sector (L, n_up), one
shape per process:

    python scripts/probe_spin_entanglement.py --sector 28:14 --cut low2 --out results.jsonl     (one step; run it under `timeout`)
    python scripts/probe_spin_entanglement.py --write-profile profiles/spin_entanglement.md --out results.jsonl   (no GPU)

Cuts: low2, low4 (the lowest sites), high2, high4 (the highest), half (the lowest L / 2 sites).  A step records, host clock around
calls that end in a synchronise, one warm-up call first:
  rdm       eigenex_spin_rdm into a preallocated array (the download of the packed result is part of the call)
  sweep     a one-chunk eigenex_spin_measure (16 site masks, 16 pair masks) of the same vector from the same process: the
            streaming yardstick that already exists
  download  eigenex_vec_download of the vector into an array that has been written before (median of the repeats)
  baseline  what a user does without it: download the vector, take the sector's states (eigenex_spin_sector_states), split
            every state into its A word, group the rows by it (one stable argsort) and multiply M M^T block by block with numpy
and, for the half cut, the fp64 FMA rate with the FMA count sum_k d_k (d_k + 1) / 2 * C(nB, n_up - k).  The two routes are compared
entry by entry.  No threshold is asserted anywhere: none of these numbers existed before."""
import argparse
import json
import sys
import time
from math import comb

sys.path.insert(0, ".")
import numpy as np


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
    """[(k, rho_k)] from the downloaded vector"""
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
        out.append((k, M @ M.T))
    return out


def step(args):
    from cmpt_eigenex_amd import capi

    L, n_up = args.sector
    mask = mask_of(L, args.cut)
    n = capi.spin_sector_dim(L, n_up)
    kf, dims, offs = capi.spin_rdm_layout(L, n_up, mask)
    nA = bin(mask).count("1")
    fmas = sum(d * (d + 1) // 2 * comb(L - nA, n_up - (kf + i)) for i, d in enumerate(dims))
    ctx = capi.Context()
    S = capi.Csr.spin_half_sector(ctx, L, n_up, [(i, (i + 1) % L, 1.0, 1.0) for i in range(L)])
    b = capi.Basis(ctx, S, n, 1)
    b.random_signs(capi.VEC_COL(0), 1, 0)
    out = np.zeros(offs[-1])
    dp = out.ctypes.data_as(capi._dp)

    def rdm():
        rc = capi.lib().eigenex_spin_rdm(b.h, capi.VEC_COL(0), mask, dp, out.size)
        assert rc == 0, capi.lib().eigenex_last_error()

    sites = [1 << i for i in range(16)]
    pairs = [(1 << i) | (1 << ((i + 1) % L)) for i in range(16)]
    rdm()
    b.spin_measure(capi.VEC_COL(0), sites, pairs)
    t_rdm, t_sweep = [], []
    for _ in range(args.repeats):
        ctx.sync()
        t0 = time.perf_counter()
        rdm()
        t_rdm.append(time.perf_counter() - t0)
        ctx.sync()
        t0 = time.perf_counter()
        b.spin_measure(capi.VEC_COL(0), sites, pairs)
        t_sweep.append(time.perf_counter() - t0)
    warm, t_down = np.zeros(n), []  # a download into pages that exist, as the packed result's are after the warm-up call
    for _ in range(args.repeats + 1):
        ctx.sync()
        t0 = time.perf_counter()
        assert capi.lib().eigenex_vec_download(b.h, capi.VEC_COL(0), warm.ctypes.data_as(capi._dp)) == 0
        t_down.append(time.perf_counter() - t0)
    t_down = float(np.median(t_down[1:]))
    t0 = time.perf_counter()
    ref = numpy_route(capi, b, L, n_up, mask)
    t_base = time.perf_counter() - t0
    worst = 0.0
    for i, (k, m) in enumerate(ref):
        got = out[offs[i] : offs[i + 1]].reshape(dims[i], dims[i]).T
        assert k == kf + i and m.shape == got.shape
        worst = max(worst, float(np.abs(got - m).max()))
    rec = dict(L=L, n_up=n_up, cut=args.cut, mask=mask, rows=n, nA=nA, blocks=len(dims), largest_block=max(dims), out_doubles=int(offs[-1]), fmas=fmas,
               rdm_ms=[t * 1e3 for t in t_rdm], sweep_ms=[t * 1e3 for t in t_sweep], baseline_ms=t_base * 1e3, download_ms=t_down * 1e3, largest_difference=worst,
               trace=float(sum(np.trace(m) for _, m in ref)))
    print(json.dumps(rec), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    for h in (b, S, ctx):
        h.close()


def write_profile(args):
    recs = [json.loads(line) for line in open(args.out) if line.strip()]
    want = [(L, k, cut) for (L, k) in ((24, 12), (28, 14)) for cut in ("low2", "high2", "low4", "high4", "half")]
    have = {(r["L"], r["n_up"], r["cut"]): r for r in recs}
    med = lambda v: float(np.median(v))  # noqa: E731
    lines = ["# Reduced density matrix of a state: `eigenex_spin_rdm` against a `spin_measure` sweep and against numpy", "",
             "`scripts/probe_spin_entanglement.py` on one MI355X, one process per shape, periodic Heisenberg chain, a random-sign vector in",
             "the sector `(L, n_up)`; host clock around calls that end in a synchronise; one warm-up call, then the repeats of `eigenex_spin_rdm`",
             "and of a one-chunk `eigenex_spin_measure` (16 site and 16 pair masks) in turn, then the numpy route once.  `rdm` includes the",
             "download of the packed result.  `low` cuts own the lowest sites (the rows of a 64-row panel run along the lanes of the gather), `high`",
             "cuts the highest (the b's do, as in every 16-row panel).  Median (min – max) in ms.", "",
             "| `(L, n_up)` | cut | rows | blocks, largest | `rdm` | one-chunk sweep | `rdm` / sweep | download + numpy | largest difference |", "|---|---|---|---|---|---|---|---|---|"]
    missing = []
    for key in want:
        r = have.get(key)
        if r is None:
            missing.append(key)
            continue
        t, s = r["rdm_ms"], r["sweep_ms"]
        lines.append(f"| ({r['L']},{r['n_up']}) | {r['cut']} (nA = {r['nA']}) | {r['rows']:,} | {r['blocks']}, {r['largest_block']} | {med(t):.2f} ({min(t):.2f} – {max(t):.2f}) | "
                     f"{med(s):.2f} ({min(s):.2f} – {max(s):.2f}) | {med(t) / med(s):.1f} | {r['baseline_ms']:.0f} | {r['largest_difference']:.1e} |")
    lines += ["", "Half cuts, the achieved fp64 FMA rate with the FMA count `Σ_k d_k (d_k + 1) / 2 · C(nB, n_up − k)` (the lower triangle alone; the", "kernel computes whole 64 × 64 tiles, so it executes more).  At a half cut the packed output has exactly as many doubles as the vector",
              "(`Σ_k C(L/2, k)² = C(L, L/2)`), so a download of the vector into an array whose pages exist, timed in the same process, estimates the download inside the call:", "",
              "| `(L, n_up)` | FMAs | packed output | `rdm` median | download of the vector | GFMA/s of the call | GFMA/s without the download (estimate) |", "|---|---|---|---|---|---|---|"]
    for key in want:
        r = have.get(key)
        if r is not None and r["cut"] == "half":
            t = med(r["rdm_ms"]) * 1e-3
            dn = r["download_ms"] * 1e-3
            rest = f"{r['fmas'] / (t - dn) / 1e9:.1f}" if t > dn else "n/a"
            lines.append(f"| ({r['L']},{r['n_up']}) | {r['fmas']:.3e} | {8 * r['out_doubles'] / 1e6:.1f} MB | {t * 1e3:.2f} ms | {dn * 1e3:.2f} ms | {r['fmas'] / t / 1e9:.1f} | {rest} |")
    lines += ["", "Not taken: " + (", ".join(f"({L},{k}) {cut}" for (L, k, cut) in missing) if missing else "none of the shapes above") +
              "; `(30,15)` and `(32,16)`; a full-space operator; any hardware counter of `k_spin_rdm`; the spread between processes and boxes."]
    with open(args.write_profile, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


ap = argparse.ArgumentParser()
ap.add_argument("--sector", type=pair, default=(24, 12))
ap.add_argument("--cut", choices=["low2", "high2", "low4", "high4", "half"], default="low2")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default="spin_entanglement.jsonl")
ap.add_argument("--write-profile", default=None)
args = ap.parse_args()
write_profile(args) if args.write_profile else step(args)
