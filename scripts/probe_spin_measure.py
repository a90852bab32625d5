"""All pairs and all sites of one vector of the periodic spin-1/2 Heisenberg chain in the sector of n_up sites up, two ways, in
one process per run:
  (a) one eigenex_spin_measure: L site masks and L (L - 1) / 2 pair masks on the diagonal list, the pair masks on the flip list
      -- <Sz_i>, <Sz_i Sz_j> and <Sx_i Sx_j + Sy_i Sy_j> of every site and pair;
  (b) the route without it: per pair one single-bond operator handle (Jz = Jxy = 1), a state on it, and one eigenex_apply with
      its dot -- <S_i.S_j> alone, without the split into zz and xy and without the sites, which favours this route.
Host clock around the calls; both end in a synchronise.  For (b) the time of the applications alone and the time with the
handles, states and uploads of the vector are printed separately.  The two routes are compared pair by pair.
usage: python scripts/probe_spin_measure.py [--sectors 24:12 28:14] [--repeats 3]"""
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
ap.add_argument("--sectors", type=pair, nargs="+", default=[(24, 12), (28, 14)])
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

ctx = capi.Context()

for (L, n_up) in args.sectors:
    n = capi.spin_sector_dim(L, n_up)
    tag = f"({L},{n_up})"
    pairs = [(i, j) for i in range(L) for j in range(i + 1, L)]
    pair_masks = [(1 << i) | (1 << j) for (i, j) in pairs]
    diag_masks = [1 << i for i in range(L)] + pair_masks
    print(f"{tag}: {n} rows, vector {8 * n / 1e9:.2f} GB, {L} sites, {len(pairs)} pairs", flush=True)
    S = capi.Csr.spin_half_sector(ctx, L, n_up, [(i, (i + 1) % L, 1.0, 1.0) for i in range(L)])
    b = capi.Basis(ctx, S, n, 1)
    b.random_signs(capi.VEC_COL(0), 1, 0)
    b.spin_measure(capi.VEC_COL(0), diag_masks[:1], pair_masks[:1])  # first launches
    fused = []
    for rep in range(args.repeats):
        ctx.sync()
        t0 = time.perf_counter()
        diag, flip, norm2 = b.spin_measure(capi.VEC_COL(0), diag_masks, pair_masks)
        fused.append(time.perf_counter() - t0)
        print(f"{tag} rep {rep} eigenex_spin_measure, {len(diag_masks)} + {len(pair_masks)} terms: {fused[-1] * 1e3:10.2f} ms", flush=True)
    dots = (diag[L:] / 4 + flip / 2) / norm2
    x = b.download(capi.VEC_COL(0))
    b.close()
    old_apply, old_total = [], []
    for rep in range(args.repeats):
        t_apply, t_all, worst = 0.0, time.perf_counter(), 0.0
        for k, (i, j) in enumerate(pairs):
            B = capi.Csr.spin_half_sector(ctx, L, n_up, [(i, j, 1.0, 1.0)])
            bb = capi.Basis(ctx, B, n, 1)
            bb.upload(capi.VEC_COL(0), x)
            ctx.sync()
            t0 = time.perf_counter()
            dot = bb.apply(capi.VEC_COL(0), capi.VEC_V, 0.0, want_dot=True)
            t_apply += time.perf_counter() - t0
            worst = max(worst, abs(dot / norm2 - dots[k]))
            bb.close()
            B.close()
        old_apply.append(t_apply)
        old_total.append(time.perf_counter() - t_all)
        print(f"{tag} rep {rep} one handle and one eigenex_apply per pair: applications {t_apply * 1e3:10.2f} ms, with handles, states and uploads "
              f"{old_total[-1] * 1e3:10.2f} ms; largest difference of <S_i.S_j> between the routes {worst:.3e}", flush=True)
    f, a = np.array(fused), np.array(old_apply)
    print(f"{tag}: fused median {np.median(f) * 1e3:.2f} ms (min {f.min() * 1e3:.2f}, max {f.max() * 1e3:.2f}); per-pair applications median {np.median(a) * 1e3:.2f} ms "
          f"(min {a.min() * 1e3:.2f}, max {a.max() * 1e3:.2f}); ratio of the medians {np.median(a) / np.median(f):.2f}", flush=True)
    S.close()
ctx.close()
