// Hand-written gfx950 (CDNA4, wave64) kernels for the Krylov inner loop.
//
// Reference operations realised here:
//   a1/a2/a3  v_ = A*u (+shift*u), alpha = u.v          lanczos.hpp:389-395, :442-448; arnoldi.hpp:333-336, :369-372
//   a4        w = v_ - alpha_k u_k - beta_{k-1} u_{k-1}  lanczos.hpp:403-408
//   a5        Gram-Schmidt dots + updates                lanczos.hpp:143-146, :416-425; arnoldi.hpp:96-99, :380-383
//   a6        beta = ||w||, residue = ||v_||             lanczos.hpp:429; arnoldi.hpp:348, :385
//   a7        u_{k+1} = w/beta, q_k = v_/residue         lanczos.hpp:439; arnoldi.hpp:365
//
// Every kernel is HBM-bound (<= 0.25 flop/byte): no MFMA.  Design rules applied:
// 16-byte loads (double2) with consecutive lanes on consecutive addresses, several
// independent loads in flight per lane, wave64 __shfl_down reductions, per-wave LDS
// accumulators, fixed-order second-stage reductions (bit-reproducible, no float
// atomics), persistent grids that walk the rows as one frontier so operator-input
// re-reads are served by L2 / Infinity Cache.
#include "kernels.hpp"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace eigenex {

namespace {

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;  // lane 0 holds the sum
}

// Sum over the 256-thread block in a fixed order; every thread gets the result.
__device__ __forceinline__ double block_sum(double x, double* lds4) {
  x = wave_sum(x);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) lds4[wave] = x;
  __syncthreads();
  return (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
}

// InlineFin, shared part: the same sum as k_reduce_fin (strided per-thread sums, then block_sum), in every workgroup
__device__ __forceinline__ double inline_fin_sum(const InlineFin& f, double* lds4) {
  double s = 0.0;
  for (int b = threadIdx.x; b < f.nblocks; b += kBlock) s += f.partials[b];
  return block_sum(s, lds4);
}

// add_product_nofma (a + b*c, the product rounded first): spmv_index.hpp

// One row of a Chebyshev step (kernels.hpp: ChebStep), every product rounded before it is added: returns t_next, *acc_out = acc
__device__ __forceinline__ double cheb_row_nofma(double a, double t_prev, double acc, const ChebStep& ch, double* acc_out) {
#pragma clang fp contract(off)
  const double ca = ch.c * a;
  const double t = ch.first ? ca : ca - t_prev;
  const double head = ch.first ? ch.mu0 * t_prev : acc;
  const double term = ch.mu * t;
  *acc_out = head + term;
  return t;
}

__device__ __forceinline__ void fin_norm_apply(Ctrl* ctrl, double nrm2, double threshold, int mode, double* beta);
__device__ __forceinline__ void fin_alpha_apply(Ctrl* ctrl, double val, double* alpha, int first);

__device__ __forceinline__ double2 ld2(const double* p) { return *reinterpret_cast<const double2*>(p); }
__device__ __forceinline__ void st2(double* p, double2 v) { *reinterpret_cast<double2*>(p) = v; }

// Once-read streams -- the basis columns in k_dots / k_update / k_ritz, the split tiles' values -- use non-temporal 16-byte loads,
// and the vectors a kernel writes in full (w in k_update, y and u in k_spmv) non-temporal stores: they do not displace the
// operator input and the work vectors from L2 / Infinity Cache, and the HBM streams themselves run faster (r3, same box:
// 512^3 46.99/47.42 -> 49.43/49.49 it/s with the loads, 49.67 with the stores; 128^3 4,059 -> 4,444; config 3 3,218 -> 3,349).
// NOT the three-term inputs of load_w0 (v, u_k, u_{k-1}): measured 3 % slower in k_dots with nt; and in k_spmv the val/col
// loads are non-temporal only on request (flag bit 1): 13 % slower on the 512^3 stencil.
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef double v2d_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int4 nt_ld_i4(const int32_t* p) {
  const v4i_t v = __builtin_nontemporal_load(reinterpret_cast<const v4i_t*>(p));
  return make_int4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ double2 nt_ld_d2(const double* p) {
  const v2d_t v = __builtin_nontemporal_load(reinterpret_cast<const v2d_t*>(p));
  return make_double2(v.x, v.y);
}
__device__ __forceinline__ void nt_st2(double* p, double2 v) {
  v2d_t t;
  t.x = v.x, t.y = v.y;
  __builtin_nontemporal_store(t, reinterpret_cast<v2d_t*>(p));
}

__device__ __forceinline__ const double* column_ptr(const ColumnSet& cs, int ci) {
  return ci < cs.count ? cs.V + (int64_t)(cs.first + ci * cs.stride) * cs.ldv
                       : cs.Q + (int64_t)(ci - cs.count) * cs.ldq;
}

// w0 for the 8 rows of this thread in tile `base`: src, or the three-term
// recurrence (src - a*u_k) - b*u_{k-1} evaluated with explicit fma so that the
// dots kernel and the update kernel produce bit-identical w0.
template <bool FULL>
__device__ __forceinline__ void load_w0(double2 (&w)[4], const double* src, const ThreeTerm& tt,
                                        double a, double b, int64_t base, int64_t n, double2 (*keep_uk)[4] = nullptr,
                                        double2 (*keep_ukm1)[4] = nullptr) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = base + i * (2 * kBlock);
    double2 u = make_double2(0.0, 0.0), um = make_double2(0.0, 0.0);
    if (FULL || row < n) {
      double2 s = ld2(src + row);
      if (tt.uk) {
        u = ld2(tt.uk + row);
        s.x = fma(-a, u.x, s.x);
        s.y = fma(-a, u.y, s.y);
        if (tt.ukm1) {
          um = ld2(tt.ukm1 + row);
          s.x = fma(-b, um.x, s.x);
          s.y = fma(-b, um.y, s.y);
        }
      }
      w[i] = s;
    } else {
      w[i] = make_double2(0.0, 0.0);
    }
    if (keep_uk) (*keep_uk)[i] = u;
    if (keep_ukm1) (*keep_ukm1)[i] = um;
  }
}

// The three-term vectors u_k, u_{k-1} are also the last two basis columns of a full
// re-orthogonalisation pass (columns 0..k): their tiles are taken from the registers / caches that
// formed w0 instead of being streamed from HBM a second time (2 of j+3 column reads per pass).
__device__ __forceinline__ int tail_columns(const ThreeTerm& tt, const ColumnSet& cs) {
  if (!tt.uk || cs.stride != 1 || cs.count < 1) return 0;
  const double* last = cs.V + (int64_t)(cs.first + cs.count - 1) * cs.ldv;
  if (last != tt.uk) return 0;
  if (tt.ukm1 && cs.count >= 2 && tt.ukm1 == last - cs.ldv) return 2;
  return 1;
}

template <bool FULL>
__device__ __forceinline__ void load_col(double2 (&x)[4], const double* __restrict__ p, int64_t base, int64_t n) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = base + i * (2 * kBlock);
    x[i] = (FULL || row < n) ? nt_ld_d2(p + row) : make_double2(0.0, 0.0);
  }
}

// ---------------------------------------------------------------------------
// dots: partial h_c = sum_rows conj(col_c[row]) * w0[row] for every selected column.
// One pass over the selected part of the slab; 16 x 16-B loads in flight per lane.
// All lengths are in doubles: a complex vector of N entries is 2N interleaved doubles
// and one double2 load is one complex entry (CPLX) or two real rows.  The three-term
// recurrence has real coefficients (lanczos.hpp:403-408), so w0 is formed the same way.
// ---------------------------------------------------------------------------
template <bool CPLX>
__device__ __forceinline__ void dotc8(const double2 (&w)[4], const double2 (&x)[4], double& sr, double& si) {
  sr = 0.0;
  si = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    sr = fma(x[i].x, w[i].x, sr);
    sr = fma(x[i].y, w[i].y, sr);
    if (CPLX) {  // conj(x) * w, imaginary part
      si = fma(x[i].x, w[i].y, si);
      si = fma(-x[i].y, w[i].x, si);
    }
  }
}

// Sums four per-lane values (one per column) over the wave with 7 shuffle+add steps instead of
// 4 x 6: halves are swapped pairwise (offsets 32, 16) so that afterwards the 16-lane group g holds
// column g, then a 4-step butterfly inside the group.  Every lane of group g returns column g's sum.
__device__ __forceinline__ double wave_sum4(double s0, double s1, double s2, double s3, int lane) {
  const bool up = (lane & 32) != 0;
  double keep0 = up ? s2 : s0, keep1 = up ? s3 : s1;
  const double send0 = up ? s0 : s2, send1 = up ? s1 : s3;
  keep0 += __shfl_xor(send0, 32, 64);
  keep1 += __shfl_xor(send1, 32, 64);
  const bool up2 = (lane & 16) != 0;
  double k = up2 ? keep1 : keep0;
  const double snd = up2 ? keep0 : keep1;
  k += __shfl_xor(snd, 16, 64);
  k += __shfl_xor(k, 8, 64);
  k += __shfl_xor(k, 4, 64);
  k += __shfl_xor(k, 2, 64);
  k += __shfl_xor(k, 1, 64);
  return k;
}

// DUAL: a second source vector src2 (no recurrence) is dotted with the same column tiles in the same pass; its sums go
// to wave_acc2.  Used by the fused-alpha Lanczos step (library.hip: lanczos_call), where the Gram column V^H u_k is needed
// next to V^H v; the column tiles are loaded once for both.
template <bool FULL, bool CPLX, bool RED4, bool DUAL>
__device__ __forceinline__ void dots_tile(const double* __restrict__ src, const ThreeTerm& tt, double a, double b,
                                          const double* __restrict__ src2, const ColumnSet& cs, int ncols, int64_t base,
                                          int64_t n, double* wave_acc, double* wave_acc2) {
  constexpr int ES = CPLX ? 2 : 1;
  const int lane = threadIdx.x & 63;
  double2 w[4], w2[4];
  load_w0<FULL>(w, src, tt, a, b, base, n);
  if (DUAL) load_col<FULL>(w2, src2, base, n);
  // columns are visited from the last one down: with full re-orthogonalisation the first group then
  // contains u_k and u_{k-1}, whose tiles load_w0 has just pulled through L1/L2 (no second HBM read);
  // every h_c is an independent sum, so the order does not touch the results.
  auto add4 = [&](double* acc, int ci, double r0, double r1, double r2, double r3, double i0, double i1, double i2, double i3) {
    if (RED4) {
      const double kr = wave_sum4(r0, r1, r2, r3, lane);
      double ki = 0.0;
      if (CPLX) ki = wave_sum4(i0, i1, i2, i3, lane);
      if ((lane & 15) == 0) {
        acc[ES * (ci + (lane >> 4))] += kr;
        if (CPLX) acc[ES * (ci + (lane >> 4)) + 1] += ki;
      }
      return;
    }
    r0 = wave_sum(r0);
    r1 = wave_sum(r1);
    r2 = wave_sum(r2);
    r3 = wave_sum(r3);
    if (CPLX) {
      i0 = wave_sum(i0);
      i1 = wave_sum(i1);
      i2 = wave_sum(i2);
      i3 = wave_sum(i3);
    }
    if (lane == 0) {
      acc[ES * (ci + 0)] += r0;
      acc[ES * (ci + 1)] += r1;
      acc[ES * (ci + 2)] += r2;
      acc[ES * (ci + 3)] += r3;
      if (CPLX) {
        acc[ES * (ci + 0) + 1] += i0;
        acc[ES * (ci + 1) + 1] += i1;
        acc[ES * (ci + 2) + 1] += i2;
        acc[ES * (ci + 3) + 1] += i3;
      }
    }
  };
  const int rem = ncols & 3;
  for (int ci = ncols - 4; ci >= 0; ci -= 4) {
    double2 x0[4], x1[4], x2[4], x3[4];
    load_col<FULL>(x3, column_ptr(cs, ci + 3), base, n);
    load_col<FULL>(x2, column_ptr(cs, ci + 2), base, n);
    load_col<FULL>(x1, column_ptr(cs, ci + 1), base, n);
    load_col<FULL>(x0, column_ptr(cs, ci + 0), base, n);
    double r0, r1, r2, r3, i0, i1, i2, i3;
    dotc8<CPLX>(w, x0, r0, i0);
    dotc8<CPLX>(w, x1, r1, i1);
    dotc8<CPLX>(w, x2, r2, i2);
    dotc8<CPLX>(w, x3, r3, i3);
    add4(wave_acc, ci, r0, r1, r2, r3, i0, i1, i2, i3);
    if (DUAL) {
      dotc8<CPLX>(w2, x0, r0, i0);
      dotc8<CPLX>(w2, x1, r1, i1);
      dotc8<CPLX>(w2, x2, r2, i2);
      dotc8<CPLX>(w2, x3, r3, i3);
      add4(wave_acc2, ci, r0, r1, r2, r3, i0, i1, i2, i3);
    }
  }
  for (int ci = rem - 1; ci >= 0; --ci) {
    double2 x0[4];
    load_col<FULL>(x0, column_ptr(cs, ci), base, n);
    double r0, i0;
    dotc8<CPLX>(w, x0, r0, i0);
    r0 = wave_sum(r0);
    if (CPLX) i0 = wave_sum(i0);
    if (lane == 0) {
      wave_acc[ES * ci] += r0;
      if (CPLX) wave_acc[ES * ci + 1] += i0;
    }
    if (DUAL) {
      dotc8<CPLX>(w2, x0, r0, i0);
      r0 = wave_sum(r0);
      if (CPLX) i0 = wave_sum(i0);
      if (lane == 0) {
        wave_acc2[ES * ci] += r0;
        if (CPLX) wave_acc2[ES * ci + 1] += i0;
      }
    }
  }
}

// partials[(ES*c + part)*pstride + block]; DUAL: the second source's sums in partials2, same layout
template <bool CPLX, bool RED4, bool DUAL>
__global__ __launch_bounds__(kBlock) void k_dots(const double* __restrict__ src, ThreeTerm tt, const double* __restrict__ src2,
                                                 ColumnSet cs, int64_t n, int64_t ntiles, double* __restrict__ partials,
                                                 double* __restrict__ partials2, int pstride, const Ctrl* ctrl,  // no __restrict__: fin.ctrl aliases it
                                                 InlineFin fin, InlineDecide dec) {
  extern __shared__ double lds[];  // [DUAL ? 2 : 1][4 waves][ES*ncols]
  __shared__ double lds4[4];
  if (dec.pass2) {  // this launch opens the conditional second Gram-Schmidt pass: does it run?  (k_reduce_decide, taken here)
    const bool dead = ctrl->stopped != 0;
    double s = 0.0, sb = 0.0;
    if (!dead) {
      for (int b = threadIdx.x; b < dec.after_n; b += kBlock) s += dec.after_partials[b];
      if (dec.before_partials)
        for (int b = threadIdx.x; b < dec.before_n; b += kBlock) sb += dec.before_partials[b];
    }
    s = block_sum(s, lds4);
    if (dec.before_partials) sb = block_sum(sb, lds4);
    else if (!dead) sb = *dec.nrm2_before;
    const bool again = !dead && s < dec.eta2 * sb;  // Daniel-Gragg-Kaufman-Stewart: the first pass cancelled more than half of the vector
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (!dead) {
        if (dec.before_partials) *dec.nrm2_before = sb;
        *dec.nrm2_first = s;
      }
      dec.pass2->stopped = again ? 0 : 1;
    }
    if (!again) return;
  } else if (ctrl->stopped) {
    return;
  }
  constexpr int ES = CPLX ? 2 : 1;
  const int ncols = cs.count + cs.nq;
  const int nacc = ES * ncols;
  const int wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < (DUAL ? 8 : 4) * nacc; i += kBlock) lds[i] = 0.0;
  __syncthreads();
  double a = 0.0;
  if (fin.partials) {  // alpha_k (lanczos.hpp:448) from the operator kernel's partials; workgroup 0 appends it to the series
    a = inline_fin_sum(fin, lds4);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      fin.out[0] = a;
      fin_alpha_apply(fin.ctrl, a, fin.series, fin.mode == kFinishAlphaFirst);
    }
  } else if (tt.uk) {
    a = *tt.a;
  }
  const double b = (tt.uk && tt.ukm1) ? *tt.b : 0.0;
  double* wave_acc = lds + wave * nacc;
  double* wave_acc2 = lds + (4 + wave) * nacc;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * kTileRows + 2 * threadIdx.x;
    if ((tile + 1) * kTileRows <= n)
      dots_tile<true, CPLX, RED4, DUAL>(src, tt, a, b, src2, cs, ncols, base, n, wave_acc, wave_acc2);
    else
      dots_tile<false, CPLX, RED4, DUAL>(src, tt, a, b, src2, cs, ncols, base, n, wave_acc, wave_acc2);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nacc; c += kBlock) {
    partials[(int64_t)c * pstride + blockIdx.x] = (lds[c] + lds[nacc + c]) + (lds[2 * nacc + c] + lds[3 * nacc + c]);
    if (DUAL) {
      const double* l2 = lds + 4 * nacc;
      partials2[(int64_t)c * pstride + blockIdx.x] = (l2[c] + l2[nacc + c]) + (l2[2 * nacc + c] + l2[3 * nacc + c]);
    }
  }
}

// ---------------------------------------------------------------------------
// update: dst = w0 - sum_c h_c * col_c (c ascending, the reference's order of
// subtraction), fused ||dst||^2.  Second pass over the selected part of the slab.
// ---------------------------------------------------------------------------
template <bool CPLX>
__device__ __forceinline__ void axmy8(double2 (&w)[4], const double* __restrict__ h, int ci, const double2 (&x)[4]) {
  if (!CPLX) {
    const double hr = h[ci];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[i].x = fma(-hr, x[i].x, w[i].x);
      w[i].y = fma(-hr, x[i].y, w[i].y);
    }
  } else {  // w -= (hr + i hi) * (x.x + i x.y)
    const double hr = h[2 * ci], hi = h[2 * ci + 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[i].x = fma(hi, x[i].y, fma(-hr, x[i].x, w[i].x));
      w[i].y = fma(-hi, x[i].x, fma(-hr, x[i].y, w[i].y));
    }
  }
}

template <bool FULL, bool CPLX>
__device__ __forceinline__ double update_tile(const double* src, double* dst,  // may alias (in-place update)
                                              const ThreeTerm& tt, double a, double b, const ColumnSet& cs, int ncols,
                                              int ntail, const double* __restrict__ h, int64_t base, int64_t n) {
  double2 w[4], uk[4], ukm1[4];
  load_w0<FULL>(w, src, tt, a, b, base, n, &uk, &ukm1);
  // basis columns [0, nv) stream from HBM; the last `ntail` basis columns are u_{k-1}, u_k, still in
  // registers from the three-term recurrence; then the orthogonalizing vectors.  Subtraction order
  // stays c ascending, as in the reference.
  const int nv = cs.count - ntail;
  auto from_memory = [&](int lo, int hi) {
    int ci = lo;
    for (; ci + 4 <= hi; ci += 4) {
      double2 x0[4], x1[4], x2[4], x3[4];
      load_col<FULL>(x0, column_ptr(cs, ci + 0), base, n);
      load_col<FULL>(x1, column_ptr(cs, ci + 1), base, n);
      load_col<FULL>(x2, column_ptr(cs, ci + 2), base, n);
      load_col<FULL>(x3, column_ptr(cs, ci + 3), base, n);
      axmy8<CPLX>(w, h, ci + 0, x0);
      axmy8<CPLX>(w, h, ci + 1, x1);
      axmy8<CPLX>(w, h, ci + 2, x2);
      axmy8<CPLX>(w, h, ci + 3, x3);
    }
    for (; ci < hi; ++ci) {
      double2 x0[4];
      load_col<FULL>(x0, column_ptr(cs, ci), base, n);
      axmy8<CPLX>(w, h, ci, x0);
    }
  };
  from_memory(0, nv);
  if (ntail == 2) axmy8<CPLX>(w, h, cs.count - 2, ukm1);
  if (ntail >= 1) axmy8<CPLX>(w, h, cs.count - 1, uk);
  from_memory(cs.count, ncols);
  double nrm = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = base + i * (2 * kBlock);
    if (FULL || row < n) {
      nt_st2(dst + row, w[i]);
      nrm = fma(w[i].x, w[i].x, nrm);
      nrm = fma(w[i].y, w[i].y, nrm);
    }
  }
  return nrm;
}

// RED: the second-stage sums of the preceding dots pass are taken here (InlineReduce) -- its own instantiation, so that the
// common kernel keeps its registers (with both paths in one kernel: 136 VGPRs and three waves per SIMD instead of 128 and four)
template <bool CPLX, bool RED>
__global__ __launch_bounds__(kBlock) void k_update(const double* src, double* dst, ThreeTerm tt, ColumnSet cs,
                                                   const double* __restrict__ h, int64_t n, int64_t ntiles,
                                                   double* __restrict__ partials, const Ctrl* __restrict__ ctrl, InlineReduce red) {
  extern __shared__ double h_lds[];  // RED: red.ncoef coefficients
  __shared__ double lds4[4];
  if (ctrl->stopped) return;
  const int ncols = cs.count + cs.nq;
  const double a = tt.uk ? *tt.a : 0.0;
  const double b = (tt.uk && tt.ukm1) ? *tt.b : 0.0;
  const int ntail = tail_columns(tt, cs);
  if (RED) {  // k_reduce's sums, coefficient by coefficient in its order; workgroup 0 leaves them where k_reduce would have
    for (int c = 0; c < red.ncoef; ++c) {
      const double* p = red.partials + (int64_t)c * red.pstride;
      double sc = 0.0;
      for (int bb = threadIdx.x; bb < red.nblocks; bb += kBlock) sc += p[bb];
      sc = block_sum(sc, lds4);
      if (threadIdx.x == 0) h_lds[c] = sc;
    }
    __syncthreads();
    if (blockIdx.x == 0)
      for (int c = threadIdx.x; c < red.ncoef; c += kBlock) red.out[c] = h_lds[c];
  }
  const double* hh = RED ? h_lds : h;
  double nrm = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * kTileRows + 2 * threadIdx.x;
    if ((tile + 1) * kTileRows <= n)
      nrm += update_tile<true, CPLX>(src, dst, tt, a, b, cs, ncols, ntail, hh, base, n);
    else
      nrm += update_tile<false, CPLX>(src, dst, tt, a, b, cs, ncols, ntail, hh, base, n);
  }
  nrm = block_sum(nrm, lds4);
  if (threadIdx.x == 0) partials[blockIdx.x] = nrm;
}

// ---------------------------------------------------------------------------
// second-stage reduction: out[c] = sum_b partials[c*pstride + b], one block per
// column, fixed summation tree (results are reproducible run to run).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_reduce(const double* __restrict__ partials, int pstride, int nblocks,
                                                   double* __restrict__ out, const Ctrl* __restrict__ ctrl) {
  __shared__ double lds4[4];
  if (ctrl->stopped) return;
  const double* p = partials + (int64_t)blockIdx.x * pstride;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += kBlock) s += p[b];
  s = block_sum(s, lds4);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---------------------------------------------------------------------------
// One-sweep Lanczos step (kernels.hpp: SweepStep; lag_terms.hpp has the scheme): the dots of k_dots and the subtraction
// of k_update over ONE pass of the slab -- 8N(k+4) bytes per step instead of 8N(2k+5).  Same tiles, persistent grid,
// non-temporal 16-byte column loads, per-wave LDS sums and partials layout as k_dots; four columns in flight beside the
// four vectors a lane carries (w0, w, u_k, u_{k-1}).  Columns are visited in ascending order, which fixes the bits of u and w.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void lag_apply8(double2 (&u)[4], double2 (&w)[4], double cj, double fj, bool with_w, const double2 (&x)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u[i].x = fma(-cj, x[i].x, u[i].x);
    u[i].y = fma(-cj, x[i].y, u[i].y);
    if (with_w) {
      w[i].x = fma(-fj, x[i].x, w[i].x);
      w[i].y = fma(-fj, x[i].y, w[i].y);
    }
  }
}

// Parked stores (k_sweep<false, DEPTH> with DEPTH 1 or 2): a tile's two results wait in LDS, each lane's own eight 16-byte values in
// its own places (so no barrier stands between parking and release), and go out while later tiles' columns stream: behind the loads
// of the first column group at which the chip-wide clock (wall_clock64) has entered another slot of 2^shift ticks than the one the
// oldest parked tile was parked in.  All workgroups see the same boundaries, so their stores reach HBM together, as one burst per
// slot instead of a trickle into the read stream (scripts/microbench/sweep_stores.hip, profiles/sweep_stores.md,
// profiles/sweep_park_depth.md).  The parking is a queue of DEPTH tiles: a boundary releases all of them, oldest first; nothing
// waits: a tile that finds the queue full at its end sends the oldest out then.  The same values to the same addresses as the
// direct stores; rows are guarded from each parked tile's own base.  kernels.hpp (launch_sweep) says when and how deep a launch parks.
template <int DEPTH>
struct SweepPark {
  static_assert(DEPTH == 1 || DEPTH == 2, "one or two parked tiles");
  double2* slots;     // the workgroup's DEPTH * kSweepParkBytes of LDS: [DEPTH][8][kBlock], per place [0, 4) column k, [4, 8) w
  int64_t tile[2];    // the parked tiles, oldest first, or -1; wave-uniform, as everything below
  uint64_t slot[2];   // the clock slots they were parked in; the oldest's decides for all
  int head;           // the place of the oldest; the newer one (DEPTH 2) lies at the other place
  int shift;
  __device__ __forceinline__ bool full() const { return tile[DEPTH - 1] >= 0; }
  __device__ __forceinline__ double2* free_place() const { return slots + (tile[0] < 0 ? head : head ^ 1) * (8 * kBlock); }
  __device__ __forceinline__ void note(int64_t t, uint64_t sl) {  // behind the values written to free_place()
    if (tile[0] < 0)
      tile[0] = t, slot[0] = sl;
    else
      tile[1] = t, slot[1] = sl;
  }
};
template <int DEPTH>
__device__ __forceinline__ void sweep_release_oldest(SweepPark<DEPTH>& pk, double* ukcol, double* w, int64_t n) {
  const double2* from = pk.slots + pk.head * (8 * kBlock);
  const int64_t pbase = pk.tile[0] * kTileRows + 2 * threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = pbase + i * (2 * kBlock);
    if (row < n) {
      nt_st2(ukcol + row, from[i * kBlock + threadIdx.x]);
      nt_st2(w + row, from[(4 + i) * kBlock + threadIdx.x]);
    }
  }
  pk.tile[0] = pk.tile[1], pk.slot[0] = pk.slot[1], pk.tile[1] = -1;
  if (DEPTH == 2) pk.head ^= 1;
}
template <int DEPTH>
__device__ __forceinline__ void sweep_release_all(SweepPark<DEPTH>& pk, double* ukcol, double* w, int64_t n) {
  if (pk.tile[0] >= 0) sweep_release_oldest(pk, ukcol, w, n);
  if (DEPTH == 2 && pk.tile[0] >= 0) sweep_release_oldest(pk, ukcol, w, n);
}
template <int DEPTH>
__device__ __forceinline__ void sweep_release_at_boundary(SweepPark<DEPTH>& pk, double* ukcol, double* w, int64_t n) {
  if (pk.tile[0] >= 0 && (wall_clock64() >> pk.shift) != pk.slot[0]) sweep_release_all(pk, ukcol, w, n);
}

template <bool FULL, bool CORRECT, int PARK = 0>  // PARK: the depth of the parking, 0 = direct stores
__device__ __forceinline__ double sweep_tile(const SweepStep& st, double scale, double a, double b, const double* cl, const double* fl,
                                             double* wave_acc, int64_t base, int64_t n, SweepPark<PARK ? PARK : 1>* pk = nullptr,
                                             int64_t tile = 0) {
  static_assert(!(PARK && CORRECT), "the closing pass stores directly");
  const int lane = threadIdx.x & 63;
  const int k = st.k;
  const double* ukm1 = st.V + (int64_t)(k - 1) * st.ldv;  // only dereferenced for k > 0
  double* ukcol = const_cast<double*>(st.V) + (int64_t)k * st.ldv;
  double2 w0[4], w[4], u[4], um[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = base + i * (2 * kBlock);
    u[i] = w0[i] = w[i] = um[i] = make_double2(0.0, 0.0);
    if (FULL || row < n) {
      const double2 t = ld2(st.w + row);
      u[i] = make_double2(t.x * scale, t.y * scale);  // the operator's product, the same bits as the column it stored
      if (!CORRECT) {
        double2 s = ld2(st.v + row);
        s.x = fma(-a, u[i].x, s.x);
        s.y = fma(-a, u[i].y, s.y);
        if (k > 0) {
          um[i] = ld2(ukm1 + row);
          s.x = fma(-b, um[i].x, s.x);
          s.y = fma(-b, um[i].y, s.y);
        }
        w0[i] = w[i] = s;
      }
    }
  }
  // columns [0, nv) stream from HBM; column k-1 is still in registers from the recurrence (not in the closing pass)
  const int nv = CORRECT ? k : (k > 0 ? k - 1 : 0);
  int ci = 0;
  for (; ci + 4 <= nv; ci += 4) {
    double2 x0[4], x1[4], x2[4], x3[4];
    load_col<FULL>(x0, st.V + (int64_t)(ci + 0) * st.ldv, base, n);
    load_col<FULL>(x1, st.V + (int64_t)(ci + 1) * st.ldv, base, n);
    load_col<FULL>(x2, st.V + (int64_t)(ci + 2) * st.ldv, base, n);
    load_col<FULL>(x3, st.V + (int64_t)(ci + 3) * st.ldv, base, n);
    if (PARK) sweep_release_at_boundary(*pk, ukcol, st.w, n);
    if (!CORRECT) {
      double r0, r1, r2, r3, im;
      dotc8<false>(w0, x0, r0, im);
      dotc8<false>(w0, x1, r1, im);
      dotc8<false>(w0, x2, r2, im);
      dotc8<false>(w0, x3, r3, im);
      const double kr = wave_sum4(r0, r1, r2, r3, lane);
      if ((lane & 15) == 0) wave_acc[ci + (lane >> 4)] += kr;
    }
    lag_apply8(u, w, cl[ci + 0], CORRECT ? 0.0 : fl[ci + 0], !CORRECT, x0);
    lag_apply8(u, w, cl[ci + 1], CORRECT ? 0.0 : fl[ci + 1], !CORRECT, x1);
    lag_apply8(u, w, cl[ci + 2], CORRECT ? 0.0 : fl[ci + 2], !CORRECT, x2);
    lag_apply8(u, w, cl[ci + 3], CORRECT ? 0.0 : fl[ci + 3], !CORRECT, x3);
  }
  for (; ci < nv; ++ci) {
    double2 x0[4];
    load_col<FULL>(x0, st.V + (int64_t)ci * st.ldv, base, n);
    if (PARK) sweep_release_at_boundary(*pk, ukcol, st.w, n);
    if (!CORRECT) {
      double r0, im;
      dotc8<false>(w0, x0, r0, im);
      r0 = wave_sum(r0);
      if (lane == 0) wave_acc[ci] += r0;
    }
    lag_apply8(u, w, cl[ci], CORRECT ? 0.0 : fl[ci], !CORRECT, x0);
  }
  double nrm = 0.0;
  if (!CORRECT) {
    double r0, r1 = 0.0, im;
    if (k > 0) {
      dotc8<false>(w0, um, r1, im);
      lag_apply8(u, w, cl[k - 1], fl[k - 1], true, um);
    }
    dotc8<false>(w0, u, r0, im);  // the corrected tile of column k is in registers
    const double fk = fl[k];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[i].x = fma(-fk, u[i].x, w[i].x);
      w[i].y = fma(-fk, u[i].y, w[i].y);
    }
    r0 = wave_sum(r0);
    if (k > 0) r1 = wave_sum(r1);
    if (lane == 0) {
      wave_acc[k] += r0;
      if (k > 0) wave_acc[k - 1] += r1;
    }
  }
  if (PARK) {
    if (pk->full()) sweep_release_oldest(*pk, ukcol, st.w, n);  // no boundary has passed: the place is needed now
    double2* place = pk->free_place();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      place[i * kBlock + threadIdx.x] = u[i];
      place[(4 + i) * kBlock + threadIdx.x] = w[i];
      const int64_t row = base + i * (2 * kBlock);
      if (FULL || row < n) {
        nrm = fma(w[i].x, w[i].x, nrm);
        nrm = fma(w[i].y, w[i].y, nrm);
      }
    }
    pk->note(tile, wall_clock64() >> pk->shift);
    return nrm;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = base + i * (2 * kBlock);
    if (FULL || row < n) {
      nt_st2(ukcol + row, u[i]);
      if (!CORRECT) {
        nt_st2(st.w + row, w[i]);  // in place: this lane has read these rows of the pending vector above
        nrm = fma(w[i].x, w[i].x, nrm);
        nrm = fma(w[i].y, w[i].y, nrm);
      }
    }
  }
  return nrm;
}

// PARK (the full sweep only, launch_sweep decides): parking for PARK tiles of kSweepParkBytes in front of the sums; park_shift =
// log2 of the slot
template <bool CORRECT, int PARK>
__global__ __launch_bounds__(kBlock) void k_sweep(SweepStep st, InlineFin fin, int64_t n, int64_t ntiles, double* __restrict__ dpartials,
                                                  int pstride, double* __restrict__ npartials, const Ctrl* ctrl,  // no __restrict__: fin.ctrl aliases it
                                                  int park_shift) {
  extern __shared__ __align__(16) double lds_all[];  // PARK parked tiles; [4 waves][k+1] sums of d, then c (k+1, c[k] = 0), then f (k+1)
  __shared__ double lds4[4];
  if (ctrl->stopped) return;
  double* lds = lds_all + PARK * (kSweepParkBytes / (int)sizeof(double));
  const int k = st.k, nacc = k + 1;
  double* cl = lds + 4 * nacc;
  double* fl = cl + nacc;
  for (int i = threadIdx.x; i < 4 * nacc; i += kBlock) lds[i] = 0.0;
  for (int i = threadIdx.x; i < nacc; i += kBlock) cl[i] = i < k ? st.lag[kLagC + i] : 0.0;
  // a' (lanczos.hpp:448, of the raw column): the operator's partials in k_reduce_fin's order, or the slot the host names
  const double a = fin.partials ? inline_fin_sum(fin, lds4) : *st.a_raw;
  __syncthreads();
  const double da = lag_alpha_correction(k, st.beta, cl);
  if (!CORRECT) {  // the same O(k) arithmetic in every workgroup; workgroup 0 leaves f for k_lag_terms
    for (int i = threadIdx.x; i < nacc; i += kBlock) {
      const double fi = lag_f_entry(i, k, st.alpha, st.beta, cl, a, da);
      fl[i] = fi;
      if (blockIdx.x == 0) st.lag[st.f_off + i] = fi;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st.lag[0] = a;
    if (fin.partials) {
      fin.out[0] = a;
      fin_alpha_apply(fin.ctrl, a - da, fin.series, fin.mode == kFinishAlphaFirst);
    } else if (k > 0) {
      st.alpha[k] = a - da;  // the series holds the raw a' (k_reduce_fin) or this very value (a batch closed before this step)
    }
  }
  __syncthreads();
  const double scale = *st.scale;
  const double b = k > 0 ? st.beta[k - 1] : 0.0;
  double* wave_acc = lds + (threadIdx.x >> 6) * nacc;
  double nrm = 0.0;
  SweepPark<PARK ? PARK : 1> pk{reinterpret_cast<double2*>(lds_all), {-1, -1}, {0, 0}, 0, park_shift};
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * kTileRows + 2 * threadIdx.x;
    if ((tile + 1) * kTileRows <= n)
      nrm += sweep_tile<true, CORRECT, PARK>(st, scale, a, b, cl, fl, wave_acc, base, n, &pk, tile);
    else
      nrm += sweep_tile<false, CORRECT, PARK>(st, scale, a, b, cl, fl, wave_acc, base, n, &pk, tile);
  }
  if (PARK) sweep_release_all(pk, const_cast<double*>(st.V) + (int64_t)k * st.ldv, st.w, n);  // nothing stays parked, oldest first
  if (CORRECT) return;
  __syncthreads();
  for (int c = threadIdx.x; c < nacc; c += kBlock)
    dpartials[(int64_t)c * pstride + blockIdx.x] = (lds[c] + lds[nacc + c]) + (lds[2 * nacc + c] + lds[3 * nacc + c]);
  nrm = block_sum(nrm, lds4);
  if (threadIdx.x == 0) npartials[blockIdx.x] = nrm;
}

// behind the full sweep (kernels.hpp: launch_lag_terms), one workgroup of up to kLagWaves waves: a wave per coefficient and round,
// lanes strided over the partials.  The chain sweep -> this -> operator is serial on the stream and each round is one latency-bound
// load, so the rounds are what it costs: ceil((k+1)/16) instead of ceil((k+1)/4).  beta is formed by the first four waves alone,
// with block_sum's strides and order (the number inline_fin_sum gives the operator kernel), and handed to the others through LDS.
constexpr int kLagWaves = 16;
__global__ __launch_bounds__(64 * kLagWaves) void k_lag_terms(int k, const double* __restrict__ dpartials, int pstride, int nblocks,
                                                              const double* __restrict__ npartials, double* lag, int f_off, double threshold,
                                                              Ctrl* ctrl, Ctrl* repair) {
  __shared__ double lds4[4];
  __shared__ double wmax[kLagWaves];
  if (ctrl->stopped) {
    if (threadIdx.x == 0) repair->stopped = 1;
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  if (wave < kBlock / 64) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kBlock) s += npartials[b];
    s = wave_sum(s);
    if (lane == 0) lds4[wave] = s;
  }
  __syncthreads();
  const double beta = sqrt((lds4[0] + lds4[1]) + (lds4[2] + lds4[3]));
  double m = 0.0;
  for (int c = wave; c <= k; c += nwaves) {
    const double* p = dpartials + (int64_t)c * pstride;
    double d = 0.0;
    for (int b = lane; b < nblocks; b += 64) d += p[b];
    d = wave_sum(d);
    if (lane == 0) {
      const double cc = lag_next_coefficient(d, lag[f_off + c], beta, threshold);
      lag[kLagC + c] = cc;
      m = fmax(m, fabs(cc));
    }
  }
  if (lane == 0) wmax[wave] = m;
  __syncthreads();
  double mx = 0.0;
  for (int w = 0; w < nwaves; ++w) mx = fmax(mx, wmax[w]);
  const bool armed = mx > kLagGuard;
  if (armed)
    for (int c = threadIdx.x; c <= k; c += blockDim.x) lag[kLagC + c] = 0.0;  // the repair leaves nothing pending
  if (threadIdx.x == 0) {
    repair->stopped = armed ? 0 : 1;
    if (armed) ctrl->repairs++;
  }
}

// The scalars of a closing pass (k_sweep<true>'s prologue, the same arithmetic on one thread): a' kept in lag[0], alpha_k = a' - da
// into the series.  The column part of the pass waits until something reads the column (library.hip: settle_columns).
__global__ void k_close_scalars(int k, const double* a_raw, double* alpha, const double* __restrict__ beta, double* lag, const Ctrl* __restrict__ ctrl) {
  if (ctrl->stopped) return;
  const double a = *a_raw;
  const double da = lag_alpha_correction(k, beta, lag + kLagC);
  lag[0] = a;
  if (k > 0) alpha[k] = a - da;
}

// ---------------------------------------------------------------------------
// Chebyshev filter step (kernels.hpp: ChebStep).  cheb_store: one row, in the epilogue of the one-pass real CSR kernels (a =
// the row sum with the shift -center applied, x = the row's own operator input = t_k).  k_cheb_combine: the same arithmetic
// behind any other operator kernel, which has stored a as y: a stream over y, t_prev and acc with k_update's tiles and
// persistent grid, 16-byte accesses, non-temporal stores of the two vectors it writes in full.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void cheb_store(const ChebStep& ch, int64_t r, double a, double x) {
  const double tp = ch.first ? x : ch.t_prev[r];
  const double acc = ch.first ? 0.0 : ch.acc[r];
  double acc_new;
  const double t = cheb_row_nofma(a, tp, acc, ch, &acc_new);
  __builtin_nontemporal_store(t, &ch.t_next[r]);
  __builtin_nontemporal_store(acc_new, &ch.acc[r]);
}

template <bool FULL>
__device__ __forceinline__ void cheb_tile(const double* __restrict__ y, const ChebStep& ch, int64_t base, int64_t n) {
  double2 a[4], tp[4], ac[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = base + i * (2 * kBlock);
    a[i] = tp[i] = ac[i] = make_double2(0.0, 0.0);
    if (FULL || row < n) {
      a[i] = nt_ld_d2(y + row);
      tp[i] = ld2(ch.t_prev + row);
      if (!ch.first) ac[i] = ld2(ch.acc + row);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = base + i * (2 * kBlock);
    if (FULL || row < n) {
      double2 t, an;
      t.x = cheb_row_nofma(a[i].x, tp[i].x, ac[i].x, ch, &an.x);
      t.y = cheb_row_nofma(a[i].y, tp[i].y, ac[i].y, ch, &an.y);
      nt_st2(ch.t_next + row, t);
      nt_st2(ch.acc + row, an);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_cheb_combine(const double* __restrict__ y, ChebStep ch, int64_t n, int64_t ntiles,
                                                         const Ctrl* __restrict__ ctrl) {
  if (ctrl->stopped) return;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * kTileRows + 2 * threadIdx.x;
    if ((tile + 1) * kTileRows <= n)
      cheb_tile<true>(y, ch, base, n);
    else
      cheb_tile<false>(y, ch, base, n);
  }
}

// ---------------------------------------------------------------------------
// Chebyshev moments step (kernels.hpp: MomentStep): the recurrence of the filter step without the accumulator, and the two
// dot products of a kernel-polynomial step, <t_{k+1}, t_{k+1}> and <t_{k+1}, t_k>, as per-workgroup partial sums (fixed order:
// per-thread fma chains over the thread's rows, block_sum).  moment_store: one row, in the epilogue of the one-pass real CSR
// kernels (x = the row's own operator input = t_k).  k_cheb_moments: behind any other operator kernel, which has stored a as y;
// k_cheb_combine's tiles and grid.  t_{k-1} is read once and t_{k+1} written once with the loads / stores cheb_store uses.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double moment_row_nofma(double a, double t_prev, const MomentStep& mo) {
#pragma clang fp contract(off)
  const double ca = mo.c * a;
  return mo.first ? ca : ca - t_prev;
}
__device__ __forceinline__ double moment_store(const MomentStep& mo, int64_t r, double a) {
  const double tp = mo.first ? 0.0 : mo.t_prev[r];
  const double t = moment_row_nofma(a, tp, mo);
  __builtin_nontemporal_store(t, &mo.t_next[r]);
  return t;
}

template <bool FULL>
__device__ __forceinline__ void moments_tile(const double* __restrict__ y, const MomentStep& mo, int64_t base, int64_t n, double* tt, double* tx) {
  double2 a[4], tp[4], x[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = base + i * (2 * kBlock);
    a[i] = tp[i] = x[i] = make_double2(0.0, 0.0);
    if (FULL || row < n) {
      a[i] = nt_ld_d2(y + row);
      x[i] = ld2(mo.t_cur + row);
      if (!mo.first) tp[i] = ld2(mo.t_prev + row);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = base + i * (2 * kBlock);
    if (FULL || row < n) {
      double2 t;
      t.x = moment_row_nofma(a[i].x, tp[i].x, mo);
      t.y = moment_row_nofma(a[i].y, tp[i].y, mo);
      nt_st2(mo.t_next + row, t);
      *tt = fma(t.x, t.x, *tt);
      *tt = fma(t.y, t.y, *tt);
      *tx = fma(t.x, x[i].x, *tx);
      *tx = fma(t.y, x[i].y, *tx);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_cheb_moments(const double* __restrict__ y, MomentStep mo, int64_t n, int64_t ntiles,
                                                         double* __restrict__ partials, const Ctrl* __restrict__ ctrl) {
  __shared__ double lds4[4];
  if (ctrl->stopped) return;
  double tt = 0.0, tx = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * kTileRows + 2 * threadIdx.x;
    if ((tile + 1) * kTileRows <= n)
      moments_tile<true>(y, mo, base, n, &tt, &tx);
    else
      moments_tile<false>(y, mo, base, n, &tt, &tx);
  }
  tt = block_sum(tt, lds4);
  tx = block_sum(tx, lds4);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = tt;
    partials[mo.pstride + blockIdx.x] = tx;
  }
}

// out[r] = +1 or -1 from random_sign_bit(seed, stream, row0 + r) (kernels.hpp), r < n; es = 2: (+-1, 0) pairs
__global__ __launch_bounds__(kBlock) void k_random_signs(double* __restrict__ out, int64_t n, int64_t row0, int es, uint64_t seed, uint64_t stream) {
  const uint64_t key = random_sign_key(seed, stream);
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) {
    const double v = random_sign_bit(key, (uint64_t)(row0 + r)) ? -1.0 : 1.0;
    if (es == 2)
      st2(out + 2 * r, make_double2(v, 0.0));
    else
      out[r] = v;
  }
}

// ---------------------------------------------------------------------------
// CSR SpMV, "stream" formulation: a tile of 256 rows owns a contiguous range of
// stored entries.  Phase 1 streams val/col with aligned 16-B loads (4 entries per
// lane), gathers x (L2/MALL-served) and parks the rounded products in LDS
// (index skewed by i>>5 so that the row phase is bank-conflict free for any
// row length).  Phase 2: one thread per row adds its products in stored order
// (multiply, then add: bit-identical to the row loop of oracle/krylov_ref.c).
// Epilogue fuses the shift, the store of the scaled input into the basis slab
// and the partial dot alpha = u.v.
// ---------------------------------------------------------------------------
// skew(), the chunk / lane / row-window arithmetic: spmv_index.hpp (the host replay tests/cpp/spmv_replay_host.cpp runs the same functions)

// Tile schedule of a persistent SpMV workgroup.  Plain: tiles b, b+G, ...: the grid advances over the rows as one
// frontier of G tiles per step.  XCD-sliced (flag bit 0): workgroups b and b+8 share an XCD (round-robin
// dispatch), so within every frontier step XCD x = b%8 takes the contiguous eighth [x*G/8, (x+1)*G/8) of the
// step's tiles: neighbouring rows' operator-input lines are then fetched into one L2 instead of eight, and the
// frontier stays single (splitting the whole row range into eight far-apart chunks, tried first, cost 7 %).
// Placement only changes speed, never results.
struct TileRange {
  int64_t first, step, end;
};
__device__ __forceinline__ TileRange spmv_tiles(int64_t ntiles, int xcd_sliced) {
  const int64_t G = gridDim.x, b = blockIdx.x;
  if (xcd_sliced && (G & 7) == 0) return TileRange{(b & 7) * (G >> 3) + (b >> 3), G, ntiles};
  return TileRange{b, G, ntiles};
}

// InlineArnoldiBegin: returns true if the step must not run (the same test in every workgroup); *scale = 1/residue.
// With tail_k >= 0 the previous step is finished first (k_arnoldi_tail): every workgroup forms the same residue from the
// second pass's partial sums (or takes the first pass's norm) and the step index from the argument -- it reads nothing that
// workgroup 0 changes; *res_out / *nrm2_out / *k_out are what the record needs (*nrm2_out only with tail_k >= 0).
__device__ __forceinline__ bool arnoldi_begin_inline(const InlineArnoldiBegin& ab, double* scale, double* lds4, double* res_out, double* nrm2_out,
                                                      int* k_out) {
  int k;
  double res, nrm2 = 0.0;
  if (ab.tail_k >= 0) {
    const bool second = ab.pass2->stopped == 0;
    double s = 0.0;
    if (second && threadIdx.x < kBlock)  // k_arnoldi_tail's sum: 256 strided partial sums, then the four-wave tree (also in a 1024-thread workgroup)
      for (int b = threadIdx.x; b < ab.tail_nblocks; b += kBlock) s += ab.tail_partials[b];
    s = wave_sum(s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && threadIdx.x < kBlock) lds4[threadIdx.x >> 6] = s;
    __syncthreads();
    s = (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
    nrm2 = second ? s : *ab.nrm2_first;
    res = sqrt(nrm2);  // arnoldi.hpp:348, :385
    k = ab.tail_k + 1;
  } else {
    k = ab.ctrl->nvec;
    res = ab.ctrl->residue;
  }
  const bool stop = (int64_t)k == ab.n_global || res <= ab.threshold || k >= ab.cap;  // arnoldiStepIsUtmost  arnoldi.hpp:277-288
  *scale = 1.0 / res;                                                                   // arnoldi.hpp:365
  *res_out = res;
  *nrm2_out = nrm2;
  *k_out = k;
  return stop;
}
// workgroup 0, all threads (the copy of h into H is spread over them); `stop`, `scale`, `res`, `nrm2`, `k` as derived above
__device__ __forceinline__ void arnoldi_begin_record(const InlineArnoldiBegin& ab, bool stop, double scale, double res, double nrm2, int k) {
  if (ab.tail_k >= 0) {  // k_arnoldi_tail for the vector with index tail_k = k - 1
    const bool second = ab.pass2->stopped == 0;
    const int kk = ab.tail_k;
    for (int i = threadIdx.x; i < (kk + 1) * ab.es; i += blockDim.x) {
      double hv = ab.h[i];
      if (second && i < ab.ncoef) hv += ab.h2[i], ab.h[i] = hv;
      ab.H[(int64_t)kk * ab.ldh * ab.es + i] = hv;  // arnoldi.hpp:380-383
    }
    if (second)
      for (int i = (kk + 1) * ab.es + threadIdx.x; i < ab.ncoef; i += blockDim.x) ab.h[i] += ab.h2[i];  // coefficients of the orthogonalizing vectors
    if (threadIdx.x == 0) {
      *ab.nrm2_final = nrm2;  // as k_arnoldi_tail stores it (not res * res: the round trip through sqrt can move an ulp)
      for (int e = 0; e < ab.es; ++e) ab.H[((int64_t)kk * ab.ldh + kk + 1) * ab.es + e] = 0.0;  // arnoldi.hpp:384
      ab.ctrl->residue = res;
      ab.ctrl->nvec = kk + 1;
      ab.ctrl->nalpha = kk + 1;
      ab.ctrl->iterations++;
      ab.ctrl->calls_true++;
    }
  }
  if (threadIdx.x != 0) return;
  if (stop) {
    ab.ctrl->stopped = 1;
    return;
  }
  if (ab.ctrl->keep_coupling)
    ab.ctrl->keep_coupling = 0;  // first step after a Krylov-Schur restart: H[k][k-1] = residue * Q[m-1][k-1] is already there
  else
    ab.H[((int64_t)(k - 1) * ab.ldh + k) * ab.es] = res;  // arnoldi.hpp:363 (imaginary part stays 0)
  ab.ctrl->scale = scale;
}

// LONG_ROWS: the row phase reads sixteen products at a time (operators with >= 16 entries per row on average; the short-row form
// is kept as it was: the same loop in the long-row kernel costs the 7-point stencil 1.8 % through its register allocation)
// OFF: type of the row pointers.  int32_t: a shard with < 2^31 stored entries (every BASELINE config but one 768^3 shard).
// int64_t (r3; the reference's Index is 64-bit, lanczos.hpp:108-116): the offsets of a TILE are taken relative to the tile's
// first entry rounded down to a multiple of 4 -- `base`, which moves the col / val pointers -- so that everything behind the
// row-pointer loads is the same 32-bit arithmetic (spmv_index.hpp) for both types; with int32_t the base is the constant 0.
template <bool LONG_ROWS, class OFF, bool NT>
__global__ __launch_bounds__(kBlock) void k_spmv(const OFF* __restrict__ rowptr, const int32_t* __restrict__ col_all,
                                                 const double* __restrict__ val_all, const double* __restrict__ x_ext,
                                                 const double* __restrict__ scale_ptr, double shift,
                                                 double* __restrict__ y, double* __restrict__ u_out, int64_t n,
                                                 int64_t ntiles, double* __restrict__ partials, int spmv_flags,
                                                 int pass, const Ctrl* ctrl, InlineFin fin, InlineArnoldiBegin ab,
                                                 const int32_t* __restrict__ tile_list) {  // no __restrict__ on ctrl: fin.ctrl / ab.ctrl alias it
  constexpr bool CHEB = false, MOM = false;
  const ChebStep ch{};
  const MomentStep mo{};
#include "spmv_body.hpp"
}
// the same rows with a Chebyshev step in the epilogue (no hooks, no partial dots): the body is compiled a second time, so that
// k_spmv keeps its arguments and, instruction for instruction, its code
template <bool LONG_ROWS, class OFF, bool NT>
__global__ __launch_bounds__(kBlock) void k_spmv_cheb(const OFF* __restrict__ rowptr, const int32_t* __restrict__ col_all,
                                                      const double* __restrict__ val_all, const double* __restrict__ x_ext,
                                                      const double* __restrict__ scale_ptr, double shift, double* __restrict__ u_out,
                                                      int64_t n, int64_t ntiles, int spmv_flags, const Ctrl* __restrict__ ctrl,
                                                      const int32_t* __restrict__ tile_list, ChebStep ch) {
  constexpr bool CHEB = true, MOM = false;
  constexpr int pass = 0;
  double* const y = nullptr;
  double* const partials = nullptr;
  const InlineFin fin{};
  const InlineArnoldiBegin ab{};
  const MomentStep mo{};
#include "spmv_body.hpp"
}
// a third compile: the moments step (moment_store) in the epilogue, its two partial dots in partials[block] and
// partials[mo.pstride + block]; no hooks, y never written
template <bool LONG_ROWS, class OFF, bool NT>
__global__ __launch_bounds__(kBlock) void k_spmv_moments(const OFF* __restrict__ rowptr, const int32_t* __restrict__ col_all,
                                                         const double* __restrict__ val_all, const double* __restrict__ x_ext,
                                                         const double* __restrict__ scale_ptr, double shift, double* __restrict__ partials,
                                                         int64_t n, int64_t ntiles, int spmv_flags, const Ctrl* __restrict__ ctrl,
                                                         const int32_t* __restrict__ tile_list, MomentStep mo) {
  constexpr bool CHEB = false, MOM = true;
  constexpr int pass = 0;
  double* const y = nullptr;
  double* const u_out = nullptr;
  const InlineFin fin{};
  const InlineArnoldiBegin ab{};
  const ChebStep ch{};
#include "spmv_body.hpp"
}

// ---------------------------------------------------------------------------
// Row-coded operator (row_codes.hpp): one 8- or 16-byte record per row instead of rowptr / col / val.  k_spmv's tiles,
// persistent grid, tile order and tile lists, its prologue (InlineFin, InlineArnoldiBegin) and its epilogue, so that the
// partial dots are the same numbers; one thread per row.  The row walks its slots in slot order (= stored order):
// x = x_ext[r + d_s] * scale, prod = pal[code] * x, sum = sum + prod from 0.0 -- the plain kernel's products and sums.
// REC = record bytes (8 or 16).  The palette sits in LDS; the records are read once (non-temporal, one tile ahead).
// Operators in one pass only: of the pass bits, kPassSelfNorm alone.
// ---------------------------------------------------------------------------
typedef unsigned long long v2u64_t __attribute__((ext_vector_type(2)));
template <int REC>
__device__ __forceinline__ void row_code_load(const uint64_t* __restrict__ rec, int64_t row, uint64_t* w) {
  if constexpr (REC == 8) {
    w[0] = __builtin_nontemporal_load(reinterpret_cast<const unsigned long long*>(rec) + row);
  } else {
    const v2u64_t v = __builtin_nontemporal_load(reinterpret_cast<const v2u64_t*>(rec) + row);
    w[0] = v.x, w[1] = v.y;
  }
}

template <int REC>
__global__ __launch_bounds__(kBlock) void k_spmv_rows(RowCodeView op, const double* __restrict__ x_ext,
                                                      const double* __restrict__ scale_ptr, double shift,
                                                      double* __restrict__ y, double* __restrict__ u_out, int64_t n,
                                                      int64_t ntiles, double* __restrict__ partials, int spmv_flags,
                                                      int pass, const Ctrl* ctrl, InlineFin fin, InlineArnoldiBegin ab,
                                                      const int32_t* __restrict__ tile_list) {  // no __restrict__ on ctrl: fin.ctrl / ab.ctrl alias it
  constexpr bool CHEB = false, MOM = false;
  const ChebStep ch{};
  const MomentStep mo{};
#include "spmv_rows_body.hpp"
}
template <int REC>  // as k_spmv_cheb
__global__ __launch_bounds__(kBlock) void k_spmv_rows_cheb(RowCodeView op, const double* __restrict__ x_ext, const double* __restrict__ scale_ptr,
                                                           double shift, double* __restrict__ u_out, int64_t n, int64_t ntiles, int spmv_flags,
                                                           const Ctrl* __restrict__ ctrl, const int32_t* __restrict__ tile_list, ChebStep ch) {
  constexpr bool CHEB = true, MOM = false;
  constexpr int pass = 0;
  double* const y = nullptr;
  double* const partials = nullptr;
  const InlineFin fin{};
  const InlineArnoldiBegin ab{};
  const MomentStep mo{};
#include "spmv_rows_body.hpp"
}
template <int REC>  // as k_spmv_moments
__global__ __launch_bounds__(kBlock) void k_spmv_rows_moments(RowCodeView op, const double* __restrict__ x_ext, const double* __restrict__ scale_ptr,
                                                              double shift, double* __restrict__ partials, int64_t n, int64_t ntiles, int spmv_flags,
                                                              const Ctrl* __restrict__ ctrl, const int32_t* __restrict__ tile_list, MomentStep mo) {
  constexpr bool CHEB = false, MOM = true;
  constexpr int pass = 0;
  double* const y = nullptr;
  double* const u_out = nullptr;
  const InlineFin fin{};
  const InlineArnoldiBegin ab{};
  const ChebStep ch{};
#include "spmv_rows_body.hpp"
}

// ---------------------------------------------------------------------------
// CSR SpMV for operators whose gathers are scattered over an input larger than L2 (BASELINE config 3: 10^6 rows,
// 32 random columns each), "column-sorted row tiles".  Measured on the stream form above (rocprofv3 PMC,
// profiles/r02_config3_pmc.md): every gather is its own L2 request (8.8e6 TCP->TCC reads for 8.0e6 gathers per
// pass, L2 hit rate 0.88), the L1s wait on their pending-request limit 72 % of the time, 296 cycles per request: the
// pass is bound by L2 REQUESTS, not bytes.  The only lever is fewer requests per gather, i.e. lanes of one wave
// hitting the same 128-byte line -- which needs (a) many gathers per input line inside one workgroup's working set and
// (b) visiting them in column order.  So:
//   * a workgroup of 1024 threads owns a tile of 4096 rows and walks the K column slices (<= 256 KB of input each,
//     L2-resident; all workgroups are in the same slice at about the same time) INSIDE the kernel, row sums in
//     registers: no carry through memory between slices;
//   * the entries of one (tile, slice) -- ~4096 on config 3, 2 per input line -- are STORED sorted by column
//     (8-byte value + 4 bytes holding the column's position in the slice and a 16-bit slot = place of the entry in row
//     order: 12 bytes per entry like plain CSR), so consecutive lanes gather from the same
//     or neighbouring lines; products are scattered into LDS by slot (index skewed like above);
//   * row phase: every thread adds the products of its 4 rows in stored order, slice after slice = the stored
//     order of the row when its columns ascend: still bit-identical to the oracle's row loop.
// Gather skeleton (scripts/microbench/gather_sorted.hip): 168-196 G gathers/s in row order, 255-288 sorted.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double block_sum16(double x, double* lds16) {
  x = wave_sum(x);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) lds16[wave] = x;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < kSortBlock / 64; ++w) t += lds16[w];
  return t;
}

// entries of one segment held in registers between the loads and their use: two rounds of 4 per lane (<= 8192 entries)
struct SortedRegs {
  uint4 ca, cb;  // packed (column position in the slice | slot << 16)
  double2 a01, a23, b01, b23;
  bool in0, in1;
};
struct SortedX {
  double a0, a1, a2, a3, b0, b1, b2, b3;
};
__device__ __forceinline__ void sorted_load(SortedRegs& g, const SortedOperatorView& op, int e0, int e1, int tid) {
  const int q0 = e0 + 4 * tid, q1 = q0 + 4 * kSortBlock;
  g.in0 = q0 < e1, g.in1 = q1 < e1;
  if (g.in0) {
    g.ca = *reinterpret_cast<const uint4*>(op.cp + q0);
    g.a01 = ld2(op.val + q0);
    g.a23 = ld2(op.val + q0 + 2);
  }
  if (g.in1) {
    g.cb = *reinterpret_cast<const uint4*>(op.cp + q1);
    g.b01 = ld2(op.val + q1);
    g.b23 = ld2(op.val + q1 + 2);
  }
}
// index into the operator input of the column at position `c & 0xffff` of slice k
__device__ __forceinline__ int64_t sorted_index(const SortedOperatorView& op, int64_t slice_pos0, unsigned c) {
  const int64_t p = slice_pos0 + (c & 0xffffu);
  return p < op.n_low ? op.npad + p : (p < op.n_low + op.nloc ? p - op.n_low : op.npad + p - op.nloc);
}
__device__ __forceinline__ void sorted_gather(SortedX& x, const SortedRegs& g, const SortedOperatorView& op, int k,
                                              const double* __restrict__ x_ext) {
  const int64_t p0 = (int64_t)k * op.slice_width;
  x.a0 = x.a1 = x.a2 = x.a3 = x.b0 = x.b1 = x.b2 = x.b3 = 0.0;
  if (g.in0)  // all eight in flight
    x.a0 = x_ext[sorted_index(op, p0, g.ca.x)], x.a1 = x_ext[sorted_index(op, p0, g.ca.y)], x.a2 = x_ext[sorted_index(op, p0, g.ca.z)],
    x.a3 = x_ext[sorted_index(op, p0, g.ca.w)];
  if (g.in1)
    x.b0 = x_ext[sorted_index(op, p0, g.cb.x)], x.b1 = x_ext[sorted_index(op, p0, g.cb.y)], x.b2 = x_ext[sorted_index(op, p0, g.cb.z)],
    x.b3 = x_ext[sorted_index(op, p0, g.cb.w)];
}
__device__ __forceinline__ void sorted_scatter(const SortedRegs& g, const SortedX& x, double scale, double* prod) {
  if (g.in0) {
    prod[skew(g.ca.x >> 16)] = g.a01.x * (x.a0 * scale);
    prod[skew(g.ca.y >> 16)] = g.a01.y * (x.a1 * scale);
    prod[skew(g.ca.z >> 16)] = g.a23.x * (x.a2 * scale);
    prod[skew(g.ca.w >> 16)] = g.a23.y * (x.a3 * scale);
  }
  if (g.in1) {
    prod[skew(g.cb.x >> 16)] = g.b01.x * (x.b0 * scale);
    prod[skew(g.cb.y >> 16)] = g.b01.y * (x.b1 * scale);
    prod[skew(g.cb.z >> 16)] = g.b23.x * (x.b2 * scale);
    prod[skew(g.cb.w >> 16)] = g.b23.y * (x.b3 * scale);
  }
}

// RPT = rows per thread = tile rows / 1024: a thread owns RPT CONSECUTIVE rows (their RPT+1 slot offsets are adjacent
// 16-bit values, their outputs one or two 16-byte stores)
template <int RPT>
__global__ __launch_bounds__(kSortBlock) void k_spmv_sorted(SortedOperatorView op, const double* __restrict__ x_ext,
                                                            const double* __restrict__ scale_ptr, double shift,
                                                            double* __restrict__ y, double* __restrict__ u_out, int64_t n,
                                                            int64_t ntiles, double* __restrict__ partials, int pass,
                                                            const Ctrl* __restrict__ ctrl) {
  extern __shared__ double lds_prod[];  // two buffers of kSortBufDoubles
  __shared__ double lds16[kSortBlock / 64];
  if (ctrl->stopped) return;
  const double scale = scale_ptr ? *scale_ptr : 1.0;
  const int tid = threadIdx.x;
  const int K = op.nslices;
  constexpr int T = RPT * kSortBlock;
  double dot = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * T + (int64_t)tid * RPT;  // first row of this thread
    const int32_t* tb = op.base + tile * (K + 1);
    double sum[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) sum[i] = 0.0;
    // Pipeline over the slices, ONE barrier per segment: while the row phase of segment k runs, the gathers of segment
    // k+1 are in flight and its products go to the other LDS buffer; the entry streams run one segment ahead.  (A
    // deeper pipeline -- column indices two segments ahead -- was measured slower: 213 vs 199 us, 126 VGPRs.)
    SortedRegs g, gn;
    SortedX x;
    unsigned short o[RPT + 1], on[RPT + 1];
    auto load_offsets = [&](unsigned short (&dst)[RPT + 1], int k) {
      const uint16_t* p = op.off + (tile * K + k) * (int64_t)(T + 1) + tid * RPT;
#pragma unroll
      for (int i = 0; i <= RPT; ++i) dst[i] = p[i];
    };
    sorted_load(g, op, tb[0], tb[1], tid);
    load_offsets(o, 0);
    sorted_gather(x, g, op, 0, x_ext);
    for (int k = 0; k < K; ++k) {
      double* prod = lds_prod + (k & 1) * kSortBufDoubles;
      if (k + 1 < K) {  // (a) entry streams and offsets of the next segment
        sorted_load(gn, op, tb[k + 1], tb[k + 2], tid);
        load_offsets(on, k + 1);
      }
      sorted_scatter(g, x, scale, prod);  // (b) products of segment k (waits for its gathers)
      __syncthreads();                    // (c) the only barrier: buffer k&1 complete; buffer (k+1)&1 free since the last one
      if (k + 1 < K) sorted_gather(x, gn, op, k + 1, x_ext);  // (d) gathers of segment k+1 fly during the row phase
      // (e) row phase: stored order within the slice, multiply-then-add.  (Reading a thread's first 8 slots with
      // independent LDS loads and handing them to the rows by compares was measured slower: 184 vs 171 us.)
#pragma unroll
      for (int i = 0; i < RPT; ++i)
        for (int t = o[i]; t < o[i + 1]; ++t) sum[i] = sum[i] + prod[skew(t)];
      if (k + 1 < K) {
        g = gn;
#pragma unroll
        for (int i = 0; i <= RPT; ++i) o[i] = on[i];
      }
    }
    __syncthreads();  // the next tile's first scatter reuses buffer 0
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int64_t r = r0 + i;
      if (r < n) {
        const double xr = x_ext[r] * scale;
        double yr = sum[i];
        if (shift != 0.0) yr = add_product_nofma(yr, shift, xr);  // lanczos.hpp:390-392
        y[r] = yr;
        if (u_out) u_out[r] = xr;
        dot = (pass & kPassSelfNorm) ? fma(yr, yr, dot) : fma(xr, yr, dot);
      }
    }
  }
  if (partials) {
    dot = block_sum16(dot, lds16);
    if (tid == 0) partials[blockIdx.x] = dot;
  }
}

// ---------------------------------------------------------------------------
// Split tiles (split_layout.hpp): one workgroup per (row tile of up to 16384 rows, column group); partial row sums in LDS.
// Per chunk of <= 4096 column-sorted entries: 4 entries per lane, gathers, products rounded, acc[row] += product (no two
// entries of a chunk share a row: plain read-add-write, no atomics), one barrier.  The entry streams run two chunks ahead,
// the gathers one chunk ahead of the adds.
// ---------------------------------------------------------------------------
struct SplitRegs {
  uint4 c;
  double2 v01, v23;
  int nvalid;    // 0..4 entries of this lane in the chunk
  int64_t pos0;  // position of relative column 0
};
__device__ __forceinline__ void split_load(SplitRegs& g, const SplitOperatorView& op, int c, int c1, int tid) {
  g.nvalid = 0;
  if (c >= c1) return;
  const int4 d = op.chunk[c];
  const int q = d.x + 4 * tid;
  g.nvalid = min(4, max(0, d.y - q));
  g.pos0 = d.z;
  if (g.nvalid > 0) {
    g.c = *reinterpret_cast<const uint4*>(op.cp + q);  // (plain: the gathers wait for it; nt measured 5 % slower)
    g.v01 = nt_ld_d2(op.val + q);
    g.v23 = nt_ld_d2(op.val + q + 2);
  }
}
__device__ __forceinline__ int64_t split_index(const SplitOperatorView& op, int64_t pos0, unsigned c) {
  const int64_t p = pos0 + (c & ((1u << kSplitRelBits) - 1));
  return p < op.n_low ? op.npad + p : (p < op.n_low + op.nloc ? p - op.n_low : op.npad + p - op.nloc);
}
__device__ __forceinline__ void split_gather(double (&x)[4], const SplitRegs& g, const SplitOperatorView& op,
                                             const double* __restrict__ x_ext) {
  x[0] = x[1] = x[2] = x[3] = 0.0;
  if (g.nvalid > 0) x[0] = x_ext[split_index(op, g.pos0, g.c.x)];
  if (g.nvalid > 1) x[1] = x_ext[split_index(op, g.pos0, g.c.y)];
  if (g.nvalid > 2) x[2] = x_ext[split_index(op, g.pos0, g.c.z)];
  if (g.nvalid > 3) x[3] = x_ext[split_index(op, g.pos0, g.c.w)];
}
// acc[row] += product: the product is rounded first (a separate multiply), the add is an LDS atomic that returns nothing
// (ds_add_f64) -- cheaper than read-add-write, and no two entries of a chunk share a row, so nothing about it is unordered
__device__ __forceinline__ void split_add1(double* a, double p) {
  (void)__hip_atomic_fetch_add(a, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void split_add(const SplitRegs& g, const double (&x)[4], double scale, double* acc) {
  if (g.nvalid > 0) split_add1(acc + (g.c.x >> kSplitRelBits), g.v01.x * (x[0] * scale));
  if (g.nvalid > 1) split_add1(acc + (g.c.y >> kSplitRelBits), g.v01.y * (x[1] * scale));
  if (g.nvalid > 2) split_add1(acc + (g.c.z >> kSplitRelBits), g.v23.x * (x[2] * scale));
  if (g.nvalid > 3) split_add1(acc + (g.c.w >> kSplitRelBits), g.v23.y * (x[3] * scale));
}

// DEPTH = chunks whose gathers are in flight ahead of the adds (the entry streams run one chunk further ahead)
template <int DEPTH>
__global__ __launch_bounds__(kSplitBlock) void k_spmv_split(SplitOperatorView op, const double* __restrict__ x_ext,
                                                           const double* __restrict__ scale_ptr, const Ctrl* ctrl, InlineArnoldiBegin ab) {
  extern __shared__ double lds_acc[];  // tile_rows partial row sums
  __shared__ double lds4b[4];
  if (ctrl->stopped) return;
  double scale = (scale_ptr && !ab.ctrl) ? *scale_ptr : 1.0;
  if (ab.ctrl) {  // the second kernel (k_split_combine) reads the control block after workgroup 0 of this one has recorded
    double res, nrm2b;
    int kb;
    const bool stop = arnoldi_begin_inline(ab, &scale, lds4b, &res, &nrm2b, &kb);
    __syncthreads();
    if (blockIdx.x == 0) arnoldi_begin_record(ab, stop, scale, res, nrm2b, kb);
    if (stop) return;
  }
  const int tid = threadIdx.x, T = op.tile_rows;
  const int wg = blockIdx.x, tile = wg / op.groups, grp = wg - tile * op.groups;
  const int c0 = op.wg_chunk[wg], c1 = op.wg_chunk[wg + 1];
  SplitRegs r[DEPTH + 2];
  double x[DEPTH + 1][4];
#pragma unroll
  for (int d = 0; d <= DEPTH; ++d) split_load(r[d], op, c0 + d, c1, tid);
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) split_gather(x[d], r[d], op, x_ext);
  for (int i = tid; i < T; i += kSplitBlock) lds_acc[i] = 0.0;
  __syncthreads();
  for (int c = c0; c < c1; ++c) {
    split_load(r[DEPTH + 1], op, c + DEPTH + 1, c1, tid);
    split_gather(x[DEPTH], r[DEPTH], op, x_ext);
    split_add(r[0], x[0], scale, lds_acc);
    __syncthreads();  // the next chunk may hold the same rows
#pragma unroll
    for (int d = 0; d <= DEPTH; ++d) r[d] = r[d + 1];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
#pragma unroll
      for (int i = 0; i < 4; ++i) x[d][i] = x[d + 1][i];
  }
  const int64_t r0w = (int64_t)tile * T;
  double* dst = op.part + (int64_t)grp * op.part_stride + r0w;
  for (int i = tid; i < T; i += kSplitBlock)
    if (r0w + i < op.nloc) dst[i] = lds_acc[i];
}

__global__ __launch_bounds__(kBlock) void k_split_combine(const double* __restrict__ part, int64_t part_stride, int groups,
                                                         const double* __restrict__ x_ext, const double* __restrict__ scale_ptr,
                                                         double shift, double* __restrict__ y, double* __restrict__ u_out, int64_t n,
                                                         double* __restrict__ partials, int pass, const Ctrl* __restrict__ ctrl) {
  __shared__ double lds4[4];
  if (ctrl->stopped) return;
  const double scale = scale_ptr ? *scale_ptr : 1.0;
  double dot = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) {
    double yr = part[r];
    for (int g = 1; g < groups; ++g) yr = yr + part[(int64_t)g * part_stride + r];  // ascending group order
    const double xr = x_ext[r] * scale;
    if (shift != 0.0) yr = add_product_nofma(yr, shift, xr);  // lanczos.hpp:390-392
    y[r] = yr;
    if (u_out) u_out[r] = xr;
    dot = (pass & kPassSelfNorm) ? fma(yr, yr, dot) : fma(xr, yr, dot);
  }
  if (partials) {
    dot = block_sum(dot, lds4);
    if (threadIdx.x == 0) partials[blockIdx.x] = dot;
  }
}

// Complex fp64 variant (the scalar type of the reference's own samples): entries, x and
// products are 16-byte (re, im) pairs; 1024 products per LDS chunk.  Same two phases, same
// stored-order accumulation; products use separate multiplies and adds (no contraction),
// like a plain C complex multiply.  shift is complex (ArnoldiBase::eigenvalueShift_ is a
// Scalar, arnoldi.hpp:108); partials hold (re, im) of conj(u).y.

__device__ __forceinline__ double2 cmul_nofma(double2 a, double2 b) {
#pragma clang fp contract(off)
  double2 r;
  r.x = a.x * b.x - a.y * b.y;
  r.y = a.x * b.y + a.y * b.x;
  return r;
}

// Split tiles, complex fp64: the same layout with 16-byte (re, im) values, inputs and accumulators (tiles of <= 8192 rows:
// 128 KB of LDS); products are plain complex multiplies without contraction (like k_spmv_z), their parts are added to the row's
// accumulator parts by two LDS atomics.
struct SplitRegsZ {
  uint4 c;
  double2 v0, v1, v2, v3;
  int nvalid;
  int64_t pos0;
};
__device__ __forceinline__ void split_load_z(SplitRegsZ& g, const SplitOperatorView& op, int c, int c1, int tid) {
  g.nvalid = 0;
  if (c >= c1) return;
  const int4 d = op.chunk[c];
  const int q = d.x + 4 * tid;
  g.nvalid = min(4, max(0, d.y - q));
  g.pos0 = d.z;
  if (g.nvalid > 0) {
    const double* v = op.val + 2 * (int64_t)q;
    g.c = *reinterpret_cast<const uint4*>(op.cp + q);
    g.v0 = nt_ld_d2(v), g.v1 = nt_ld_d2(v + 2), g.v2 = nt_ld_d2(v + 4), g.v3 = nt_ld_d2(v + 6);
  }
}
__device__ __forceinline__ void split_gather_z(double2 (&x)[4], const SplitRegsZ& g, const SplitOperatorView& op,
                                               const double2* __restrict__ x_ext) {
  x[0] = x[1] = x[2] = x[3] = make_double2(0.0, 0.0);
  if (g.nvalid > 0) x[0] = x_ext[split_index(op, g.pos0, g.c.x)];
  if (g.nvalid > 1) x[1] = x_ext[split_index(op, g.pos0, g.c.y)];
  if (g.nvalid > 2) x[2] = x_ext[split_index(op, g.pos0, g.c.z)];
  if (g.nvalid > 3) x[3] = x_ext[split_index(op, g.pos0, g.c.w)];
}
__device__ __forceinline__ void split_add1_z(double* acc, unsigned c, double2 v, double2 x, double scale) {
  const double2 p = cmul_nofma(v, make_double2(x.x * scale, x.y * scale));
  double* a = acc + 2 * (int64_t)(c >> kSplitRelBits);
  split_add1(a, p.x);
  split_add1(a + 1, p.y);
}
__global__ __launch_bounds__(kSplitBlock) void k_spmv_split_z(SplitOperatorView op, const double2* __restrict__ x_ext,
                                                             const double* __restrict__ scale_ptr, const Ctrl* __restrict__ ctrl) {
  extern __shared__ double lds_acc[];  // tile_rows (re, im) pairs
  if (ctrl->stopped) return;
  const double scale = scale_ptr ? *scale_ptr : 1.0;
  const int tid = threadIdx.x, T = op.tile_rows;
  const int wg = blockIdx.x, tile = wg / op.groups, grp = wg - tile * op.groups;
  const int c0 = op.wg_chunk[wg], c1 = op.wg_chunk[wg + 1];
  SplitRegsZ r0, r1, r2;
  double2 x0[4], x1[4];
  split_load_z(r0, op, c0, c1, tid);
  split_load_z(r1, op, c0 + 1, c1, tid);
  split_gather_z(x0, r0, op, x_ext);
  for (int i = tid; i < 2 * T; i += kSplitBlock) lds_acc[i] = 0.0;
  __syncthreads();
  for (int c = c0; c < c1; ++c) {
    split_load_z(r2, op, c + 2, c1, tid);
    split_gather_z(x1, r1, op, x_ext);
    if (r0.nvalid > 0) split_add1_z(lds_acc, r0.c.x, r0.v0, x0[0], scale);
    if (r0.nvalid > 1) split_add1_z(lds_acc, r0.c.y, r0.v1, x0[1], scale);
    if (r0.nvalid > 2) split_add1_z(lds_acc, r0.c.z, r0.v2, x0[2], scale);
    if (r0.nvalid > 3) split_add1_z(lds_acc, r0.c.w, r0.v3, x0[3], scale);
    __syncthreads();  // the next chunk may hold the same rows
    r0 = r1, r1 = r2;
#pragma unroll
    for (int i = 0; i < 4; ++i) x0[i] = x1[i];
  }
  const int64_t r0w = (int64_t)tile * T;
  double* dst = op.part + 2 * ((int64_t)grp * op.part_stride + r0w);
  for (int i = tid; i < 2 * T; i += kSplitBlock)
    if (r0w + (i >> 1) < op.nloc) dst[i] = lds_acc[i];
}

__global__ __launch_bounds__(kBlock) void k_split_combine_z(const double2* __restrict__ part, int64_t part_stride, int groups,
                                                           const double2* __restrict__ x_ext, const double* __restrict__ scale_ptr,
                                                           double shift_re, double shift_im, double2* __restrict__ y,
                                                           double2* __restrict__ u_out, int64_t n, double* __restrict__ partials,
                                                           int pstride, int pass, const Ctrl* __restrict__ ctrl) {
  __shared__ double lds4[4];
  if (ctrl->stopped) return;
  const double scale = scale_ptr ? *scale_ptr : 1.0;
  const bool has_shift = shift_re != 0.0 || shift_im != 0.0;
  double dr = 0.0, di = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) {
    double2 yr = part[r];
    for (int g = 1; g < groups; ++g) {  // ascending group order
      const double2 t = part[(int64_t)g * part_stride + r];
      yr.x = yr.x + t.x;
      yr.y = yr.y + t.y;
    }
    double2 xr = x_ext[r];
    xr.x *= scale;
    xr.y *= scale;
    if (has_shift) {
      const double2 t = cmul_nofma(make_double2(shift_re, shift_im), xr);
      yr.x = yr.x + t.x;
      yr.y = yr.y + t.y;
    }
    y[r] = yr;
    if (u_out) u_out[r] = xr;
    if (pass & kPassSelfNorm) {
      dr = fma(yr.x, yr.x, fma(yr.y, yr.y, dr));  // |y|^2
    } else {
      dr = fma(xr.x, yr.x, fma(xr.y, yr.y, dr));  // conj(u) * y
      di = fma(xr.x, yr.y, fma(-xr.y, yr.x, di));
    }
  }
  if (partials) {
    dr = block_sum(dr, lds4);
    di = block_sum(di, lds4);
    if (threadIdx.x == 0) {
      partials[blockIdx.x] = dr;
      partials[pstride + blockIdx.x] = di;
    }
  }
}

template <bool LONG_ROWS>  // as for k_spmv: eight (re, im) products read before they are added, for operators with long rows
__global__ __launch_bounds__(kBlock) void k_spmv_z(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                   const double2* __restrict__ val, const double2* __restrict__ x_ext,
                                                   const double* __restrict__ scale_ptr, double shift_re,
                                                   double shift_im, double2* __restrict__ y,
                                                   double2* __restrict__ u_out, int64_t n, int64_t ntiles,
                                                   double* __restrict__ partials, int pstride, int spmv_flags,
                                                   int pass, const Ctrl* __restrict__ ctrl) {
  __shared__ double2 prod[kSpmvProdSlotsZ];
  __shared__ double lds4[4];
  if (ctrl->stopped) return;
  const double scale = scale_ptr ? *scale_ptr : 1.0;
  const int tid = threadIdx.x;
  const bool has_shift = shift_re != 0.0 || shift_im != 0.0;
  double dr = 0.0, di = 0.0;
  const TileRange tr = spmv_tiles(ntiles, spmv_flags & 1);
  for (int64_t tile = tr.first; tile < tr.end; tile += tr.step) {
    const int64_t r0 = tile * kSpmvRows;
    const int64_t r = r0 + tid;
    int rs = 0, re = 0;
    if (r < n) {
      rs = rowptr[r];
      re = rowptr[r + 1];
    }
    const int64_t rend = (r0 + kSpmvRows < n) ? r0 + kSpmvRows : n;
    const int p0 = rowptr[r0];
    const int p1 = rowptr[rend];
    const int pa = spmv_aligned_start(p0);
    double2 sum = ((pass & kPassCarry) && r < n) ? y[r] : make_double2(0.0, 0.0);
    for (int cb = pa; cb < p1; cb += kSpmvChunkZ) {
      const int cend = spmv_chunk_end(cb, p1, kSpmvChunkZ);
      for (int q = cb + 4 * tid; q < cend; q += 4 * kBlock) {
        const int4 c4 = *reinterpret_cast<const int4*>(col + q);
        const double2 v0 = val[q], v1 = val[q + 1], v2 = val[q + 2], v3 = val[q + 3];
        double2 x0 = x_ext[c4.x], x1 = x_ext[c4.y], x2 = x_ext[c4.z], x3 = x_ext[c4.w];
        x0.x *= scale, x0.y *= scale, x1.x *= scale, x1.y *= scale;
        x2.x *= scale, x2.y *= scale, x3.x *= scale, x3.y *= scale;
        const int li = q - cb;
        prod[skewz(li + 0)] = cmul_nofma(v0, x0);
        prod[skewz(li + 1)] = cmul_nofma(v1, x1);
        prod[skewz(li + 2)] = cmul_nofma(v2, x2);
        prod[skewz(li + 3)] = cmul_nofma(v3, x3);
      }
      __syncthreads();
      const int lo = rs > cb ? rs : cb;
      const int hi = re < cend ? re : cend;
      int p = lo;
      for (; LONG_ROWS && p + 8 <= hi; p += 8) {
        double2 t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = prod[skewz(p + i - cb)];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          sum.x = sum.x + t[i].x;
          sum.y = sum.y + t[i].y;
        }
      }
      for (; p < hi; ++p) {
        const double2 t = prod[skewz(p - cb)];
        sum.x = sum.x + t.x;
        sum.y = sum.y + t.y;
      }
      __syncthreads();
    }
    if ((pass & kPassNotLast) && r < n) {
      y[r] = sum;
    } else if (r < n) {
      double2 xr = x_ext[r];
      xr.x *= scale;
      xr.y *= scale;
      double2 yr = sum;
      if (has_shift) {
        const double2 t = cmul_nofma(make_double2(shift_re, shift_im), xr);
        yr.x = yr.x + t.x;
        yr.y = yr.y + t.y;
      }
      y[r] = yr;
      if (u_out) u_out[r] = xr;
      if (pass & kPassSelfNorm) {
        dr = fma(yr.x, yr.x, fma(yr.y, yr.y, dr));  // |y|^2
      } else {
        dr = fma(xr.x, yr.x, fma(xr.y, yr.y, dr));   // conj(u) * y
        di = fma(xr.x, yr.y, fma(-xr.y, yr.x, di));
      }
    }
  }
  if (partials) {
    dr = block_sum(dr, lds4);
    di = block_sum(di, lds4);
    if (tid == 0) {
      partials[blockIdx.x] = dr;
      partials[pstride + blockIdx.x] = di;
    }
  }
}

// ---------------------------------------------------------------------------
// Block-sparse operator (kernels.hpp: BlockOperatorView), row-per-thread: thread = row, walking its strip's
// columns (stride = rows of the group).  The lanes of one group read consecutive addresses and share the
// column index and the input element of each step, so a wave's load covers (64/rows) contiguous runs of
// rows*8 bytes, all of whose bytes are used; no LDS, no search.  Products are rounded, then added, strip
// columns ascending: the same sums as the CSR row loop.  (An LDS-staged entry-parallel form like k_spmv, with
// a per-tile group table and a hint table for the entry -> group lookup, was built first and ran at less than
// half the speed of the CSR kernel: 0.34 vs 0.18 ms per application at N = 2e6; this form: 0.147 ms.)
// ---------------------------------------------------------------------------
// r3: the input elements of a tile's strips are gathered ONCE per (group, strip column) into LDS by the whole workgroup --
// the cols array is contiguous over consecutive groups, so the tile's gathers are one flat range -- instead of once per
// (row, strip column) by every row's lane: rocprofv3 had shown two thirds of the kernel's 8.3e7 L1 accesses per launch to be
// those per-step index and input loads (profiles/r02_block_sectors.md), with only 55 value requests in flight per CU.  The
// row walk is then value loads (sixteen in flight) and LDS reads that broadcast within a group.  Same products, same
// order: bit-identical to the direct form, which remains for tiles whose strips have more columns than the LDS buffer.
constexpr int kBlockStage = 2048;  // staged input elements per tile (16 KB)
template <int NB, bool STAGED>
__device__ __forceinline__ double block_row_walk(const double* __restrict__ v, int64_t nr, int width, const double* xs,
                                                 const int32_t* __restrict__ cl, const double* __restrict__ x_ext, double scale) {
  double sum = 0.0;
  int j = 0;
  for (; j + NB <= width; j += NB) {
    double a[NB], xv[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) a[t] = v[(int64_t)(j + t) * nr];
#pragma unroll
    for (int t = 0; t < NB; ++t) xv[t] = STAGED ? xs[j + t] : x_ext[cl[j + t]] * scale;
#pragma unroll
    for (int t = 0; t < NB; ++t) sum = add_product_nofma(sum, a[t], xv[t]);
  }
  if (NB > 8 && j + 8 <= width) {
    double a[8], xv[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) a[t] = v[(int64_t)(j + t) * nr];
#pragma unroll
    for (int t = 0; t < 8; ++t) xv[t] = STAGED ? xs[j + t] : x_ext[cl[j + t]] * scale;
#pragma unroll
    for (int t = 0; t < 8; ++t) sum = add_product_nofma(sum, a[t], xv[t]);
    j += 8;
  }
  if (j < width) {  // the last 1..7 columns: their loads in flight together, like a full batch (a serial tail loop cost 3 % at
                    // strip width 30 -- BASELINE config 5's 10-row sectors -- and 8 % at width 6)
    const int m = width - j;
    double a[7], xv[7];
#pragma unroll
    for (int t = 0; t < 7; ++t) a[t] = t < m ? v[(int64_t)(j + t) * nr] : 0.0;
#pragma unroll
    for (int t = 0; t < 7; ++t) xv[t] = t < m ? (STAGED ? xs[j + t] : x_ext[cl[j + t]] * scale) : 0.0;
#pragma unroll
    for (int t = 0; t < 7; ++t)
      if (t < m) sum = add_product_nofma(sum, a[t], xv[t]);
  }
  return sum;
}

__global__ __launch_bounds__(kBlock) void k_block_spmv(BlockOperatorView op, const double* __restrict__ x_ext,
                                                            const double* __restrict__ scale_ptr, double shift,
                                                            double* __restrict__ y, double* __restrict__ u_out, int64_t n,
                                                            int64_t ntiles, double* __restrict__ partials, int pass,
                                                            const Ctrl* __restrict__ ctrl) {
  __shared__ double lds4[4];
  __shared__ double xs[kBlockStage];
  if (ctrl->stopped) return;
  const double scale = scale_ptr ? *scale_ptr : 1.0;
  double dot = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * kBlock, r = r0 + threadIdx.x;
    const int64_t rlast = (r0 + kBlock < n ? r0 + kBlock : n) - 1;
    const int64_t c_first = op.gcol[op.rowgrp[r0]], c_end = op.gcol[op.rowgrp[rlast] + 1];  // the tile's strip columns: one range of cols
    const bool staged = c_end - c_first <= kBlockStage;
    if (staged) {
      for (int i = threadIdx.x; i < (int)(c_end - c_first); i += kBlock) xs[i] = x_ext[op.cols[c_first + i]] * scale;
      __syncthreads();
    }
    if (r < n) {
      const int g = op.rowgrp[r];
      const int gr0 = op.grow0[g], nr = op.grow0[g + 1] - gr0;
      const int64_t ge = op.gent[g];
      const int width = (int)((op.gent[g + 1] - ge) / nr);
      const double* v = op.bval + ge + (r - gr0);
      const int64_t gc = op.gcol[g];
      const double sum = staged ? block_row_walk<16, true>(v, nr, width, xs + (gc - c_first), nullptr, nullptr, scale)
                                : block_row_walk<8, false>(v, nr, width, nullptr, op.cols + gc, x_ext, scale);
      const double xr = x_ext[r] * scale;
      double yr = sum;
      if (shift != 0.0) yr = add_product_nofma(yr, shift, xr);  // lanczos.hpp:390-392
      y[r] = yr;
      if (u_out) u_out[r] = xr;
      dot = (pass & kPassSelfNorm) ? fma(yr, yr, dot) : fma(xr, yr, dot);
    }
    if (staged) __syncthreads();  // the next tile's staging overwrites xs
  }
  if (partials) {
    dot = block_sum(dot, lds4);
    if (threadIdx.x == 0) partials[blockIdx.x] = dot;
  }
}

// ---------------------------------------------------------------------------
// Matrix-free spin-1/2 operator, one row per lane under the contract of k_block_spmv; spin_rows.hpp has the row walk (the lane's
// state, the diagonal, the flips in batches of kSpinBatch) and these kernels call it with the accessors below.  The kernel
// streams no operator at all: the model tables (SpinOperatorView, the head of SpinSectorView) are a few hundred bytes that every
// lane reads at the same index (scalar loads).  No LDS staging of x.
//   SECTOR = false (spin_model.hpp): row s is state s, only op->model is read and the table pointers are null.  A flip reads
//     x[s ^ mask], which keeps the lane's low bits: a mask above bit 5 moves a wave's 512 contiguous bytes to another place as a
//     whole, one inside bits 0..5 permutes the wave's own 512 bytes, bits 6..7 stay in the tile.
//   SECTOR = true (spin_sector.hpp): row r is the state of rank r, unranked from the binomials C(p, k), which the workgroup keeps
//     in LDS (k differs between lanes, so the read is a per-lane LDS address).  No per-row state array in memory: the operator
//     is the model table and the two rank tables (at most 2^16 words each: they stay in L2).
// The sums are those of the CSR row loop over eigenex_spin_csr's / eigenex_spin_sector_csr's rows.
// ---------------------------------------------------------------------------
struct SpinBinomials32 {  // C(p, k) in LDS
  const uint32_t* c;
  __device__ __forceinline__ uint32_t operator()(int i) const { return c[i]; }
};
struct SpinRankTables {
  const uint32_t *lo_rank, *hi_base;
  __device__ __forceinline__ uint32_t hi(uint32_t i) const { return hi_base[i]; }
  __device__ __forceinline__ uint32_t lo(uint32_t i) const { return lo_rank[i]; }
};
// Every kernel of a vector's elements is written once for E = double and E = SpinZ (spin_rows.hpp), an interleaved complex
// vector.  SpinElement<E> has what the device adds: the type an element is loaded and stored as (one 8-byte or one 16-byte
// access) and the accessor of the walk.
struct SpinVector {
  const double* x;
  __device__ __forceinline__ double operator()(uint32_t i) const { return x[i]; }
};
struct SpinVectorZ {
  const double2* x;
  __device__ __forceinline__ SpinZ operator()(uint32_t i) const {
    const double2 v = x[i];
    return SpinZ{v.x, v.y};
  }
};
template <class E>
struct SpinElement {
  using Stored = double;
  using Vector = SpinVector;
};
template <>
struct SpinElement<SpinZ> {
  using Stored = double2;
  using Vector = SpinVectorZ;
};
__device__ __forceinline__ double spin_loaded(double v) { return v; }
__device__ __forceinline__ SpinZ spin_loaded(double2 v) { return SpinZ{v.x, v.y}; }
__device__ __forceinline__ double spin_stored(double v) { return v; }
__device__ __forceinline__ double2 spin_stored(SpinZ v) { return make_double2(v.re, v.im); }

// the workgroup's copy of the binomials; the caller synchronises
__device__ __forceinline__ void spin_stage_binomials(const SpinSectorView* __restrict__ op, uint32_t* binom) {
  constexpr int kCols = kSectorMaxSites + 1;
  for (int i = threadIdx.x; i < kSectorMaxSites * kCols; i += kBlock) binom[i] = op->binom[i / kCols][i % kCols];
}

// y = (H + shift) (x * scale).  On an interleaved complex vector it is the same real operator: the row walk is taken once per row
// for both parts (state, diagonal, flip targets and the rank-table gathers), x is gathered as 16-byte loads and each part
// accumulates the real sum of that part (spin_rows.hpp: spin_add_flips).  The shift is then complex, and the two partial dots,
// conj(u) . y or |y|^2, follow k_spmv_z, with the second set at partials[pstride + workgroup] -- except that a norm
// (kPassSelfNorm) leaves the second set unwritten: it is one real sum with one set of readers, and one of its callers hands
// over a buffer of pstride doubles (library.hip: palpha).  The two arguments that only a complex vector has, shift_im and
// pstride, are expansions of the pack ComplexOnly: <int> for E = SpinZ, empty for double, whose kernel so keeps its single
// shift and its one set of partials.  (As scalar arguments and not as members of E or of a struct: the loads of a struct argument
// are not merged with the other arguments' loads.)  u_out, the pass bits and ctrl->stopped are the same for both.
template <class>
using SpinShiftIm = double;

template <bool SECTOR, class E, class... ComplexOnly>
__global__ __launch_bounds__(kBlock) void k_spin_spmv(const SpinSectorView* __restrict__ op, const uint32_t* __restrict__ lo_rank,
                                                      const uint32_t* __restrict__ hi_base,
                                                      const typename SpinElement<E>::Stored* __restrict__ x_ext,
                                                      const double* __restrict__ scale_ptr, double shift, SpinShiftIm<ComplexOnly>... shift_im,
                                                      typename SpinElement<E>::Stored* __restrict__ y,
                                                      typename SpinElement<E>::Stored* __restrict__ u_out, int64_t n, int64_t ntiles,
                                                      double* __restrict__ partials, ComplexOnly... pstride, int pass,
                                                      const Ctrl* __restrict__ ctrl) {
  static_assert(sizeof...(ComplexOnly) == (std::is_same<E, SpinZ>::value ? 1 : 0), "shift_im and pstride for complex vectors only");
  constexpr bool COMPLEX = std::is_same<E, SpinZ>::value;
  __shared__ double lds4[4];
  __shared__ uint32_t binom[SECTOR ? kSectorMaxSites * (kSectorMaxSites + 1) : 1];
  if (ctrl->stopped) return;
  int n_up = 0, h = 0;
  uint32_t lo_mask = 0;
  if constexpr (SECTOR) {
    spin_stage_binomials(op, binom);
    __syncthreads();
    n_up = op->n_up, h = op->h, lo_mask = op->lo_mask;
  }
  const double scale = scale_ptr ? *scale_ptr : 1.0;
  bool has_shift = false;  // a complex shift is tested once, here
  if constexpr (COMPLEX) has_shift = shift != 0.0 || (shift_im + ...) != 0.0;
  const SpinOperatorView* model = &op->model;
  const int n_sites = model->n_sites, ndiag = model->ndiag, nflip = model->nflip;
  const SpinRankTables tab{lo_rank, hi_base};
  double dot = 0.0, dot_im = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r = tile * kBlock + threadIdx.x;
    if (r < n) {
      const uint32_t s = SECTOR ? spin_unrank_row(SpinBinomials32{binom}, n_sites, n_up, (uint32_t)r).s : (uint32_t)r;
      const double d = spin_row_diagonal(model->dmask, model->dval, ndiag, s);
      const E xr = spin_scaled(spin_loaded(x_ext[r]), scale);  // the row's own element by its 64-bit index, not through the accessor
      E yr = spin_add_product(E{}, d, xr);
      for (int t0 = 0; t0 < nflip; t0 += kSpinBatch) {
        bool on[kSpinBatch];
        uint32_t base[kSpinBatch], low[kSpinBatch];
        E xv[kSpinBatch];
        spin_flip_targets<SECTOR>(model->fmask + t0, s, tab, h, lo_mask, on, base, low);
        spin_gather(typename SpinElement<E>::Vector{x_ext}, base, low, xv);
        yr = spin_add_flips(yr, model->fval + t0, on, xv, scale);
      }
      if constexpr (COMPLEX) {
        if (has_shift) {
          const double2 t = cmul_nofma(make_double2(shift, (shift_im + ...)), spin_stored(xr));
          yr.re = yr.re + t.x;
          yr.im = yr.im + t.y;
        }
      } else {
        if (shift != 0.0) yr = add_product_nofma(yr, shift, xr);  // lanczos.hpp:390-392
      }
      y[r] = spin_stored(yr);
      if (u_out) u_out[r] = spin_stored(xr);
      if constexpr (COMPLEX) {
        if (pass & kPassSelfNorm) {
          dot = fma(yr.re, yr.re, fma(yr.im, yr.im, dot));  // |y|^2
        } else {
          dot = fma(xr.re, yr.re, fma(xr.im, yr.im, dot));  // conj(u) * y
          dot_im = fma(xr.re, yr.im, fma(-xr.im, yr.re, dot_im));
        }
      } else {
        dot = (pass & kPassSelfNorm) ? fma(yr, yr, dot) : fma(xr, yr, dot);
      }
    }
  }
  if (partials) {
    dot = block_sum(dot, lds4);
    if constexpr (COMPLEX) dot_im = block_sum(dot_im, lds4);
    if (threadIdx.x == 0) {
      partials[blockIdx.x] = dot;
      // a norm is one set of partials: its readers have room for one
      if constexpr (COMPLEX)
        if (!(pass & kPassSelfNorm)) partials[(pstride + ...) + blockIdx.x] = dot_im;
    }
  }
}

// ---------------------------------------------------------------------------
// Spin correlations of one vector (spin_measure.hpp has the definition and SpinMeasureChunk): x streams past once per chunk of
// kSpinMeasureChunk diagonal and as many flip masks and no vector is written.  One row per lane, 256-row tiles, the operator
// kernels' persistent grid, state and batches (spin_rows.hpp); the chunk is a table that every lane reads at the same index
// (scalar loads).  The 2 C + 1 sums (norm2, diag, flip) stay in registers across the tile loop -- every register index is a
// constant after unrolling, a batch is skipped as a whole where the chunk has no term in it -- and leave through block_sum into
// partials[sum * pstride + workgroup]; k_spin_measure_reduce adds those in k_reduce_fin's order.  No atomics: a result depends on
// the grid only through the grouping of the partial sums.  ctrl->stopped is not consulted: a measurement is not a Krylov step.
// Of an interleaved complex vector (E = SpinZ) the sums are the Hermitian ones of spin_measure.hpp: |x_s|^2 for x_s^2 and
// Re(conj(x_s) x_{s ^ mask}) for the product of a flip, two fmas per term (real part, then imaginary part); chunks, registers,
// partials and the second stage are the same, and x is read as 16-byte loads.
// ---------------------------------------------------------------------------
template <bool SECTOR, class E>
__global__ __launch_bounds__(kBlock) void k_spin_measure(const SpinMeasureChunk* __restrict__ ch, const SpinSectorView* __restrict__ op,
                                                         const uint32_t* __restrict__ lo_rank, const uint32_t* __restrict__ hi_base,
                                                         const typename SpinElement<E>::Stored* __restrict__ x, int64_t n, int64_t ntiles,
                                                         double* __restrict__ partials, int pstride) {
  constexpr int C = kSpinMeasureChunk;
  __shared__ double lds4[4];
  __shared__ uint32_t binom[SECTOR ? kSectorMaxSites * (kSectorMaxSites + 1) : 1];
  int n_sites = 0, n_up = 0, h = 0;
  uint32_t lo_mask = 0;
  if constexpr (SECTOR) {
    spin_stage_binomials(op, binom);
    __syncthreads();
    n_sites = op->model.n_sites, n_up = op->n_up, h = op->h, lo_mask = op->lo_mask;
  }
  const int ndiag = ch->ndiag, nflip = ch->nflip;
  const SpinRankTables tab{lo_rank, hi_base};
  double nrm = 0.0, dg[C], fl[C];
#pragma unroll
  for (int t = 0; t < C; ++t) dg[t] = 0.0, fl[t] = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r = tile * kBlock + threadIdx.x;
    if (r < n) {
      const uint32_t s = SECTOR ? spin_unrank_row(SpinBinomials32{binom}, n_sites, n_up, (uint32_t)r).s : (uint32_t)r;
      E xs;  // the row's own element: a real one by its 64-bit index, a complex one through the 32-bit accessor, as measured
      if constexpr (std::is_same<E, SpinZ>::value)
        xs = SpinVectorZ{x}((uint32_t)r);
      else
        xs = x[r];
      nrm = spin_norm_add(nrm, xs);
#pragma unroll
      for (int t0 = 0; t0 < C; t0 += kSpinBatch)
        if (t0 < ndiag) spin_measure_diagonals(xs, s, ch->dmask + t0, dg + t0);
#pragma unroll
      for (int t0 = 0; t0 < C; t0 += kSpinBatch)
        if (t0 < nflip) {
          bool on[kSpinBatch];
          uint32_t base[kSpinBatch], low[kSpinBatch];
          E xv[kSpinBatch];
          spin_flip_targets<SECTOR>(ch->fmask + t0, s, tab, h, lo_mask, on, base, low);
          spin_gather(typename SpinElement<E>::Vector{x}, base, low, xv);
          spin_measure_flips(xs, on, xv, fl + t0);
        }
    }
  }
  const auto put = [&](int a, double mine) {  // sum a of this workgroup: 0 norm2, 1 + t diag, 1 + C + t flip
    const double v = block_sum(mine, lds4);
    if (threadIdx.x == 0) partials[(int64_t)a * pstride + blockIdx.x] = v;
  };
  put(0, nrm);
#pragma unroll
  for (int t = 0; t < C; ++t) put(1 + t, dg[t]);
#pragma unroll
  for (int t = 0; t < C; ++t) put(1 + C + t, fl[t]);
}

// Second stage of k_spin_measure, one workgroup per sum (0: norm2, 1..C: diag, C+1..2C: flip), the partials of the nblocks
// workgroups added in k_reduce_fin's order.  A sum beyond the chunk's live terms has no destination and is dropped.
__global__ __launch_bounds__(kBlock) void k_spin_measure_reduce(const double* __restrict__ partials, int pstride, int nblocks, int ndiag,
                                                                int nflip, double* __restrict__ diag_out, double* __restrict__ flip_out,
                                                                double* __restrict__ norm_out) {
  constexpr int C = kSpinMeasureChunk;
  __shared__ double lds4[4];
  const int a = blockIdx.x;
  double* dst = a == 0 ? norm_out : (a <= C ? (a - 1 < ndiag ? diag_out + (a - 1) : nullptr) : (a - 1 - C < nflip ? flip_out + (a - 1 - C) : nullptr));
  if (!dst) return;  // the same for the whole workgroup
  const double* p = partials + (int64_t)a * pstride;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += kBlock) s += p[b];
  s = block_sum(s, lds4);
  if (threadIdx.x == 0) *dst = s;
}

// ---------------------------------------------------------------------------
// The observables of one vector against basis columns (spin_measure_columns.hpp has the definition, spin_rows.hpp the row:
// spin_measure_columns_row): out[t][j] = <V_j| A_t |x> for one chunk of kSpinMeasureChunk diagonal and as many flip masks
// (SpinMeasureChunk, read by every lane at the same index and never written) and ncols <= J = kSpinMeasureColumns columns
// V, V + ldv, ...  k_spin_measure's persistent grid, 256-row tiles, LDS binomials and batches.  Per row the lane's state, its
// own element of x, the rank-table gathers and the gathered x are taken once and meet J column elements, loaded non-temporally
// as the basis is in k_dots.  A column beyond ncols is read as column ncols - 1 (inside the basis; its sums have no destination),
// so a sum's bits do not depend on what else shares the launch.  The 2 C J sums stay in registers across the tile loop and leave
// through block_sum into partials[sum * pstride + workgroup], sum = t * J + j (diag) and (C + t) * J + j (flip);
// k_spin_measure_columns_reduce adds those in k_reduce_fin's order.  No atomics.  ctrl->stopped is not consulted.
// The column chunk J.  Per row and launch the basis contributes 8 J bytes, and whatever J is the basis streams past
// ceil(terms / C) times in all.  What falls with J is the rest of the row, which is paid once per launch: the own element (8
// bytes from HBM or L2), up to 16 gathers of x (128 bytes, L2 at best) and in a sector 32 rank-table gathers (128 bytes, L2),
// and the unranking.  At J = 1 that is 264 bytes of gathers per 8 basis bytes, at J = 4 per 32.  The sums cost 2 C J = 128
// doubles = 256 VGPRs at J = 4, next to one batch (on, base, low, xv: about 40) and the row: J = 8 would need 512 for the sums
// alone and cannot be had without spilling.  J = 4 compiles to 256 VGPRs + 32 (sector) or 38 (full space) AGPRs, one wave per
// SIMD, without scratch.  The fmas are 2 C = 32 per basis element whatever J is, 0.7 of the columns' HBM time at 64 fp64 fmas
// per clock and CU.  Measured (profiles/spin_thermal.md), neither bounds the kernel: at one wave per SIMD nothing hides the chain
// load - unrank - gather - gather of a row, and a pass of the basis takes 9 (diagonal terms only) to 18 (16 + 16 terms) times
// eigenex_dots' sweep of the same columns.  A smaller J buys occupancy with as many more launches: the sums per SIMD, J times the
// waves, stay what the register file holds.  What would help is more rows in flight per lane (the sums are shared between them,
// only the row's own 50 registers multiply); not done here.
// ---------------------------------------------------------------------------
template <bool SECTOR>
__global__ __launch_bounds__(kBlock) void k_spin_measure_columns(const SpinMeasureChunk* __restrict__ ch, const SpinSectorView* __restrict__ op,
                                                                 const uint32_t* __restrict__ lo_rank, const uint32_t* __restrict__ hi_base,
                                                                 const double* __restrict__ x, const double* __restrict__ V, int64_t ldv,
                                                                 int ncols, int64_t n, int64_t ntiles, double* __restrict__ partials,
                                                                 int pstride) {
  constexpr int C = kSpinMeasureChunk, J = kSpinMeasureColumns;
  __shared__ double lds4[4];
  __shared__ uint32_t binom[SECTOR ? kSectorMaxSites * (kSectorMaxSites + 1) : 1];
  int n_sites = 0, n_up = 0, h = 0;
  uint32_t lo_mask = 0;
  if constexpr (SECTOR) {
    spin_stage_binomials(op, binom);
    __syncthreads();
    n_sites = op->model.n_sites, n_up = op->n_up, h = op->h, lo_mask = op->lo_mask;
  }
  const int ndiag = ch->ndiag, nflip = ch->nflip;
  const SpinRankTables tab{lo_rank, hi_base};
  const double* col[J];
#pragma unroll
  for (int j = 0; j < J; ++j) col[j] = V + (int64_t)(j < ncols ? j : ncols - 1) * ldv;
  double dg[C * J], fl[C * J];
#pragma unroll
  for (int i = 0; i < C * J; ++i) dg[i] = 0.0, fl[i] = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r = tile * kBlock + threadIdx.x;
    if (r < n) {
      double v[J];
#pragma unroll
      for (int j = 0; j < J; ++j) v[j] = __builtin_nontemporal_load(col[j] + r);
      const uint32_t s = SECTOR ? spin_unrank_row(SpinBinomials32{binom}, n_sites, n_up, (uint32_t)r).s : (uint32_t)r;
      spin_measure_columns_row<SECTOR>(ch->dmask, ndiag, ch->fmask, nflip, s, x[r], SpinVector{x}, tab, h, lo_mask, v, dg, fl);
    }
  }
  const auto put = [&](int a, double mine) {
    const double sum = block_sum(mine, lds4);
    if (threadIdx.x == 0) partials[(int64_t)a * pstride + blockIdx.x] = sum;
  };
  // a batch without a term has nothing but zeros: its sums are not reduced, and the second stage does not read them
#pragma unroll
  for (int t0 = 0; t0 < C; t0 += kSpinBatch)
    if (t0 < ndiag) {
#pragma unroll
      for (int i = t0 * J; i < (t0 + kSpinBatch) * J; ++i) put(i, dg[i]);
    }
#pragma unroll
  for (int t0 = 0; t0 < C; t0 += kSpinBatch)
    if (t0 < nflip) {
#pragma unroll
      for (int i = t0 * J; i < (t0 + kSpinBatch) * J; ++i) put(C * J + i, fl[i]);
    }
}

// Second stage of k_spin_measure_columns, one workgroup per sum a = (kind * C + t) * J + j, the partials of the nblocks workgroups
// added in k_reduce_fin's order and stored to diag_out[t * ldo + j] (kind 0) or flip_out[t * ldo + j] (kind 1).  A sum beyond the
// chunk's live terms or the launch's live columns has no destination and is dropped.
__global__ __launch_bounds__(kBlock) void k_spin_measure_columns_reduce(const double* __restrict__ partials, int pstride, int nblocks, int ndiag,
                                                                        int nflip, int ncols, int ldo, double* __restrict__ diag_out,
                                                                        double* __restrict__ flip_out) {
  constexpr int C = kSpinMeasureChunk, J = kSpinMeasureColumns;
  __shared__ double lds4[4];
  const int a = blockIdx.x, kind = a / (C * J), t = (a % (C * J)) / J, j = a % J;
  if (j >= ncols || t >= (kind == 0 ? ndiag : nflip)) return;  // the same for the whole workgroup
  double* dst = (kind == 0 ? diag_out : flip_out) + (int64_t)t * ldo + j;
  const double* p = partials + (int64_t)a * pstride;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += kBlock) s += p[b];
  s = block_sum(s, lds4);
  if (threadIdx.x == 0) *dst = s;
}

// ---------------------------------------------------------------------------
// A sum of site operators applied to a vector (spin_site.hpp has the definition and SpinSiteTable; spin_rows.hpp the walk): one
// row of the DESTINATION per lane, 256-row tiles, the operator kernels' persistent grid and LDS binomials.  dst_op is the
// destination operator's view (its binomials and n_up unrank the row; not read in the full space), src_lo and src_hi are the
// SOURCE operator's rank tables: a flipped state has the source's number of up sites.  A lane without a term ranks the table's
// fallback state, row 0 of the source, and its sum ignores what it loaded (spin_rows.hpp says why its own row will not do).
// The table is read by every lane at the same index (scalar loads); x is not staged in LDS.  Z reads and writes only the lane's
// own element, so y may be x there; for the flips the caller keeps them apart.  norm2 = sum y_r^2 leaves through block_sum
// into partials[workgroup]; k_spin_measure_reduce adds those in k_reduce_fin's order.  No atomics.  ctrl->stopped is not
// consulted: this is not a Krylov step.
// Of an interleaved complex vector (E = SpinZ) the coefficients are complex and the table's real_coef says whether any has an
// imaginary part; without one, each part of y is the real kernel's y of that part of x.  x is gathered as 16-byte loads, y is one
// 16-byte store, norm2 = sum |y_r|^2; the state, the targets and the rank-table gathers are taken once per row for both parts.
// ---------------------------------------------------------------------------
template <bool SECTOR, class E>
__global__ __launch_bounds__(kBlock) void k_spin_site_apply(const SpinSiteTable* __restrict__ tb, const SpinSectorView* __restrict__ dst_op,
                                                            const uint32_t* __restrict__ src_lo, const uint32_t* __restrict__ src_hi,
                                                            const typename SpinElement<E>::Stored* x, typename SpinElement<E>::Stored* y,
                                                            int64_t n, int64_t ntiles, double* __restrict__ partials) {
  __shared__ double lds4[4];
  __shared__ uint32_t binom[SECTOR ? kSectorMaxSites * (kSectorMaxSites + 1) : 1];
  int n_up = 0, h = 0;
  uint32_t lo_mask = 0;
  if constexpr (SECTOR) {
    spin_stage_binomials(dst_op, binom);
    __syncthreads();
    n_up = dst_op->n_up, h = dst_op->h, lo_mask = dst_op->lo_mask;
  }
  const int kind = tb->kind, n_sites = tb->n_sites;
  const uint32_t site_mask = tb->site_mask, fallback = tb->fallback;
  bool real_coef = true;  // read once, here: the branches on it are uniform; a real vector has no imaginary coefficients
  if constexpr (std::is_same<E, SpinZ>::value) real_coef = tb->real_coef != 0;
  const SpinRankTables tab{src_lo, src_hi};
  double nrm = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r = tile * kBlock + threadIdx.x;
    if (r < n) {
      const uint32_t s = SECTOR ? spin_unrank_row(SpinBinomials32{binom}, n_sites, n_up, (uint32_t)r).s : (uint32_t)r;
      E yr = E{};
      if (kind == kSpinSiteZ) {
        const E w = spin_site_weights(SpinSiteCoefficients{tb->half, tb->half_im, real_coef}, n_sites, s, E{});
        yr = spin_site_product(w, real_coef, spin_loaded(x[r]));
      } else {
        const uint32_t has = kind == kSpinSitePlus ? s : ~s & site_mask;
        for (int i0 = 0; i0 < n_sites; i0 += kSpinBatch) {
          bool on[kSpinBatch];
          uint32_t base[kSpinBatch], low[kSpinBatch];
          E xv[kSpinBatch];
          spin_site_targets<SECTOR>(i0, s, has, fallback, tab, h, lo_mask, on, base, low);
          spin_gather(typename SpinElement<E>::Vector{x}, base, low, xv);
          yr = spin_site_add(yr, SpinSiteCoefficients{tb->coef + i0, tb->coef_im + i0, real_coef}, on, xv);
        }
      }
      y[r] = spin_stored(yr);
      nrm = spin_norm_add(nrm, yr);
    }
  }
  nrm = block_sum(nrm, lds4);
  if (threadIdx.x == 0) partials[blockIdx.x] = nrm;
}

// ---------------------------------------------------------------------------
// Matrix-free spin-1/2 operator in a momentum sector (spin_momentum.hpp has the definition, spin_rows.hpp the walk): one row
// per lane, 256-row tiles, the persistent grid and the pass, shift, u_out, partials and ctrl->stopped conventions of
// k_spin_spmv<SECTOR, E>.  The lane's state is its representative reps[r], one coalesced load; its period comes from the same
// orbit walk as the flips'.  The model tables are read by every lane at the same index (scalar loads); ratio, phase and inv_sqrt
// are indexed per lane and live in LDS (9.5 KB).  reps and bucket are searched per term, `steps` dependent 4-byte gathers
// inside one bucket, which is a contiguous run of reps.  x is gathered as 8-byte or 16-byte loads, kSpinBatch at a time, all
// issued before the first product is added.  The sums are those of the CSR row loop over eigenex_spin_momentum_csr's rows:
// k_spmv's for E = double on val.re at a real momentum, k_spmv_z's for E = SpinZ.
// ---------------------------------------------------------------------------
// The state word is a parameter: Word = uint32_t for sectors of up to 32 sites, uint64_t for those of up to 48 (reps is then
// 8 bytes per row, still one coalesced load, and the LDS tables are 19.9 KB).  SpinWord<Word> (spin_rows.hpp) has the table sizes
// of either and SpinMomentumViewOf<Word> is its view; the kernel text is the same.
template <class Word>
struct SpinMomentumLookupOf {
  const Word* reps_;
  const uint32_t* bucket_;
  __device__ __forceinline__ Word reps(uint32_t i) const { return reps_[i]; }
  __device__ __forceinline__ uint32_t bucket(uint32_t i) const { return bucket_[i]; }
};
using SpinMomentumLookup = SpinMomentumLookupOf<uint32_t>;
template <class Word>
struct SpinMomentumLdsOf {  // the workgroup's copy of SpinMomentumTablesOf<Word>
  const double* t;
  static constexpr int kPitch = SpinWord<Word>::kRatioPitch, kMaxPeriod = SpinWord<Word>::kMaxPeriod;
  static constexpr int kRatio = 0, kInvSqrt = kPitch * kPitch, kPhaseRe = kInvSqrt + kPitch, kPhaseIm = kPhaseRe + kMaxPeriod,
                       kSize = kPhaseIm + kMaxPeriod;
  __device__ __forceinline__ double ratio(int i) const { return t[kRatio + i]; }
  __device__ __forceinline__ double inv_sqrt(int i) const { return t[kInvSqrt + i]; }
  __device__ __forceinline__ double phase_re(int i) const { return t[kPhaseRe + i]; }
  __device__ __forceinline__ double phase_im(int i) const { return t[kPhaseIm + i]; }
};
using SpinMomentumLds = SpinMomentumLdsOf<uint32_t>;
static_assert(sizeof(SpinMomentumTables) == sizeof(double) * SpinMomentumLds::kSize, "the LDS copy is the struct, member by member");
static_assert(sizeof(SpinMomentum64Tables) == sizeof(double) * SpinMomentumLdsOf<uint64_t>::kSize, "the LDS copy is the struct, member by member");
// the caller synchronises
template <class View>
__device__ __forceinline__ void spin_stage_momentum_tables(const View* __restrict__ op, double* tab) {
  const double* src = reinterpret_cast<const double*>(&op->tab);
  constexpr int kSize = (int)(sizeof(op->tab) / sizeof(double));
  for (int i = threadIdx.x; i < kSize; i += kBlock) tab[i] = src[i];
}

template <class E, class Word, class... ComplexOnly>
__global__ __launch_bounds__(kBlock) void k_spin_momentum_spmv(const SpinMomentumViewOf<Word>* __restrict__ op,
                                                               const Word* __restrict__ reps, const uint32_t* __restrict__ bucket,
                                                               const typename SpinElement<E>::Stored* __restrict__ x_ext,
                                                               const double* __restrict__ scale_ptr, double shift,
                                                               SpinShiftIm<ComplexOnly>... shift_im, typename SpinElement<E>::Stored* __restrict__ y,
                                                               typename SpinElement<E>::Stored* __restrict__ u_out, int64_t n, int64_t ntiles,
                                                               double* __restrict__ partials, ComplexOnly... pstride, int pass,
                                                               const Ctrl* __restrict__ ctrl) {
  static_assert(sizeof...(ComplexOnly) == (std::is_same<E, SpinZ>::value ? 1 : 0), "shift_im and pstride for complex vectors only");
  constexpr bool COMPLEX = std::is_same<E, SpinZ>::value;
  __shared__ double lds4[4];
  __shared__ double tables[SpinMomentumLdsOf<Word>::kSize];
  if (ctrl->stopped) return;
  spin_stage_momentum_tables(op, tables);
  __syncthreads();
  const double scale = scale_ptr ? *scale_ptr : 1.0;
  bool has_shift = false;  // a complex shift is tested once, here
  if constexpr (COMPLEX) has_shift = shift != 0.0 || (shift_im + ...) != 0.0;
  const auto* model = &op->model;
  const int n_sites = model->n_sites, ndiag = model->ndiag, nflip = model->nflip;
  const int cell = op->cell, n_trans = op->n_trans, h = op->h, steps = op->steps;
  const Word compatible = op->compatible;
  const SpinMomentumLookupOf<Word> lk{reps, bucket};
  const SpinMomentumLdsOf<Word> tb{tables};
  double dot = 0.0, dot_im = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r = tile * kBlock + threadIdx.x;
    if (r < n) {
      const Word s = reps[r];
      const int period = spin_orbit(s, n_sites, cell, n_trans).period;
      const double d = spin_row_diagonal(model->dmask, model->dval, ndiag, s);
      const E xraw = spin_loaded(x_ext[r]);
      const E xr = spin_scaled(xraw, scale);
      E yr = spin_momentum_add(E{}, SpinZ{d, 0.0}, xraw, scale);
      for (int t0 = 0; t0 < nflip; t0 += kSpinBatch) {
        bool on[kSpinBatch];
        uint32_t column[kSpinBatch];
        int ri[kSpinBatch], li[kSpinBatch];
        E xv[kSpinBatch];
        spin_momentum_targets(model->fmask + t0, s, period, n_sites, cell, n_trans, compatible, h, steps, lk, on, column, ri, li);
        spin_momentum_gather(typename SpinElement<E>::Vector{x_ext}, column, xv);
        yr = spin_momentum_add_flips(yr, model->fval + t0, tb, on, ri, li, xv, scale);
      }
      if constexpr (COMPLEX) {
        if (has_shift) {
          const double2 t = cmul_nofma(make_double2(shift, (shift_im + ...)), spin_stored(xr));
          yr.re = yr.re + t.x;
          yr.im = yr.im + t.y;
        }
      } else {
        if (shift != 0.0) yr = add_product_nofma(yr, shift, xr);  // lanczos.hpp:390-392
      }
      y[r] = spin_stored(yr);
      if (u_out) u_out[r] = spin_stored(xr);
      if constexpr (COMPLEX) {
        if (pass & kPassSelfNorm) {
          dot = fma(yr.re, yr.re, fma(yr.im, yr.im, dot));  // |y|^2
        } else {
          dot = fma(xr.re, yr.re, fma(xr.im, yr.im, dot));  // conj(u) * y
          dot_im = fma(xr.re, yr.im, fma(-xr.im, yr.re, dot_im));
        }
      } else {
        dot = (pass & kPassSelfNorm) ? fma(yr, yr, dot) : fma(xr, yr, dot);
      }
    }
  }
  if (partials) {
    dot = block_sum(dot, lds4);
    if constexpr (COMPLEX) dot_im = block_sum(dot_im, lds4);
    if (threadIdx.x == 0) {
      partials[blockIdx.x] = dot;
      // a norm is one set of partials: its readers have room for one
      if constexpr (COMPLEX)
        if (!(pass & kPassSelfNorm)) partials[(pstride + ...) + blockIdx.x] = dot_im;
    }
  }
}

// Diagonal correlations of one vector in the momentum basis (spin_momentum.hpp has the definition and the chunk): x and reps
// stream past once per chunk of kSpinMeasureChunk masks and no vector is written.  One row per lane, 256-row tiles, the
// persistent grid; the lane's state is reps[r], one coalesced load, and every lane rotates it n_trans times, the chunk's masks
// applied to each rotation (spin_rows.hpp: spin_momentum_measure_diagonals).  The C + 1 sums stay in registers across the tile
// loop and leave through block_sum into partials[sum * pstride + workgroup]; k_spin_measure_reduce adds those in k_reduce_fin's
// order (its flip sums are not written and not read).  No atomics.  ctrl->stopped is not consulted.
template <class E, class Word>
__global__ __launch_bounds__(kBlock) void k_spin_momentum_measure(const SpinMomentumMeasureChunk* __restrict__ ch, const Word* __restrict__ reps,
                                                                  const typename SpinElement<E>::Stored* __restrict__ x, int n_sites, int cell,
                                                                  int n_trans, int64_t n, int64_t ntiles, double* __restrict__ partials,
                                                                  int pstride) {
  constexpr int C = kSpinMeasureChunk;
  __shared__ double lds4[4];
  const int ndiag = ch->ndiag;
  double nrm = 0.0, dg[C];
#pragma unroll
  for (int t = 0; t < C; ++t) dg[t] = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r = tile * kBlock + threadIdx.x;
    if (r < n) {
      const Word s = reps[r];
      const E xs = spin_loaded(x[r]);
      nrm = spin_norm_add(nrm, xs);
      const double w = spin_momentum_weight(xs);
#pragma unroll
      for (int t0 = 0; t0 < C; t0 += kSpinBatch)
        if (t0 < ndiag) spin_momentum_measure_diagonals(w, s, ch->dmask + t0, n_sites, cell, n_trans, dg + t0);
    }
  }
  const auto put = [&](int a, double mine) {  // sum a of this workgroup: 0 norm2, 1 + t diag
    const double v = block_sum(mine, lds4);
    if (threadIdx.x == 0) partials[(int64_t)a * pstride + blockIdx.x] = v;
  };
  put(0, nrm);
#pragma unroll
  for (int t = 0; t < C; ++t) put(1 + t, dg[t]);
}

// expand (spin_momentum.hpp): y = the Sz-sector vector of the momentum vector x.  One row of the DESTINATION per lane, unranked
// with the destination's binomials (dst_op; LDS); the orbit, the lookup, one gather and one product are spin_momentum_expand_row.
// A lane whose representative does not carry the momentum looks up the sector's first row and writes 0.  norm2 = sum |y_r|^2
// leaves through block_sum into partials[workgroup]; k_spin_measure_reduce adds those in k_reduce_fin's order.  No atomics.
// ctrl->stopped is not consulted: this is not a Krylov step.
template <class E>
__global__ __launch_bounds__(kBlock) void k_spin_momentum_expand(const SpinMomentumView* __restrict__ op, const SpinSectorView* __restrict__ dst_op,
                                                                 const uint32_t* __restrict__ reps, const uint32_t* __restrict__ bucket,
                                                                 const typename SpinElement<E>::Stored* __restrict__ x,
                                                                 typename SpinElement<E>::Stored* __restrict__ y, int64_t n, int64_t ntiles,
                                                                 double* __restrict__ partials) {
  __shared__ double lds4[4];
  __shared__ double tables[SpinMomentumLds::kSize];
  __shared__ uint32_t binom[kSectorMaxSites * (kSectorMaxSites + 1)];
  spin_stage_binomials(dst_op, binom);
  spin_stage_momentum_tables(op, tables);
  __syncthreads();
  const int n_sites = op->model.n_sites, n_up = op->n_up, cell = op->cell, n_trans = op->n_trans, h = op->h, steps = op->steps;
  const uint32_t compatible = op->compatible, fallback = op->first_rep;
  const SpinMomentumLookup lk{reps, bucket};
  const SpinMomentumLds tb{tables};
  double nrm = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r = tile * kBlock + threadIdx.x;
    if (r < n) {
      const uint32_t s = spin_unrank_row(SpinBinomials32{binom}, n_sites, n_up, (uint32_t)r).s;
      const E yr = spin_momentum_expand_row(s, n_sites, cell, n_trans, compatible, fallback, h, steps, lk, tb, typename SpinElement<E>::Vector{x}, E{});
      y[r] = spin_stored(yr);
      nrm = spin_norm_add(nrm, yr);
    }
  }
  nrm = block_sum(nrm, lds4);
  if (threadIdx.x == 0) partials[blockIdx.x] = nrm;
}

// ---------------------------------------------------------------------------
// A sum of site operators that carries a momentum, from one momentum sector into another (spin_momentum_site.hpp has the
// definition and SpinMomentumSiteTable; spin_rows.hpp the walk): one row of the DESTINATION sector per lane, 256-row tiles, the
// persistent grid.  The lane's state is the destination's representative dst_reps[r], one coalesced load; its period comes from
// one orbit walk.  Everything else is the SOURCE sector's: src_op (geometry, h, steps and the ratio and phase tables, staged in
// LDS: 9.5 KB / 19.9 KB), src_reps and src_bucket, which the flipped states are searched in.  The coefficient table is read by
// every lane at the same index (scalar loads).  The sites go kSpinBatch at a time: the orbits, the searches and the gathers of a
// batch are all issued before its first fma, with the operator kernel's fixed trip counts.  A lane without the term, or whose
// representative does not carry the source momentum, looks up the source's first row and ignores the value, as expand does, so
// that no load is branched around and every search stays inside the source list.  Z reads one element and writes the lane's
// own; where source and destination are one sector (p = 0) that element is the lane's own, so y may be x there -- x and y are
// not __restrict__ -- and for everything else the caller keeps them apart.  norm2 = sum |y_r|^2 leaves through block_sum into
// partials[workgroup]; k_spin_measure_reduce adds those in k_reduce_fin's order.  No atomics.  ctrl->stopped is not consulted:
// this is not a Krylov step.
// ---------------------------------------------------------------------------
template <class E, class Word>
__global__ __launch_bounds__(kBlock) void k_spin_momentum_site_apply(const SpinMomentumSiteTable* __restrict__ tb,
                                                                     const SpinMomentumViewOf<Word>* __restrict__ src_op,
                                                                     const Word* __restrict__ src_reps, const uint32_t* __restrict__ src_bucket,
                                                                     const Word* __restrict__ dst_reps, const typename SpinElement<E>::Stored* x,
                                                                     typename SpinElement<E>::Stored* y, int64_t n, int64_t ntiles,
                                                                     double* __restrict__ partials) {
  __shared__ double lds4[4];
  __shared__ double tables[SpinMomentumLdsOf<Word>::kSize];
  spin_stage_momentum_tables(src_op, tables);
  __syncthreads();
  const int kind = tb->kind, n_sites = src_op->model.n_sites;
  const int cell = src_op->cell, n_trans = src_op->n_trans, h = src_op->h, steps = src_op->steps;
  const Word site_mask = src_op->site_mask, compatible = (Word)tb->compatible, fallback = (Word)tb->first_rep;
  bool real_coef = true;  // read once, here: the branches on it are uniform; a real vector has no imaginary coefficients
  if constexpr (std::is_same<E, SpinZ>::value) real_coef = tb->real_coef != 0;
  const SpinMomentumLookupOf<Word> lk{src_reps, src_bucket};
  const SpinMomentumLdsOf<Word> tab{tables};
  const typename SpinElement<E>::Vector xs{x};
  double nrm = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r = tile * kBlock + threadIdx.x;
    if (r < n) {
      const Word s = dst_reps[r];
      const int period = spin_orbit(s, n_sites, cell, n_trans).period;
      E yr = E{};
      if (kind == kSpinSiteZ) {
        yr = spin_momentum_site_z_row(s, period, n_sites, compatible, fallback, h, steps, lk, SpinSiteCoefficients{tb->half, tb->half_im, real_coef}, xs,
                                      E{});
      } else {
        const Word has = kind == kSpinSitePlus ? s : Word(~s & site_mask);
        for (int i0 = 0; i0 < n_sites; i0 += kSpinBatch) {
          bool on[kSpinBatch];
          uint32_t column[kSpinBatch];
          int ri[kSpinBatch], li[kSpinBatch];
          E xv[kSpinBatch];
          spin_momentum_site_targets(i0, s, has, period, n_sites, cell, n_trans, compatible, fallback, h, steps, lk, on, column, ri, li);
          spin_momentum_gather(xs, column, xv);
          yr = spin_momentum_site_add(yr, SpinSiteCoefficients{tb->coef + i0, tb->coef_im + i0, real_coef}, tab, on, ri, li, xv);
        }
      }
      y[r] = spin_stored(yr);
      nrm = spin_norm_add(nrm, yr);
    }
  }
  nrm = block_sum(nrm, lds4);
  if (threadIdx.x == 0) partials[blockIdx.x] = nrm;
}

// ---------------------------------------------------------------------------
// The reduced density matrix of one vector (spin_rdm.hpp has the definition, the work table and the slicing rule;
// spin_rdm_rows.hpp the index arithmetic and the panel shape per element, SpinRdmGeometry): rho_A = M M^H with
// M[a, b] = x[rank(dep_A(a) | dep_B(b))] never stored.  One workgroup per work item (block k, tile pair (ti, tj <= ti), slice
// of the b range).  Per chunk of CHUNK b's the workgroup
//   1. forms the states dep_B(b) once (LDS binomials, spin_rdm_party_state with (nB, n_up - k)); the states dep_A(a) of its
//      TILE rows (and of the other tile's rows) were formed once per item;
//   2. gathers the TILE x CHUNK panel of x into LDS, one panel for a diagonal pair, two otherwise: LOADS loads per lane and
//      panel, all issued before the first is stored (spin_rdm_element: a padded lane loads row 0 and stores 0).  Panels are
//      b-major;
//   3. accumulates in registers by plain fp64 fma, a 4 x 4 register tile per lane: TILE = 64 is 16 x 16 lanes that each take every
//      b of the chunk; TILE = 16 is 4 x 4 lanes per group and kSpinRdmSmallGroups groups that take the chunk's b's round robin
//      (b = group, group + 16, ...) and whose tiles are added in ascending group order through LDS at the end.
// Each entry i >= j of the tile is written by one lane to this slice's partials; k_spin_rdm_reduce adds the slices.  No atomics:
// a result depends on the grid only through the number of slices.  ctrl->stopped is not consulted: this is not a Krylov step.
// The plan, the items, the slices, the party states, the padding rule and the order of the sums are the same for both elements;
// what differs is the arithmetic and the shape of the panels.
//   E = double (eigenex_spin_rdm): CHUNK = kSpinRdmBigChunk / kSpinRdmSmallChunk, 8 loads per lane and panel.  The pitch is
//     TILE + 2 doubles and a lane's four rows are 4 t .. 4 t + 3: two 16-byte LDS reads, and a gather whose b's run along the
//     lanes is a 4-way bank conflict on its stores, not a 64-way one.
//   E = SpinZ (eigenex_spin_rdm_z; spin_rdm_host_z is the definition): a panel element is one 16-byte load of x behind one walk
//     of the rank tables and one 16-byte LDS store; the chunk is kSpinRdmBigChunkZ / kSpinRdmSmallChunkZ b's (four gathers per
//     lane and panel), the pitch TILE + 1 pairs, and a lane's four rows are t, t + SIDE, t + 2 SIDE, t + 3 SIDE, each one
//     16-byte LDS read (spin_rdm.hpp has the LDS budgets and the bank argument).  Per pair of rows and per b four fmas in the
//     definition's order (spin_rdm_fma) into a 4 x 4 register tile of (re, im): 32 fp64 accumulators.  The 16 groups' tiles go
//     through red[] twice, the real parts, then the imaginary ones.  The imaginary part of a diagonal entry is not stored:
//     +0.0 is (spin_rdm_entry).
// ---------------------------------------------------------------------------
template <bool SECTOR, int TILE, class E>
__global__ __launch_bounds__(kBlock) void k_spin_rdm(const SpinRdmTable* __restrict__ tb, const SpinRdmItem* __restrict__ items,
                                                     const SpinSectorView* __restrict__ op, const uint32_t* __restrict__ lo_rank,
                                                     const uint32_t* __restrict__ hi_base,
                                                     const typename SpinElement<E>::Stored* __restrict__ x,
                                                     typename SpinElement<E>::Stored* __restrict__ partials) {
  using G = SpinRdmGeometry<E, TILE>;
  using Stored = typename SpinElement<E>::Stored;
  constexpr int CHUNK = G::CHUNK, PANEL = G::PANEL, SIDE = G::SIDE;
  constexpr int GROUPS = TILE == kSpinRdmBigTile ? 1 : kSpinRdmSmallGroups;
  constexpr int LOADS = TILE * CHUNK / kBlock;
  static_assert(SIDE * SIDE * GROUPS == kBlock && TILE * CHUNK % kBlock == 0 && CHUNK <= kBlock && CHUNK % GROUPS == 0, "tile shape");
  static_assert(GROUPS == 1 || TILE * TILE == kBlock, "the group sums are added by one lane per entry");
  __shared__ __attribute__((aligned(16))) Stored panel[(GROUPS == 1 ? 2 : 1) * PANEL];  // a 16-row block has one tile: no second panel
  __shared__ double red[GROUPS > 1 ? GROUPS * TILE * TILE : 1];
  __shared__ uint32_t sa_i[TILE], sa_j[TILE], sb[CHUNK];
  __shared__ uint32_t binom[SECTOR ? kSectorMaxSites * (kSectorMaxSites + 1) : 1];
  int h = 0;
  uint32_t lo_mask = 0;
  if constexpr (SECTOR) {
    spin_stage_binomials(op, binom);
    __syncthreads();
    h = op->h, lo_mask = op->lo_mask;
  }
  const SpinRdmItem it = items[blockIdx.x];
  const SpinRdmBlock* bk = tb->block + it.block;
  const int d = bk->d, k = bk->k, nA = tb->nA, nB = tb->nB, kb = tb->n_up - k;
  const uint32_t mask_a = tb->mask_a, mask_b = tb->mask_b, fallback = tb->fallback;
  const bool along_a = TILE == kSpinRdmBigTile && tb->along_a != 0, diagonal = it.ti == it.tj;
  const int i0 = it.ti * TILE, j0 = it.tj * TILE;
  const int tid = threadIdx.x;
  const SpinBinomials32 bin{binom};
  const SpinRankTables tab{lo_rank, hi_base};
  const typename SpinElement<E>::Vector xv{x};
  if (tid < TILE) {
    sa_i[tid] = spin_rdm_party_state<SECTOR>(bin, nA, k, mask_a, (uint32_t)(i0 + tid), i0 + tid < d);
    sa_j[tid] = spin_rdm_party_state<SECTOR>(bin, nA, k, mask_a, (uint32_t)(j0 + tid), j0 + tid < d);
  }
  const int group = tid / (SIDE * SIDE), tx = tid % SIDE, ty = tid % (SIDE * SIDE) / SIDE;
  const int other = diagonal || GROUPS > 1 ? 0 : PANEL;  // where the rows a_j of the pair lie: a diagonal pair has one panel
  double re[4][4], im[4][4];  // the accumulators part by part (spin_rdm_fma); a real vector leaves im alone
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) re[r][c] = 0.0, im[r][c] = 0.0;
  for (uint32_t b0 = it.b_begin; b0 < it.b_end; b0 += CHUNK) {
    __syncthreads();  // sa_i and sa_j are written; the last chunk's panels are read
    if (tid < CHUNK) sb[tid] = spin_rdm_party_state<SECTOR>(bin, nB, kb, mask_b, b0 + tid, tid < it.b_end - b0);
    __syncthreads();
    E va[LOADS], vb[LOADS];
#pragma unroll
    for (int q = 0; q < LOADS; ++q) {
      int row, bj;
      spin_rdm_panel_slot(along_a, TILE, CHUNK, q * kBlock + tid, &row, &bj);
      const bool live_b = (uint32_t)bj < it.b_end - b0;
      va[q] = spin_rdm_element<SECTOR>(tab, xv, h, lo_mask, sa_i[row], sb[bj], live_b && i0 + row < d, fallback);
      if (other != 0) vb[q] = spin_rdm_element<SECTOR>(tab, xv, h, lo_mask, sa_j[row], sb[bj], live_b && j0 + row < d, fallback);
    }
#pragma unroll
    for (int q = 0; q < LOADS; ++q) {
      int row, bj;
      spin_rdm_panel_slot(along_a, TILE, CHUNK, q * kBlock + tid, &row, &bj);
      panel[G::panel_column(bj) + row] = spin_stored(va[q]);
      if (other != 0) panel[other + G::panel_column(bj) + row] = spin_stored(vb[q]);
    }
    __syncthreads();
    for (int bj = group; bj < CHUNK; bj += GROUPS) {
      E a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        a[r] = spin_loaded(panel[G::panel_column(bj) + G::lane_row(tx, r)]);
        b[r] = spin_loaded(panel[other + G::panel_column(bj) + G::lane_row(ty, r)]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) spin_rdm_fma(a[r], b[c], re[r][c], im[r][c]);
    }
  }
  Stored* out = partials + bk->part_offset + (int64_t)it.slice * d * d;
  if constexpr (GROUPS == 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = i0 + G::lane_row(tx, r), j = j0 + G::lane_row(ty, c);
        if (i < d && j < d && i >= j) out[i + (int64_t)j * d] = spin_stored(spin_rdm_entry<E>(re[r][c], im[r][c], i == j));
      }
  } else {
    // The groups' tiles are added through red[], one double per entry and group; of a complex vector part by part, the real
    // parts, then the imaginary ones.  The one pass of a real vector is written out and does not go through group_sum: the
    // compiler pairs the stores of the two forms differently.
    double sr = 0.0, si = 0.0;
    if constexpr (std::is_same<E, SpinZ>::value) {
      const auto group_sum = [&](const double(&part)[4][4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) red[group * TILE * TILE + G::lane_row(ty, c) * TILE + G::lane_row(tx, r)] = part[r][c];
        __syncthreads();
        double sum = 0.0;
        for (int g = 0; g < GROUPS; ++g) sum += red[g * TILE * TILE + tid];
        return sum;
      };
      sr = group_sum(re);
      __syncthreads();  // the real parts are read
      si = group_sum(im);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) red[group * TILE * TILE + G::lane_row(ty, c) * TILE + G::lane_row(tx, r)] = re[r][c];
      __syncthreads();
      for (int g = 0; g < GROUPS; ++g) sr += red[g * TILE * TILE + tid];
    }
    const int i = i0 + tid % TILE, j = j0 + tid / TILE;
    if (i < d && j < d && i >= j) out[i + (int64_t)j * d] = spin_stored(spin_rdm_entry<E>(sr, si, i == j));
  }
}

// Second stage of k_spin_rdm, one lane per entry of the packed output: the lane of an entry i >= j adds the block's slices in
// ascending order with plain adds, part by part, and writes (i, j) and (j, i) from the same value: a real entry twice, a complex
// one with the imaginary part negated in (j, i), and on the diagonal once with the imaginary part +0.0.  The lane of an entry
// i < j writes nothing.
template <class E>
__global__ __launch_bounds__(kBlock) void k_spin_rdm_reduce(const SpinRdmTable* __restrict__ tb,
                                                            const typename SpinElement<E>::Stored* __restrict__ partials,
                                                            typename SpinElement<E>::Stored* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= tb->total) return;
  int n = 0;
  while (n + 1 < tb->n_blocks && e >= tb->block[n + 1].out_offset) ++n;
  const SpinRdmBlock* bk = tb->block + n;
  const int64_t d = bk->d, local = e - bk->out_offset;
  const int64_t i = local % d, j = local / d;
  if (i < j) return;
  const typename SpinElement<E>::Stored* p = partials + bk->part_offset + i + j * d;
  E sum = E{};
  for (int s = 0; s < bk->nslices; ++s) sum = spin_sum(sum, spin_loaded(p[(int64_t)s * d * d]));
  if constexpr (std::is_same<E, SpinZ>::value) {
    if (i == j) {
      out[bk->out_offset + i + j * d] = make_double2(sum.re, 0.0);
    } else {
      out[bk->out_offset + i + j * d] = make_double2(sum.re, sum.im);
      out[bk->out_offset + j + i * d] = make_double2(sum.re, -sum.im);
    }
  } else {
    out[bk->out_offset + i + j * d] = sum;
    out[bk->out_offset + j + i * d] = sum;
  }
}

// complex blocks: entries, input and sums are (re, im) pairs; products without contraction and added part by
// part, exactly like k_spmv_z
template <int NB, bool STAGED>
__device__ __forceinline__ double2 block_row_walk_z(const double2* __restrict__ v, int64_t nr, int width, const double2* xs,
                                                    const int32_t* __restrict__ cl, const double2* __restrict__ x_ext, double scale) {
  double2 sum = make_double2(0.0, 0.0);
  auto input = [&](int j) {
    if (STAGED) return xs[j];
    double2 x = x_ext[cl[j]];
    x.x *= scale, x.y *= scale;
    return x;
  };
  int j = 0;
  for (; j + NB <= width; j += NB) {
    double2 a[NB], xv[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) a[t] = v[(int64_t)(j + t) * nr];
#pragma unroll
    for (int t = 0; t < NB; ++t) xv[t] = input(j + t);
#pragma unroll
    for (int t = 0; t < NB; ++t) {
      const double2 p = cmul_nofma(a[t], xv[t]);
      sum.x = sum.x + p.x;
      sum.y = sum.y + p.y;
    }
  }
  for (; j < width; ++j) {
    const double2 p = cmul_nofma(v[(int64_t)j * nr], input(j));
    sum.x = sum.x + p.x;
    sum.y = sum.y + p.y;
  }
  return sum;
}

__global__ __launch_bounds__(kBlock) void k_block_spmv_z(BlockOperatorView op, const double2* __restrict__ x_ext,
                                                         const double* __restrict__ scale_ptr, double shift_re,
                                                         double shift_im, double2* __restrict__ y,
                                                         double2* __restrict__ u_out, int64_t n, int64_t ntiles,
                                                         double* __restrict__ partials, int pstride, int pass,
                                                         const Ctrl* __restrict__ ctrl) {
  __shared__ double lds4[4];
  __shared__ double2 xs[kBlockStage / 2];  // the tile's input elements, gathered once per (group, strip column) as in k_block_spmv
  if (ctrl->stopped) return;
  const double scale = scale_ptr ? *scale_ptr : 1.0;
  const bool has_shift = shift_re != 0.0 || shift_im != 0.0;
  const double2* bval = reinterpret_cast<const double2*>(op.bval);
  double dr = 0.0, di = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * kBlock, r = r0 + threadIdx.x;
    const int64_t rlast = (r0 + kBlock < n ? r0 + kBlock : n) - 1;
    const int64_t c_first = op.gcol[op.rowgrp[r0]], c_end = op.gcol[op.rowgrp[rlast] + 1];
    const bool staged = c_end - c_first <= kBlockStage / 2;
    if (staged) {
      for (int i = threadIdx.x; i < (int)(c_end - c_first); i += kBlock) {
        double2 x = x_ext[op.cols[c_first + i]];
        x.x *= scale, x.y *= scale;
        xs[i] = x;
      }
      __syncthreads();
    }
    if (r < n) {
      const int g = op.rowgrp[r];
      const int gr0 = op.grow0[g], nr = op.grow0[g + 1] - gr0;
      const int64_t ge = op.gent[g];
      const int width = (int)((op.gent[g + 1] - ge) / nr);
      const double2* v = bval + ge + (r - gr0);
      const int64_t gc = op.gcol[g];
      const double2 sum = staged ? block_row_walk_z<8, true>(v, nr, width, xs + (gc - c_first), nullptr, nullptr, scale)
                                 : block_row_walk_z<4, false>(v, nr, width, nullptr, op.cols + gc, x_ext, scale);
      double2 xr = x_ext[r];
      xr.x *= scale;
      xr.y *= scale;
      double2 yr = sum;
      if (has_shift) {
        const double2 t = cmul_nofma(make_double2(shift_re, shift_im), xr);
        yr.x = yr.x + t.x;
        yr.y = yr.y + t.y;
      }
      y[r] = yr;
      if (u_out) u_out[r] = xr;
      if (pass & kPassSelfNorm) {
        dr = fma(yr.x, yr.x, fma(yr.y, yr.y, dr));  // |y|^2
      } else {
        dr = fma(xr.x, yr.x, fma(xr.y, yr.y, dr));  // conj(u) * y
        di = fma(xr.x, yr.y, fma(-xr.y, yr.x, di));
      }
    }
    if (staged) __syncthreads();
  }
  if (partials) {
    dr = block_sum(dr, lds4);
    di = block_sum(di, lds4);
    if (threadIdx.x == 0) {
      partials[blockIdx.x] = dr;
      partials[pstride + blockIdx.x] = di;
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_scale(const double* __restrict__ x, const double* __restrict__ scale_dev,
                                                  double scale_host, double* __restrict__ out, int64_t n,
                                                  const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stopped) return;
  const double s = scale_dev ? *scale_dev : scale_host;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    out[i] = x[i] * s;
}

__global__ __launch_bounds__(kBlock) void k_shift_dot(double* __restrict__ y, const double* __restrict__ u,
                                                      double shift, int64_t n, double* __restrict__ partials,
                                                      const Ctrl* __restrict__ ctrl) {
  __shared__ double lds4[4];
  if (ctrl->stopped) return;
  double dot = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const double ui = u[i];
    double yi = y[i];
    if (shift != 0.0) {
      yi = add_product_nofma(yi, shift, ui);
      y[i] = yi;
    }
    dot = fma(ui, yi, dot);
  }
  dot = block_sum(dot, lds4);
  if (threadIdx.x == 0) partials[blockIdx.x] = dot;
}

// complex: y += shift*u, partials = (re, im) of conj(u).y
__global__ __launch_bounds__(kBlock) void k_shift_dot_z(double2* __restrict__ y, const double2* __restrict__ u,
                                                        double shift_re, double shift_im, int64_t n,
                                                        double* __restrict__ partials, int pstride,
                                                        const Ctrl* __restrict__ ctrl) {
  __shared__ double lds4[4];
  if (ctrl->stopped) return;
  const bool has_shift = shift_re != 0.0 || shift_im != 0.0;
  double dr = 0.0, di = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const double2 ui = u[i];
    double2 yi = y[i];
    if (has_shift) {
      const double2 t = cmul_nofma(make_double2(shift_re, shift_im), ui);
      yi.x = yi.x + t.x;
      yi.y = yi.y + t.y;
      y[i] = yi;
    }
    dr = fma(ui.x, yi.x, fma(ui.y, yi.y, dr));
    di = fma(ui.x, yi.y, fma(-ui.y, yi.x, di));
  }
  dr = block_sum(dr, lds4);
  di = block_sum(di, lds4);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = dr;
    partials[pstride + blockIdx.x] = di;
  }
}

// es = doubles per entry (1 real, 2 complex)
__global__ __launch_bounds__(kBlock) void k_pack(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                 int64_t count, int es, double* __restrict__ out,
                                                 const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stopped) return;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count * es; i += (int64_t)gridDim.x * kBlock)
    out[i] = x[(int64_t)idx[i / es] * es + (i % es)];
}

__global__ void k_sum_shards(PtrPack bufs, int nshards, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int k = 0; k < nshards; ++k) s += bufs.p[k][i];
  for (int k = 0; k < nshards; ++k) bufs.p[k][i] = s;
}

// ---- scalar finalisers -----------------------------------------------------
__device__ __forceinline__ void fin_norm_apply(Ctrl* ctrl, double nrm2, double threshold, int mode, double* beta) {
  const double nrm = sqrt(nrm2);
  if (mode == kFinInit) {
    if (nrm < threshold) {  // lanczos.hpp:316-318, arnoldi.hpp:262-264
      ctrl->stopped = 1;
    } else {
      ctrl->scale = 1.0 / nrm;
    }
  } else if (mode == kFinLanczos) {
    beta[ctrl->nbeta++] = nrm;  // lanczos.hpp:429 (kept on breakdown, :433-436)
    if (nrm <= threshold)
      ctrl->stopped = 1;
    else
      ctrl->scale = 1.0 / nrm;
  } else {
    ctrl->residue = nrm;  // arnoldi.hpp:348, :385
  }
}
__global__ void k_fin_norm(Ctrl* ctrl, const double* nrm2, double threshold, int mode, double* beta) {
  if (threadIdx.x != 0 || ctrl->stopped) return;
  fin_norm_apply(ctrl, *nrm2, threshold, mode, beta);
}

__device__ __forceinline__ void fin_alpha_apply(Ctrl* ctrl, double val, double* alpha, int first);

// Second-stage sum of ONE scalar (ncomp = 1) or a (re, im) pair and the step decision that follows it, in one
// launch: used when nothing has to be all-reduced in between (one shard, no communicator).  Same sums as k_reduce,
// same decisions as k_fin_norm / k_fin_alpha; two dependent tiny launches (~4-5 us each on the device) become one.
__global__ __launch_bounds__(kBlock) void k_reduce_fin(const double* __restrict__ partials, int pstride, int nblocks,
                                                       int ncomp, double* __restrict__ out, Ctrl* ctrl, int mode,
                                                       double* series, double threshold) {
  __shared__ double lds4[4];
  if (ctrl->stopped) return;
  double v[2] = {0.0, 0.0};
  for (int c = 0; c < ncomp; ++c) {
    const double* p = partials + (int64_t)c * pstride;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kBlock) s += p[b];
    v[c] = block_sum(s, lds4);
  }
  if (threadIdx.x != 0) return;
  for (int c = 0; c < ncomp; ++c) out[c] = v[c];
  if (mode == kFinishAlpha || mode == kFinishAlphaFirst)
    fin_alpha_apply(ctrl, v[0], series, mode == kFinishAlphaFirst);
  else
    fin_norm_apply(ctrl, v[0], threshold, mode, series);
}

__device__ __forceinline__ void fin_alpha_apply(Ctrl* ctrl, double val, double* alpha, int first) {
  alpha[ctrl->nalpha++] = val;  // lanczos.hpp:395, :448
  ctrl->nvec++;
  ctrl->calls_true++;
  if (!first) ctrl->iterations++;  // lanczos.hpp:450 (not on the first call, :378-398)
}
__global__ void k_fin_alpha(Ctrl* ctrl, const double* val, double* alpha, int first) {
  if (threadIdx.x != 0 || ctrl->stopped) return;
  fin_alpha_apply(ctrl, *val, alpha, first);
}

// Fused-alpha Lanczos step (library.hip: lanczos_call): fused = all-reduced [alpha_k (2 slots), g = V^H (v - beta u_{k-1})
// (ncoef doubles), G = V^H u_k (ncoef doubles)].  h = g - alpha_k G = V^H (v - alpha_k u_k - beta u_{k-1}) up to rounding
// (alpha, beta real: the same formula on every double, complex or not), and alpha_k joins the series exactly as
// k_fin_alpha would have done after the operator (lanczos.hpp:395, :448-450).
__global__ __launch_bounds__(kBlock) void k_form_h(Ctrl* ctrl, const double* __restrict__ fused, int ncoef, double* __restrict__ h,
                                                   double* alpha, int first) {
  if (ctrl->stopped) return;
  const double a = fused[0];
  const double* g = fused + 2;
  const double* G = g + ncoef;
  for (int i = threadIdx.x; i < ncoef; i += kBlock) h[i] = fma(-a, G[i], g[i]);
  if (threadIdx.x == 0) fin_alpha_apply(ctrl, a, alpha, first);
}

__global__ void k_arnoldi_begin(Ctrl* ctrl, double threshold, int64_t n_global, int cap, double* H, int ldh, int es) {
  if (threadIdx.x != 0 || ctrl->stopped) return;
  const int k = ctrl->nvec;
  // arnoldiStepIsUtmost  arnoldi.hpp:277-288
  if ((int64_t)k == n_global || ctrl->residue <= threshold || k >= cap) {
    ctrl->stopped = 1;
    return;
  }
  if (ctrl->keep_coupling)
    ctrl->keep_coupling = 0;  // first step after a Krylov-Schur restart (see arnoldi_begin_record)
  else
    H[((int64_t)(k - 1) * ldh + k) * es] = ctrl->residue;  // arnoldi.hpp:363 (imaginary part stays 0)
  ctrl->scale = 1.0 / ctrl->residue;                     // arnoldi.hpp:365
}

__global__ void k_arnoldi_end(Ctrl* ctrl, const double* h, double* H, int ldh, int es) {
  if (ctrl->stopped) return;
  const int k = ctrl->nvec;  // index of the vector just added
  for (int i = threadIdx.x; i < (k + 1) * es; i += blockDim.x) H[(int64_t)k * ldh * es + i] = h[i];  // arnoldi.hpp:380-383
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int e = 0; e < es; ++e) H[((int64_t)k * ldh + k + 1) * es + e] = 0.0;  // arnoldi.hpp:384
    ctrl->nvec = k + 1;
    ctrl->nalpha = k + 1;
    ctrl->iterations++;
    ctrl->calls_true++;
  }
}

// Adaptive second Gram-Schmidt pass (Daniel-Gragg-Kaufman-Stewart): the first pass has cancelled too much of the
// vector when ||w_after||^2 < eta^2 ||w_before||^2 (eta = 1/sqrt 2).  pass2 is a second control block whose
// `stopped` flag the second-pass kernels obey: they run only when the criterion asks for them.
__global__ void k_decide_second_pass(const Ctrl* ctrl, Ctrl* pass2, const double* nrm2_before, const double* nrm2_after, double eta2) {
  if (threadIdx.x != 0) return;
  const bool again = !ctrl->stopped && (*nrm2_after < eta2 * *nrm2_before);
  pass2->stopped = again ? 0 : 1;
}
// nrm2_final = the second pass's norm if it ran, else the first pass's
__global__ void k_select_norm(const Ctrl* pass2, const double* nrm2_first, const double* nrm2_second, double* nrm2_final) {
  if (threadIdx.x != 0) return;
  *nrm2_final = pass2->stopped ? *nrm2_first : *nrm2_second;
}

// One shard: the sum of the first pass's norm partials and the DGKS decision in one launch
__global__ __launch_bounds__(kBlock) void k_reduce_decide(const double* __restrict__ partials, int nblocks, double* nrm2_first,
                                                          const Ctrl* ctrl, Ctrl* pass2, double* nrm2_before, double eta2,
                                                          const double* __restrict__ before_partials, int before_nblocks) {
  __shared__ double lds4[4];
  double s = 0.0, sb = 0.0;
  if (!ctrl->stopped) {
    for (int b = threadIdx.x; b < nblocks; b += kBlock) s += partials[b];
    if (before_partials)  // ||v||^2 of the operator's output, left as partial sums by the operator kernel: k_reduce's sum, taken here
      for (int b = threadIdx.x; b < before_nblocks; b += kBlock) sb += before_partials[b];
  }
  s = block_sum(s, lds4);
  if (before_partials) sb = block_sum(sb, lds4);
  if (threadIdx.x != 0) return;
  if (ctrl->stopped) {
    pass2->stopped = 1;
    return;
  }
  if (before_partials) *nrm2_before = sb;
  *nrm2_first = s;
  pass2->stopped = (s < eta2 * *nrm2_before) ? 0 : 1;
}

// One shard: everything that follows the (conditional) second pass of an Arnoldi step in one launch -- the second
// norm's sum, h += h2, the choice of the norm, residue = sqrt(norm) (k_fin_norm, kFinArnoldi) and k_arnoldi_end.
__global__ __launch_bounds__(kBlock) void k_arnoldi_tail(const double* __restrict__ partials, int nblocks, Ctrl* ctrl,
                                                         const Ctrl* pass2, double* h, const double* h2, int ncoef,
                                                         const double* nrm2_first, double* nrm2_final, double* H, int ldh, int es) {
  __shared__ double lds4[4];
  if (ctrl->stopped) return;
  const bool second = pass2->stopped == 0;
  double s = 0.0;
  if (second)
    for (int b = threadIdx.x; b < nblocks; b += kBlock) s += partials[b];
  s = block_sum(s, lds4);
  if (second)
    for (int i = threadIdx.x; i < ncoef; i += kBlock) h[i] += h2[i];
  __syncthreads();
  const int k = ctrl->nvec;  // index of the vector just added
  for (int i = threadIdx.x; i < (k + 1) * es; i += kBlock) H[(int64_t)k * ldh * es + i] = h[i];  // arnoldi.hpp:380-383
  __syncthreads();
  if (threadIdx.x == 0) {
    const double nrm2 = second ? s : *nrm2_first;
    *nrm2_final = nrm2;
    ctrl->residue = sqrt(nrm2);  // arnoldi.hpp:348, :385
    for (int e = 0; e < es; ++e) H[((int64_t)k * ldh + k + 1) * es + e] = 0.0;  // arnoldi.hpp:384
    ctrl->nvec = k + 1;
    ctrl->nalpha = k + 1;
    ctrl->iterations++;
    ctrl->calls_true++;
  }
}

// dst[i] += src[i] (coefficients of a second Gram-Schmidt pass folded into the first)
__global__ void k_add_small(double* dst, const double* src, int n, const Ctrl* ctrl) {
  if (ctrl->stopped) return;
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] += src[i];
}

// thick restart: the kept Ritz vectors sit in columns 0..nkeep-1, the old residual vector u_m in column
// nkeep; T' = diag(theta) bordered by the couplings, so alpha[nkeep] = old alpha[m], beta[nkeep-1] = s_{nkeep-1}
__global__ void k_restart_fix(Ctrl* ctrl, double* alpha, double* beta, int m, int nkeep, double coupling_last) {
  if (threadIdx.x != 0) return;
  alpha[nkeep] = alpha[m];
  if (nkeep > 0) beta[nkeep - 1] = coupling_last;
  ctrl->stopped = 0;
  ctrl->nvec = nkeep + 1;
  ctrl->nalpha = nkeep + 1;
  ctrl->nbeta = nkeep;
}

// Krylov-Schur restart: the kept vectors V_m Q sit in columns 0..nkeep-1 and A (V_m Q) = (V_m Q) B_top + w b^T with
// b = residue * Q[m-1, :], so the projected matrix is B: full in rows 0..nkeep-1, the coupling row b in row nkeep, nothing below.
// The next step would store the residue at H[nkeep][nkeep-1] (k_arnoldi_begin); keep_coupling tells it to leave b's last entry.
// Everything of H outside B is zeroed: the steps that follow write the Hessenberg part of their columns only.
__global__ __launch_bounds__(kBlock) void k_arnoldi_restart_fix(Ctrl* ctrl, double* __restrict__ H, int ldh, int ncols, int es,
                                                                const double* __restrict__ B, int ldb, int nkeep) {
  const int rows = ldh * es, brows = (nkeep + 1) * es;
  for (int c = 0; c < ncols; ++c)
    for (int i = threadIdx.x; i < rows; i += kBlock) H[(int64_t)c * rows + i] = (c < nkeep && i < brows) ? B[(int64_t)c * ldb * es + i] : 0.0;
  if (threadIdx.x != 0) return;
  ctrl->stopped = 0;
  ctrl->nvec = nkeep;
  ctrl->nalpha = nkeep;
  ctrl->keep_coupling = 1;
}

__global__ void k_accept_vector(Ctrl* ctrl) {
  if (threadIdx.x != 0 || ctrl->stopped) return;
  ctrl->nvec++;
}

// ---- validation of a CSR handed over in device memory (eigenex_csr_upload_device) -----------------
// bad[0] += rows whose row pointers decrease or leave [0, nnz]; bad[1] += column indices outside [0, ncols)
__global__ __launch_bounds__(kBlock) void k_check_csr(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      int64_t n, int64_t nnz, int64_t ncols, unsigned int* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  unsigned int b0 = 0, b1 = 0;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
    const int64_t a = rowptr[r], e = rowptr[r + 1];
    if (a < 0 || e < a || e > nnz) ++b0;
  }
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < nnz; p += stride) {
    const int64_t c = col[p];
    if (c < 0 || c >= ncols) ++b1;
  }
  if (b0) atomicAdd(bad, b0);
  if (b1) atomicAdd(bad + 1, b1);
}

// ---- synthetic operator ------------------------------------------------------
// number of stored entries in rows [0, i) of the n^3 7-point Dirichlet Laplacian
__device__ __forceinline__ int64_t lap_prefix(int64_t i, int64_t n) {
  const int64_t n2 = n * n, n3 = n2 * n;
  const int64_t cx0 = (i + n - 1) / n;
  const int64_t cx1 = i / n;
  const int64_t m = i % n2;
  const int64_t cy0 = (i / n2) * n + (m < n ? m : n);
  const int64_t cy1 = (i / n2) * n + (m > n2 - n ? m - (n2 - n) : 0);
  const int64_t cz0 = i < n2 ? i : n2;
  const int64_t cz1 = i > n3 - n2 ? i - (n3 - n2) : 0;
  return 7 * i - (cx0 + cx1 + cy0 + cy1 + cz0 + cz1);
}

template <class OFF>
__global__ __launch_bounds__(kBlock) void k_laplacian3d(int64_t n, int64_t rb, int64_t re, int64_t lower_start,
                                                        int64_t n_lower, int64_t halo_base,
                                                        OFF* __restrict__ rowptr, int32_t* __restrict__ col,
                                                        double* __restrict__ val) {
  const int64_t nloc = re - rb;
  const int64_t n2 = n * n;
  const int64_t pb = lap_prefix(rb, n);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= nloc; i += (int64_t)gridDim.x * kBlock) {
    const int64_t r = rb + i;
    int64_t p = lap_prefix(r, n) - pb;
    rowptr[i] = (OFF)p;
    if (i == nloc) break;
    const int64_t x = r % n, yy = (r / n) % n, z = r / n2;
    auto emit = [&](int64_t c, double v) {
      int64_t lc;
      if (c >= rb && c < re)
        lc = c - rb;
      else if (c < rb)
        lc = halo_base + (c - lower_start);
      else
        lc = halo_base + n_lower + (c - re);
      col[p] = (int32_t)lc;
      val[p] = v;
      ++p;
    };
    if (z > 0) emit(r - n2, -1.0);
    if (yy > 0) emit(r - n, -1.0);
    if (x > 0) emit(r - 1, -1.0);
    emit(r, 6.0);
    if (x < n - 1) emit(r + 1, -1.0);
    if (yy < n - 1) emit(r + n, -1.0);
    if (z < n - 1) emit(r + n2, -1.0);
  }
}

// ---- Ritz vectors: X = V * S, up to 8 columns per pass over V ----------------
// NE output columns per pass over the basis, 4 rows (2 x double2) per thread and column, the m loop unrolled so
// that 8 independent 16-byte loads are in flight per lane.  St is the coefficient block of this pass, packed
// [nvec][NE] (zero-padded behind nev) so that the NE coefficients of one basis column are one scalar load burst.
// Rows behind n inside the padded column stride are zero in V and are written back as zeros.
template <int NE, bool NORM>
__global__ __launch_bounds__(kBlock) void k_ritz(const double* __restrict__ V, int64_t ldv, int nvec,
                                                 const double* __restrict__ St, int nev, double* __restrict__ X,
                                                 int64_t ldx, int64_t n, int64_t ntiles, double* __restrict__ partials,
                                                 int pstride) {
  __shared__ double lds4[4];
  constexpr int kRows = 4 * kBlock;  // rows per tile
  double nrm[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) nrm[e] = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * kRows + 2 * threadIdx.x, r1 = r0 + 2 * kBlock;
    const bool in0 = r0 < n, in1 = r1 < n;
    double2 a0[NE], a1[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) a0[e] = a1[e] = make_double2(0.0, 0.0);
    const double* vp = V;
#pragma unroll 4
    for (int m = 0; m < nvec; ++m, vp += ldv) {
      const double2 v0 = in0 ? nt_ld_d2(vp + r0) : make_double2(0.0, 0.0);
      const double2 v1 = in1 ? nt_ld_d2(vp + r1) : make_double2(0.0, 0.0);
      const double* sp = St + (int64_t)m * NE;
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        const double c = sp[e];
        a0[e].x = fma(c, v0.x, a0[e].x);  // lanczos.hpp:802-804 (m ascending)
        a0[e].y = fma(c, v0.y, a0[e].y);
        a1[e].x = fma(c, v1.x, a1[e].x);
        a1[e].y = fma(c, v1.y, a1[e].y);
      }
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      if (e < nev) {
        double* xp = X + (int64_t)e * ldx;
        if (in0) st2(xp + r0, a0[e]);
        if (in1) st2(xp + r1, a1[e]);
        if (NORM) nrm[e] = fma(a0[e].x, a0[e].x, fma(a0[e].y, a0[e].y, fma(a1[e].x, a1[e].x, fma(a1[e].y, a1[e].y, nrm[e]))));
      }
    }
  }
  if (NORM) {
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      if (e < nev) {
        const double t = block_sum(nrm[e], lds4);
        if (threadIdx.x == 0) partials[(int64_t)e * pstride + blockIdx.x] = t;
      }
    }
  }
}

// ---- compression of a complex basis with complex coefficients: X = V * C, up to 8 columns per pass ----
// The Krylov-Schur restart of a complex Arnoldi run (library.hip: eigenex_arnoldi_restart).  Same streaming shape as k_ritz: a
// persistent grid over tiles, one 16-byte non-temporal load = one complex entry per lane, two entries per thread and column,
// the m loop unrolled by 4 so that 8 independent loads are in flight per lane; the 8 complex coefficients of a basis column
// (Ct packed [nvec][NE], zero-padded behind nev) sit at a wave-uniform address: one scalar load burst.  Each output entry is
// summed in registers over m ascending, so nothing is shared between workgroups.  n counts complex entries; ldv, ldx doubles.
template <int NE>
__global__ __launch_bounds__(kBlock) void k_compress_z(const double* __restrict__ V, int64_t ldv, int nvec,
                                                       const double* __restrict__ Ct, int nev, double* __restrict__ X,
                                                       int64_t ldx, int64_t n, int64_t ntiles) {
  constexpr int kRows = 2 * kBlock;  // complex entries per tile
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * kRows + threadIdx.x, r1 = r0 + kBlock;
    const bool in0 = r0 < n, in1 = r1 < n;
    double2 a0[NE], a1[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) a0[e] = a1[e] = make_double2(0.0, 0.0);
    const double* vp = V;
#pragma unroll 4
    for (int m = 0; m < nvec; ++m, vp += ldv) {
      const double2 v0 = in0 ? nt_ld_d2(vp + 2 * r0) : make_double2(0.0, 0.0);
      const double2 v1 = in1 ? nt_ld_d2(vp + 2 * r1) : make_double2(0.0, 0.0);
      const double* cp = Ct + (int64_t)m * (2 * NE);
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        const double cr = cp[2 * e], ci = cp[2 * e + 1];
        a0[e].x = fma(-ci, v0.y, fma(cr, v0.x, a0[e].x));  // (cr + i ci)(vx + i vy), m ascending
        a0[e].y = fma(ci, v0.x, fma(cr, v0.y, a0[e].y));
        a1[e].x = fma(-ci, v1.y, fma(cr, v1.x, a1[e].x));
        a1[e].y = fma(ci, v1.x, fma(cr, v1.y, a1[e].y));
      }
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      if (e < nev) {
        double* xp = X + (int64_t)e * ldx;
        if (in0) st2(xp + 2 * r0, a0[e]);
        if (in1) st2(xp + 2 * r1, a1[e]);
      }
    }
  }
}

// first local entry with |z| > 0 per column: out[3e] = entry index (n if none), out[3e+1..3e+2] = (re, im).
// es = doubles per entry; ldx in doubles.
__global__ __launch_bounds__(kBlock) void k_first_nonzero(const double* __restrict__ X, int64_t ldx, int64_t n, int es,
                                                          double* __restrict__ out) {
  __shared__ long long best[kBlock];
  const double* x = X + (int64_t)blockIdx.x * ldx;
  long long found = n;
  // chunks of 256*16 entries in order; stop at the first chunk that has a hit
  for (int64_t c0 = 0; c0 < n && found == n; c0 += kBlock * 16) {
    long long mine = n;
    for (int j = 0; j < 16; ++j) {
      const int64_t i = c0 + j * kBlock + threadIdx.x;
      if (i < n && i < mine) {
        const bool nz = es == 1 ? fabs(x[i]) > 0.0 : (fabs(x[2 * i]) > 0.0 || fabs(x[2 * i + 1]) > 0.0);
        if (nz) mine = i;
      }
    }
    best[threadIdx.x] = mine;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
      if (threadIdx.x < s && best[threadIdx.x + s] < best[threadIdx.x]) best[threadIdx.x] = best[threadIdx.x + s];
      __syncthreads();
    }
    found = best[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[3 * blockIdx.x] = (double)found;
    out[3 * blockIdx.x + 1] = found < n ? x[found * es] : 0.0;
    out[3 * blockIdx.x + 2] = (found < n && es == 2) ? x[found * es + 1] : 0.0;
  }
}

// column e *= (factors[2e] + i factors[2e+1])  (real columns use the real part only)
__global__ __launch_bounds__(kBlock) void k_scale_columns(double* __restrict__ X, int64_t ldx, int64_t n, int es,
                                                          const double* __restrict__ factors) {
  double* x = X + (int64_t)blockIdx.y * ldx;
  const double fr = factors[2 * blockIdx.y], fi = factors[2 * blockIdx.y + 1];
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    if (es == 1) {
      x[i] *= fr;
    } else {
      const double a = x[2 * i], b = x[2 * i + 1];
      x[2 * i] = a * fr - b * fi;
      x[2 * i + 1] = a * fi + b * fr;
    }
  }
}

// Ritz vectors with complex coefficients: raw columns 2e (V*s_re) and 2e+1 (V*s_im) -> out column e
// (interleaved complex, ldo entries): x = Xa + i Xb.  Real basis: (Xa[i], Xb[i]); complex basis:
// (Xa.re - Xb.im, Xa.im + Xb.re).  partials[e*pstride + block] = partial ||x||^2.
__global__ __launch_bounds__(kBlock) void k_ritz_combine(const double* __restrict__ X, int64_t ldx, int nc, int64_t n,
                                                         int es, double* __restrict__ out, int64_t ldo,
                                                         double* __restrict__ partials, int pstride) {
  __shared__ double lds4[4];
  for (int e = 0; e < nc; ++e) {
    const double* xa = X + (int64_t)(2 * e) * ldx;
    const double* xb = xa + ldx;
    double2* o = reinterpret_cast<double2*>(out) + (int64_t)e * ldo;
    double nrm = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
      double2 z;
      if (es == 1)
        z = make_double2(xa[i], xb[i]);
      else
        z = make_double2(xa[2 * i] - xb[2 * i + 1], xa[2 * i + 1] + xb[2 * i]);
      o[i] = z;
      nrm = fma(z.x, z.x, fma(z.y, z.y, nrm));
    }
    nrm = block_sum(nrm, lds4);
    if (threadIdx.x == 0) partials[(int64_t)e * pstride + blockIdx.x] = nrm;
  }
}

int g_num_cu = 256;

}  // namespace

int grid_for_tiles(int64_t ntiles, int blocks_per_cu) {
  int64_t cap = (int64_t)g_num_cu * blocks_per_cu;
  int64_t g = ntiles < cap ? ntiles : cap;
  return g < 1 ? 1 : (int)g;
}

void set_num_cu(int n) { g_num_cu = n > 0 ? n : 256; }

void launch_dots(hipStream_t s, const double* src, ThreeTerm tt, ColumnSet cs, int64_t n, double* partials,
                 int pstride, int grid, const Ctrl* ctrl, bool cplx, const double* src2, double* partials2, const InlineFin* fin,
                 const InlineDecide* dec) {
  const int ncols = cs.count + cs.nq;
  if (ncols <= 0) return;
  const int64_t ntiles = (n + kTileRows - 1) / kTileRows;
  const size_t shmem = (size_t)(src2 ? 8 : 4) * ncols * (cplx ? 2 : 1) * sizeof(double);
  static const bool red4 = [] {
    const char* e = getenv("EIGENEX_DOTS_RED4");
    return e ? atoi(e) != 0 : true;
  }();
  const InlineFin nofin{nullptr, 0, 0, 0.0, nullptr, nullptr, nullptr};
  const InlineFin f = fin ? *fin : nofin;
  const InlineDecide nodec{nullptr, nullptr, 0, nullptr, 0, 0.0, nullptr, nullptr};
  const InlineDecide dd = dec ? *dec : nodec;
#define EIGENEX_LAUNCH_DOTS(C, R, D) \
  hipLaunchKernelGGL((k_dots<C, R, D>), dim3(grid), dim3(kBlock), shmem, s, src, tt, src2, cs, n, ntiles, partials, partials2, pstride, ctrl, f, dd)
  if (src2) {
    if (cplx)
      EIGENEX_LAUNCH_DOTS(true, true, true);
    else
      EIGENEX_LAUNCH_DOTS(false, true, true);
  } else if (cplx) {
    if (red4)
      EIGENEX_LAUNCH_DOTS(true, true, false);
    else
      EIGENEX_LAUNCH_DOTS(true, false, false);
  } else {
    if (red4)
      EIGENEX_LAUNCH_DOTS(false, true, false);
    else
      EIGENEX_LAUNCH_DOTS(false, false, false);
  }
#undef EIGENEX_LAUNCH_DOTS
}

void launch_update(hipStream_t s, const double* src, double* dst, ThreeTerm tt, ColumnSet cs, const double* h,
                   int64_t n, double* partials, int grid, const Ctrl* ctrl, bool cplx, const InlineReduce* red) {
  const int64_t ntiles = (n + kTileRows - 1) / kTileRows;
  const InlineReduce nored{nullptr, 0, 0, 0, nullptr};
  const InlineReduce r = red ? *red : nored;
  const size_t shmem = red ? sizeof(double) * (size_t)red->ncoef : 0;
  if (red && cplx)
    hipLaunchKernelGGL((k_update<true, true>), dim3(grid), dim3(kBlock), shmem, s, src, dst, tt, cs, h, n, ntiles, partials, ctrl, r);
  else if (red)
    hipLaunchKernelGGL((k_update<false, true>), dim3(grid), dim3(kBlock), shmem, s, src, dst, tt, cs, h, n, ntiles, partials, ctrl, r);
  else if (cplx)
    hipLaunchKernelGGL((k_update<true, false>), dim3(grid), dim3(kBlock), 0, s, src, dst, tt, cs, h, n, ntiles, partials, ctrl, r);
  else
    hipLaunchKernelGGL((k_update<false, false>), dim3(grid), dim3(kBlock), 0, s, src, dst, tt, cs, h, n, ntiles, partials, ctrl, r);
}

void launch_sweep(hipStream_t s, const SweepStep& st, const InlineFin* fin, int64_t n, double* dpartials, int pstride, double* npartials,
                  int grid, const Ctrl* ctrl) {
  const int64_t ntiles = (n + kTileRows - 1) / kTileRows;
  const size_t shmem = sizeof(double) * 6 * (size_t)(st.k + 1);
  const InlineFin nofin{nullptr, 0, 0, 0.0, nullptr, nullptr, nullptr};
  const InlineFin f = fin ? *fin : nofin;
  // EIGENEX_SWEEP_DIRECT_STORES=1: the full sweep stores at each tile's end, as the closing pass does.  EIGENEX_SWEEP_PARK_TILES=1|2
  // caps the depth of the parking.  EIGENEX_SWEEP_SLOT_SHIFT=s: slots of 2^s ticks instead of the depth's measured default
  // (measurements; tests: with a large s no boundary ever passes).  All read once per process.
  static const bool direct = getenv("EIGENEX_SWEEP_DIRECT_STORES") != nullptr;
  static const int max_depth = [] {
    const char* e = getenv("EIGENEX_SWEEP_PARK_TILES");
    return e ? std::min(2, std::max(1, atoi(e))) : 2;
  }();
  static const struct Shifts {
    int of_depth[3];
    Shifts() {
      int dev = 0, khz = 0;  // the chip-wide clock's rate
      if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
      const char* e = getenv("EIGENEX_SWEEP_SLOT_SHIFT");
      const double us[3] = {0.0, kSweepSlotMicroseconds, kSweepSlotMicroseconds2};
      of_depth[0] = 0;
      for (int d = 1; d <= 2; ++d) {
        int sh = 0;
        while (sh < 40 && 1.5 * (double)((uint64_t)1 << sh) < us[d] * 1e-3 * khz) ++sh;  // the nearest power of two
        of_depth[d] = e ? std::min(62, std::max(0, atoi(e))) : sh;
      }
    }
  } shifts;
  // the deepest parking that fits beside the sums within the budget, so that two workgroups per CU still fit
  int depth = direct ? 0 : max_depth;
  while (depth > 0 && (size_t)depth * kSweepParkBytes + shmem + kSweepStaticLds > (size_t)kSweepLdsBudget) --depth;
  auto big_lds = [](const void* fn) {  // more than 64 KB of dynamic LDS has to be asked for once per instantiation
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kSweepLdsBudget - kSweepStaticLds) == hipSuccess;
  };
  if (st.correct_only) {
    hipLaunchKernelGGL((k_sweep<true, 0>), dim3(grid), dim3(kBlock), shmem, s, st, f, n, ntiles, dpartials, pstride, npartials, ctrl, 0);
  } else if (depth == 0) {
    hipLaunchKernelGGL((k_sweep<false, 0>), dim3(grid), dim3(kBlock), shmem, s, st, f, n, ntiles, dpartials, pstride, npartials, ctrl, 0);
  } else if (depth == 1) {
    static const bool asked = big_lds(reinterpret_cast<const void*>(&k_sweep<false, 1>));
    (void)asked;  // a launch the runtime refuses shows in the caller's launch check
    hipLaunchKernelGGL((k_sweep<false, 1>), dim3(grid), dim3(kBlock), kSweepParkBytes + shmem, s, st, f, n, ntiles, dpartials, pstride, npartials,
                       ctrl, shifts.of_depth[1]);
  } else {
    static const bool asked = big_lds(reinterpret_cast<const void*>(&k_sweep<false, 2>));
    (void)asked;
    hipLaunchKernelGGL((k_sweep<false, 2>), dim3(grid), dim3(kBlock), 2 * kSweepParkBytes + shmem, s, st, f, n, ntiles, dpartials, pstride,
                       npartials, ctrl, shifts.of_depth[2]);
  }
}

void launch_lag_terms(hipStream_t s, int k, const double* dpartials, int pstride, int nblocks, const double* npartials, double* lag,
                      int f_off, double threshold, Ctrl* ctrl, Ctrl* repair) {
  const int waves = std::min(kLagWaves, std::max(kBlock / 64, k + 1));
  hipLaunchKernelGGL(k_lag_terms, dim3(1), dim3(64 * waves), 0, s, k, dpartials, pstride, nblocks, npartials, lag, f_off, threshold, ctrl, repair);
}

void launch_close_scalars(hipStream_t s, int k, const double* a_raw, double* alpha, const double* beta, double* lag, const Ctrl* ctrl) {
  hipLaunchKernelGGL(k_close_scalars, dim3(1), dim3(1), 0, s, k, a_raw, alpha, beta, lag, ctrl);
}

void launch_spmv_z(hipStream_t s, const int32_t* rowptr, const int32_t* col, const double* val, const double* x_ext,
                   const double* scale, double shift_re, double shift_im, double* y, double* u_out, int64_t n,
                   double* partials, int pstride, int grid, const Ctrl* ctrl, int spmv_flags, int pass) {
  const int64_t ntiles = (n + kSpmvRows - 1) / kSpmvRows;
  if (spmv_flags & kSpmvLongRows)
    hipLaunchKernelGGL(k_spmv_z<true>, dim3(grid), dim3(kBlock), 0, s, rowptr, col, reinterpret_cast<const double2*>(val),
                       reinterpret_cast<const double2*>(x_ext), scale, shift_re, shift_im, reinterpret_cast<double2*>(y),
                       reinterpret_cast<double2*>(u_out), n, ntiles, partials, pstride, spmv_flags, pass, ctrl);
  else
    hipLaunchKernelGGL(k_spmv_z<false>, dim3(grid), dim3(kBlock), 0, s, rowptr, col, reinterpret_cast<const double2*>(val),
                       reinterpret_cast<const double2*>(x_ext), scale, shift_re, shift_im, reinterpret_cast<double2*>(y),
                       reinterpret_cast<double2*>(u_out), n, ntiles, partials, pstride, spmv_flags, pass, ctrl);
}

void launch_shift_dot_z(hipStream_t s, double* y, const double* u, double shift_re, double shift_im, int64_t n,
                        double* partials, int pstride, int grid, const Ctrl* ctrl) {
  hipLaunchKernelGGL(k_shift_dot_z, dim3(grid), dim3(kBlock), 0, s, reinterpret_cast<double2*>(y),
                     reinterpret_cast<const double2*>(u), shift_re, shift_im, n, partials, pstride, ctrl);
}

void launch_reduce(hipStream_t s, const double* partials, int pstride, int nblocks, int ncols, double* out,
                   const Ctrl* ctrl) {
  if (ncols <= 0) return;
  hipLaunchKernelGGL(k_reduce, dim3(ncols), dim3(kBlock), 0, s, partials, pstride, nblocks, out, ctrl);
}

template <class OFF>
static void launch_spmv_t(hipStream_t s, const OFF* rowptr, const int32_t* col, const double* val, const double* x_ext,
                          const double* scale, double shift, double* y, double* u_out, int64_t n, double* partials, int grid,
                          const Ctrl* ctrl, int spmv_flags, int pass, const InlineFin* fin, const InlineArnoldiBegin* begin,
                          const int32_t* tile_list, int64_t list_len, const ChebStep* cheb, const MomentStep* mom) {
  const int64_t ntiles = tile_list ? list_len : (n + kSpmvRows - 1) / kSpmvRows;
  if (ntiles <= 0) return;
  const InlineFin nofin{nullptr, 0, 0, 0.0, nullptr, nullptr, nullptr};
  const InlineArnoldiBegin nobegin{nullptr, 0.0, 0, 0, nullptr, 0, 0, -1, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr};
  const bool nt = (spmv_flags & 2) != 0;
  if (mom) {  // the moments epilogue: no hooks, two partial dots
#define EIGENEX_LAUNCH_SPMV_MOM(LONG, NTV)                                                                                                     \
  hipLaunchKernelGGL((k_spmv_moments<LONG, OFF, NTV>), dim3(grid), dim3(kBlock), 0, s, rowptr, col, val, x_ext, scale, shift, partials, n, ntiles, \
                     spmv_flags, ctrl, tile_list, *mom)
    if (spmv_flags & kSpmvLongRows) {
      if (nt) EIGENEX_LAUNCH_SPMV_MOM(true, true);
      else EIGENEX_LAUNCH_SPMV_MOM(true, false);
    } else {
      if (nt) EIGENEX_LAUNCH_SPMV_MOM(false, true);
      else EIGENEX_LAUNCH_SPMV_MOM(false, false);
    }
#undef EIGENEX_LAUNCH_SPMV_MOM
    return;
  }
  if (cheb) {  // the Chebyshev epilogue: no hooks, no partial dots
#define EIGENEX_LAUNCH_SPMV_CHEB(LONG, NTV)                                                                                                \
  hipLaunchKernelGGL((k_spmv_cheb<LONG, OFF, NTV>), dim3(grid), dim3(kBlock), 0, s, rowptr, col, val, x_ext, scale, shift, u_out, n, ntiles, \
                     spmv_flags, ctrl, tile_list, *cheb)
    if (spmv_flags & kSpmvLongRows) {
      if (nt) EIGENEX_LAUNCH_SPMV_CHEB(true, true);
      else EIGENEX_LAUNCH_SPMV_CHEB(true, false);
    } else {
      if (nt) EIGENEX_LAUNCH_SPMV_CHEB(false, true);
      else EIGENEX_LAUNCH_SPMV_CHEB(false, false);
    }
#undef EIGENEX_LAUNCH_SPMV_CHEB
    return;
  }
#define EIGENEX_LAUNCH_SPMV(LONG, NTV)                                                                                              \
  hipLaunchKernelGGL((k_spmv<LONG, OFF, NTV>), dim3(grid), dim3(kBlock), 0, s, rowptr, col, val, x_ext, scale, shift, y, u_out, n, \
                     ntiles, partials, spmv_flags, pass, ctrl, fin ? *fin : nofin, begin ? *begin : nobegin, tile_list)
  if (spmv_flags & kSpmvLongRows) {
    if (nt) EIGENEX_LAUNCH_SPMV(true, true);
    else EIGENEX_LAUNCH_SPMV(true, false);
  } else {
    if (nt) EIGENEX_LAUNCH_SPMV(false, true);
    else EIGENEX_LAUNCH_SPMV(false, false);
  }
#undef EIGENEX_LAUNCH_SPMV
}
void launch_spmv(hipStream_t s, const int32_t* rowptr, const int32_t* col, const double* val, const double* x_ext,
                 const double* scale, double shift, double* y, double* u_out, int64_t n, double* partials, int grid,
                 const Ctrl* ctrl, int spmv_flags, int pass, const InlineFin* fin, const InlineArnoldiBegin* begin,
                 const int32_t* tile_list, int64_t list_len, const ChebStep* cheb, const MomentStep* mom) {
  launch_spmv_t(s, rowptr, col, val, x_ext, scale, shift, y, u_out, n, partials, grid, ctrl, spmv_flags, pass, fin, begin, tile_list, list_len, cheb, mom);
}
void launch_spmv64(hipStream_t s, const int64_t* rowptr, const int32_t* col, const double* val, const double* x_ext,
                   const double* scale, double shift, double* y, double* u_out, int64_t n, double* partials, int grid,
                   const Ctrl* ctrl, int spmv_flags, int pass, const InlineFin* fin, const InlineArnoldiBegin* begin,
                   const int32_t* tile_list, int64_t list_len, const ChebStep* cheb, const MomentStep* mom) {
  launch_spmv_t(s, rowptr, col, val, x_ext, scale, shift, y, u_out, n, partials, grid, ctrl, spmv_flags, pass, fin, begin, tile_list, list_len, cheb, mom);
}
void launch_spmv_rows(hipStream_t s, const RowCodeView& op, const double* x_ext, const double* scale, double shift, double* y,
                      double* u_out, int64_t n, double* partials, int grid, const Ctrl* ctrl, int spmv_flags, int pass,
                      const InlineFin* fin, const InlineArnoldiBegin* begin, const int32_t* tile_list, int64_t list_len,
                      const ChebStep* cheb, const MomentStep* mom) {
  const int64_t ntiles = tile_list ? list_len : (n + kSpmvRows - 1) / kSpmvRows;
  if (ntiles <= 0) return;
  const InlineFin nofin{nullptr, 0, 0, 0.0, nullptr, nullptr, nullptr};
  const InlineArnoldiBegin nobegin{nullptr, 0.0, 0, 0, nullptr, 0, 0, -1, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr};
  if (mom && op.rec_bytes == 8)
    hipLaunchKernelGGL(k_spmv_rows_moments<8>, dim3(grid), dim3(kBlock), 0, s, op, x_ext, scale, shift, partials, n, ntiles, spmv_flags, ctrl, tile_list, *mom);
  else if (mom)
    hipLaunchKernelGGL(k_spmv_rows_moments<16>, dim3(grid), dim3(kBlock), 0, s, op, x_ext, scale, shift, partials, n, ntiles, spmv_flags, ctrl, tile_list, *mom);
  else if (cheb && op.rec_bytes == 8)
    hipLaunchKernelGGL(k_spmv_rows_cheb<8>, dim3(grid), dim3(kBlock), 0, s, op, x_ext, scale, shift, u_out, n, ntiles, spmv_flags, ctrl, tile_list, *cheb);
  else if (cheb)
    hipLaunchKernelGGL(k_spmv_rows_cheb<16>, dim3(grid), dim3(kBlock), 0, s, op, x_ext, scale, shift, u_out, n, ntiles, spmv_flags, ctrl, tile_list, *cheb);
  else if (op.rec_bytes == 8)
    hipLaunchKernelGGL(k_spmv_rows<8>, dim3(grid), dim3(kBlock), 0, s, op, x_ext, scale, shift, y, u_out, n, ntiles, partials,
                       spmv_flags, pass, ctrl, fin ? *fin : nofin, begin ? *begin : nobegin, tile_list);
  else
    hipLaunchKernelGGL(k_spmv_rows<16>, dim3(grid), dim3(kBlock), 0, s, op, x_ext, scale, shift, y, u_out, n, ntiles, partials,
                       spmv_flags, pass, ctrl, fin ? *fin : nofin, begin ? *begin : nobegin, tile_list);
}

// Device encoder of a generated CSR shard (row_code_encode, the host's function): records for rows [0, nrec_rows), rows >= n all
// absent; a row that does not fit the tables sets *bad
template <class OFF>
__global__ __launch_bounds__(kBlock) void k_encode_rows(const OFF* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const double* __restrict__ val, int64_t n, int64_t nrec_rows, RowCodeSlots slots,
                                                        int nslots, RowCodePalette pal, int rec_bytes, uint8_t* __restrict__ rec,
                                                        unsigned int* bad) {
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < nrec_rows; r += (int64_t)gridDim.x * kBlock) {
    uint8_t b[kRowCodeMaxSlots];
    bool ok = true;
    if (r < n) {
      const OFF p = rowptr[r];
      ok = row_code_encode(r, col + p, val + p, (int64_t)(rowptr[r + 1] - p), slots.off, nslots, pal.bits, pal.n, b, rec_bytes);
    } else {
      for (int i = 0; i < rec_bytes; ++i) b[i] = (uint8_t)kRowCodeAbsent;
    }
    if (!ok) atomicAdd(bad, 1u);
    for (int i = 0; i < rec_bytes; ++i) rec[r * rec_bytes + i] = b[i];
  }
}
void launch_encode_rows(hipStream_t s, const int32_t* rowptr, const int64_t* rowptr64, const int32_t* col, const double* val, int64_t n,
                        int64_t nrec_rows, const RowCodeSlots& slots, int nslots, const RowCodePalette& pal, int rec_bytes, uint8_t* rec,
                        unsigned int* bad) {
  const int grid = (int)std::min<int64_t>((nrec_rows + kBlock - 1) / kBlock, 65536);
  if (grid <= 0) return;
  if (rowptr64)
    hipLaunchKernelGGL(k_encode_rows<int64_t>, dim3(grid), dim3(kBlock), 0, s, rowptr64, col, val, n, nrec_rows, slots, nslots, pal,
                       rec_bytes, rec, bad);
  else
    hipLaunchKernelGGL(k_encode_rows<int32_t>, dim3(grid), dim3(kBlock), 0, s, rowptr, col, val, n, nrec_rows, slots, nslots, pal,
                       rec_bytes, rec, bad);
}

void launch_spmv_sorted(hipStream_t s, const SortedOperatorView& op, const double* x_ext, const double* scale, double shift, double* y,
                        double* u_out, int64_t n, double* partials, const Ctrl* ctrl, int pass) {
  const size_t shmem = sizeof(double) * 2 * kSortBufDoubles;
  static const bool attr_set = [shmem] {
    bool ok = true;
    ok &= hipFuncSetAttribute(reinterpret_cast<const void*>(k_spmv_sorted<4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem) == hipSuccess;
    ok &= hipFuncSetAttribute(reinterpret_cast<const void*>(k_spmv_sorted<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem) == hipSuccess;
    ok &= hipFuncSetAttribute(reinterpret_cast<const void*>(k_spmv_sorted<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem) == hipSuccess;
    return ok;
  }();
  (void)attr_set;
  const int64_t ntiles = (n + op.tile_rows - 1) / op.tile_rows;
  const dim3 grid(sorted_grid(n, op.tile_rows)), block(kSortBlock);
  if (op.tile_rows == 4 * kSortBlock)
    hipLaunchKernelGGL(k_spmv_sorted<4>, grid, block, shmem, s, op, x_ext, scale, shift, y, u_out, n, ntiles, partials, pass, ctrl);
  else if (op.tile_rows == 2 * kSortBlock)
    hipLaunchKernelGGL(k_spmv_sorted<2>, grid, block, shmem, s, op, x_ext, scale, shift, y, u_out, n, ntiles, partials, pass, ctrl);
  else
    hipLaunchKernelGGL(k_spmv_sorted<1>, grid, block, shmem, s, op, x_ext, scale, shift, y, u_out, n, ntiles, partials, pass, ctrl);
}

int split_combine_grid(int64_t n) { return grid_for_tiles((n + 2 * kBlock - 1) / (2 * kBlock), 8); }

// gathers one chunk ahead, LDS atomics (ds_add_f64, nothing returned): measured 121 us on BASELINE config 3 against 125 / 123 us
// two / three chunks ahead and 126-130 us with read-add-write (scripts/microbench/split_tiles.hip)
static const auto k_spmv_split_used = k_spmv_split<1>;
bool prepare_spmv_split() {  // the kernel needs up to 128 KB of dynamic LDS: allowed once, at upload (not inside a stream capture)
  static const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(k_spmv_split_used), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(sizeof(double) * kSplitMaxTileRows)) == hipSuccess &&
                         hipFuncSetAttribute(reinterpret_cast<const void*>(k_spmv_split_z), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(sizeof(double) * kSplitMaxTileRows)) == hipSuccess;
  return ok;
}

void launch_spmv_split(hipStream_t s, const SplitOperatorView& op, const double* x_ext, const double* scale, double shift, double* y,
                       double* u_out, int64_t n, double* partials, const Ctrl* ctrl, int pass, const InlineArnoldiBegin* begin) {
  const auto kernel = k_spmv_split_used;
  (void)prepare_spmv_split();
  const InlineArnoldiBegin nobegin{nullptr, 0.0, 0, 0, nullptr, 0, 0, -1, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr};
  const int64_t ntiles = (n + op.tile_rows - 1) / op.tile_rows;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(ntiles * op.groups)), dim3(kSplitBlock), sizeof(double) * op.tile_rows, s, op, x_ext,
                     scale, ctrl, begin ? *begin : nobegin);
  hipLaunchKernelGGL(k_split_combine, dim3(split_combine_grid(n)), dim3(kBlock), 0, s, op.part, op.part_stride, op.groups, x_ext, scale,
                     shift, y, u_out, n, partials, pass, ctrl);
}

void launch_spmv_split_z(hipStream_t s, const SplitOperatorView& op, const double* x_ext, const double* scale, double shift_re,
                         double shift_im, double* y, double* u_out, int64_t n, double* partials, int pstride, const Ctrl* ctrl, int pass) {
  (void)prepare_spmv_split();
  const int64_t ntiles = (n + op.tile_rows - 1) / op.tile_rows;
  hipLaunchKernelGGL(k_spmv_split_z, dim3((unsigned)(ntiles * op.groups)), dim3(kSplitBlock), sizeof(double) * 2 * op.tile_rows, s, op,
                     reinterpret_cast<const double2*>(x_ext), scale, ctrl);
  hipLaunchKernelGGL(k_split_combine_z, dim3(split_combine_grid(n)), dim3(kBlock), 0, s, reinterpret_cast<const double2*>(op.part),
                     op.part_stride, op.groups, reinterpret_cast<const double2*>(x_ext), scale, shift_re, shift_im,
                     reinterpret_cast<double2*>(y), reinterpret_cast<double2*>(u_out), n, partials, pstride, pass, ctrl);
}

int sorted_grid(int64_t n, int tile_rows) { return grid_for_tiles((n + tile_rows - 1) / tile_rows, 1); }

void launch_block_spmv(hipStream_t s, const BlockOperatorView& op, const double* x_ext, const double* scale, double shift,
                       double* y, double* u_out, int64_t n, double* partials, int grid, const Ctrl* ctrl, int pass) {
  hipLaunchKernelGGL(k_block_spmv, dim3(grid), dim3(kBlock), 0, s, op, x_ext, scale, shift, y, u_out, n,
                     (n + kBlock - 1) / kBlock, partials, pass, ctrl);
}

void launch_block_spmv_z(hipStream_t s, const BlockOperatorView& op, const double* x_ext, const double* scale, double shift_re,
                         double shift_im, double* y, double* u_out, int64_t n, double* partials, int pstride, int grid,
                         const Ctrl* ctrl, int pass) {
  hipLaunchKernelGGL(k_block_spmv_z, dim3(grid), dim3(kBlock), 0, s, op, reinterpret_cast<const double2*>(x_ext), scale, shift_re,
                     shift_im, reinterpret_cast<double2*>(y), reinterpret_cast<double2*>(u_out), n, (n + kBlock - 1) / kBlock, partials,
                     pstride, pass, ctrl);
}

void launch_spin_spmv(hipStream_t s, const SpinSectorView* op, const uint32_t* lo_rank, const uint32_t* hi_base, const double* x_ext,
                      const double* scale, double shift, double* y, double* u_out, int64_t n, double* partials, int grid, const Ctrl* ctrl,
                      int pass) {
  const auto kernel = lo_rank ? k_spin_spmv<true, double> : k_spin_spmv<false, double>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, s, op, lo_rank, hi_base, x_ext, scale, shift, y, u_out, n, (n + kBlock - 1) / kBlock,
                     partials, pass, ctrl);
}

void launch_spin_spmv_z(hipStream_t s, const SpinSectorView* op, const uint32_t* lo_rank, const uint32_t* hi_base, const double* x_ext,
                        const double* scale, double shift_re, double shift_im, double* y, double* u_out, int64_t n, double* partials,
                        int pstride, int grid, const Ctrl* ctrl, int pass) {
  const auto kernel = lo_rank ? k_spin_spmv<true, SpinZ, int> : k_spin_spmv<false, SpinZ, int>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, s, op, lo_rank, hi_base, reinterpret_cast<const double2*>(x_ext), scale, shift_re,
                     shift_im, reinterpret_cast<double2*>(y), reinterpret_cast<double2*>(u_out), n, (n + kBlock - 1) / kBlock,
                     partials, pstride, pass, ctrl);
}

// The launchers below take es, the doubles per element of the vector (1: real, 2: interleaved complex), and the vector, the
// partials and the result as pointers to double whatever the element.
template <class E>
static const typename SpinElement<E>::Stored* spin_elements(const double* p) {
  return reinterpret_cast<const typename SpinElement<E>::Stored*>(p);
}
template <class E>
static typename SpinElement<E>::Stored* spin_elements(double* p) {
  return reinterpret_cast<typename SpinElement<E>::Stored*>(p);
}

template <class E>
static void spin_measure_launch(hipStream_t s, const SpinMeasureChunk* chunk, const SpinSectorView* op, const uint32_t* lo_rank,
                                const uint32_t* hi_base, const double* x, int64_t n, double* partials, int pstride, int grid) {
  const auto kernel = lo_rank ? k_spin_measure<true, E> : k_spin_measure<false, E>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, s, chunk, op, lo_rank, hi_base, spin_elements<E>(x), n, (n + kBlock - 1) / kBlock,
                     partials, pstride);
}
void launch_spin_measure(hipStream_t s, int es, const SpinMeasureChunk* chunk, const SpinSectorView* op, const uint32_t* lo_rank,
                         const uint32_t* hi_base, const double* x, int64_t n, double* partials, int pstride, int grid) {
  (es == 2 ? spin_measure_launch<SpinZ> : spin_measure_launch<double>)(s, chunk, op, lo_rank, hi_base, x, n, partials, pstride, grid);
}

void launch_spin_measure_reduce(hipStream_t s, const double* partials, int pstride, int nblocks, int ndiag, int nflip, double* diag_out,
                                double* flip_out, double* norm_out) {
  hipLaunchKernelGGL(k_spin_measure_reduce, dim3(2 * kSpinMeasureChunk + 1), dim3(kBlock), 0, s, partials, pstride, nblocks, ndiag, nflip,
                     diag_out, flip_out, norm_out);
}

void launch_spin_measure_columns(hipStream_t s, const SpinMeasureChunk* chunk, const SpinSectorView* op, const uint32_t* lo_rank,
                                 const uint32_t* hi_base, const double* x, const double* V, int64_t ldv, int ncols, int64_t n, double* partials,
                                 int pstride, int grid) {
  const auto kernel = lo_rank ? k_spin_measure_columns<true> : k_spin_measure_columns<false>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, s, chunk, op, lo_rank, hi_base, x, V, ldv, ncols, n, (n + kBlock - 1) / kBlock, partials,
                     pstride);
}

void launch_spin_measure_columns_reduce(hipStream_t s, const double* partials, int pstride, int nblocks, int ndiag, int nflip, int ncols, int ldo,
                                        double* diag_out, double* flip_out) {
  hipLaunchKernelGGL(k_spin_measure_columns_reduce, dim3(2 * kSpinMeasureChunk * kSpinMeasureColumns), dim3(kBlock), 0, s, partials, pstride,
                     nblocks, ndiag, nflip, ncols, ldo, diag_out, flip_out);
}

template <class E>
static void spin_site_apply_launch(hipStream_t s, const SpinSiteTable* table, const SpinSectorView* dst_op, const uint32_t* src_lo,
                                   const uint32_t* src_hi, const double* x, double* y, int64_t n, double* partials, int grid) {
  const auto kernel = src_lo ? k_spin_site_apply<true, E> : k_spin_site_apply<false, E>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, s, table, dst_op, src_lo, src_hi, spin_elements<E>(x), spin_elements<E>(y), n,
                     (n + kBlock - 1) / kBlock, partials);
}
void launch_spin_site_apply(hipStream_t s, int es, const SpinSiteTable* table, const SpinSectorView* dst_op, const uint32_t* src_lo,
                            const uint32_t* src_hi, const double* x, double* y, int64_t n, double* partials, int grid) {
  (es == 2 ? spin_site_apply_launch<SpinZ> : spin_site_apply_launch<double>)(s, table, dst_op, src_lo, src_hi, x, y, n, partials, grid);
}

template <class Word>
static void spin_momentum_spmv_launch(hipStream_t s, int es, const SpinMomentumViewOf<Word>* op, const Word* reps, const uint32_t* bucket,
                                      const double* x_ext, const double* scale, double shift_re, double shift_im, double* y, double* u_out,
                                      int64_t n, double* partials, int pstride, int grid, const Ctrl* ctrl, int pass) {
  const int64_t ntiles = (n + kBlock - 1) / kBlock;
  if (es == 2)
    hipLaunchKernelGGL((k_spin_momentum_spmv<SpinZ, Word, int>), dim3(grid), dim3(kBlock), 0, s, op, reps, bucket, spin_elements<SpinZ>(x_ext),
                       scale, shift_re, shift_im, spin_elements<SpinZ>(y), spin_elements<SpinZ>(u_out), n, ntiles, partials, pstride, pass, ctrl);
  else
    hipLaunchKernelGGL((k_spin_momentum_spmv<double, Word>), dim3(grid), dim3(kBlock), 0, s, op, reps, bucket, x_ext, scale, shift_re, y, u_out, n,
                       ntiles, partials, pass, ctrl);
}
void launch_spin_momentum_spmv(hipStream_t s, int es, const SpinMomentumView* op, const uint32_t* reps, const uint32_t* bucket,
                               const double* x_ext, const double* scale, double shift_re, double shift_im, double* y, double* u_out, int64_t n,
                               double* partials, int pstride, int grid, const Ctrl* ctrl, int pass) {
  spin_momentum_spmv_launch<uint32_t>(s, es, op, reps, bucket, x_ext, scale, shift_re, shift_im, y, u_out, n, partials, pstride, grid, ctrl, pass);
}
void launch_spin_momentum_spmv(hipStream_t s, int es, const SpinMomentum64View* op, const uint64_t* reps, const uint32_t* bucket,
                               const double* x_ext, const double* scale, double shift_re, double shift_im, double* y, double* u_out, int64_t n,
                               double* partials, int pstride, int grid, const Ctrl* ctrl, int pass) {
  spin_momentum_spmv_launch<uint64_t>(s, es, op, reps, bucket, x_ext, scale, shift_re, shift_im, y, u_out, n, partials, pstride, grid, ctrl, pass);
}

template <class E, class Word>
static void spin_momentum_measure_launch(hipStream_t s, const SpinMomentumMeasureChunk* chunk, const Word* reps, const double* x, int n_sites,
                                         int cell, int n_trans, int64_t n, double* partials, int pstride, int grid) {
  hipLaunchKernelGGL((k_spin_momentum_measure<E, Word>), dim3(grid), dim3(kBlock), 0, s, chunk, reps, spin_elements<E>(x), n_sites, cell, n_trans, n,
                     (n + kBlock - 1) / kBlock, partials, pstride);
}
void launch_spin_momentum_measure(hipStream_t s, int es, const SpinMomentumMeasureChunk* chunk, const uint32_t* reps, const double* x, int n_sites,
                                  int cell, int n_trans, int64_t n, double* partials, int pstride, int grid) {
  (es == 2 ? spin_momentum_measure_launch<SpinZ, uint32_t> : spin_momentum_measure_launch<double, uint32_t>)(s, chunk, reps, x, n_sites, cell, n_trans,
                                                                                                          n, partials, pstride, grid);
}
void launch_spin_momentum_measure(hipStream_t s, int es, const SpinMomentumMeasureChunk* chunk, const uint64_t* reps, const double* x, int n_sites,
                                  int cell, int n_trans, int64_t n, double* partials, int pstride, int grid) {
  (es == 2 ? spin_momentum_measure_launch<SpinZ, uint64_t> : spin_momentum_measure_launch<double, uint64_t>)(s, chunk, reps, x, n_sites, cell, n_trans,
                                                                                                          n, partials, pstride, grid);
}

template <class E>
static void spin_momentum_expand_launch(hipStream_t s, const SpinMomentumView* op, const SpinSectorView* dst_op, const uint32_t* reps,
                                        const uint32_t* bucket, const double* x, double* y, int64_t n, double* partials, int grid) {
  hipLaunchKernelGGL(k_spin_momentum_expand<E>, dim3(grid), dim3(kBlock), 0, s, op, dst_op, reps, bucket, spin_elements<E>(x), spin_elements<E>(y),
                     n, (n + kBlock - 1) / kBlock, partials);
}
void launch_spin_momentum_expand(hipStream_t s, int es, const SpinMomentumView* op, const SpinSectorView* dst_op, const uint32_t* reps,
                                 const uint32_t* bucket, const double* x, double* y, int64_t n, double* partials, int grid) {
  (es == 2 ? spin_momentum_expand_launch<SpinZ> : spin_momentum_expand_launch<double>)(s, op, dst_op, reps, bucket, x, y, n, partials, grid);
}

template <class Word>
static void spin_momentum_site_apply_launch(hipStream_t s, int es, const SpinMomentumSiteTable* table, const SpinMomentumViewOf<Word>* src_op,
                                            const Word* src_reps, const uint32_t* src_bucket, const Word* dst_reps, const double* x, double* y,
                                            int64_t n, double* partials, int grid) {
  const int64_t ntiles = (n + kBlock - 1) / kBlock;
  if (es == 2)
    hipLaunchKernelGGL((k_spin_momentum_site_apply<SpinZ, Word>), dim3(grid), dim3(kBlock), 0, s, table, src_op, src_reps, src_bucket, dst_reps,
                       spin_elements<SpinZ>(x), spin_elements<SpinZ>(y), n, ntiles, partials);
  else
    hipLaunchKernelGGL((k_spin_momentum_site_apply<double, Word>), dim3(grid), dim3(kBlock), 0, s, table, src_op, src_reps, src_bucket, dst_reps, x,
                       y, n, ntiles, partials);
}
void launch_spin_momentum_site_apply(hipStream_t s, int es, const SpinMomentumSiteTable* table, const SpinMomentumView* src_op,
                                     const uint32_t* src_reps, const uint32_t* src_bucket, const uint32_t* dst_reps, const double* x, double* y,
                                     int64_t n, double* partials, int grid) {
  spin_momentum_site_apply_launch<uint32_t>(s, es, table, src_op, src_reps, src_bucket, dst_reps, x, y, n, partials, grid);
}
void launch_spin_momentum_site_apply(hipStream_t s, int es, const SpinMomentumSiteTable* table, const SpinMomentum64View* src_op,
                                     const uint64_t* src_reps, const uint32_t* src_bucket, const uint64_t* dst_reps, const double* x, double* y,
                                     int64_t n, double* partials, int grid) {
  spin_momentum_site_apply_launch<uint64_t>(s, es, table, src_op, src_reps, src_bucket, dst_reps, x, y, n, partials, grid);
}

template <class E>
static void spin_rdm_launch(hipStream_t s, bool big, const SpinRdmTable* table, const SpinRdmItem* items, int n_items,
                            const SpinSectorView* op, const uint32_t* lo_rank, const uint32_t* hi_base, const double* x, double* partials) {
  const auto kernel = big ? (lo_rank ? k_spin_rdm<true, kSpinRdmBigTile, E> : k_spin_rdm<false, kSpinRdmBigTile, E>)
                          : (lo_rank ? k_spin_rdm<true, kSpinRdmSmallTile, E> : k_spin_rdm<false, kSpinRdmSmallTile, E>);
  hipLaunchKernelGGL(kernel, dim3(n_items), dim3(kBlock), 0, s, table, items, op, lo_rank, hi_base, spin_elements<E>(x),
                     spin_elements<E>(partials));
}
void launch_spin_rdm(hipStream_t s, int es, bool big, const SpinRdmTable* table, const SpinRdmItem* items, int n_items,
                     const SpinSectorView* op, const uint32_t* lo_rank, const uint32_t* hi_base, const double* x, double* partials) {
  if (n_items <= 0) return;
  (es == 2 ? spin_rdm_launch<SpinZ> : spin_rdm_launch<double>)(s, big, table, items, n_items, op, lo_rank, hi_base, x, partials);
}

template <class E>
static void spin_rdm_reduce_launch(hipStream_t s, const SpinRdmTable* table, int64_t total, const double* partials, double* out) {
  hipLaunchKernelGGL(k_spin_rdm_reduce<E>, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, table,
                     spin_elements<E>(partials), spin_elements<E>(out));
}
void launch_spin_rdm_reduce(hipStream_t s, int es, const SpinRdmTable* table, int64_t total, const double* partials, double* out) {
  (es == 2 ? spin_rdm_reduce_launch<SpinZ> : spin_rdm_reduce_launch<double>)(s, table, total, partials, out);
}

void launch_scale(hipStream_t s, const double* x, const double* scale_dev, double scale_host, double* out, int64_t n,
                  const Ctrl* ctrl) {
  const int grid = grid_for_tiles((n + kBlock - 1) / kBlock, 8);
  hipLaunchKernelGGL(k_scale, dim3(grid), dim3(kBlock), 0, s, x, scale_dev, scale_host, out, n, ctrl);
}

void launch_shift_dot(hipStream_t s, double* y, const double* u, double shift, int64_t n, double* partials, int grid,
                      const Ctrl* ctrl) {
  hipLaunchKernelGGL(k_shift_dot, dim3(grid), dim3(kBlock), 0, s, y, u, shift, n, partials, ctrl);
}

void launch_cheb_combine(hipStream_t s, const double* y, const ChebStep& step, int64_t n, int grid, const Ctrl* ctrl) {
  const int64_t ntiles = (n + kTileRows - 1) / kTileRows;
  hipLaunchKernelGGL(k_cheb_combine, dim3(grid), dim3(kBlock), 0, s, y, step, n, ntiles, ctrl);
}

void launch_cheb_moments(hipStream_t s, const double* y, const MomentStep& step, int64_t n, double* partials, int grid, const Ctrl* ctrl) {
  const int64_t ntiles = (n + kTileRows - 1) / kTileRows;
  hipLaunchKernelGGL(k_cheb_moments, dim3(grid), dim3(kBlock), 0, s, y, step, n, ntiles, partials, ctrl);
}

void launch_random_signs(hipStream_t s, double* out, int64_t n, int64_t row0, int es, uint64_t seed, uint64_t stream) {
  if (n <= 0) return;
  const int grid = grid_for_tiles((n + kBlock - 1) / kBlock, 8);
  hipLaunchKernelGGL(k_random_signs, dim3(grid), dim3(kBlock), 0, s, out, n, row0, es, seed, stream);
}

void launch_pack(hipStream_t s, const double* x, const int32_t* idx, int64_t count, int es, double* out,
                 const Ctrl* ctrl) {
  if (count <= 0) return;
  const int grid = grid_for_tiles((count * es + kBlock - 1) / kBlock, 8);
  hipLaunchKernelGGL(k_pack, dim3(grid), dim3(kBlock), 0, s, x, idx, count, es, out, ctrl);
}

void launch_sum_shards(hipStream_t s, const PtrPack& bufs, int nshards, int n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_sum_shards, dim3((n + 63) / 64), dim3(64), 0, s, bufs, nshards, n);
}

void launch_reduce_fin(hipStream_t s, const double* partials, int pstride, int nblocks, int ncomp, double* out, Ctrl* ctrl,
                       int mode, double* series, double threshold) {
  hipLaunchKernelGGL(k_reduce_fin, dim3(1), dim3(kBlock), 0, s, partials, pstride, nblocks, ncomp, out, ctrl, mode, series, threshold);
}

void launch_fin_norm(hipStream_t s, Ctrl* ctrl, const double* nrm2, double threshold, int mode, double* beta) {
  hipLaunchKernelGGL(k_fin_norm, dim3(1), dim3(64), 0, s, ctrl, nrm2, threshold, mode, beta);
}

void launch_fin_alpha(hipStream_t s, Ctrl* ctrl, const double* val, double* alpha, int first, int /*cap*/) {
  hipLaunchKernelGGL(k_fin_alpha, dim3(1), dim3(64), 0, s, ctrl, val, alpha, first);
}

void launch_form_h(hipStream_t s, Ctrl* ctrl, const double* fused, int ncoef, double* h, double* alpha, int first) {
  hipLaunchKernelGGL(k_form_h, dim3(1), dim3(kBlock), 0, s, ctrl, fused, ncoef, h, alpha, first);
}

void launch_arnoldi_begin(hipStream_t s, Ctrl* ctrl, double threshold, int64_t n_global, int cap, double* H,
                          int ldh, int es) {
  hipLaunchKernelGGL(k_arnoldi_begin, dim3(1), dim3(64), 0, s, ctrl, threshold, n_global, cap, H, ldh, es);
}

void launch_arnoldi_end(hipStream_t s, Ctrl* ctrl, const double* h, double* H, int ldh, int es) {
  hipLaunchKernelGGL(k_arnoldi_end, dim3(1), dim3(kBlock), 0, s, ctrl, h, H, ldh, es);
}

void launch_decide_second_pass(hipStream_t s, const Ctrl* ctrl, Ctrl* pass2, const double* nrm2_before, const double* nrm2_after, double eta2) {
  hipLaunchKernelGGL(k_decide_second_pass, dim3(1), dim3(64), 0, s, ctrl, pass2, nrm2_before, nrm2_after, eta2);
}
void launch_select_norm(hipStream_t s, const Ctrl* pass2, const double* nrm2_first, const double* nrm2_second, double* nrm2_final) {
  hipLaunchKernelGGL(k_select_norm, dim3(1), dim3(64), 0, s, pass2, nrm2_first, nrm2_second, nrm2_final);
}

void launch_reduce_decide(hipStream_t s, const double* partials, int nblocks, double* nrm2_first, const Ctrl* ctrl, Ctrl* pass2,
                          double* nrm2_before, double eta2, const double* before_partials, int before_nblocks) {
  hipLaunchKernelGGL(k_reduce_decide, dim3(1), dim3(kBlock), 0, s, partials, nblocks, nrm2_first, ctrl, pass2, nrm2_before, eta2,
                     before_partials, before_nblocks);
}
void launch_arnoldi_tail(hipStream_t s, const double* partials, int nblocks, Ctrl* ctrl, const Ctrl* pass2, double* h, const double* h2,
                         int ncoef, const double* nrm2_first, double* nrm2_final, double* H, int ldh, int es) {
  hipLaunchKernelGGL(k_arnoldi_tail, dim3(1), dim3(kBlock), 0, s, partials, nblocks, ctrl, pass2, h, h2, ncoef, nrm2_first, nrm2_final, H,
                     ldh, es);
}

void launch_add_small(hipStream_t s, double* dst, const double* src, int n, const Ctrl* ctrl) {
  if (n > 0) hipLaunchKernelGGL(k_add_small, dim3(1), dim3(kBlock), 0, s, dst, src, n, ctrl);
}

void launch_restart_fix(hipStream_t s, Ctrl* ctrl, double* alpha, double* beta, int m, int nkeep, double coupling_last) {
  hipLaunchKernelGGL(k_restart_fix, dim3(1), dim3(64), 0, s, ctrl, alpha, beta, m, nkeep, coupling_last);
}

void launch_arnoldi_restart_fix(hipStream_t s, Ctrl* ctrl, double* H, int ldh, int ncols, int es, const double* B_dev, int ldb, int nkeep) {
  hipLaunchKernelGGL(k_arnoldi_restart_fix, dim3(1), dim3(kBlock), 0, s, ctrl, H, ldh, ncols, es, B_dev, ldb, nkeep);
}

void launch_accept_vector(hipStream_t s, Ctrl* ctrl) {
  hipLaunchKernelGGL(k_accept_vector, dim3(1), dim3(64), 0, s, ctrl);
}

void launch_laplacian3d(hipStream_t s, int64_t n, int64_t rb, int64_t re, int64_t lower_start, int64_t n_lower,
                        int64_t halo_base, int32_t* rowptr, int64_t* rowptr64, int32_t* col, double* val) {
  const int64_t work = re - rb + 1;
  const int grid = grid_for_tiles((work + kBlock - 1) / kBlock, 8);
  if (rowptr64)
    hipLaunchKernelGGL(k_laplacian3d<int64_t>, dim3(grid), dim3(kBlock), 0, s, n, rb, re, lower_start, n_lower, halo_base, rowptr64, col, val);
  else
    hipLaunchKernelGGL(k_laplacian3d<int32_t>, dim3(grid), dim3(kBlock), 0, s, n, rb, re, lower_start, n_lower, halo_base, rowptr, col, val);
}

void launch_ritz(hipStream_t s, const double* V, int64_t ldv, int nvec, const double* St_dev, int ne_pack, int nev,
                 double* X, int64_t ldx, int64_t n, double* partials, int pstride, int grid) {
  const int64_t ntiles = (n + 4 * kBlock - 1) / (4 * kBlock);
  if (ne_pack == 16)
    hipLaunchKernelGGL((k_ritz<16, false>), dim3(grid), dim3(kBlock), 0, s, V, ldv, nvec, St_dev, nev, X, ldx, n, ntiles, partials, pstride);
  else
    hipLaunchKernelGGL((k_ritz<8, true>), dim3(grid), dim3(kBlock), 0, s, V, ldv, nvec, St_dev, nev, X, ldx, n, ntiles, partials, pstride);
}

void launch_compress_z(hipStream_t s, const double* V, int64_t ldv, int nvec, const double* Ct_dev, int nev, double* X, int64_t ldx,
                       int64_t n, int grid) {
  const int64_t ntiles = (n + 2 * kBlock - 1) / (2 * kBlock);
  hipLaunchKernelGGL((k_compress_z<8>), dim3(grid), dim3(kBlock), 0, s, V, ldv, nvec, Ct_dev, nev, X, ldx, n, ntiles);
}

void launch_check_csr(hipStream_t s, const int32_t* rowptr, const int32_t* col, int64_t n, int64_t nnz, int64_t ncols, unsigned int* bad) {
  const int grid = grid_for_tiles((std::max<int64_t>(n, nnz) + kBlock - 1) / kBlock, 8);
  hipLaunchKernelGGL(k_check_csr, dim3(grid), dim3(kBlock), 0, s, rowptr, col, n, nnz, ncols, bad);
}

void launch_first_nonzero(hipStream_t s, const double* X, int64_t ldx, int ncol, int64_t n, int es, double* out) {
  hipLaunchKernelGGL(k_first_nonzero, dim3(ncol), dim3(kBlock), 0, s, X, ldx, n, es, out);
}

void launch_scale_columns(hipStream_t s, double* X, int64_t ldx, int ncol, int64_t n, int es, const double* factors_dev) {
  const int gx = grid_for_tiles((n + kBlock - 1) / kBlock, 4);
  hipLaunchKernelGGL(k_scale_columns, dim3(gx, ncol), dim3(kBlock), 0, s, X, ldx, n, es, factors_dev);
}

void launch_ritz_combine(hipStream_t s, const double* X, int64_t ldx, int nc, int64_t n, int es, double* out,
                         int64_t ldo, double* partials, int pstride, int grid) {
  hipLaunchKernelGGL(k_ritz_combine, dim3(grid), dim3(kBlock), 0, s, X, ldx, nc, n, es, out, ldo, partials, pstride);
}

}  // namespace eigenex
