// Kernel launch interface of the gfx950 Krylov step library (internal).
// Everything here is stream-ordered and never synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lag_terms.hpp"
#include "row_codes.hpp"
#include "spin_measure.hpp"
#include "spin_rdm.hpp"
#include "spin_model.hpp"
#include "spin_momentum.hpp"
#include "spin_momentum_site.hpp"
#include "spin_rows.hpp"
#include "spin_sector.hpp"
#include "spin_site.hpp"
#include "split_layout.hpp"
#include "spmv_index.hpp"

namespace eigenex {

// Device-resident control block of one Krylov state (replicated on every shard:
// all shards see identical all-reduced scalars, so they take identical decisions).
struct Ctrl {
  int stopped;     // a step returned false on the device; later kernels are no-ops
  int nvec;        // lanczosvectors_.size() / arnoldivectors_.size()
  int nalpha;      // alpha_.size() / h_.size()
  int nbeta;       // beta_.size()
  int iterations;  // iterations_
  int calls_true;  // calls that returned true
  int keep_coupling;  // set by a Krylov-Schur restart (k_arnoldi_restart_fix): the next Arnoldi begin leaves H[k][k-1] as the
                      // restart wrote it instead of storing the residue there, and clears the flag.  0 everywhere else.
  int repairs;     // one-sweep Lanczos steps whose pending vector the guard sent through the two-sweep pass (sticky until the state is cleared)
  double scale;    // 1/beta_k or 1/residue_: factor applied to the operator input
  double residue;  // Arnoldi residue_
};

// kBlock (256 threads = 4 wave64), kSpmvRows, kSpmvChunk: spmv_index.hpp (shared with the host replay of k_spmv)
constexpr int kRowsPerThread = 8;    // vector kernels: 4 x double2 per thread per column
constexpr int kTileRows = kBlock * kRowsPerThread;  // 2048 rows per tile

struct ColumnSet {     // which vectors a dots/update pass runs over, in reference order
  const double* V;     // basis slab, column c at V + c*ldv
  int64_t ldv;
  int first, stride, count;   // basis columns first, first+stride, ... (count of them)
  const double* Q;     // orthogonalizingVectors_ slab
  int64_t ldq;
  int nq;
};

struct ThreeTerm {     // w0 = src - a*u_k - b*u_{k-1}   (lanczos.hpp:403-408); disabled if uk == nullptr
  const double* uk;
  const double* ukm1;  // nullptr for k == 0
  const double* a;     // device scalars
  const double* b;
};

// A step decision that a CONSUMER kernel takes itself from the producer's per-workgroup partial sums (one shard, no
// communicator, nothing to all-reduce in between): every workgroup repeats the second-stage sum in the fixed order of
// k_reduce_fin and arrives at the same number, workgroup 0 records it (series, counters, control block).  Saves the
// dependent one-block launch between producer and consumer: 6 -> 4 launches per Lanczos step.  partials == nullptr: off.
struct InlineFin {
  const double* partials;
  int nblocks;
  int mode;          // a FinNormMode (consumer = operator kernel) or a FinAlphaMode (consumer = dots kernel)
  double threshold;
  double* series;    // beta resp. alpha
  Ctrl* ctrl;        // the state's control block, writable
  double* out;       // where k_reduce_fin would have left the sum (hbuf slot)
};

// The start of an Arnoldi step (k_arnoldi_begin: arnoldiStepIsUtmost arnoldi.hpp:277-288, h_{k,k-1} = residue :363, the
// scale 1/residue :365) taken by the operator kernel itself, like InlineFin: every workgroup derives the same decision and
// the same scale from the control block, workgroup 0 records them.  One launch less per Arnoldi step on one shard.
// ctrl == nullptr: off.
struct InlineArnoldiBegin {
  Ctrl* ctrl;
  double threshold;
  int64_t n_global;
  int cap;
  double* H;
  int ldh, es;
  // r3: the END of the previous step (k_arnoldi_tail: the second pass's norm, h += h2, the choice of the norm, residue,
  // column k of H, the counters) taken here too, in front of the begin: tail_k >= 0 is the index of the vector the previous
  // step added (known to the host), so that no workgroup needs a counter that workgroup 0 is changing.  -1: off.
  int tail_k;
  const double* tail_partials;  // ||w||^2 partial sums of the second pass's update kernel
  int tail_nblocks;
  const Ctrl* pass2;            // stopped == 0: the second pass ran
  double* h;
  const double* h2;
  int ncoef;
  const double* nrm2_first;
  double* nrm2_final;
};

// The decision "second Gram-Schmidt pass or not" (k_reduce_decide) taken by the FIRST kernel of that pass itself: every
// workgroup of k_dots adds the first pass's norm partials (and the operator's ||v||^2 partials) in k_reduce's order and
// arrives at the same verdict; workgroup 0 records it (pass2->stopped, the two norms) for the kernels that follow.
// pass2 == nullptr: off.
struct InlineDecide {
  Ctrl* pass2;
  const double* after_partials;
  int after_n;
  const double* before_partials;  // nullptr: *nrm2_before already holds ||v||^2
  int before_n;
  double eta2;
  double* nrm2_first;
  double* nrm2_before;
};

// The second-stage sums of a dots pass (k_reduce: h_c = sum_b partials[c*pstride + b]) taken by the update kernel that
// consumes them: every workgroup forms all ncoef sums in k_reduce's order into LDS (workgroup 0 also leaves them in `out`).
// Only for the conditional second pass, which normally does not run: there it saves a launch per step, and when it does run
// the repeated sums (ncoef x nblocks loads per workgroup) are small beside the pass over the basis.  partials == nullptr: off.
struct InlineReduce {
  const double* partials;
  int pstride, nblocks, ncoef;
  double* out;
};

// One degree of a Chebyshev filter  p(A) x = sum_k mu[k] T_k((A - center)/halfwidth) x  for the rows of a launch.  With
// a = (A t_k - center t_k)[row], the operator kernels' row sum and shift epilogue (shift = -center):
//   first:  t_1 = c*a (c = 1/halfwidth),                 acc = mu0*t_0 + mu*t_1      (mu = mu[1]; t_prev = t_0 = x)
//   later:  t_{k+1} = c*a - t_{k-1} (c = 2/halfwidth),   acc = acc + mu*t_{k+1}      (mu = mu[k+1])
// every product rounded before it is added (no FMA), so that the operator kernels that take the step in their epilogue and
// k_cheb_combine behind any other operator kernel give the same bits.  t_next may be t_prev (each row is read before it is
// written, by one thread); neither may be the operator input, which is gathered from meanwhile.
struct ChebStep {
  const double* t_prev;  // the fused operator kernels take t_0 from their own input instead (first step)
  double* t_next;
  double* acc;
  double c, mu0, mu;
  int first;
};

// One degree of a Chebyshev moments run (kernel polynomial method): the recurrence of ChebStep without the accumulator,
//   first:  t_1 = c*a (c = 1/halfwidth);   later:  t_{k+1} = c*a - t_{k-1} (c = 2/halfwidth),
// products rounded before they are added, and per workgroup the partial sums of <t_{k+1}, t_{k+1}> (partials[block]) and
// <t_{k+1}, t_k> (partials[pstride + block]); t_k is the operator input.  t_next may be t_prev, neither may be the operator input.
struct MomentStep {
  const double* t_prev;  // unused in the first step
  double* t_next;
  const double* t_cur;   // t_k for k_cheb_moments; the fused operator kernels take it from their own input
  double c;
  int first;
  int pstride;
};

// Random signs: entry `row` (GLOBAL row number) of vector `stream` of the family `seed` is -1 if the top bit of
//   key = mix((mix(seed + G) ^ stream) + G),   h = mix((key ^ row) + G)            (arithmetic modulo 2^64)
// is set, else +1, with G = 0x9E3779B97F4A7C15 and the splitmix64 finaliser
//   mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31.
// A function of (seed, stream, row) alone: the same vector under every sharding.  tests/density_reference.py restates it.
__host__ __device__ inline uint64_t random_sign_mix(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
__host__ __device__ inline uint64_t random_sign_key(uint64_t seed, uint64_t stream) {
  const uint64_t G = 0x9E3779B97F4A7C15ull;
  return random_sign_mix((random_sign_mix(seed + G) ^ stream) + G);
}
__host__ __device__ inline bool random_sign_bit(uint64_t key, uint64_t row) { return (random_sign_mix((key ^ row) + 0x9E3779B97F4A7C15ull) >> 63) != 0; }

// One-sweep Lanczos step k (lag_terms.hpp has the scheme; kernels.hip: k_sweep).  The pending raw vector in w makes column k
// as u~ = w*scale, the product the operator formed; the sweep recomputes it from w and never reads the column, so that the
// column may already hold its corrected form (the end of a batch) without the sweep seeing a difference.  The sweep (full or
// correct_only) is column k's ONLY writer: the operator of a one-sweep step does not store u~ (library.hip: ApplyPass::store_u),
// and between that operator and the sweep or closing pass that follows it nothing reads column k (the repair pass of step k-1
// runs over columns 0..k-1, a stopped state never gets the column, a batch ends with the scalars of the closing pass and whatever
// would read the column next runs the pass itself first: library.hip, settle_columns).  Column 0 of the first
// call is stored by its operator.
//   full:          w0 = (v - a' u~) - beta_{k-1} u_{k-1};  per row tile, j ascending over columns 0..k-1:  d_j = x_j . w0,
//                  u -= c_j x_j,  w -= f_j x_j;  then d_k = u . w0,  w -= f_k u;  column k = u,  w stored in place of the pending
//                  vector, partial ||w||^2.  Workgroup 0 records alpha_k = a' - da, a' (lag[0]) and f (lag + f_off).
//   correct_only:  column k = u~ - sum_j c_j x_j, nothing else is read or written; workgroup 0 records a' and alpha_k.  The closing pass.
// a' = the sum of the operator's partials (fin, which then appends alpha_k to the series as k_dots does), or *a_raw.
constexpr int kLagC = 8;  // lag[kLagC + j] = c_j
struct SweepStep {
  int k;
  const double* V;  // basis slab, column j at V + j*ldv
  int64_t ldv;
  const double* v;
  double* w;
  const double* scale;
  const double* a_raw;
  double* alpha;       // series: alpha[0..k) read, alpha[k] written (fin == nullptr, k > 0)
  const double* beta;  // series: beta[0..k)
  double* lag;
  int f_off;
  int correct_only;
};
// d partials: dpartials[j*pstride + block], j <= k (k_dots' layout); ||w||^2 partials: npartials[block]
// The full sweep parks each tile's two results in LDS and stores them from a later tile, at a boundary of the chip-wide clock
// (kernels.hip: SweepPark).  launch_sweep takes the deepest parking, two tiles or one, that fits beside the 6 (k + 1) doubles of
// sums and coefficients within kSweepLdsBudget, so that two workgroups per CU still fit: two tiles up to k = 339, one up to
// k = 1022 (EIGENEX_SWEEP_PARK_TILES=1 keeps it at one).  Otherwise, in the closing pass and under EIGENEX_SWEEP_DIRECT_STORES=1
// every tile stores at its end.  The switches are read once per process.  All paths write the same bytes.
constexpr int kSweepParkBytes = 2 * kTileRows * (int)sizeof(double);  // 32 KB: column k and w of one tile
constexpr int kSweepLdsBudget = 80 * 1024;                            // per workgroup: half a CU's LDS
constexpr int kSweepStaticLds = 4 * (int)sizeof(double);              // k_sweep's block_sum scratch
// The clock slot: about 80 us (2^13 ticks of the 100 MHz clock).  Measured at 512^3 over k = 0..99 against 2^11..2^16 ticks and no
// boundary at all (profiles/sweep_stores.md): shorter slots split the workgroups' stores into more and smaller bursts, longer ones
// let most tiles leave unsynchronised at their successor's end, which gains nothing.  No result depends on it.
constexpr double kSweepSlotMicroseconds = 80.0;
// The slot with two parked tiles, chosen the same way against 2^14 and 2^15 ticks (profiles/sweep_park_depth.md): the same 2^13.
// The second tile pays where a tile is shorter than a slot (k below about 58), not by allowing a longer slot.
constexpr double kSweepSlotMicroseconds2 = 80.0;
void launch_sweep(hipStream_t s, const SweepStep& st, const InlineFin* fin, int64_t n, double* dpartials, int pstride, double* npartials,
                  int grid, const Ctrl* ctrl);
// behind the full sweep of step k, one workgroup: d_j = sum of its partials (fixed order), beta_k^2 = sum of the norm partials in
// inline_fin_sum's order (the number the operator kernel will take), c_j = (d_j - f_j)/beta_k into lag[kLagC + j], j <= k.
// max |c| > kLagGuard: c = 0, repair->stopped = 0 (the kernels of the repair pass run), ++ctrl->repairs; else repair->stopped = 1.
void launch_lag_terms(hipStream_t s, int k, const double* dpartials, int pstride, int nblocks, const double* npartials, double* lag,
                      int f_off, double threshold, Ctrl* ctrl, Ctrl* repair);
// the scalar part of the closing pass for column k, one thread: lag[0] = a' = *a_raw, alpha[k] = a' - da (k_sweep's own arithmetic,
// the same bits); the column part is a correct_only sweep with a_raw = lag, whenever it is run
void launch_close_scalars(hipStream_t s, int k, const double* a_raw, double* alpha, const double* beta, double* lag, const Ctrl* ctrl);

int grid_for_tiles(int64_t ntiles, int blocks_per_cu);
void set_num_cu(int n);

// partials[c*pstride + block], c < ncols: per-block partial dot of w0 with column c
// Vector lengths `n` of dots/update are in DOUBLES (a complex vector of N entries = 2N interleaved doubles);
// cplx selects conjugate-linear complex arithmetic; complex partials occupy rows 2c (re) and 2c+1 (im).
// src2 != nullptr: the same columns are also dotted with src2 (no recurrence) in the same pass, sums in partials2
// fin (real, single source only): alpha_k = sum of the operator kernel's partials, taken inside this kernel (InlineFin)
void launch_dots(hipStream_t s, const double* src, ThreeTerm tt, ColumnSet cs, int64_t n, double* partials,
                 int pstride, int grid, const Ctrl* ctrl, bool cplx, const double* src2 = nullptr, double* partials2 = nullptr,
                 const InlineFin* fin = nullptr, const InlineDecide* dec = nullptr);
// fused-alpha Lanczos step: h[i] = g[i] - alpha*G[i] from fused = [alpha, -, g (ncoef), G (ncoef)]; alpha joins the series
void launch_form_h(hipStream_t s, Ctrl* ctrl, const double* fused, int ncoef, double* h, double* alpha, int first);
// dst = w0 - sum_c h[c]*col_c (sequential in c); partials[block] = partial ||dst||^2
void launch_update(hipStream_t s, const double* src, double* dst, ThreeTerm tt, ColumnSet cs, const double* h,
                   int64_t n, double* partials, int grid, const Ctrl* ctrl, bool cplx, const InlineReduce* red = nullptr);
constexpr int kInlineReduceMaxCoef = 4096;  // 32 KB of LDS for the coefficients
// complex operator: n = rows; val/x/y/u_out interleaved (re, im); partials[block] = re, partials[pstride+block] = im of conj(u).y
void launch_spmv_z(hipStream_t s, const int32_t* rowptr, const int32_t* col, const double* val, const double* x_ext,
                   const double* scale, double shift_re, double shift_im, double* y, double* u_out, int64_t n,
                   double* partials, int pstride, int grid, const Ctrl* ctrl, int spmv_flags = 0, int pass = 0);
void launch_shift_dot_z(hipStream_t s, double* y, const double* u, double shift_re, double shift_im, int64_t n,
                        double* partials, int pstride, int grid, const Ctrl* ctrl);
// out[c] = sum_b partials[c*pstride + b], fixed order (deterministic second stage)
void launch_reduce(hipStream_t s, const double* partials, int pstride, int nblocks, int ncols, double* out,
                   const Ctrl* ctrl);
// y = A*(x*scale) + shift*(x*scale); u_out = x*scale (optional); partials[block] = partial (x*scale).y (optional)
// Column-blocked operators run one launch per pass: `pass` bit 0 (kPassCarry) = the row sums start from y (left by
// the previous pass), bit 1 (kPassNotLast) = store the raw row sums only (no shift, u_out, dot).
// bit 2 (kPassSelfNorm): the partials hold ||y||^2 instead of (x*scale).y (adaptive Gram-Schmidt of the Arnoldi step)
enum { kPassCarry = 1, kPassNotLast = 2, kPassSelfNorm = 4 };
// `spmv_flags`: bit 0 = XCD-contiguous tiles, bit 1 = non-temporal val/col loads (both the caller's tuning), bit 2
// (kSpmvLongRows) = the kernel variant for long rows; the host-side launchers of the CSR kernels choose it by this bit
enum { kSpmvLongRows = 4 };
// fin: beta_k = sqrt(sum of the update kernel's partials), breakdown test and scale = 1/beta_k taken inside this kernel
void launch_spmv(hipStream_t s, const int32_t* rowptr, const int32_t* col, const double* val, const double* x_ext,
                 const double* scale, double shift, double* y, double* u_out, int64_t n, double* partials, int grid,
                 const Ctrl* ctrl, int spmv_flags = 0, int pass = 0, const InlineFin* fin = nullptr,
                 const InlineArnoldiBegin* begin = nullptr, const int32_t* tile_list = nullptr, int64_t list_len = 0,
                 const ChebStep* cheb = nullptr, const MomentStep* mom = nullptr);
// (mom: the kernel takes a moments step in its epilogue: only x_ext, scale, shift, partials (two sets, mom->pstride apart) are used)
// (cheb: the kernel takes a Chebyshev step in its epilogue instead of storing y -- y, partials and the hooks are unused then)
// (tile_list: the launch covers the 256-row tiles tile_list[0 .. list_len) only -- interior / boundary launches of a shard)
// the same with 64-bit row pointers (plain real CSR in one pass): a shard may hold >= 2^31 stored entries; col stays int32
void launch_spmv64(hipStream_t s, const int64_t* rowptr, const int32_t* col, const double* val, const double* x_ext,
                   const double* scale, double shift, double* y, double* u_out, int64_t n, double* partials, int grid,
                   const Ctrl* ctrl, int spmv_flags = 0, int pass = 0, const InlineFin* fin = nullptr,
                   const InlineArnoldiBegin* begin = nullptr, const int32_t* tile_list = nullptr, int64_t list_len = 0,
                   const ChebStep* cheb = nullptr, const MomentStep* mom = nullptr);
// Row-coded operator (real fp64 in one pass; row_codes.hpp, kernels.hip: k_spmv_rows): rec = one record of rec_bytes (8 or 16)
// per row of every 256-row tile, pal = npal values, slots = the offsets.  Same tiles, grid, partial dots and hooks as launch_spmv.
struct RowCodeView {
  const uint64_t* rec;
  const double* pal;
  int npal, rec_bytes;
  RowCodeSlots slots;
};
void launch_spmv_rows(hipStream_t s, const RowCodeView& op, const double* x_ext, const double* scale, double shift, double* y,
                      double* u_out, int64_t n, double* partials, int grid, const Ctrl* ctrl, int spmv_flags = 0, int pass = 0,
                      const InlineFin* fin = nullptr, const InlineArnoldiBegin* begin = nullptr, const int32_t* tile_list = nullptr,
                      int64_t list_len = 0, const ChebStep* cheb = nullptr, const MomentStep* mom = nullptr);
// records of a device-resident CSR shard (rowptr or rowptr64) for rows [0, nrec_rows) with given tables; *bad counts rows that
// do not fit them
struct RowCodePalette {
  uint64_t bits[kRowCodeMaxValues];
  int n;
};
void launch_encode_rows(hipStream_t s, const int32_t* rowptr, const int64_t* rowptr64, const int32_t* col, const double* val, int64_t n,
                        int64_t nrec_rows, const RowCodeSlots& slots, int nslots, const RowCodePalette& pal, int rec_bytes, uint8_t* rec,
                        unsigned int* bad);
// Column-sorted row tiles (real fp64; kernels.hip: k_spmv_sorted): tile t = rows [t*T, (t+1)*T), T = tile_rows, slice k =
// the k-th range of the operator input (global column order).  Segment (t, k) = entries base[t*(K+1)+k] .. base[t*(K+1)+k+1)
// of cp/val, sorted by column, padded to a multiple of 4 (val 0, a spare slot); slot = place of the entry in row order
// inside the segment; off[(t*K+k)*(T+1) + i] = first slot of row i of the tile (so a row's products are added
// in stored order).  At most kSortCap - 4 entries per segment.
constexpr int kSortRows = 4096;
constexpr int kSortBlock = 1024;
constexpr int kSortCap = 8192;            // entries of one segment (two rounds of 4 per lane); two LDS buffers of this size
constexpr int kSortBufDoubles = kSortCap + kSortCap / 32 + 8;
constexpr int kSortSliceElems = 32768;    // <= 256 KB of fp64 input per slice
struct SortedOperatorView {
  const int32_t* base;
  const uint32_t* cp;   // per entry: column position inside its slice (low 16 bits) | row-order slot (high 16 bits)
  const double* val;
  const uint16_t* off;
  int nslices;
  int tile_rows;        // 4096, 2048 or 1024: the largest for which every segment fits the product buffer
  int slice_width;      // positions per slice (<= 32768); position = place of a column in GLOBAL column order
  int64_t n_low, npad, nloc;  // position p -> index into the operator input: p < n_low: halo slot p (at npad + p);
                              // p < n_low + nloc: own row p - n_low; else halo slot p - nloc (at npad + p - nloc)
};
int sorted_grid(int64_t n, int tile_rows);
void launch_spmv_sorted(hipStream_t s, const SortedOperatorView& op, const double* x_ext, const double* scale, double shift, double* y,
                        double* u_out, int64_t n, double* partials, const Ctrl* ctrl, int pass = 0);
// Split tiles (real fp64; kernels.hip: k_spmv_split + k_split_combine; layout and reasons in split_layout.hpp): workgroup
// w = tile*groups + group walks the chunks wg_chunk[w] .. wg_chunk[w+1); chunk c = entries chunk[4c] .. chunk[4c+1) of cp/val,
// chunk[4c+2] = position (global column order) of its first column; cp = row in tile << 18 | position - that.  The
// partial row sums of group g go to part[g*part_stride + row]; k_split_combine adds them in ascending group order and does
// what the other operator kernels do in their epilogue (shift, u_out, partial dot).
struct SplitOperatorView {
  const int32_t* wg_chunk;
  const int4* chunk;
  const uint32_t* cp;
  const double* val;
  int groups, tile_rows;
  int64_t n_low, npad, nloc;  // position -> index into the operator input, as for SortedOperatorView
  double* part;
  int64_t part_stride;
};
// complex: val / x / y / u_out / part hold (re, im) pairs, tile_rows <= 8192; partials as launch_spmv_z
void launch_spmv_split_z(hipStream_t s, const SplitOperatorView& op, const double* x_ext, const double* scale, double shift_re,
                         double shift_im, double* y, double* u_out, int64_t n, double* partials, int pstride, const Ctrl* ctrl, int pass = 0);
int split_combine_grid(int64_t n);
bool prepare_spmv_split();
void launch_spmv_split(hipStream_t s, const SplitOperatorView& op, const double* x_ext, const double* scale, double shift, double* y,
                       double* u_out, int64_t n, double* partials, const Ctrl* ctrl, int pass = 0, const InlineArnoldiBegin* begin = nullptr);
// Block-sparse operator (the reference's BlockTensor<Scalar,2> layout, block_tensor.hpp:1193-1206, real or complex fp64):
// 8 bytes per stored entry plus one column index per block COLUMN (4/rows bytes per entry) instead of CSR's 12.
//   group g = the rows of one sector that this shard owns, rows grow0[g] .. grow0[g+1].  Its blocks, side by side,
//             are one dense column-major strip rows(g) x W(g) at bval[gent[g]]; the input column of strip column j
//             is cols[gcol[g] + j] (local/halo numbering); rowgrp[r] = group of row r
// Summation order: strip columns ascending = block by block, columns ascending = the stored order of the
// flattened rows, products rounded before they are added -- bit-identical to k_spmv on the CSR form.
struct BlockOperatorView {
  const double* bval;
  const int64_t* gent;
  const int64_t* gcol;
  const int32_t* cols;
  const int32_t* grow0;
  const int32_t* rowgrp;
};
void launch_block_spmv(hipStream_t s, const BlockOperatorView& op, const double* x_ext, const double* scale, double shift,
                       double* y, double* u_out, int64_t n, double* partials, int grid, const Ctrl* ctrl, int pass = 0);
// complex blocks: bval holds (re, im) pairs, gent counts entries; x/y/u_out interleaved; partials as launch_spmv_z
void launch_block_spmv_z(hipStream_t s, const BlockOperatorView& op, const double* x_ext, const double* scale, double shift_re,
                         double shift_im, double* y, double* u_out, int64_t n, double* partials, int pstride, int grid,
                         const Ctrl* ctrl, int pass = 0);
// Matrix-free spin-1/2 operator (eigenex_spin_upload, eigenex_spin_sector_upload; spin_model.hpp and spin_sector.hpp have the
// row definitions, spin_rows.hpp the walk): row s is its diagonal entry followed by its flips, products rounded before they are
// added, in table order -- the rows eigenex_spin_csr / eigenex_spin_sector_csr write, so bit-identical to k_spmv on that CSR.
// op, lo_rank and hi_base live in device memory.  Full space: lo_rank = hi_base = nullptr, only op->model is read, n = 2^n_sites
// rows, row s is state s.  A sector of fixed magnetisation: the two rank tables of the sector, n = C(n_sites, n_up) rows, row r
// is the state of rank r, unranked by the lane; columns are ranks.
// same contract as launch_block_spmv (one row per lane, 256-row tiles)
void launch_spin_spmv(hipStream_t s, const SpinSectorView* op, const uint32_t* lo_rank, const uint32_t* hi_base, const double* x_ext,
                      const double* scale, double shift, double* y, double* u_out, int64_t n, double* partials, int grid, const Ctrl* ctrl,
                      int pass = 0);
// the same real operator on interleaved complex vectors (eigenex_spin_upload_z, eigenex_spin_sector_upload_z): each part of y is
// launch_spin_spmv's sum of that part of x, the row walked once; complex shift, u_out and partials as launch_spmv_z
void launch_spin_spmv_z(hipStream_t s, const SpinSectorView* op, const uint32_t* lo_rank, const uint32_t* hi_base, const double* x_ext,
                        const double* scale, double shift_re, double shift_im, double* y, double* u_out, int64_t n, double* partials,
                        int pstride, int grid, const Ctrl* ctrl, int pass = 0);
// Spin correlations of the vector x over the rows of a matrix-free spin operator (eigenex_spin_measure; spin_measure.hpp has the
// definition): one chunk of terms per launch (device memory); op, lo_rank and hi_base as for launch_spin_spmv (full space: null
// tables, op is not read).  x is only read; the grid's partial sums go to partials[sum * pstride + workgroup], sum = 0 (norm2),
// 1 + t (diag), 1 + kSpinMeasureChunk + t (flip): (2 * kSpinMeasureChunk + 1) * pstride doubles, pstride >= grid.  Always runs.
// es is the doubles per element of x, here and below: 1 a real vector, 2 an interleaved complex one (16-byte aligned), of which
// the sums are the Hermitian ones of spin_measure.hpp, with the same partials and second stage.
void launch_spin_measure(hipStream_t s, int es, const SpinMeasureChunk* chunk, const SpinSectorView* op, const uint32_t* lo_rank,
                         const uint32_t* hi_base, const double* x, int64_t n, double* partials, int pstride, int grid);
// its second stage: the partials of nblocks workgroups added in a fixed order, the chunk's ndiag and nflip live sums stored to
// diag_out[t] and flip_out[t], norm2 to *norm_out unless that is NULL
void launch_spin_measure_reduce(hipStream_t s, const double* partials, int pstride, int nblocks, int ndiag, int nflip, double* diag_out,
                                double* flip_out, double* norm_out);
// The observables of the real vector x against ncols = 1 .. kSpinMeasureColumns columns V, V + ldv, ... (eigenex_spin_measure_columns;
// spin_measure_columns.hpp has the definition): one chunk of terms and one chunk of columns per launch; chunk, op, lo_rank and
// hi_base as for launch_spin_measure.  x and V are only read and may overlap.  The grid's partial sums go to partials[sum *
// pstride + workgroup], sum = t * J + j (diag) and (kSpinMeasureChunk + t) * J + j (flip), J = kSpinMeasureColumns: 2 *
// kSpinMeasureChunk * J * pstride doubles, pstride >= grid; the sums of a batch of kSpinBatch terms without a live term are not
// written.  Always runs.
void launch_spin_measure_columns(hipStream_t s, const SpinMeasureChunk* chunk, const SpinSectorView* op, const uint32_t* lo_rank,
                                 const uint32_t* hi_base, const double* x, const double* V, int64_t ldv, int ncols, int64_t n, double* partials,
                                 int pstride, int grid);
// its second stage: the partials of nblocks workgroups added in a fixed order, the live sums stored to diag_out[t * ldo + j] and
// flip_out[t * ldo + j], t below the chunk's ndiag or nflip, j below ncols
void launch_spin_measure_columns_reduce(hipStream_t s, const double* partials, int pstride, int nblocks, int ndiag, int nflip, int ncols, int ldo,
                                        double* diag_out, double* flip_out);
// A sum of site operators applied to x, y = O x (eigenex_spin_site_apply; spin_site.hpp has the definition and the table): one
// launch.  table, dst_op, src_lo and src_hi live in device memory.  y has n rows, those of the DESTINATION operator, whose view
// dst_op is; src_lo and src_hi are the rank tables of the SOURCE operator, on whose rows x lives (full space: null tables, dst_op
// is not read).  y may be x for Z only.  The grid's partial sums of y_r^2 go to partials[workgroup], `grid` doubles; their second
// stage is launch_spin_measure_reduce(s, partials, grid, grid, 0, 0, nullptr, nullptr, norm_out).  Always runs.  es = 2: x and y
// are interleaved complex vectors, the table's complex coefficients apply and the sums are those of |y_r|^2.
void launch_spin_site_apply(hipStream_t s, int es, const SpinSiteTable* table, const SpinSectorView* dst_op, const uint32_t* src_lo,
                            const uint32_t* src_hi, const double* x, double* y, int64_t n, double* partials, int grid);
// The reduced density matrix of x over the rows of a matrix-free spin operator (eigenex_spin_rdm; spin_rdm.hpp has the definition
// and the work table): one workgroup per item, n_items of them, with 64-row tiles (big) or one 16-row tile; table, items, op,
// lo_rank and hi_base live in device memory (full space: null tables, op is not read).  x is only read; slice s of a block writes
// the entries i >= j of its tile to partials[block.part_offset + s * d * d + i + j * d].  Always runs.
void launch_spin_rdm(hipStream_t s, int es, bool big, const SpinRdmTable* table, const SpinRdmItem* items, int n_items,
                     const SpinSectorView* op, const uint32_t* lo_rank, const uint32_t* hi_base, const double* x, double* partials);
// its second stage: every entry i >= j of every block is the sum of its slices in ascending order, written to (i, j) and (j, i)
// of out (table->total doubles, `total` on the host)
void launch_spin_rdm_reduce(hipStream_t s, int es, const SpinRdmTable* table, int64_t total, const double* partials, double* out);
// For an interleaved complex x (es = 2; eigenex_spin_rdm_z) the two stages take the same table and items; partials and out hold
// (re, im) pairs at the same indices, so 2 * part_total and 2 * total doubles, 16-byte aligned like x.
// Matrix-free spin-1/2 operator in a momentum sector (eigenex_spin_momentum_upload; spin_momentum.hpp has the definition,
// spin_rows.hpp the walk): row r is the representative reps[r], its diagonal entry followed by the bond flips whose orbit carries
// the momentum, in table order -- the rows eigenex_spin_momentum_csr writes, so bit-identical to k_spmv (es = 1, a real momentum,
// val.re) or k_spmv_z (es = 2) on that CSR.  op, reps (n entries) and bucket live in device memory.  The contract of
// launch_spin_spmv / launch_spin_spmv_z; pstride is read for es = 2 only.
void launch_spin_momentum_spmv(hipStream_t s, int es, const SpinMomentumView* op, const uint32_t* reps, const uint32_t* bucket,
                               const double* x_ext, const double* scale, double shift_re, double shift_im, double* y, double* u_out, int64_t n,
                               double* partials, int pstride, int grid, const Ctrl* ctrl, int pass = 0);
// ... with 64-bit states (eigenex_spin_momentum64_upload): the same kernel text on uint64_t words, 8 bytes per row of reps,
// bit-identical to the CSR upload of eigenex_spin_momentum64_csr's rows.  The same contract.
void launch_spin_momentum_spmv(hipStream_t s, int es, const SpinMomentum64View* op, const uint64_t* reps, const uint32_t* bucket,
                               const double* x_ext, const double* scale, double shift_re, double shift_im, double* y, double* u_out, int64_t n,
                               double* partials, int pstride, int grid, const Ctrl* ctrl, int pass = 0);
// Diagonal correlations in the momentum basis (eigenex_spin_momentum_measure; spin_momentum.hpp has the definition): one chunk
// of masks over the n rows of x, whose states are reps, of either word.  The grid's partial sums go to
// partials[sum * pstride + workgroup], sum 0 norm2 and 1 + t the chunk's mask t; second stage launch_spin_measure_reduce with
// nflip = 0.  Always runs; writes no vector.
void launch_spin_momentum_measure(hipStream_t s, int es, const SpinMomentumMeasureChunk* chunk, const uint32_t* reps, const double* x, int n_sites,
                                  int cell, int n_trans, int64_t n, double* partials, int pstride, int grid);
void launch_spin_momentum_measure(hipStream_t s, int es, const SpinMomentumMeasureChunk* chunk, const uint64_t* reps, const double* x, int n_sites,
                                  int cell, int n_trans, int64_t n, double* partials, int pstride, int grid);
// expand (eigenex_spin_momentum_expand): y, the n = C(n_sites, n_up) rows of the sector operator whose view dst_op is, from the
// momentum vector x on the rows of op.  The grid's partial sums of |y_r|^2 go to partials[workgroup]; second stage as for
// launch_spin_site_apply.  Always runs.
void launch_spin_momentum_expand(hipStream_t s, int es, const SpinMomentumView* op, const SpinSectorView* dst_op, const uint32_t* reps,
                                 const uint32_t* bucket, const double* x, double* y, int64_t n, double* partials, int grid);
// A sum of site operators between two momentum sectors (eigenex_spin_momentum_site_apply(_z); spin_momentum_site.hpp has the
// definition and the table): y, the n rows of the destination sector whose representatives dst_reps are, from x on the rows of
// the source sector (src_op, src_reps, src_bucket), of either word.  y may be x for Z where the two sectors are one.  The grid's
// partial sums of |y_r|^2 go to partials[workgroup]; second stage as for launch_spin_site_apply.  Always runs.
void launch_spin_momentum_site_apply(hipStream_t s, int es, const SpinMomentumSiteTable* table, const SpinMomentumView* src_op,
                                     const uint32_t* src_reps, const uint32_t* src_bucket, const uint32_t* dst_reps, const double* x, double* y,
                                     int64_t n, double* partials, int grid);
void launch_spin_momentum_site_apply(hipStream_t s, int es, const SpinMomentumSiteTable* table, const SpinMomentum64View* src_op,
                                     const uint64_t* src_reps, const uint32_t* src_bucket, const uint64_t* dst_reps, const double* x, double* y,
                                     int64_t n, double* partials, int grid);
// host-operator path: u_out = x*scale
void launch_scale(hipStream_t s, const double* x, const double* scale_dev, double scale_host, double* out, int64_t n,
                  const Ctrl* ctrl);
// host-operator path: y += shift*u ; partials[block] = partial u.y
void launch_shift_dot(hipStream_t s, double* y, const double* u, double shift, int64_t n, double* partials, int grid,
                      const Ctrl* ctrl);
// the Chebyshev step behind an operator kernel that has stored y = (A - center) t_k: n in DOUBLES (complex vectors: 2N, the
// coefficients are real); reads y, t_prev and acc, writes t_next and acc
void launch_cheb_combine(hipStream_t s, const double* y, const ChebStep& step, int64_t n, int grid, const Ctrl* ctrl);
// the moments step behind an operator kernel that has stored y = (A - center) t_k: n in DOUBLES (a complex vector's plain real dot
// over 2N doubles is Re<t_k, t_{k+1}>); reads y, step.t_cur and step.t_prev, writes step.t_next and the two partial sums per workgroup
void launch_cheb_moments(hipStream_t s, const double* y, const MomentStep& step, int64_t n, double* partials, int grid, const Ctrl* ctrl);
// out[r*es] = +-1 (random_sign_bit of the global row row0 + r), imaginary parts 0, r < n
void launch_random_signs(hipStream_t s, double* out, int64_t n, int64_t row0, int es, uint64_t seed, uint64_t stream);
// gather send buffer: out[i] = x[idx[i]]
void launch_pack(hipStream_t s, const double* x, const int32_t* idx, int64_t count, int es, double* out,
                 const Ctrl* ctrl);
// loopback all-reduce: every p[s][i] = sum_s p[s][i] (fixed order); pointers travel as kernel arguments
constexpr int kMaxLoopbackShards = 64;
struct PtrPack {
  double* p[kMaxLoopbackShards];
};
void launch_sum_shards(hipStream_t s, const PtrPack& bufs, int nshards, int n);

// ---- scalar finalisers (one thread) ----
enum FinNormMode { kFinInit = 0, kFinLanczos = 1, kFinArnoldi = 2 };
enum FinAlphaMode { kFinishAlpha = 8, kFinishAlphaFirst = 9 };
// one launch for "sum the per-block partials of one scalar / (re, im) pair" + the decision k_fin_norm (mode = a
// FinNormMode, series = beta) or k_fin_alpha (mode = a FinAlphaMode, series = alpha) takes from it
void launch_reduce_fin(hipStream_t s, const double* partials, int pstride, int nblocks, int ncomp, double* out, Ctrl* ctrl,
                       int mode, double* series, double threshold);
// nrm2 = ||w||^2 (all-reduced).  kFinInit: fail if sqrt < threshold, else scale = 1/nrm.
// kFinLanczos: beta.push_back(sqrt); breakdown if <= threshold else scale = 1/beta.
// kFinArnoldi: residue = sqrt.
void launch_fin_norm(hipStream_t s, Ctrl* ctrl, const double* nrm2, double threshold, int mode, double* beta);
// Lanczos: alpha.push_back(*val); counts as a successful call; first==1: no iteration increment
void launch_fin_alpha(hipStream_t s, Ctrl* ctrl, const double* val, double* alpha, int first, int cap);
// Arnoldi start of a later call: stop if residue <= threshold or basis full, else H[k][k-1] = residue, scale = 1/residue
void launch_arnoldi_begin(hipStream_t s, Ctrl* ctrl, double threshold, int64_t n_global, int cap, double* H, int ldh,
                          int es);
// Arnoldi end of a call: H[0..k][k] = h[0..k], H[k+1][k] = 0, ++iterations
void launch_arnoldi_end(hipStream_t s, Ctrl* ctrl, const double* h, double* H, int ldh, int es);
void launch_add_small(hipStream_t s, double* dst, const double* src, int n, const Ctrl* ctrl);
// adaptive second Gram-Schmidt pass: pass2->stopped = !(nrm2_after < eta2*nrm2_before) (or ctrl stopped)
void launch_decide_second_pass(hipStream_t s, const Ctrl* ctrl, Ctrl* pass2, const double* nrm2_before, const double* nrm2_after, double eta2);
void launch_select_norm(hipStream_t s, const Ctrl* pass2, const double* nrm2_first, const double* nrm2_second, double* nrm2_final);
// single-shard merges of the tiny launches around the conditional second pass (see kernels.hip)
// before_partials != nullptr: ||v||^2 before the pass is still the operator kernel's partial sums; they are added here (in
// k_reduce's order) and the sum is left in *nrm2_before
void launch_reduce_decide(hipStream_t s, const double* partials, int nblocks, double* nrm2_first, const Ctrl* ctrl, Ctrl* pass2,
                          double* nrm2_before, double eta2, const double* before_partials = nullptr, int before_nblocks = 0);
void launch_arnoldi_tail(hipStream_t s, const double* partials, int nblocks, Ctrl* ctrl, const Ctrl* pass2, double* h, const double* h2,
                         int ncoef, const double* nrm2_first, double* nrm2_final, double* H, int ldh, int es);
void launch_restart_fix(hipStream_t s, Ctrl* ctrl, double* alpha, double* beta, int m, int nkeep, double coupling_last);
// Krylov-Schur restart of an Arnoldi state: columns 0..nkeep-1 of H (ldh x ncols) = B ((nkeep+1) x nkeep, leading dimension ldb
// entries, es doubles per entry), everything else of H zeroed; nvec = nalpha = nkeep, stopped = 0, keep_coupling = 1
void launch_arnoldi_restart_fix(hipStream_t s, Ctrl* ctrl, double* H, int ldh, int ncols, int es, const double* B_dev, int ldb, int nkeep);
// vector accepted into the basis: ++nvec  (after the operator has been applied with `scale`)
void launch_accept_vector(hipStream_t s, Ctrl* ctrl);

// counts malformed row pointers (bad[0]) and out-of-range columns (bad[1]) of a device-resident CSR
void launch_check_csr(hipStream_t s, const int32_t* rowptr, const int32_t* col, int64_t n, int64_t nnz, int64_t ncols, unsigned int* bad);
// synthetic 7-point Laplacian rows [rb, re) of an n^3 grid; cols remapped to local/halo numbering
// rowptr64 != nullptr: 64-bit row pointers (a shard with >= 2^31 stored entries), rowptr unused
void launch_laplacian3d(hipStream_t s, int64_t n, int64_t rb, int64_t re, int64_t lower_start, int64_t n_lower,
                        int64_t halo_base, int32_t* rowptr, int64_t* rowptr64, int32_t* col, double* val);

// Ritz vectors / basis compression: X[:, e] = sum_m St[m*ne_pack + e] * V[:, m] for e < nev <= ne_pack; St is the
// coefficient block packed [nvec][ne_pack], zero-padded.  ne_pack = 8: also partial squared norms of the results
// (partials[e*pstride + block]); ne_pack = 16: no norms (thick-restart compression).  X columns need the padded
// stride of the basis (rows behind n are written as zeros).
void launch_ritz(hipStream_t s, const double* V, int64_t ldv, int nvec, const double* St_dev, int ne_pack, int nev,
                 double* X, int64_t ldx, int64_t n, double* partials, int pstride, int grid);
// Compression of a COMPLEX basis with COMPLEX coefficients in one pass (Krylov-Schur restart): X[:, e] = sum_m Ct[m*8 + e] * V[:, m],
// e < nev <= 8; V, X and Ct hold (re, im) pairs, Ct is packed [nvec][8] and zero-padded, n counts complex entries, ldv / ldx doubles.
void launch_compress_z(hipStream_t s, const double* V, int64_t ldv, int nvec, const double* Ct_dev, int nev, double* X, int64_t ldx,
                       int64_t n, int grid);
// per column: first local ENTRY with |z| > 0 (n if none) and its value: out[3e] = index, out[3e+1..2] = (re, im);
// es = doubles per entry, ldx in doubles
void launch_first_nonzero(hipStream_t s, const double* X, int64_t ldx, int ncol, int64_t n, int es, double* out);
// column e *= factors[2e] + i*factors[2e+1] (real columns: real part only)
void launch_scale_columns(hipStream_t s, double* X, int64_t ldx, int ncol, int64_t n, int es, const double* factors_dev);
// complex coefficients: out column e = X[:,2e] + i*X[:,2e+1] (basis real or complex), partial squared norms
void launch_ritz_combine(hipStream_t s, const double* X, int64_t ldx, int nc, int64_t n, int es, double* out,
                         int64_t ldo, double* partials, int pstride, int grid);

}  // namespace eigenex
