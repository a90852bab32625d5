// The reduced density matrix of a real vector over the rows of a spin-1/2 operator (host side, no HIP): the definition, the
// argument check, the layout of the result, the work table of the kernels (kernels.hip: k_spin_rdm<SECTOR, TILE, E>,
// k_spin_rdm_reduce<E>, each written once for real and complex vectors) and the
// host evaluation.  Shared by the library (eigenex_spin_rdm, eigenex_spin_rdm_layout, eigenex_spin_rdm_host) and by the host
// programs tests/cpp/spin_rdm_sanitize.cpp and spin_rdm_z_sanitize.cpp, which run this file under AddressSanitizer + UBSan.
//
// The state is a real vector x over the rows of spin_model.hpp (n_up = -1: the full space, row s is state s) or of
// spin_sector.hpp (row r is the state of rank r among the states with n_up sites up).  The subsystem A is a 32-bit site mask
// mask_a:
//   nA = popcount(mask_a), nB = n_sites - nA, mask_b = the complement of mask_a within the n_sites sites
//   dep_A(a) deposits the nA-bit word a into mask_a: bit j of a goes to the j-th lowest set bit of the mask; dep_B likewise
// Full space: one block, d = 2^nA,
//   rho[a, a'] = sum_{b = 0}^{2^nB - 1} x[dep_A(a) | dep_B(b)] * x[dep_A(a') | dep_B(b)]
// Sector: rho_A is block-diagonal in the number k of up sites inside A.  Blocks k = kmin .. kmax, kmin = max(0, n_up - nB),
// kmax = min(nA, n_up); block k has d_k = C(nA, k) rows, row i is a = spin_sector_unrank(nA, k, i); b runs over
// spin_sector_unrank(nB, n_up - k, j), j = 0 .. C(nB, n_up - k) - 1; the vector element is x[rank(dep_A(a) | dep_B(b))].
// Output: the blocks packed in ascending k, each a full d_k x d_k column-major matrix, both triangles stored, out[i,j] and
// out[j,i] the same bits.  The sums are raw and unnormalised, like spin_measure: the trace is sum x^2.  The host definition
// adds the b terms in ascending order, one fma per term.
//
// A complex vector (interleaved (re, im) pairs; eigenex_spin_rdm_z, eigenex_spin_rdm_host_z; the kernels with E = SpinZ):
// rho_k = M_k M_k^H, rho[i, j] = sum_b M[i, b] conj(M[j, b]), over the same blocks, layout, limit and
// argument check.  Output: the blocks packed in ascending k, each a full column-major d_k x d_k matrix of interleaved (re, im)
// pairs, 2 * offsets[n_blocks] doubles; raw sums, the trace is sum |x|^2.  Two properties are part of the definition and every
// evaluation keeps them bit for bit: Im rho[i, i] is stored as +0.0 (not the computed chain: with fma the two products of a
// diagonal term do not cancel exactly), and (j, i) is written from the two values of (i, j) with the imaginary part negated.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include "spin_measure.hpp"

namespace eigenex {

constexpr int kSpinRdmMaxBlock = 4096;                   // rows of one block: nA <= 12 in the full space, <= 14 in a sector
constexpr int kSpinRdmMaxBlocks = kSectorMaxSites + 1;   // k = 0 .. 32
constexpr int kSpinRdmBigTile = 64, kSpinRdmSmallTile = 16;     // blocks above 16 rows, blocks of at most 16 rows
constexpr int kSpinRdmBigChunk = 32, kSpinRdmSmallChunk = 128;  // b's staged in LDS at a time, per tile size
constexpr int kSpinRdmSmallGroups = 16;                  // a 16-tile workgroup splits a chunk's b's over 16 groups of 16 threads
// The complex kernel (k_spin_rdm<SECTOR, TILE, SpinZ>) stages half as many b's, so that its panels of 16-byte elements take the real kernel's LDS:
//   64-row tile: CHUNK = 16, two panels of 16 x (64 + 1) pairs = 33 280 B; with the staged states and (in a sector) the
//     binomials 38 080 B per workgroup (real kernel: 38 656 B); four 16-byte gathers per lane and panel
//   16-row tile: CHUNK = 64, one panel of 64 x (16 + 1) pairs = 17 408 B; the 16 groups' tiles go through red[] of the real
//     kernel's size, 32 768 B, twice (the real parts, then the imaginary ones), not through one of twice the size, which would
//     leave one workgroup per CU: 54 720 B per workgroup in a sector (real kernel: 56 000 B); four gathers per lane
// (the byte counts are the compiler's, profiles/spin_entanglement_z.md).  The panels are b-major with a pitch of TILE + 1
// pairs (16-byte units, so every element is 16-byte aligned), and a lane's four rows are t, t + TILE/4, t + 2 TILE/4,
// t + 3 TILE/4 (spin_rdm_rows.hpp: SpinRdmGeometry<SpinZ, TILE>::lane_row), not four consecutive ones: each is one 16-byte LDS read, and the 16
// lanes of a read group then take 16 consecutive pairs, 256 bytes = one row of the 64 banks: no conflict, where the real
// kernel's four consecutive doubles per lane are a 2-way one.  A gather whose b's run along the lanes stores with a stride of
// TILE + 1 pairs, 16 bytes past a multiple of the 128 bytes a store covers per cycle: eight consecutive lanes fill the 32 store
// banks once, the rate of a contiguous 16-byte store (the real kernel's TILE + 2 doubles do the same for 8-byte stores).
constexpr int kSpinRdmBigChunkZ = 16, kSpinRdmSmallChunkZ = 64;
// partial sums of one block beyond its first slice: at most 2^21 doubles (16 MiB), so that the partials of a call never exceed
// the packed output's length plus kSpinRdmMaxBlocks * 16 MiB.  The complex call (eigenex_spin_rdm_z) takes the same plan, the
// same slices, and its partials are (re, im) pairs: twice these bytes.
constexpr int64_t kSpinRdmSliceBudget = int64_t(1) << 21;

struct SpinRdmArgs {
  int n_sites, n_up;  // n_up = -1: the full space
  uint32_t mask_a;
};

// blocks, their dimensions and where they start in the packed output (offsets[n_blocks] is the output's length)
struct SpinRdmLayout {
  int nA, nB, n_blocks, k_first;  // full space: one block, k_first = 0
  uint32_t mask_b;
  int64_t dims[kSpinRdmMaxBlocks], nb[kSpinRdmMaxBlocks], offsets[kSpinRdmMaxBlocks + 1];
};

// of arguments whose geometry and mask are valid (the block limit is not looked at)
inline void spin_rdm_layout(const SpinRdmArgs& a, SpinRdmLayout& l) {
  const uint32_t all = a.n_sites < 32 ? (uint32_t(1) << a.n_sites) - 1 : 0xFFFFFFFFu;
  l.nA = __builtin_popcount(a.mask_a), l.nB = a.n_sites - l.nA, l.mask_b = all & ~a.mask_a;
  l.offsets[0] = 0;
  if (a.n_up == -1) {
    l.n_blocks = 1, l.k_first = 0;
    l.dims[0] = int64_t(1) << l.nA, l.nb[0] = int64_t(1) << l.nB;
  } else {
    const int kmin = a.n_up - l.nB > 0 ? a.n_up - l.nB : 0, kmax = l.nA < a.n_up ? l.nA : a.n_up;
    l.n_blocks = kmax - kmin + 1, l.k_first = kmin;
    for (int n = 0; n < l.n_blocks; ++n) l.dims[n] = spin_sector_dim(l.nA, kmin + n), l.nb[n] = spin_sector_dim(l.nB, a.n_up - kmin - n);
  }
  for (int n = 0; n < l.n_blocks; ++n) l.offsets[n + 1] = l.offsets[n] + l.dims[n] * l.dims[n];
}

// nullptr if the subsystem is valid, else what is wrong with it
inline const char* spin_rdm_error(const SpinRdmArgs& a) {
  if (const char* why = spin_measure_error(SpinMeasureArgs{a.n_sites, a.n_up, 0, nullptr, 0, nullptr})) return why;
  if (a.mask_a == 0) return "the subsystem mask is zero";
  if (a.n_sites < 32 && (a.mask_a >> a.n_sites) != 0) return "the subsystem mask names a site outside 0..n_sites-1";
  if (__builtin_popcount(a.mask_a) == a.n_sites) return "the subsystem leaves no site out: its complement is empty";
  SpinRdmLayout l;
  spin_rdm_layout(a, l);
  for (int n = 0; n < l.n_blocks; ++n)
    if (l.dims[n] > kSpinRdmMaxBlock) return "a block of the reduced density matrix has more than 4096 rows (at most 12 sites in the full space, 14 in a sector)";
  return nullptr;
}

// dep(w): bit j of w goes to the j-th lowest set bit of the mask, from the definition (site by site)
inline uint32_t spin_rdm_deposit(uint32_t w, uint32_t mask) {
  uint32_t s = 0;
  int j = 0;
  for (int p = 0; p < 32; ++p)
    if ((mask >> p) & 1u) {
      if ((w >> j) & 1u) s |= uint32_t(1) << p;
      ++j;
    }
  return s;
}

// The definition, evaluated: x has spin_measure_rows entries, out the layout's length.  M_k[i, j] = x[row(dep_A(a_i) | dep_B(b_j))]
// is gathered block by block; every entry of the lower triangle is one fma chain over ascending j, stored to both triangles.
inline void spin_rdm_host(const SpinRdmArgs& a, const double* x, double* out) {
  const bool sector = a.n_up != -1;
  SpinRdmLayout l;
  spin_rdm_layout(a, l);
  SpinSectorTables t;
  if (sector) spin_sector_build_tables(a.n_sites, a.n_up, t);
  for (int n = 0; n < l.n_blocks; ++n) {
    const int k = l.k_first + n;
    const size_t d = (size_t)l.dims[n], nb = (size_t)l.nb[n];
    std::vector<uint32_t> sb(nb);
    for (size_t j = 0; j < nb; ++j) sb[j] = spin_rdm_deposit(sector ? spin_sector_unrank(l.nB, a.n_up - k, (int64_t)j) : (uint32_t)j, l.mask_b);
    std::vector<double> M(d * nb);
    for (size_t i = 0; i < d; ++i) {
      const uint32_t sa = spin_rdm_deposit(sector ? spin_sector_unrank(l.nA, k, (int64_t)i) : (uint32_t)i, a.mask_a);
      for (size_t j = 0; j < nb; ++j) M[i * nb + j] = x[sector ? (size_t)spin_sector_rank(t, sa | sb[j]) : (size_t)(sa | sb[j])];
    }
    double* o = out + l.offsets[n];
    for (size_t i = 0; i < d; ++i)
      for (size_t j = 0; j <= i; ++j) {
        double acc = 0.0;
        for (size_t b = 0; b < nb; ++b) acc = std::fma(M[i * nb + b], M[j * nb + b], acc);
        o[i + j * d] = acc, o[j + i * d] = acc;
      }
  }
}

// The definition for a complex vector (x: interleaved pairs, out: 2 * the layout's length): for every i >= j one chain over
// ascending b with four fmas per term, in this order; the diagonal's imaginary part is +0.0 and (j, i) the conjugate of (i, j).
inline void spin_rdm_host_z(const SpinRdmArgs& a, const double* x, double* out) {
  const bool sector = a.n_up != -1;
  SpinRdmLayout l;
  spin_rdm_layout(a, l);
  SpinSectorTables t;
  if (sector) spin_sector_build_tables(a.n_sites, a.n_up, t);
  for (int n = 0; n < l.n_blocks; ++n) {
    const int k = l.k_first + n;
    const size_t d = (size_t)l.dims[n], nb = (size_t)l.nb[n];
    std::vector<uint32_t> sb(nb);
    for (size_t j = 0; j < nb; ++j) sb[j] = spin_rdm_deposit(sector ? spin_sector_unrank(l.nB, a.n_up - k, (int64_t)j) : (uint32_t)j, l.mask_b);
    std::vector<double> Mr(d * nb), Mi(d * nb);
    for (size_t i = 0; i < d; ++i) {
      const uint32_t sa = spin_rdm_deposit(sector ? spin_sector_unrank(l.nA, k, (int64_t)i) : (uint32_t)i, a.mask_a);
      for (size_t j = 0; j < nb; ++j) {
        const size_t r = sector ? (size_t)spin_sector_rank(t, sa | sb[j]) : (size_t)(sa | sb[j]);
        Mr[i * nb + j] = x[2 * r], Mi[i * nb + j] = x[2 * r + 1];
      }
    }
    double* o = out + 2 * l.offsets[n];
    for (size_t i = 0; i < d; ++i)
      for (size_t j = 0; j <= i; ++j) {
        double re = 0.0, im = 0.0;
        for (size_t b = 0; b < nb; ++b) {
          const double ar_i = Mr[i * nb + b], ai_i = Mi[i * nb + b], ar_j = Mr[j * nb + b], ai_j = Mi[j * nb + b];
          re = std::fma(ar_i, ar_j, re);
          re = std::fma(ai_i, ai_j, re);
          im = std::fma(ai_i, ar_j, im);
          im = std::fma(-ar_i, ai_j, im);
        }
        if (i == j) im = 0.0;
        o[2 * (i + j * d)] = re, o[2 * (i + j * d) + 1] = im;
        o[2 * (j + i * d)] = re, o[2 * (j + i * d) + 1] = i == j ? 0.0 : -im;
      }
  }
}

// ---- the work table of the kernels (device memory; every lane of a workgroup reads the same entries) ----
// A work item is (block, tile pair (ti, tj) with tj <= ti, slice of the block's b range); one workgroup per item.  The tile is
// kSpinRdmBigTile rows for a block above 16 rows, else kSpinRdmSmallTile (one tile, one pair).  Slice s of a block writes the
// entries i >= j of its tile to partials[part_offset + s * d * d + i + j * d]; k_spin_rdm_reduce adds the slices in ascending
// order and writes (i, j) and (j, i) of out[out_offset + ...] from the same value.
struct SpinRdmBlock {
  int32_t k, d, nslices, pad;
  uint32_t nb, pad2;  // C(nB, n_up - k) <= C(31, 15) < 2^32; 2^nB in the full space
  int64_t out_offset, part_offset;
};
struct SpinRdmTable {
  int32_t n_sites, n_up, nA, nB;
  uint32_t mask_a, mask_b;
  uint32_t fallback;  // the state of row 0 of the vector: what a padded lane ranks and loads instead
  int32_t along_a;    // A owns site 0: the rows of a 64-row panel run along the lanes of the gather; else, and in every 16-row panel, the b's do
  int32_t n_blocks, k_first;
  int64_t total, part_total;  // doubles of the packed output and of the partials
  SpinRdmBlock block[kSpinRdmMaxBlocks];
};
struct SpinRdmItem {
  int32_t block, ti, tj, slice;
  uint32_t b_begin, b_end;
};
struct SpinRdmPlan {
  SpinRdmTable table;
  std::vector<SpinRdmItem> big, small;  // the items of the 64-row and of the 16-row kernel
};

inline int spin_rdm_tile(int64_t d) { return d > kSpinRdmSmallTile ? kSpinRdmBigTile : kSpinRdmSmallTile; }
inline int64_t spin_rdm_tile_pairs(int64_t d) {
  const int64_t t = (d + spin_rdm_tile(d) - 1) / spin_rdm_tile(d);
  return t * (t + 1) / 2;
}

// The number of b slices of a block of d rows and nb b's, a pure function of the geometry, the mask (through d, nb and pairs,
// the tile pairs of all blocks) and the state's grid: enough that the items are at least `grid` (a 4 x 4 block from 4e7 rows
// still fills the device), never more than one slice per staged chunk of b's, and never more partials than kSpinRdmSliceBudget
// doubles beyond the first slice (a 3432-row block with 3432 b's takes one slice).  No slice is empty.
inline int spin_rdm_slices(int64_t d, int64_t nb, int64_t pairs, int grid) {
  const int64_t chunk = spin_rdm_tile(d) == kSpinRdmBigTile ? kSpinRdmBigChunk : kSpinRdmSmallChunk;
  int64_t want = ((grid > 1 ? grid : 1) + pairs - 1) / pairs;
  const int64_t by_chunks = (nb + chunk - 1) / chunk, by_budget = kSpinRdmSliceBudget / (d * d) > 1 ? kSpinRdmSliceBudget / (d * d) : 1;
  if (want > by_chunks) want = by_chunks;
  if (want > by_budget) want = by_budget;
  const int64_t per = (nb + want - 1) / want;
  return (int)((nb + per - 1) / per);
}

// the plan of a valid call for a state whose operator kernels run `grid` workgroups
inline void spin_rdm_build_plan(const SpinRdmArgs& a, int grid, SpinRdmPlan& p) {
  SpinRdmLayout l;
  spin_rdm_layout(a, l);
  SpinRdmTable& t = p.table;
  t = SpinRdmTable();
  t.n_sites = a.n_sites, t.n_up = a.n_up, t.nA = l.nA, t.nB = l.nB, t.mask_a = a.mask_a, t.mask_b = l.mask_b;
  t.fallback = a.n_up <= 0 ? 0u : (a.n_up >= 32 ? 0xFFFFFFFFu : (uint32_t(1) << a.n_up) - 1);  // rank 0: the lowest n_up sites up
  t.along_a = (a.mask_a & 1u) ? 1 : 0;
  t.n_blocks = l.n_blocks, t.k_first = l.k_first, t.total = l.offsets[l.n_blocks];
  int64_t pairs = 0;
  for (int n = 0; n < l.n_blocks; ++n) pairs += spin_rdm_tile_pairs(l.dims[n]);
  p.big.clear(), p.small.clear();
  int64_t part = 0;
  for (int n = 0; n < l.n_blocks; ++n) {
    SpinRdmBlock& b = t.block[n];
    const int64_t d = l.dims[n], nb = l.nb[n];
    b.k = l.k_first + n, b.d = (int32_t)d, b.nb = (uint32_t)nb, b.nslices = spin_rdm_slices(d, nb, pairs, grid);
    b.out_offset = l.offsets[n], b.part_offset = part;
    part += (int64_t)b.nslices * d * d;
    const int tile = spin_rdm_tile(d), tiles = (int)((d + tile - 1) / tile);
    const int64_t per = (nb + b.nslices - 1) / b.nslices;
    std::vector<SpinRdmItem>& items = tile == kSpinRdmBigTile ? p.big : p.small;
    for (int ti = 0; ti < tiles; ++ti)
      for (int tj = 0; tj <= ti; ++tj)
        for (int s = 0; s < b.nslices; ++s) {
          const int64_t b0 = s * per, b1 = b0 + per < nb ? b0 + per : nb;
          items.push_back(SpinRdmItem{n, ti, tj, s, (uint32_t)b0, (uint32_t)b1});
        }
  }
  t.part_total = part;
}

}  // namespace eigenex
