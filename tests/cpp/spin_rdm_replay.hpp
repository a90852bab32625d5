// The replay of k_spin_rdm<SECTOR, TILE, E> and k_spin_rdm_reduce<E> (kernels.hip) that spin_rdm_sanitize.cpp (E = double) and
// spin_rdm_z_sanitize.cpp (E = SpinZ, an interleaved complex vector) run under AddressSanitizer + UBSan, written once like the
// kernels: item by item and phase by phase with the kernel's own index functions, element helpers and panel shape
// (csrc/spin_rdm_rows.hpp: SpinRdmGeometry, through csrc/spin_rows.hpp), every access checked against its array: the binomials,
// the staged states, the rank tables, the vector, the panels with their pitch, the group sums, the partials and the output.  It
// checks that every entry i >= j of every slice is written exactly once, every output entry exactly once, that one gather serves
// an element and that a padded lane loads row 0 and stores +0.0.  Vectors, partials and results are arrays of doubles as in the
// library, sizeof(E) / sizeof(double) of them per element.
#pragma once
#include <cmath>
#include <memory>
#include <random>
#include <vector>

#include "spin_rdm.hpp"
#include "spin_rows_checked.hpp"

using eigenex::SpinRdmArgs;
using eigenex::SpinRdmBlock;
using eigenex::SpinRdmItem;
using eigenex::SpinRdmPlan;
using eigenex::SpinRdmTable;
using eigenex::SpinZ;

static inline bool plus_zero(double v) { return v == 0.0 && !std::signbit(v); }
static inline bool plus_zero(SpinZ v) { return plus_zero(v.re) && plus_zero(v.im); }
static inline bool is_nan(double v) { return std::isnan(v); }
static inline bool is_nan(SpinZ v) { return std::isnan(v.re); }
static inline void fill_nan(std::vector<double>& p) { std::fill(p.begin(), p.end(), NAN); }
static inline void fill_nan(std::vector<SpinZ>& p) { std::fill(p.begin(), p.end(), SpinZ{NAN, NAN}); }

// element i of an array of doubles
static inline void get(const std::vector<double>& p, std::size_t i, double* e) { *e = p.at(i); }
static inline void get(const std::vector<double>& p, std::size_t i, SpinZ* e) { *e = SpinZ{p.at(2 * i), p.at(2 * i + 1)}; }
static inline void set(std::vector<double>& p, std::size_t i, double e) { p.at(i) = e; }
static inline void set(std::vector<double>& p, std::size_t i, SpinZ e) { p.at(2 * i) = e.re, p.at(2 * i + 1) = e.im; }

struct Replay {
  const SpinRdmTable* tb;
  const CheckedBinomials* bin;
  CheckedTables tab;
  int h;
  std::uint32_t lo_mask;
  const std::vector<double>* x;
  std::vector<double> partials;
  std::vector<int> hits;  // writes per partial element
};

// the vector behind spin_rdm_element: one access per element; a lane that is not live must load row 0
template <class E>
struct WatchedVector {
  const std::vector<double>* x;
  mutable std::uint32_t last;
  mutable long loads;
  E operator()(std::uint32_t i) const {
    last = i, ++loads;
    E e;
    get(*x, i, &e);
    return e;
  }
};

// one workgroup of k_spin_rdm<SECTOR, TILE, E>: the phases between two barriers are loops over the 256 lanes
template <bool SECTOR, int TILE, class E>
static void replay_item(Replay& R, const SpinRdmItem& it) {
  typedef eigenex::SpinRdmGeometry<E, TILE> G;
  const int kB = eigenex::kBlock;
  const int CHUNK = G::CHUNK, PANEL = G::PANEL, SIDE = G::SIDE;
  const int GROUPS = TILE == eigenex::kSpinRdmBigTile ? 1 : eigenex::kSpinRdmSmallGroups;
  const int LOADS = TILE * CHUNK / kB;
  EXPECT(SIDE * SIDE * GROUPS == kB && TILE * CHUNK % kB == 0 && CHUNK <= kB && CHUNK % GROUPS == 0);
  const SpinRdmTable& tb = *R.tb;
  EXPECT(it.block >= 0 && it.block < tb.n_blocks);
  const SpinRdmBlock& bk = tb.block[it.block];
  const int d = bk.d, k = bk.k, kb = tb.n_up - k;
  EXPECT(eigenex::spin_rdm_tile(d) == TILE && it.b_begin < it.b_end && it.b_end <= bk.nb && it.tj <= it.ti && it.slice >= 0 && it.slice < bk.nslices);
  const bool along_a = TILE == eigenex::kSpinRdmBigTile && tb.along_a != 0, diagonal = it.ti == it.tj;
  if (GROUPS > 1) EXPECT(diagonal);
  const int i0 = it.ti * TILE, j0 = it.tj * TILE;
  EXPECT(i0 < d && j0 < d);
  std::vector<E> panel(static_cast<std::size_t>((GROUPS == 1 ? 2 : 1) * PANEL));  // the kernel's array: elements
  const int other = diagonal || GROUPS > 1 ? 0 : PANEL;
  std::vector<double> red(GROUPS > 1 ? static_cast<std::size_t>(GROUPS * TILE * TILE) : 1, NAN);
  std::vector<std::uint32_t> sa_i(TILE), sa_j(TILE), sb(static_cast<std::size_t>(CHUNK));
  const WatchedVector<E> xv{R.x, 0, 0};
  for (int tid = 0; tid < TILE; ++tid) {
    sa_i.at(tid) = eigenex::spin_rdm_party_state<SECTOR>(*R.bin, tb.nA, k, tb.mask_a, static_cast<std::uint32_t>(i0 + tid), i0 + tid < d);
    sa_j.at(tid) = eigenex::spin_rdm_party_state<SECTOR>(*R.bin, tb.nA, k, tb.mask_a, static_cast<std::uint32_t>(j0 + tid), j0 + tid < d);
    if (i0 + tid < d) {  // the shared deposit and unranking against the definition's
      const std::uint32_t w = SECTOR ? eigenex::spin_sector_unrank(tb.nA, k, i0 + tid) : static_cast<std::uint32_t>(i0 + tid);
      EXPECT(sa_i.at(tid) == eigenex::spin_rdm_deposit(w, tb.mask_a) && (sa_i.at(tid) & ~tb.mask_a) == 0);
    }
  }
  // a lane's four rows: every row of the tile belongs to exactly one (position, r)
  std::vector<int> owner(TILE, 0);
  for (int t = 0; t < SIDE; ++t)
    for (int r = 0; r < 4; ++r) {
      const int row = G::lane_row(t, r);
      EXPECT(row >= 0 && row < TILE);
      ++owner.at(row);
    }
  for (int row = 0; row < TILE; ++row) EXPECT(owner.at(row) == 1);
  std::vector<double> re(static_cast<std::size_t>(kB) * 16, 0.0), im(static_cast<std::size_t>(kB) * 16, 0.0);
  for (std::uint32_t b0 = it.b_begin; b0 < it.b_end; b0 += CHUNK) {
    for (int tid = 0; tid < CHUNK; ++tid) {
      const bool live = static_cast<std::uint32_t>(tid) < it.b_end - b0;
      sb.at(tid) = eigenex::spin_rdm_party_state<SECTOR>(*R.bin, tb.nB, kb, tb.mask_b, b0 + tid, live);
      if (live) {
        const std::uint32_t w = SECTOR ? eigenex::spin_sector_unrank(tb.nB, kb, b0 + tid) : b0 + tid;
        EXPECT(sb.at(tid) == eigenex::spin_rdm_deposit(w, tb.mask_b) && (sb.at(tid) & ~tb.mask_b) == 0);
      }
    }
    std::vector<E> va(static_cast<std::size_t>(kB * LOADS)), vb(static_cast<std::size_t>(kB * LOADS));
    for (int tid = 0; tid < kB; ++tid)
      for (int q = 0; q < LOADS; ++q) {
        int row = -1, bj = -1;
        eigenex::spin_rdm_panel_slot(along_a, TILE, CHUNK, q * kB + tid, &row, &bj);
        EXPECT(row >= 0 && row < TILE && bj >= 0 && bj < CHUNK);
        const bool live_b = static_cast<std::uint32_t>(bj) < it.b_end - b0;
        const bool live_i = live_b && i0 + row < d, live_j = live_b && j0 + row < d;
        const long before = xv.loads;
        va.at(tid * LOADS + q) = eigenex::spin_rdm_element<SECTOR>(R.tab, xv, R.h, R.lo_mask, sa_i.at(row), sb.at(bj), live_i, tb.fallback);
        EXPECT(xv.loads == before + 1);  // one gather serves an element, both parts of a complex one
        if (!live_i) EXPECT(xv.last == 0 && plus_zero(va.at(tid * LOADS + q)));
        if (other != 0) {
          vb.at(tid * LOADS + q) = eigenex::spin_rdm_element<SECTOR>(R.tab, xv, R.h, R.lo_mask, sa_j.at(row), sb.at(bj), live_j, tb.fallback);
          if (!live_j) EXPECT(xv.last == 0 && plus_zero(vb.at(tid * LOADS + q)));
        }
      }
    fill_nan(panel);  // a panel element that is read was written in this chunk
    for (int tid = 0; tid < kB; ++tid)
      for (int q = 0; q < LOADS; ++q) {
        int row, bj;
        eigenex::spin_rdm_panel_slot(along_a, TILE, CHUNK, q * kB + tid, &row, &bj);
        const int at = G::panel_column(bj) + row;
        EXPECT(at >= 0 && at < PANEL);     // inside this panel, not merely inside the array of two
        EXPECT(is_nan(panel.at(at)));      // no two lanes store one element
        panel.at(at) = va.at(tid * LOADS + q);
        if (other != 0) panel.at(other + at) = vb.at(tid * LOADS + q);
      }
    for (int tid = 0; tid < kB; ++tid) {
      const int group = tid / (SIDE * SIDE), tx = tid % SIDE, ty = tid % (SIDE * SIDE) / SIDE;
      for (int bj = group; bj < CHUNK; bj += GROUPS) {
        E a[4], b[4];
        for (int r = 0; r < 4; ++r) {
          const int ia = G::panel_column(bj) + G::lane_row(tx, r), ib = G::panel_column(bj) + G::lane_row(ty, r);
          EXPECT(ia >= 0 && ia < PANEL && ib >= 0 && ib < PANEL);
          a[r] = panel.at(ia), b[r] = panel.at(other + ib);
        }
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) {
            EXPECT(!is_nan(a[r]) && !is_nan(b[c]));
            const std::size_t at = static_cast<std::size_t>(tid) * 16 + r * 4 + c;
            eigenex::spin_rdm_fma(a[r], b[c], re[at], im[at]);
          }
      }
    }
  }
  const std::int64_t base = bk.part_offset + static_cast<std::int64_t>(it.slice) * d * d;
  const auto put = [&](int i, int j, double vr, double vi) {
    if (i < d && j < d && i >= j) {
      const std::size_t at = static_cast<std::size_t>(base + i + static_cast<std::int64_t>(j) * d);
      set(R.partials, at, eigenex::spin_rdm_entry<E>(vr, vi, i == j));
      ++R.hits.at(at);
    }
  };
  if (GROUPS == 1) {
    for (int tid = 0; tid < kB; ++tid) {
      const int tx = tid % SIDE, ty = tid / SIDE;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
          const std::size_t at = static_cast<std::size_t>(tid) * 16 + r * 4 + c;
          put(i0 + G::lane_row(tx, r), j0 + G::lane_row(ty, c), re[at], im[at]);
        }
    }
  } else {
    // the groups' tiles through red[]: the real parts and, of a complex vector, then the imaginary ones
    std::vector<double> sums(static_cast<std::size_t>(2 * kB), 0.0);
    for (int part = 0; part < static_cast<int>(sizeof(E) / sizeof(double)); ++part) {
      const std::vector<double>& acc = part == 0 ? re : im;
      std::fill(red.begin(), red.end(), NAN);
      for (int tid = 0; tid < kB; ++tid) {
        const int group = tid / (SIDE * SIDE), tx = tid % SIDE, ty = tid % (SIDE * SIDE) / SIDE;
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) {
            const std::size_t at = static_cast<std::size_t>(group * TILE * TILE + G::lane_row(ty, c) * TILE + G::lane_row(tx, r));
            EXPECT(std::isnan(red.at(at)));
            red.at(at) = acc[static_cast<std::size_t>(tid) * 16 + r * 4 + c];
          }
      }
      for (int tid = 0; tid < kB; ++tid) {
        double sum = 0.0;
        for (int g = 0; g < GROUPS; ++g) sum += red.at(g * TILE * TILE + tid);
        sums.at(static_cast<std::size_t>(2 * tid + part)) = sum;
      }
    }
    for (int tid = 0; tid < kB; ++tid) put(i0 + tid % TILE, j0 + tid / TILE, sums.at(2 * tid), sums.at(2 * tid + 1));
  }
}

// what the lane of entry (i, j), i >= j, of k_spin_rdm_reduce<E> writes: `lower` is (i, j), `upper` (j, i)
static inline void write_entry(double sum, bool diagonal, std::size_t lower, std::size_t upper, std::vector<double>& out, std::vector<int>& out_hits) {
  out.at(lower) = sum;
  ++out_hits.at(lower);
  out.at(upper) = sum;
  if (!diagonal) ++out_hits.at(upper);
}
static inline void write_entry(SpinZ sum, bool diagonal, std::size_t lower, std::size_t upper, std::vector<double>& out, std::vector<int>& out_hits) {
  if (diagonal) {
    set(out, lower, SpinZ{sum.re, 0.0});
    ++out_hits.at(lower);
  } else {
    set(out, lower, sum);
    set(out, upper, SpinZ{sum.re, -sum.im});
    ++out_hits.at(lower), ++out_hits.at(upper);
  }
}

// k_spin_rdm_reduce<E> over every lane of its grid; out_hits counts elements
template <class E>
static void replay_reduce(const Replay& R, std::vector<double>& out, std::vector<int>& out_hits) {
  const SpinRdmTable& tb = *R.tb;
  const std::int64_t lanes = (tb.total + eigenex::kBlock - 1) / eigenex::kBlock * eigenex::kBlock;
  for (std::int64_t e = 0; e < lanes; ++e) {
    if (e >= tb.total) continue;
    int n = 0;
    while (n + 1 < tb.n_blocks && e >= tb.block[n + 1].out_offset) ++n;
    const SpinRdmBlock& bk = tb.block[n];
    const std::int64_t d = bk.d, local = e - bk.out_offset, i = local % d, j = local / d;
    EXPECT(local >= 0 && j < d);
    if (i < j) continue;
    E sum = E{};
    for (int s = 0; s < bk.nslices; ++s) {
      const std::size_t at = static_cast<std::size_t>(bk.part_offset + i + j * d + static_cast<std::int64_t>(s) * d * d);
      EXPECT(R.hits.at(at) == 1);
      E p;
      get(R.partials, at, &p);
      sum = eigenex::spin_sum(sum, p);
    }
    write_entry(sum, i == j, static_cast<std::size_t>(bk.out_offset + i + j * d), static_cast<std::size_t>(bk.out_offset + j + i * d), out, out_hits);
  }
}

// The vector x of elements E over the geometry of `a`, replayed on three launch grids (1, 256 and 2048 workgroups: no slicing,
// some, as much as the rule allows) with the real call's plan, which both elements take; compare(out) sees each packed result.
template <class E, class Compare>
static void replay_grids(const SpinRdmArgs& a, const eigenex::SpinRdmLayout& l, const std::vector<double>& x, const Compare& compare) {
  const bool sector = a.n_up != -1;
  const std::size_t es = sizeof(E) / sizeof(double), total = static_cast<std::size_t>(l.offsets[l.n_blocks]);
  std::unique_ptr<eigenex::SpinSectorView> v(new eigenex::SpinSectorView());
  eigenex::SpinSectorTables t;
  if (sector) {
    eigenex::spin_sector_build_view(eigenex::SpinModelArgs{a.n_sites, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, a.n_up, *v);
    eigenex::spin_sector_build_tables(a.n_sites, a.n_up, t);
  }
  const CheckedBinomials bin(*v);
  std::vector<double> first;
  for (int grid : {1, 256, 2048}) {
    SpinRdmPlan plan;
    eigenex::spin_rdm_build_plan(a, grid, plan);
    const SpinRdmTable& tb = plan.table;
    EXPECT(tb.total == static_cast<std::int64_t>(total) && tb.n_blocks == l.n_blocks);
    std::int64_t part = 0, bound = 0;
    for (int b = 0; b < tb.n_blocks; ++b) {
      const SpinRdmBlock& bk = tb.block[b];
      EXPECT(bk.part_offset == part && bk.nslices >= 1 && bk.d == l.dims[b] && bk.nb == l.nb[b]);
      EXPECT(bk.nslices == 1 || static_cast<std::int64_t>(bk.nslices) * bk.d * bk.d <= eigenex::kSpinRdmSliceBudget);
      part += static_cast<std::int64_t>(bk.nslices) * bk.d * bk.d;
      bound += static_cast<std::int64_t>(bk.d) * bk.d + eigenex::kSpinRdmSliceBudget;
    }
    EXPECT(tb.part_total == part && part <= bound);
    Replay R{&tb, &bin, CheckedTables{&t}, sector ? v->h : 0, sector ? v->lo_mask : 0u, &x, std::vector<double>(es * static_cast<std::size_t>(part), NAN),
             std::vector<int>(static_cast<std::size_t>(part), 0)};
    for (const SpinRdmItem& it : plan.big) sector ? replay_item<true, eigenex::kSpinRdmBigTile, E>(R, it) : replay_item<false, eigenex::kSpinRdmBigTile, E>(R, it);
    for (const SpinRdmItem& it : plan.small) sector ? replay_item<true, eigenex::kSpinRdmSmallTile, E>(R, it) : replay_item<false, eigenex::kSpinRdmSmallTile, E>(R, it);
    EXPECT(plan.big.size() + plan.small.size() > 0);
    std::vector<double> out(es * total, NAN);
    std::vector<int> out_hits(total, 0);
    replay_reduce<E>(R, out, out_hits);
    for (std::size_t e = 0; e < total; ++e) EXPECT(out_hits[e] == 1);
    compare(out);
    if (grid == 1) first = out;
  }
  EXPECT(first.size() == es * total);
}

// the shapes both programs replay.  Full space: everything ragged; contiguous and interleaved deposit; exactly one 64-tile; three
// tile pairs; a 16-tile with 2^15 b's; the top site inside a 64-tile block.  Then sectors.
template <class Check>
static void for_every_shape(const Check& check_shape) {
  check_shape(3, -1, 0b010u);
  check_shape(6, -1, 0b000111u);
  check_shape(6, -1, 0b101010u);
  check_shape(10, -1, 0b0000111111u);
  check_shape(10, -1, 0b1011011101u);
  check_shape(17, -1, (1u << 16) | 1u);
  check_shape(17, -1, (1u << 16) | 0b10011000110010u);
  check_shape(4, 2, 0b0011u);
  check_shape(6, 0, 0b000101u);
  check_shape(6, 6, 0b000101u);
  check_shape(10, 5, 0b0001111000u);
  check_shape(11, 5, 0b10100100011u);
  check_shape(12, 6, 0b111111100000u);
  check_shape(32, 2, 0xC0000FFFu);
  check_shape(32, 31, 0x80000005u);
  check_shape(20, 10, 0b10000000111100110101u);
  check_shape(20, 10, (1u << 19) | (1u << 3));
  check_shape(14, 7, 0x0FFFu);
}
