// Host code of the reduced density matrix under AddressSanitizer + UBSan (device code cannot be sanitised on the GPU pool):
// csrc/spin_rdm.hpp -- the argument check, the layout, the work table and the host evaluation -- compiled into this program,
// which links nothing else.  Over the shapes of tests/test_gpu_spin_rdm.py and three launch grids (1, 256 and 2048 workgroups:
// no slicing, some, as much as the rule allows) it replays k_spin_rdm<SECTOR, TILE> and k_spin_rdm_reduce (kernels.hip) item by
// item and phase by phase with the kernel's own index functions (csrc/spin_rdm_rows.hpp through csrc/spin_rows.hpp), every
// access checked against its array: the binomials, the staged states, the rank tables, the vector, the panels with their
// pitch, the group sums, the partials and the output.  It checks that every entry i >= j of every slice is written exactly once,
// every output entry exactly once, that a padded lane loads row 0, and that the result equals spin_rdm_host within
// 2 n_b eps (|M| |M|^T): each side is within n_b eps (|M| |M|^T) of the true sum, whatever the grouping.
// Built and run by tests/test_spin_rdm_host.py; prints SPIN RDM OK and exits 0 when every check holds.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
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

struct Replay {
  const SpinRdmTable* tb;
  const CheckedBinomials* bin;
  CheckedTables tab;
  int h;
  std::uint32_t lo_mask;
  const std::vector<double>* x;
  std::vector<double> partials;
  std::vector<int> hits;  // writes per partial
};

// the vector behind spin_rdm_element: a lane that is not live must load row 0
struct WatchedVector {
  const std::vector<double>* x;
  mutable std::uint32_t last;
  double operator()(std::uint32_t i) const {
    last = i;
    return x->at(i);
  }
};

// one workgroup of k_spin_rdm<SECTOR, TILE>: the phases between two barriers are loops over the 256 lanes
template <bool SECTOR, int TILE>
static void replay_item(Replay& R, const SpinRdmItem& it) {
  const int kB = eigenex::kBlock;
  const int CHUNK = TILE == eigenex::kSpinRdmBigTile ? eigenex::kSpinRdmBigChunk : eigenex::kSpinRdmSmallChunk;
  const int GROUPS = TILE == eigenex::kSpinRdmBigTile ? 1 : eigenex::kSpinRdmSmallGroups;
  const int SIDE = TILE / 4, PITCH = TILE + 2, LOADS = TILE * CHUNK / kB;
  EXPECT(SIDE * SIDE * GROUPS == kB && TILE * CHUNK % kB == 0 && CHUNK <= kB);
  const SpinRdmTable& tb = *R.tb;
  EXPECT(it.block >= 0 && it.block < tb.n_blocks);
  const SpinRdmBlock& bk = tb.block[it.block];
  const int d = bk.d, k = bk.k, kb = tb.n_up - k;
  EXPECT(eigenex::spin_rdm_tile(d) == TILE && it.b_begin < it.b_end && it.b_end <= bk.nb && it.tj <= it.ti && it.slice >= 0 && it.slice < bk.nslices);
  const bool along_a = TILE == eigenex::kSpinRdmBigTile && tb.along_a != 0, diagonal = it.ti == it.tj;
  if (GROUPS > 1) EXPECT(diagonal);
  const int i0 = it.ti * TILE, j0 = it.tj * TILE;
  EXPECT(i0 < d && j0 < d);
  const int PANEL = CHUNK * PITCH;
  std::vector<double> panel(static_cast<std::size_t>((GROUPS == 1 ? 2 : 1) * PANEL), NAN);
  const int other = diagonal || GROUPS > 1 ? 0 : PANEL;
  std::vector<double> red(GROUPS > 1 ? static_cast<std::size_t>(GROUPS * TILE * TILE) : 1, NAN);
  std::vector<std::uint32_t> sa_i(TILE), sa_j(TILE), sb(static_cast<std::size_t>(CHUNK));
  const WatchedVector xv{R.x, 0};
  for (int tid = 0; tid < TILE; ++tid) {
    sa_i.at(tid) = eigenex::spin_rdm_party_state<SECTOR>(*R.bin, tb.nA, k, tb.mask_a, static_cast<std::uint32_t>(i0 + tid), i0 + tid < d);
    sa_j.at(tid) = eigenex::spin_rdm_party_state<SECTOR>(*R.bin, tb.nA, k, tb.mask_a, static_cast<std::uint32_t>(j0 + tid), j0 + tid < d);
    if (i0 + tid < d) {  // the shared deposit and unranking against the definition's
      const std::uint32_t w = SECTOR ? eigenex::spin_sector_unrank(tb.nA, k, i0 + tid) : static_cast<std::uint32_t>(i0 + tid);
      EXPECT(sa_i.at(tid) == eigenex::spin_rdm_deposit(w, tb.mask_a) && (sa_i.at(tid) & ~tb.mask_a) == 0);
    }
  }
  std::vector<double> acc(static_cast<std::size_t>(kB) * 16, 0.0);
  for (std::uint32_t b0 = it.b_begin; b0 < it.b_end; b0 += CHUNK) {
    for (int tid = 0; tid < CHUNK; ++tid) {
      const bool live = static_cast<std::uint32_t>(tid) < it.b_end - b0;
      sb.at(tid) = eigenex::spin_rdm_party_state<SECTOR>(*R.bin, tb.nB, kb, tb.mask_b, b0 + tid, live);
      if (live) {
        const std::uint32_t w = SECTOR ? eigenex::spin_sector_unrank(tb.nB, kb, b0 + tid) : b0 + tid;
        EXPECT(sb.at(tid) == eigenex::spin_rdm_deposit(w, tb.mask_b) && (sb.at(tid) & ~tb.mask_b) == 0);
      }
    }
    std::vector<double> va(static_cast<std::size_t>(kB * LOADS)), vb(static_cast<std::size_t>(kB * LOADS));
    for (int tid = 0; tid < kB; ++tid)
      for (int q = 0; q < LOADS; ++q) {
        int row = -1, bj = -1;
        eigenex::spin_rdm_panel_slot(along_a, TILE, CHUNK, q * kB + tid, &row, &bj);
        EXPECT(row >= 0 && row < TILE && bj >= 0 && bj < CHUNK);
        const bool live_b = static_cast<std::uint32_t>(bj) < it.b_end - b0;
        const bool live_i = live_b && i0 + row < d, live_j = live_b && j0 + row < d;
        va.at(tid * LOADS + q) = eigenex::spin_rdm_element<SECTOR>(R.tab, xv, R.h, R.lo_mask, sa_i.at(row), sb.at(bj), live_i, tb.fallback);
        if (!live_i) EXPECT(xv.last == 0 && va.at(tid * LOADS + q) == 0.0);
        if (other != 0) {
          vb.at(tid * LOADS + q) = eigenex::spin_rdm_element<SECTOR>(R.tab, xv, R.h, R.lo_mask, sa_j.at(row), sb.at(bj), live_j, tb.fallback);
          if (!live_j) EXPECT(xv.last == 0 && vb.at(tid * LOADS + q) == 0.0);
        }
      }
    std::fill(panel.begin(), panel.end(), NAN);  // a panel element that is read was written in this chunk
    for (int tid = 0; tid < kB; ++tid)
      for (int q = 0; q < LOADS; ++q) {
        int row, bj;
        eigenex::spin_rdm_panel_slot(along_a, TILE, CHUNK, q * kB + tid, &row, &bj);
        EXPECT(std::isnan(panel.at(bj * PITCH + row)));  // no two lanes store one element
        panel.at(bj * PITCH + row) = va.at(tid * LOADS + q);
        if (other != 0) panel.at(other + bj * PITCH + row) = vb.at(tid * LOADS + q);
      }
    for (int tid = 0; tid < kB; ++tid) {
      const int group = tid / (SIDE * SIDE), tx = tid % SIDE, ty = tid % (SIDE * SIDE) / SIDE;
      for (int bj = group; bj < CHUNK; bj += GROUPS) {
        double a[4], b[4];
        for (int r = 0; r < 4; ++r) a[r] = panel.at(bj * PITCH + 4 * tx + r), b[r] = panel.at(other + bj * PITCH + 4 * ty + r);
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) {
            EXPECT(!std::isnan(a[r]) && !std::isnan(b[c]));
            acc[static_cast<std::size_t>(tid) * 16 + r * 4 + c] = std::fma(a[r], b[c], acc[static_cast<std::size_t>(tid) * 16 + r * 4 + c]);
          }
      }
    }
  }
  const std::int64_t base = bk.part_offset + static_cast<std::int64_t>(it.slice) * d * d;
  const auto put = [&](int i, int j, double v) {
    if (i < d && j < d && i >= j) {
      const std::size_t at = static_cast<std::size_t>(base + i + static_cast<std::int64_t>(j) * d);
      R.partials.at(at) = v;
      ++R.hits.at(at);
    }
  };
  if (GROUPS == 1) {
    for (int tid = 0; tid < kB; ++tid) {
      const int tx = tid % SIDE, ty = tid / SIDE;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) put(i0 + 4 * tx + r, j0 + 4 * ty + c, acc[static_cast<std::size_t>(tid) * 16 + r * 4 + c]);
    }
  } else {
    for (int tid = 0; tid < kB; ++tid) {
      const int group = tid / (SIDE * SIDE), tx = tid % SIDE, ty = tid % (SIDE * SIDE) / SIDE;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) red.at(group * TILE * TILE + (4 * ty + c) * TILE + 4 * tx + r) = acc[static_cast<std::size_t>(tid) * 16 + r * 4 + c];
    }
    for (int tid = 0; tid < kB; ++tid) {
      double sum = 0.0;
      for (int g = 0; g < GROUPS; ++g) sum += red.at(g * TILE * TILE + tid);
      put(i0 + tid % TILE, j0 + tid / TILE, sum);
    }
  }
}

// k_spin_rdm_reduce over every lane of its grid
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
    double sum = 0.0;
    for (int s = 0; s < bk.nslices; ++s) {
      const std::size_t at = static_cast<std::size_t>(bk.part_offset + i + j * d + static_cast<std::int64_t>(s) * d * d);
      EXPECT(R.hits.at(at) == 1);
      sum += R.partials.at(at);
    }
    out.at(static_cast<std::size_t>(bk.out_offset + i + j * d)) = sum;
    ++out_hits.at(static_cast<std::size_t>(bk.out_offset + i + j * d));
    out.at(static_cast<std::size_t>(bk.out_offset + j + i * d)) = sum;
    if (i != j) ++out_hits.at(static_cast<std::size_t>(bk.out_offset + j + i * d));
  }
}

static void check_shape(int L, int n_up, std::uint32_t mask_a, std::mt19937& rng) {
  const bool sector = n_up != -1;
  const SpinRdmArgs a{L, n_up, mask_a};
  EXPECT(eigenex::spin_rdm_error(a) == nullptr);
  eigenex::SpinRdmLayout l;
  eigenex::spin_rdm_layout(a, l);
  const std::int64_t n = sector ? eigenex::spin_sector_dim(L, n_up) : std::int64_t(1) << L;
  std::vector<double> x(static_cast<std::size_t>(n)), ax(x.size());
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  for (std::size_t i = 0; i < x.size(); ++i) x[i] = u(rng), ax[i] = std::fabs(x[i]);
  const std::size_t total = static_cast<std::size_t>(l.offsets[l.n_blocks]);
  std::vector<double> host(total, -1.0), mag(total, -1.0);  // exactly sized: one entry too many is a heap overflow
  eigenex::spin_rdm_host(a, x.data(), host.data());
  eigenex::spin_rdm_host(SpinRdmArgs{L, n_up, mask_a}, ax.data(), mag.data());
  double trace = 0.0, norm2 = 0.0;
  for (int b = 0; b < l.n_blocks; ++b)
    for (std::int64_t i = 0; i < l.dims[b]; ++i) trace += host[static_cast<std::size_t>(l.offsets[b] + i + i * l.dims[b])];
  for (double e : x) norm2 += e * e;
  EXPECT(std::fabs(trace - norm2) <= 1e-12 * norm2);

  std::unique_ptr<eigenex::SpinSectorView> v(new eigenex::SpinSectorView());
  eigenex::SpinSectorTables t;
  if (sector) {
    eigenex::spin_sector_build_view(eigenex::SpinModelArgs{L, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, n_up, *v);
    eigenex::spin_sector_build_tables(L, n_up, t);
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
    Replay R{&tb, &bin, CheckedTables{&t}, sector ? v->h : 0, sector ? v->lo_mask : 0u, &x, std::vector<double>(static_cast<std::size_t>(part), NAN),
             std::vector<int>(static_cast<std::size_t>(part), 0)};
    for (const SpinRdmItem& it : plan.big) sector ? replay_item<true, eigenex::kSpinRdmBigTile>(R, it) : replay_item<false, eigenex::kSpinRdmBigTile>(R, it);
    for (const SpinRdmItem& it : plan.small) sector ? replay_item<true, eigenex::kSpinRdmSmallTile>(R, it) : replay_item<false, eigenex::kSpinRdmSmallTile>(R, it);
    std::vector<double> out(total, NAN);
    std::vector<int> out_hits(total, 0);
    replay_reduce(R, out, out_hits);
    for (std::size_t e = 0; e < total; ++e) EXPECT(out_hits[e] == 1);
    for (int b = 0; b < l.n_blocks; ++b) {
      const std::int64_t d = l.dims[b];
      for (std::int64_t i = 0; i < d; ++i)
        for (std::int64_t j = 0; j < d; ++j) {
          const std::size_t at = static_cast<std::size_t>(l.offsets[b] + i + j * d), mirror = static_cast<std::size_t>(l.offsets[b] + j + i * d);
          EXPECT(std::memcmp(&out[at], &out[mirror], sizeof(double)) == 0 && std::memcmp(&host[at], &host[mirror], sizeof(double)) == 0);
          const long double err = std::fabs(static_cast<long double>(out[at]) - static_cast<long double>(host[at]));
          EXPECT(err <= 2.0L * static_cast<long double>(l.nb[b]) * DBL_EPSILON * static_cast<long double>(mag[at]));
        }
    }
    if (grid == 1) first = out;
    if (plan.big.size() + plan.small.size() == static_cast<std::size_t>(0)) EXPECT(false);
  }
  EXPECT(first.size() == total);
}

static bool refused(const SpinRdmArgs& a, const char* word) {
  const char* why = eigenex::spin_rdm_error(a);
  return why != nullptr && std::strstr(why, word) != nullptr;
}

int main() {
  std::mt19937 rng(23);
  // full space: everything ragged; contiguous and interleaved deposit; exactly one 64-tile; three tile pairs; a 16-tile with
  // 2^15 b's; the top site inside a 64-tile block
  check_shape(3, -1, 0b010u, rng);
  check_shape(6, -1, 0b000111u, rng);
  check_shape(6, -1, 0b101010u, rng);
  check_shape(10, -1, 0b0000111111u, rng);
  check_shape(10, -1, 0b1011011101u, rng);
  check_shape(17, -1, (1u << 16) | 1u, rng);
  check_shape(17, -1, (1u << 16) | 0b10011000110010u, rng);
  // sectors
  check_shape(4, 2, 0b0011u, rng);
  check_shape(6, 0, 0b000101u, rng);
  check_shape(6, 6, 0b000101u, rng);
  check_shape(10, 5, 0b0001111000u, rng);
  check_shape(11, 5, 0b10100100011u, rng);
  check_shape(12, 6, 0b111111100000u, rng);
  check_shape(32, 2, 0xC0000FFFu, rng);
  check_shape(32, 31, 0x80000005u, rng);
  check_shape(20, 10, 0b10000000111100110101u, rng);
  check_shape(20, 10, (1u << 19) | (1u << 3), rng);
  check_shape(14, 7, 0x0FFFu, rng);
  // the slicing rule at the sizes the tests cannot reach: a 4 x 4 block from 2^26 rows fills a grid of 2048; a 3432-row block
  // with 3432 b's takes one slice
  EXPECT(eigenex::spin_rdm_slices(4, std::int64_t(1) << 24, 1, 2048) == 2048);
  EXPECT(eigenex::spin_rdm_slices(3432, 3432, 10000, 2048) == 1 && eigenex::spin_rdm_slices(3432, 3432, 1, 2048) == 1);
  EXPECT(eigenex::spin_rdm_slices(64, 100, 1, 2048) == 4 && eigenex::spin_rdm_slices(16, 1, 1, 2048) == 1);
  // the refusals
  EXPECT(refused(SpinRdmArgs{6, -1, 0u}, "zero") && refused(SpinRdmArgs{6, 3, 0u}, "zero"));
  EXPECT(refused(SpinRdmArgs{6, -1, 1u << 6}, "outside") && refused(SpinRdmArgs{31, 2, 1u << 31}, "outside"));
  EXPECT(refused(SpinRdmArgs{6, -1, 63u}, "leaves no site out") && refused(SpinRdmArgs{32, 2, 0xFFFFFFFFu}, "leaves no site out"));
  EXPECT(refused(SpinRdmArgs{31, -1, 1u}, "n_sites") && refused(SpinRdmArgs{33, 2, 1u}, "n_sites") && refused(SpinRdmArgs{1, -1, 1u}, "n_sites"));
  EXPECT(refused(SpinRdmArgs{6, 7, 1u}, "n_up") && refused(SpinRdmArgs{6, -2, 1u}, "n_up"));
  EXPECT(refused(SpinRdmArgs{14, -1, 0x1FFFu}, "4096") && refused(SpinRdmArgs{16, 8, 0x7FFFu}, "4096"));
  EXPECT(eigenex::spin_rdm_error(SpinRdmArgs{14, -1, 0x0FFFu}) == nullptr && eigenex::spin_rdm_error(SpinRdmArgs{28, 14, 0x3FFFu}) == nullptr);
  EXPECT(eigenex::spin_rdm_error(SpinRdmArgs{32, 2, 0x80000000u}) == nullptr);  // bit 31 is a site of 32
  if (fails) return 1;
  std::printf("SPIN RDM OK\n");
  return 0;
}
