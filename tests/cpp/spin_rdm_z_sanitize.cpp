// Host code of the reduced density matrix of a COMPLEX vector under AddressSanitizer + UBSan (device code cannot be sanitised
// on the GPU pool): csrc/spin_rdm.hpp -- the argument check, the layout, the work table and spin_rdm_host_z -- compiled into this
// program, which links nothing else.  Over the shapes of tests/test_gpu_spin_rdm_z.py and three launch grids (1, 256 and 2048
// workgroups: no slicing, some, as much as the rule allows) it replays k_spin_rdm_z<SECTOR, TILE> and k_spin_rdm_reduce_z
// (kernels.hip) item by item and phase by phase with the kernel's own index functions (csrc/spin_rdm_rows.hpp through
// csrc/spin_rows.hpp), every access checked against its array: the binomials, the staged states, the rank tables, the interleaved
// vector, the panels of CHUNK x (TILE + 1) pairs, the group sums, the partials and the output.  It checks that every entry i >= j
// of every slice is written exactly once, every output entry exactly once, that a padded lane loads row 0, that the diagonal's
// imaginary part is +0.0 and (j, i) the conjugate of (i, j) bit for bit, and that the result equals spin_rdm_host_z within twice
// the bound 2 n_b eps (|Mr||Mr|^T + |Mi||Mi|^T) resp. 2 n_b eps (|Mi||Mr|^T + |Mr||Mi|^T): each side is within that bound of the
// true sum of 2 n_b products, whatever the grouping.  The plan is spin_rdm_build_plan's, the real call's.
// Built and run by tests/test_spin_rdm_z_host.py; prints SPIN RDM Z OK and exits 0 when every check holds.
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
using eigenex::SpinZ;

struct Replay {
  const SpinRdmTable* tb;
  const CheckedBinomials* bin;
  CheckedTables tab;
  int h;
  std::uint32_t lo_mask;
  const std::vector<double>* x;   // interleaved
  std::vector<double> partials;   // interleaved pairs
  std::vector<int> hits;          // writes per partial pair
};

// the interleaved vector behind spin_rdm_element_z: one access per element; a lane that is not live must load row 0
struct WatchedVectorZ {
  const std::vector<double>* x;
  mutable std::uint32_t last;
  mutable long loads;
  SpinZ operator()(std::uint32_t i) const {
    last = i, ++loads;
    return SpinZ{x->at(2 * static_cast<std::size_t>(i)), x->at(2 * static_cast<std::size_t>(i) + 1)};
  }
};

static bool plus_zero(double v) { return v == 0.0 && !std::signbit(v); }

// one workgroup of k_spin_rdm_z<SECTOR, TILE>: the phases between two barriers are loops over the 256 lanes
template <bool SECTOR, int TILE>
static void replay_item(Replay& R, const SpinRdmItem& it) {
  const int kB = eigenex::kBlock;
  const int CHUNK = TILE == eigenex::kSpinRdmBigTile ? eigenex::kSpinRdmBigChunkZ : eigenex::kSpinRdmSmallChunkZ;
  const int GROUPS = TILE == eigenex::kSpinRdmBigTile ? 1 : eigenex::kSpinRdmSmallGroups;
  const int SIDE = TILE / 4, LOADS = TILE * CHUNK / kB;
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
  const int PANEL = CHUNK * (TILE + 1);  // the kernel's array: pairs
  std::vector<SpinZ> panel(static_cast<std::size_t>((GROUPS == 1 ? 2 : 1) * PANEL), SpinZ{NAN, NAN});
  const int other = diagonal || GROUPS > 1 ? 0 : PANEL;
  std::vector<double> red(GROUPS > 1 ? static_cast<std::size_t>(GROUPS * TILE * TILE) : 1, NAN);
  std::vector<std::uint32_t> sa_i(TILE), sa_j(TILE), sb(static_cast<std::size_t>(CHUNK));
  const WatchedVectorZ xv{R.x, 0, 0};
  for (int tid = 0; tid < TILE; ++tid) {
    sa_i.at(tid) = eigenex::spin_rdm_party_state<SECTOR>(*R.bin, tb.nA, k, tb.mask_a, static_cast<std::uint32_t>(i0 + tid), i0 + tid < d);
    sa_j.at(tid) = eigenex::spin_rdm_party_state<SECTOR>(*R.bin, tb.nA, k, tb.mask_a, static_cast<std::uint32_t>(j0 + tid), j0 + tid < d);
    if (i0 + tid < d) {
      const std::uint32_t w = SECTOR ? eigenex::spin_sector_unrank(tb.nA, k, i0 + tid) : static_cast<std::uint32_t>(i0 + tid);
      EXPECT(sa_i.at(tid) == eigenex::spin_rdm_deposit(w, tb.mask_a) && (sa_i.at(tid) & ~tb.mask_a) == 0);
    }
  }
  // a lane's four rows: every row of the tile belongs to exactly one (position, r)
  std::vector<int> owner(TILE, 0);
  for (int t = 0; t < SIDE; ++t)
    for (int r = 0; r < 4; ++r) {
      const int row = eigenex::spin_rdm_lane_row_z(SIDE, t, r);
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
    std::vector<SpinZ> va(static_cast<std::size_t>(kB * LOADS)), vb(static_cast<std::size_t>(kB * LOADS));
    for (int tid = 0; tid < kB; ++tid)
      for (int q = 0; q < LOADS; ++q) {
        int row = -1, bj = -1;
        eigenex::spin_rdm_panel_slot(along_a, TILE, CHUNK, q * kB + tid, &row, &bj);
        EXPECT(row >= 0 && row < TILE && bj >= 0 && bj < CHUNK);
        const bool live_b = static_cast<std::uint32_t>(bj) < it.b_end - b0;
        const bool live_i = live_b && i0 + row < d, live_j = live_b && j0 + row < d;
        const long before = xv.loads;
        va.at(tid * LOADS + q) = eigenex::spin_rdm_element_z<SECTOR>(R.tab, xv, R.h, R.lo_mask, sa_i.at(row), sb.at(bj), live_i, tb.fallback);
        EXPECT(xv.loads == before + 1);  // one gather serves both parts
        if (!live_i) EXPECT(xv.last == 0 && plus_zero(va.at(tid * LOADS + q).re) && plus_zero(va.at(tid * LOADS + q).im));
        if (other != 0) {
          vb.at(tid * LOADS + q) = eigenex::spin_rdm_element_z<SECTOR>(R.tab, xv, R.h, R.lo_mask, sa_j.at(row), sb.at(bj), live_j, tb.fallback);
          if (!live_j) EXPECT(xv.last == 0 && plus_zero(vb.at(tid * LOADS + q).re) && plus_zero(vb.at(tid * LOADS + q).im));
        }
      }
    std::fill(panel.begin(), panel.end(), SpinZ{NAN, NAN});  // a panel element that is read was written in this chunk
    for (int tid = 0; tid < kB; ++tid)
      for (int q = 0; q < LOADS; ++q) {
        int row, bj;
        eigenex::spin_rdm_panel_slot(along_a, TILE, CHUNK, q * kB + tid, &row, &bj);
        const int at = eigenex::spin_rdm_panel_index_z(TILE, bj, row);
        EXPECT(at >= 0 && at < PANEL);  // inside this panel, not merely inside the array of two
        EXPECT(std::isnan(panel.at(at).re));  // no two lanes store one element
        panel.at(at) = va.at(tid * LOADS + q);
        if (other != 0) panel.at(other + at) = vb.at(tid * LOADS + q);
      }
    for (int tid = 0; tid < kB; ++tid) {
      const int group = tid / (SIDE * SIDE), tx = tid % SIDE, ty = tid % (SIDE * SIDE) / SIDE;
      for (int bj = group; bj < CHUNK; bj += GROUPS) {
        SpinZ a[4], b[4];
        for (int r = 0; r < 4; ++r) {
          const int ia = eigenex::spin_rdm_panel_index_z(TILE, bj, eigenex::spin_rdm_lane_row_z(SIDE, tx, r));
          const int ib = eigenex::spin_rdm_panel_index_z(TILE, bj, eigenex::spin_rdm_lane_row_z(SIDE, ty, r));
          EXPECT(ia >= 0 && ia < PANEL && ib >= 0 && ib < PANEL);
          a[r] = panel.at(ia), b[r] = panel.at(other + ib);
        }
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) {
            EXPECT(!std::isnan(a[r].re) && !std::isnan(b[c].re));
            const std::size_t at = static_cast<std::size_t>(tid) * 16 + r * 4 + c;
            re[at] = std::fma(a[r].re, b[c].re, re[at]);
            re[at] = std::fma(a[r].im, b[c].im, re[at]);
            im[at] = std::fma(a[r].im, b[c].re, im[at]);
            im[at] = std::fma(-a[r].re, b[c].im, im[at]);
          }
      }
    }
  }
  const std::int64_t base = bk.part_offset + static_cast<std::int64_t>(it.slice) * d * d;
  const auto put = [&](int i, int j, double vr, double vi) {
    if (i < d && j < d && i >= j) {
      const std::size_t at = static_cast<std::size_t>(base + i + static_cast<std::int64_t>(j) * d);
      R.partials.at(2 * at) = vr, R.partials.at(2 * at + 1) = i == j ? 0.0 : vi;
      ++R.hits.at(at);
    }
  };
  if (GROUPS == 1) {
    for (int tid = 0; tid < kB; ++tid) {
      const int tx = tid % SIDE, ty = tid / SIDE;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
          put(i0 + eigenex::spin_rdm_lane_row_z(SIDE, tx, r), j0 + eigenex::spin_rdm_lane_row_z(SIDE, ty, c), re[static_cast<std::size_t>(tid) * 16 + r * 4 + c],
              im[static_cast<std::size_t>(tid) * 16 + r * 4 + c]);
    }
  } else {
    // the groups' tiles through red[], the real parts, then the imaginary ones
    std::vector<double> sums(static_cast<std::size_t>(2 * kB), NAN);
    for (int part = 0; part < 2; ++part) {
      const std::vector<double>& acc = part == 0 ? re : im;
      std::fill(red.begin(), red.end(), NAN);
      for (int tid = 0; tid < kB; ++tid) {
        const int group = tid / (SIDE * SIDE), tx = tid % SIDE, ty = tid % (SIDE * SIDE) / SIDE;
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) {
            const std::size_t at = static_cast<std::size_t>(group * TILE * TILE + eigenex::spin_rdm_lane_row_z(SIDE, ty, c) * TILE + eigenex::spin_rdm_lane_row_z(SIDE, tx, r));
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

// k_spin_rdm_reduce_z over every lane of its grid; out and out_hits count pairs
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
    double sr = 0.0, si = 0.0;
    for (int s = 0; s < bk.nslices; ++s) {
      const std::size_t at = static_cast<std::size_t>(bk.part_offset + i + j * d + static_cast<std::int64_t>(s) * d * d);
      EXPECT(R.hits.at(at) == 1);
      sr += R.partials.at(2 * at), si += R.partials.at(2 * at + 1);
    }
    const std::size_t lower = static_cast<std::size_t>(bk.out_offset + i + j * d), upper = static_cast<std::size_t>(bk.out_offset + j + i * d);
    if (i == j) {
      out.at(2 * lower) = sr, out.at(2 * lower + 1) = 0.0;
      ++out_hits.at(lower);
    } else {
      out.at(2 * lower) = sr, out.at(2 * lower + 1) = si;
      out.at(2 * upper) = sr, out.at(2 * upper + 1) = -si;
      ++out_hits.at(lower), ++out_hits.at(upper);
    }
  }
}

static void check_shape(int L, int n_up, std::uint32_t mask_a, std::mt19937& rng) {
  const bool sector = n_up != -1;
  const SpinRdmArgs a{L, n_up, mask_a};
  EXPECT(eigenex::spin_rdm_error(a) == nullptr);
  eigenex::SpinRdmLayout l;
  eigenex::spin_rdm_layout(a, l);
  const std::int64_t n = sector ? eigenex::spin_sector_dim(L, n_up) : std::int64_t(1) << L;
  std::vector<double> x(static_cast<std::size_t>(2 * n)), ax(x.size());
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  for (std::size_t i = 0; i < x.size(); ++i) x[i] = u(rng), ax[i] = std::fabs(x[i]);
  // the magnitudes of the bound from the real definition on a = |Re x|, b = |Im x| and a + b:
  // |Mr||Mr|^T, |Mi||Mi|^T, and (|Mr| + |Mi|)(|Mr| + |Mi|)^T minus the two = |Mr||Mi|^T + |Mi||Mr|^T
  std::vector<double> ar(static_cast<std::size_t>(n)), ai(ar.size()), sum(ar.size());
  for (std::size_t r = 0; r < ar.size(); ++r) ar[r] = ax[2 * r], ai[r] = ax[2 * r + 1], sum[r] = ar[r] + ai[r];
  const std::size_t total = static_cast<std::size_t>(l.offsets[l.n_blocks]);
  std::vector<double> host(2 * total, -1.0);  // exactly sized: one entry too many is a heap overflow
  std::vector<double> mag_rr(total, -1.0), mag_ii(total, -1.0), mag_ss(total, -1.0);
  eigenex::spin_rdm_host_z(a, x.data(), host.data());
  eigenex::spin_rdm_host(a, ar.data(), mag_rr.data());
  eigenex::spin_rdm_host(a, ai.data(), mag_ii.data());
  eigenex::spin_rdm_host(a, sum.data(), mag_ss.data());
  double trace = 0.0, norm2 = 0.0;
  for (int b = 0; b < l.n_blocks; ++b)
    for (std::int64_t i = 0; i < l.dims[b]; ++i) trace += host[2 * static_cast<std::size_t>(l.offsets[b] + i + i * l.dims[b])];
  for (double e : x) norm2 += e * e;
  EXPECT(std::fabs(trace - norm2) <= 1e-12 * norm2);

  std::unique_ptr<eigenex::SpinSectorView> v(new eigenex::SpinSectorView());
  eigenex::SpinSectorTables t;
  if (sector) {
    eigenex::spin_sector_build_view(eigenex::SpinModelArgs{L, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, n_up, *v);
    eigenex::spin_sector_build_tables(L, n_up, t);
  }
  const CheckedBinomials bin(*v);
  for (int grid : {1, 256, 2048}) {
    SpinRdmPlan plan;
    eigenex::spin_rdm_build_plan(a, grid, plan);
    const SpinRdmTable& tb = plan.table;
    EXPECT(tb.total == static_cast<std::int64_t>(total) && tb.n_blocks == l.n_blocks);
    const std::int64_t part = tb.part_total;
    Replay R{&tb, &bin, CheckedTables{&t}, sector ? v->h : 0, sector ? v->lo_mask : 0u, &x, std::vector<double>(static_cast<std::size_t>(2 * part), NAN),
             std::vector<int>(static_cast<std::size_t>(part), 0)};
    for (const SpinRdmItem& it : plan.big) sector ? replay_item<true, eigenex::kSpinRdmBigTile>(R, it) : replay_item<false, eigenex::kSpinRdmBigTile>(R, it);
    for (const SpinRdmItem& it : plan.small) sector ? replay_item<true, eigenex::kSpinRdmSmallTile>(R, it) : replay_item<false, eigenex::kSpinRdmSmallTile>(R, it);
    EXPECT(plan.big.size() + plan.small.size() > 0);
    std::vector<double> out(2 * total, NAN);
    std::vector<int> out_hits(total, 0);
    replay_reduce(R, out, out_hits);
    for (std::size_t e = 0; e < total; ++e) EXPECT(out_hits[e] == 1);
    for (int b = 0; b < l.n_blocks; ++b) {
      const std::int64_t d = l.dims[b];
      for (std::int64_t i = 0; i < d; ++i)
        for (std::int64_t j = 0; j < d; ++j) {
          const std::size_t at = static_cast<std::size_t>(l.offsets[b] + i + j * d), mirror = static_cast<std::size_t>(l.offsets[b] + j + i * d);
          for (const std::vector<double>* m : {&out, &host}) {
            const double neg = -(*m)[2 * mirror + 1];
            EXPECT(std::memcmp(&(*m)[2 * at], &(*m)[2 * mirror], sizeof(double)) == 0);
            if (i == j) EXPECT(plus_zero((*m)[2 * at + 1]));
            else EXPECT(std::memcmp(&(*m)[2 * at + 1], &neg, sizeof(double)) == 0);
          }
          const long double nb2 = 2.0L * static_cast<long double>(l.nb[b]) * DBL_EPSILON;
          const long double bound_re = nb2 * (static_cast<long double>(mag_rr[at]) + static_cast<long double>(mag_ii[at]));
          // the difference of three rounded sums of non-negative terms (each within n_b eps of its value): their rounding is added
          const long double cross = static_cast<long double>(mag_ss[at]) - static_cast<long double>(mag_rr[at]) - static_cast<long double>(mag_ii[at]);
          const long double bound_im = nb2 * (cross + static_cast<long double>(l.nb[b]) * DBL_EPSILON * 3.0L * static_cast<long double>(mag_ss[at]));
          const long double err_re = std::fabs(static_cast<long double>(out[2 * at]) - static_cast<long double>(host[2 * at]));
          const long double err_im = std::fabs(static_cast<long double>(out[2 * at + 1]) - static_cast<long double>(host[2 * at + 1]));
          EXPECT(err_re <= 2.0L * bound_re);
          EXPECT(err_im <= 2.0L * bound_im);
        }
    }
  }
}

int main() {
  std::mt19937 rng(29);
  // the shapes of tests/cpp/spin_rdm_sanitize.cpp, for the same reasons
  check_shape(3, -1, 0b010u, rng);
  check_shape(6, -1, 0b000111u, rng);
  check_shape(6, -1, 0b101010u, rng);
  check_shape(10, -1, 0b0000111111u, rng);
  check_shape(10, -1, 0b1011011101u, rng);
  check_shape(17, -1, (1u << 16) | 1u, rng);
  check_shape(17, -1, (1u << 16) | 0b10011000110010u, rng);
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
  if (fails) return 1;
  std::printf("SPIN RDM Z OK\n");
  return 0;
}
