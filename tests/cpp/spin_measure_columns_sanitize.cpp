// Host code of the columns measurement under AddressSanitizer + UBSan (device code cannot be sanitised on the GPU pool):
// csrc/spin_measure_columns.hpp -- the range check and the host evaluation -- compiled into this program, which links nothing
// else.  For the full space (L = 3, 6, 9) and the sectors (4,2), (6,0), (6,6), (11,5), (31,2), (32,2), (32,31), with the term lists
// of spin_measure_sanitize.cpp and 1, 3, 4, 5 and 9 columns of exactly the rows' length: the outputs go into exactly-sized arrays,
// and the row loop of k_spin_measure_columns<SECTOR> runs over its chunk tables and column chunks as the library launches them --
// the kernel's own function (csrc/spin_rows.hpp: spin_measure_columns_row), every load checked against its array: the lane's
// state from the binomials, the column elements (a column beyond the live ones is the last live one), the gather through hi_base
// and lo_rank, the own element where the entry is absent.  Taken over ascending rows it adds the same fma chain as the host
// evaluation (a row without the entry adds V_j(s) * 0), so the two are compared bit for bit.
// Built and run by tests/test_spin_measure_columns_host.py; prints SPIN MEASURE COLUMNS OK and exits 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "spin_measure_columns.hpp"
#include "spin_rows_checked.hpp"

using eigenex::SpinMeasureArgs;
using eigenex::SpinMeasureChunk;

struct Lists {
  std::vector<std::uint32_t> diag, flip;
};

static Lists lists_of(int L, bool sector) {
  Lists l;
  std::vector<std::uint32_t> pairs;
  for (int i = 0; i < L; ++i) l.diag.push_back(std::uint32_t(1) << i);
  for (int i = 0; i < L; ++i)
    for (int j = i + 1; j < L; ++j) pairs.push_back((std::uint32_t(1) << i) | (std::uint32_t(1) << j));
  l.diag.insert(l.diag.end(), pairs.begin(), pairs.end());
  l.diag.push_back((std::uint32_t(1) << 0) | (std::uint32_t(1) << (L / 3)) | (std::uint32_t(1) << (2 * L / 3)) | (std::uint32_t(1) << (L - 1)));
  l.diag.push_back(L == 32 ? 0xFFFFFFFFu : (std::uint32_t(1) << L) - 1);
  l.diag.push_back(pairs[0]);
  l.flip = pairs;
  l.flip.push_back(pairs[0]);
  if (!sector)
    for (int i = 0; i < L; ++i) l.flip.push_back(std::uint32_t(1) << i);
  return l;
}

// k_spin_measure_columns (kernels.hip) over ascending rows, by the kernel's own function: one chunk of terms and one chunk of
// columns per pass, as eigenex_spin_measure_columns launches them; V holds `count` columns of exactly n rows
static void replay(const SpinMeasureArgs& a, const std::vector<double>& x, const std::vector<double>& V, int count, std::vector<double>& diag,
                   std::vector<double>& flip) {
  const int C = eigenex::kSpinMeasureChunk, J = eigenex::kSpinMeasureColumns;
  const bool sector = a.n_up != -1;
  const std::int64_t n = eigenex::spin_measure_rows(a);
  EXPECT(static_cast<std::int64_t>(x.size()) == n && static_cast<std::int64_t>(V.size()) == n * count);
  std::vector<SpinMeasureChunk> chunks;
  eigenex::spin_measure_build_chunks(a, chunks);
  std::unique_ptr<eigenex::SpinSectorView> v(new eigenex::SpinSectorView());
  eigenex::SpinSectorTables t;
  if (sector) {
    eigenex::spin_sector_build_view(eigenex::SpinModelArgs{a.n_sites, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, a.n_up, *v);
    eigenex::spin_sector_build_tables(a.n_sites, a.n_up, t);
  }
  const CheckedBinomials binom(*v);
  const CheckedTables tab{&t};
  const CheckedVector xs_at{&x};
  diag.assign(static_cast<std::size_t>(a.n_diag) * static_cast<std::size_t>(count), 0.0);
  flip.assign(static_cast<std::size_t>(a.n_flip) * static_cast<std::size_t>(count), 0.0);
  for (std::size_t k = 0; k < chunks.size(); ++k) {
    const SpinMeasureChunk& ch = chunks[k];
    for (int j0 = 0; j0 < count; j0 += J) {
      const int ncols = count - j0 < J ? count - j0 : J;
      std::vector<double> dg(static_cast<std::size_t>(C * J), 0.0), fl(static_cast<std::size_t>(C * J), 0.0);
      for (std::int64_t r = 0; r < n; ++r) {
        std::uint32_t s = static_cast<std::uint32_t>(r);
        if (sector) {
          const eigenex::SpinUnranked u = eigenex::spin_unrank_row(binom, v->model.n_sites, v->n_up, s);
          EXPECT(u.left == 0 && u.k == 0 && u.s == eigenex::spin_sector_unrank(a.n_sites, a.n_up, r));
          s = u.s;
        }
        double col[eigenex::kSpinMeasureColumns];
        for (int j = 0; j < J; ++j) col[j] = V.at(static_cast<std::size_t>((j0 + (j < ncols ? j : ncols - 1)) * n + r));
        const double xs = xs_at(static_cast<std::uint32_t>(r));
        if (sector)
          eigenex::spin_measure_columns_row<true>(ch.dmask, ch.ndiag, ch.fmask, ch.nflip, s, xs, xs_at, tab, v->h, v->lo_mask, col, dg.data(), fl.data());
        else
          eigenex::spin_measure_columns_row<false>(ch.dmask, ch.ndiag, ch.fmask, ch.nflip, s, xs, xs_at, tab, 0, 0u, col, dg.data(), fl.data());
      }
      // the second stage's destinations: term k C + t, column j0 + j, live ones only
      for (int i = 0; i < ch.ndiag; ++i)
        for (int j = 0; j < ncols; ++j) diag.at((k * C + static_cast<std::size_t>(i)) * count + j0 + j) = dg.at(static_cast<std::size_t>(i * J + j));
      for (int i = 0; i < ch.nflip; ++i)
        for (int j = 0; j < ncols; ++j) flip.at((k * C + static_cast<std::size_t>(i)) * count + j0 + j) = fl.at(static_cast<std::size_t>(i * J + j));
    }
  }
}

static void check_shape(int L, int n_up, std::mt19937& rng) {
  const bool sector = n_up != -1;
  const Lists l = lists_of(L, sector);
  const SpinMeasureArgs a{L, n_up, static_cast<int>(l.diag.size()), l.diag.data(), static_cast<int>(l.flip.size()), l.flip.data()};
  EXPECT(eigenex::spin_measure_error(a) == nullptr);
  const std::int64_t n = eigenex::spin_measure_rows(a);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  std::vector<double> x(static_cast<std::size_t>(n));
  for (auto& e : x) e = u(rng);
  for (int count : {1, 3, 4, 5, 9}) {
    std::vector<double> V(static_cast<std::size_t>(n) * count);  // exactly sized: one row too many is a heap overflow
    for (auto& e : V) e = u(rng);
    std::vector<double> hd(l.diag.size() * count, -1.0), hf(l.flip.size() * count, -1.0), kd, kf;
    eigenex::spin_measure_columns_host(a, x.data(), V.data(), n, count, hd.data(), hf.data());
    replay(a, x, V, count, kd, kf);
    EXPECT(same_bits(hd, kd) && same_bits(hf, kf));
    // the duplicates, every column
    const std::size_t dup_f = l.flip.size() - 1 - (sector ? 0 : static_cast<std::size_t>(L));
    for (int j = 0; j < count; ++j)
      EXPECT(hd[(l.diag.size() - 1) * count + j] == hd[static_cast<std::size_t>(L) * count + j] && hf[dup_f * count + j] == hf[static_cast<std::size_t>(j)]);
    // either output may be absent
    eigenex::spin_measure_columns_host(a, x.data(), V.data(), n, count, nullptr, nullptr);
  }
  // with the vector itself as the column, the diagonal sums are the measurement's, bit for bit
  std::vector<double> md(l.diag.size(), -1.0), mf(l.flip.size(), -1.0), cd(l.diag.size(), -2.0), cf(l.flip.size(), -2.0);
  eigenex::spin_measure_host(a, x.data(), md.data(), mf.data(), nullptr);
  eigenex::spin_measure_columns_host(a, x.data(), x.data(), n, 1, cd.data(), cf.data());
  EXPECT(same_bits(md, cd) && same_bits(mf, cf));
}

static bool refused(int first, int count, int held, const char* word) {
  const char* why = eigenex::spin_measure_columns_error(first, count, held);
  return why != nullptr && std::strstr(why, word) != nullptr;
}

int main() {
  std::mt19937 rng(13);
  for (int L : {3, 6, 9}) check_shape(L, -1, rng);
  const int sectors[7][2] = {{4, 2}, {6, 0}, {6, 6}, {11, 5}, {31, 2}, {32, 2}, {32, 31}};
  for (const auto& s : sectors) check_shape(s[0], s[1], rng);
  // the column range
  EXPECT(eigenex::spin_measure_columns_error(0, 1, 1) == nullptr && eigenex::spin_measure_columns_error(3, 5, 8) == nullptr &&
         eigenex::spin_measure_columns_error(0, 8, 8) == nullptr);
  EXPECT(refused(0, 0, 8, "count") && refused(0, -1, 8, "count") && refused(-1, 2, 8, "first") && refused(4, 5, 8, "exceeds") &&
         refused(8, 1, 8, "exceeds") && refused(0x7fffffff, 0x7fffffff, 8, "exceeds"));
  if (fails) return 1;
  std::printf("SPIN MEASURE COLUMNS OK\n");
  return 0;
}
