// Host code of the spin measurement under AddressSanitizer + UBSan (device code cannot be sanitised on the GPU pool):
// csrc/spin_measure.hpp -- the argument check, the chunk table and the host evaluation -- compiled into this program, which
// links nothing else.  For the full space (L = 3, 6, 9) and the sectors (4,2), (6,0), (6,6), (11,5), (31,2), (32,2), (32,31), with
// every site, every pair, a four-site string, the all-sites mask and a duplicate (and every one-bit flip in the full space):
// the outputs go into exactly-sized arrays, and the row loop of k_spin_measure<SECTOR, double> runs on its chunk table -- the kernel's own
// functions (csrc/spin_rows.hpp), every load checked against its array: the lane's state from the binomials, the batches, the
// gather through hi_base and lo_rank, the own element where the entry is absent.  Taken over ascending rows it adds the same fma
// chain as the host evaluation (a lane without the entry adds x_s * 0), so the two are compared bit for bit.
// Built and run by tests/test_spin_measure_host.py; prints SPIN MEASURE OK and exits 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "spin_measure.hpp"
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

// k_spin_measure (kernels.hip) over ascending rows, by the kernel's own functions: one chunk per pass, sums per chunk slot,
// every load checked
static void replay(const SpinMeasureArgs& a, const std::vector<double>& x, std::vector<double>& diag, std::vector<double>& flip, double* norm2) {
  const int C = eigenex::kSpinMeasureChunk, B = eigenex::kSpinBatch;
  const bool sector = a.n_up != -1;
  const std::int64_t n = eigenex::spin_measure_rows(a);
  EXPECT(static_cast<std::int64_t>(x.size()) == n);
  std::vector<SpinMeasureChunk> chunks;
  eigenex::spin_measure_build_chunks(a, chunks);
  EXPECT(static_cast<int>(chunks.size()) == eigenex::spin_measure_chunks(a.n_diag, a.n_flip) && !chunks.empty());
  std::unique_ptr<eigenex::SpinSectorView> v(new eigenex::SpinSectorView());
  eigenex::SpinSectorTables t;
  if (sector) {
    eigenex::spin_sector_build_view(eigenex::SpinModelArgs{a.n_sites, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, a.n_up, *v);
    eigenex::spin_sector_build_tables(a.n_sites, a.n_up, t);
  }
  const CheckedBinomials binom(*v);
  const CheckedTables tab{&t};
  const CheckedVector xs_at{&x};
  diag.assign(static_cast<std::size_t>(a.n_diag), 0.0);
  flip.assign(static_cast<std::size_t>(a.n_flip), 0.0);
  int live_d = 0, live_f = 0;
  for (std::size_t k = 0; k < chunks.size(); ++k) {
    const SpinMeasureChunk& ch = chunks[k];
    EXPECT(ch.ndiag >= 0 && ch.ndiag <= C && ch.nflip >= 0 && ch.nflip <= C);
    for (int i = ch.ndiag; i < C; ++i) EXPECT(ch.dmask[i] == 0);
    for (int i = ch.nflip; i < C; ++i) EXPECT(ch.fmask[i] == 0);
    live_d += ch.ndiag, live_f += ch.nflip;
    double nrm = 0.0, dg[eigenex::kSpinMeasureChunk] = {0.0}, fl[eigenex::kSpinMeasureChunk] = {0.0};
    for (std::int64_t r = 0; r < n; ++r) {
      std::uint32_t s = static_cast<std::uint32_t>(r);
      if (sector) {
        const eigenex::SpinUnranked u = eigenex::spin_unrank_row(binom, v->model.n_sites, v->n_up, s);
        EXPECT(u.left == 0 && u.k == 0 && u.s == eigenex::spin_sector_unrank(a.n_sites, a.n_up, r));
        s = u.s;
      }
      const double xs = xs_at(static_cast<std::uint32_t>(r));
      nrm = eigenex::spin_norm_add(nrm, xs);
      for (int t0 = 0; t0 < C; t0 += B)
        if (t0 < ch.ndiag) eigenex::spin_measure_diagonals(xs, s, ch.dmask + t0, dg + t0);
      for (int t0 = 0; t0 < C; t0 += B)
        if (t0 < ch.nflip) {
          bool on[eigenex::kSpinBatch];
          std::uint32_t base[eigenex::kSpinBatch], low[eigenex::kSpinBatch];
          double xv[eigenex::kSpinBatch];
          if (sector)
            eigenex::spin_flip_targets<true>(ch.fmask + t0, s, tab, v->h, v->lo_mask, on, base, low);
          else
            eigenex::spin_flip_targets<false>(ch.fmask + t0, s, tab, 0, 0u, on, base, low);
          expect_targets(ch.fmask + t0, on, base, low, r);
          eigenex::spin_gather(xs_at, base, low, xv);
          eigenex::spin_measure_flips(xs, on, xv, fl + t0);
        }
    }
    for (int i = 0; i < ch.ndiag; ++i) diag.at(k * C + static_cast<std::size_t>(i)) = dg[i];
    for (int i = 0; i < ch.nflip; ++i) flip.at(k * C + static_cast<std::size_t>(i)) = fl[i];
    if (k == 0) *norm2 = nrm;
  }
  EXPECT(live_d == a.n_diag && live_f == a.n_flip);
}

static void check_shape(int L, int n_up, std::mt19937& rng) {
  const bool sector = n_up != -1;
  const Lists l = lists_of(L, sector);
  const SpinMeasureArgs a{L, n_up, static_cast<int>(l.diag.size()), l.diag.data(), static_cast<int>(l.flip.size()), l.flip.data()};
  EXPECT(eigenex::spin_measure_error(a) == nullptr);
  const std::int64_t n = eigenex::spin_measure_rows(a);
  std::vector<double> x(static_cast<std::size_t>(n));
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  for (auto& e : x) e = u(rng);
  std::vector<double> hd(l.diag.size(), -1.0), hf(l.flip.size(), -1.0), kd, kf;  // exactly sized: one entry too many is a heap overflow
  double hn = -1.0, kn = -1.0;
  eigenex::spin_measure_host(a, x.data(), hd.data(), hf.data(), &hn);
  replay(a, x, kd, kf, &kn);
  EXPECT(same_bits(hd, kd) && same_bits(hf, kf) && std::memcmp(&hn, &kn, sizeof(double)) == 0);
  EXPECT(hn > 0.0);
  EXPECT(hd[l.diag.size() - 1] == hd[static_cast<std::size_t>(L)] && hf[l.flip.size() - 1 - (sector ? 0 : static_cast<std::size_t>(L))] == hf[0]);  // the duplicates
  // every output may be absent, and so may both lists
  eigenex::spin_measure_host(a, x.data(), nullptr, nullptr, nullptr);
  const SpinMeasureArgs none{L, n_up, 0, nullptr, 0, nullptr};
  EXPECT(eigenex::spin_measure_error(none) == nullptr && eigenex::spin_measure_chunks(0, 0) == 1);
  double only = -1.0;
  eigenex::spin_measure_host(none, x.data(), nullptr, nullptr, &only);
  std::vector<double> nd, nf;
  double rn = -1.0;
  replay(none, x, nd, nf, &rn);
  EXPECT(std::memcmp(&only, &hn, sizeof(double)) == 0 && std::memcmp(&rn, &hn, sizeof(double)) == 0 && nd.empty() && nf.empty());
}

static bool refused(const SpinMeasureArgs& a, const char* word) {
  const char* why = eigenex::spin_measure_error(a);
  return why != nullptr && std::strstr(why, word) != nullptr;
}

int main() {
  std::mt19937 rng(11);
  for (int L : {3, 6, 9}) check_shape(L, -1, rng);
  const int sectors[7][2] = {{4, 2}, {6, 0}, {6, 6}, {11, 5}, {31, 2}, {32, 2}, {32, 31}};
  for (const auto& s : sectors) check_shape(s[0], s[1], rng);
  // chunk counts at the boundaries
  EXPECT(eigenex::spin_measure_chunks(16, 0) == 1 && eigenex::spin_measure_chunks(17, 3) == 2 && eigenex::spin_measure_chunks(3, 33) == 3 &&
         eigenex::spin_measure_chunks(1024, 1024) == 64);
  // the refusals
  {
    const std::uint32_t ok[2] = {3u, 5u}, zero[2] = {3u, 0u}, high[1] = {1u << 6}, three[1] = {7u}, one[1] = {4u}, top[1] = {0x80000001u};
    EXPECT(eigenex::spin_measure_error(SpinMeasureArgs{6, -1, 2, ok, 2, ok}) == nullptr);
    EXPECT(eigenex::spin_measure_error(SpinMeasureArgs{6, 3, 2, ok, 2, ok}) == nullptr);
    EXPECT(eigenex::spin_measure_error(SpinMeasureArgs{6, -1, 1, three, 1, one}) == nullptr);  // a string on the diagonal, Sx in the full space
    EXPECT(eigenex::spin_measure_error(SpinMeasureArgs{32, 2, 1, top, 1, top}) == nullptr);    // bit 31 is a site of 32
    EXPECT(refused(SpinMeasureArgs{6, -1, 2, zero, 0, nullptr}, "zero") && refused(SpinMeasureArgs{6, -1, 0, nullptr, 2, zero}, "zero"));
    EXPECT(refused(SpinMeasureArgs{6, -1, 1, high, 0, nullptr}, "outside") && refused(SpinMeasureArgs{6, 3, 0, nullptr, 1, high}, "outside"));
    EXPECT(refused(SpinMeasureArgs{31, 2, 1, top, 0, nullptr}, "outside"));
    EXPECT(refused(SpinMeasureArgs{6, -1, 0, nullptr, 1, three}, "one or two"));
    EXPECT(refused(SpinMeasureArgs{6, 3, 0, nullptr, 1, one}, "conserve"));
    EXPECT(refused(SpinMeasureArgs{6, -1, -1, ok, 0, nullptr}, "n_diag") && refused(SpinMeasureArgs{6, -1, 0, nullptr, 1025, ok}, "n_flip"));
    EXPECT(refused(SpinMeasureArgs{6, -1, 2, nullptr, 0, nullptr}, "NULL") && refused(SpinMeasureArgs{6, -1, 0, nullptr, 1, nullptr}, "NULL"));
    EXPECT(refused(SpinMeasureArgs{31, -1, 0, nullptr, 0, nullptr}, "n_sites") && refused(SpinMeasureArgs{33, 2, 0, nullptr, 0, nullptr}, "n_sites") &&
           refused(SpinMeasureArgs{1, -1, 0, nullptr, 0, nullptr}, "n_sites"));
    EXPECT(refused(SpinMeasureArgs{6, 7, 0, nullptr, 0, nullptr}, "n_up") && refused(SpinMeasureArgs{6, -2, 0, nullptr, 0, nullptr}, "n_up"));
  }
  if (fails) return 1;
  std::printf("SPIN MEASURE OK\n");
  return 0;
}
