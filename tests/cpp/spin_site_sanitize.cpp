// Host code of the site operators under AddressSanitizer + UBSan (device code cannot be sanitised on the GPU pool):
// csrc/spin_site.hpp -- the argument check, the kernel's table and the host evaluation -- compiled into this program, which
// links nothing else.  NOT part of the reference.  For every shape the row loop of k_spin_site_apply (kernels.hip) runs on
// that table over every row of the destination -- the kernel's own functions (csrc/spin_rows.hpp), every load checked against
// its array: the lane's state from the binomials with the DESTINATION's n_up, the site batches, the gather through the
// SOURCE's hi_base and lo_rank, row 0 of the source where the row has no such term.  y and norm2 must equal
// spin_site_apply_host as numbers (they are the same operations in the same order, so they are compared bit for bit).
// Sectors: (4,2), (6,0) -> PLUS, (6,6) -> MINUS, (9,4) (odd L: the h = (L + 1) / 2 split), (13,1), (12,6), (17,8) (three site
// batches, the last one partial) and (32,1) -> MINUS (a one-row destination, bit 31); the full space at L = 3, 8, 9.
// Built and run by tests/test_spin_site_host.py; prints SPIN SITE OK and exits 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "spin_site.hpp"
#include "spin_rows_checked.hpp"

using eigenex::SpinSiteArgs;
using eigenex::SpinSiteTable;

// k_spin_site_apply over ascending rows, by the kernel's own functions, every load checked
static void replay(const SpinSiteArgs& a, const std::vector<double>& x, std::vector<double>& y, double* norm2) {
  const int B = eigenex::kSpinBatch;
  const bool sector = a.n_up_src != -1;
  const std::int64_t n = eigenex::spin_site_rows(a.n_sites, a.n_up_dst);
  EXPECT(static_cast<std::int64_t>(x.size()) == eigenex::spin_site_rows(a.n_sites, a.n_up_src));
  SpinSiteTable tb;
  eigenex::spin_site_build_table(a, tb);
  EXPECT(tb.kind == a.kind && tb.n_sites == a.n_sites);
  for (int i = a.n_sites; i < eigenex::kSectorMaxSites; ++i) EXPECT(tb.coef[i] == 0.0 && tb.half[i] == 0.0);
  std::unique_ptr<eigenex::SpinSectorView> dst(new eigenex::SpinSectorView());
  eigenex::SpinSectorTables src;  // empty in the full space, which must not look at them
  if (sector) {
    eigenex::spin_sector_build_view(eigenex::SpinModelArgs{a.n_sites, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, a.n_up_dst, *dst);
    eigenex::spin_sector_build_tables(a.n_sites, a.n_up_src, src);
    EXPECT(eigenex::spin_sector_rank(src, tb.fallback) == 0 && __builtin_popcount(tb.fallback) == a.n_up_src);
  } else {
    EXPECT(tb.fallback == 0u);
  }
  const CheckedBinomials binom(*dst);
  const CheckedTables tab{&src};
  const CheckedVector xs_at{&x};
  y.assign(static_cast<std::size_t>(n), -1.0);
  double nrm = 0.0;
  for (std::int64_t r = 0; r < n; ++r) {
    std::uint32_t s = static_cast<std::uint32_t>(r);
    if (sector) {
      const eigenex::SpinUnranked u = eigenex::spin_unrank_row(binom, tb.n_sites, dst->n_up, s);
      EXPECT(u.left == 0 && u.k == 0 && u.s == eigenex::spin_sector_unrank(a.n_sites, a.n_up_dst, r));
      s = u.s;
    }
    double yr = 0.0;
    if (tb.kind == eigenex::kSpinSiteZ) {
      yr = eigenex::spin_site_weight(tb.half, tb.n_sites, s) * xs_at(static_cast<std::uint32_t>(r));
    } else {
      const std::uint32_t has = tb.kind == eigenex::kSpinSitePlus ? s : ~s & tb.site_mask;
      for (int i0 = 0; i0 < tb.n_sites; i0 += B) {
        EXPECT(i0 + B <= eigenex::kSectorMaxSites);
        bool on[eigenex::kSpinBatch];
        std::uint32_t base[eigenex::kSpinBatch], low[eigenex::kSpinBatch];
        double xv[eigenex::kSpinBatch];
        if (sector)
          eigenex::spin_site_targets<true>(i0, s, has, tb.fallback, tab, dst->h, dst->lo_mask, on, base, low);
        else
          eigenex::spin_site_targets<false>(i0, s, has, tb.fallback, tab, 0, 0u, on, base, low);
        for (int t = 0; t < B; ++t) {
          const int i = i0 + t;
          const bool want = i < a.n_sites && (((s >> i) & 1u) != 0) == (a.kind == eigenex::kSpinSitePlus);
          EXPECT(on[t] == want);
          if (!on[t]) EXPECT(base[t] + low[t] == 0u);  // a lane without the term reads row 0 of the source
          if (on[t] && sector) EXPECT(base[t] + low[t] == eigenex::spin_sector_rank(src, s ^ (std::uint32_t(1) << i)));
          if (on[t] && !sector) EXPECT(base[t] + low[t] == (s ^ (std::uint32_t(1) << i)));
        }
        eigenex::spin_gather(xs_at, base, low, xv);
        yr = eigenex::spin_site_add(yr, tb.coef + i0, on, xv);
      }
    }
    y.at(static_cast<std::size_t>(r)) = yr;
    nrm = std::fma(yr, yr, nrm);
  }
  *norm2 = nrm;
}

static void check_shape(int L, int n_up, int kind, std::mt19937& rng) {
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  std::vector<double> coef(static_cast<std::size_t>(L));  // exactly sized: one read too many is a heap overflow
  for (auto& c : coef) c = u(rng);
  coef[static_cast<std::size_t>(L / 2)] = 0.0;
  const SpinSiteArgs a{L, n_up, kind, coef.data(), L, eigenex::spin_site_dst_up(n_up, kind)};
  EXPECT(eigenex::spin_site_error(a) == nullptr);
  std::vector<double> x(static_cast<std::size_t>(eigenex::spin_site_rows(L, n_up)));
  for (auto& e : x) e = u(rng);
  std::vector<double> hy(static_cast<std::size_t>(eigenex::spin_site_rows(L, a.n_up_dst)), -1.0), ky;
  double hn = -1.0, kn = -1.0;
  eigenex::spin_site_apply_host(a, x.data(), hy.data(), &hn);
  replay(a, x, ky, &kn);
  EXPECT(same_bits(hy, ky) && std::memcmp(&hn, &kn, sizeof(double)) == 0);
  EXPECT(hn > 0.0);
  eigenex::spin_site_apply_host(a, x.data(), hy.data(), nullptr);  // norm2 may be absent
  if (kind == eigenex::kSpinSiteZ) {  // in place
    std::vector<double> v = x;
    eigenex::spin_site_apply_host(a, v.data(), v.data(), nullptr);
    EXPECT(same_bits(v, ky));
  }
}

static bool refused(const SpinSiteArgs& a, const char* word) {
  const char* why = eigenex::spin_site_error(a);
  return why != nullptr && std::strstr(why, word) != nullptr;
}

int main() {
  std::mt19937 rng(23);
  const int Z = eigenex::kSpinSiteZ, P = eigenex::kSpinSitePlus, M = eigenex::kSpinSiteMinus;
  for (int L : {3, 8, 9})
    for (int kind : {Z, P, M}) check_shape(L, -1, kind, rng);
  const int all[5][2] = {{4, 2}, {9, 4}, {13, 1}, {12, 6}, {17, 8}};
  for (const auto& s : all)
    for (int kind : {Z, P, M}) check_shape(s[0], s[1], kind, rng);
  check_shape(6, 0, P, rng), check_shape(6, 0, Z, rng);    // a one-row source
  check_shape(6, 6, M, rng), check_shape(6, 6, Z, rng);
  check_shape(32, 1, M, rng), check_shape(32, 1, Z, rng);  // a one-row destination; bit 31
  check_shape(32, 31, P, rng);
  // the refusals
  {
    const double ok[32] = {1.0, -2.0, 0.0, 4.0, 5.0, 6.0, 7.0, 8.0};
    double inf[6] = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0}, nan[6] = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0};
    inf[5] = INFINITY, nan[0] = NAN;
    EXPECT(eigenex::spin_site_error(SpinSiteArgs{6, 3, Z, ok, 6, 3}) == nullptr && eigenex::spin_site_error(SpinSiteArgs{6, 3, P, ok, 6, 4}) == nullptr);
    EXPECT(eigenex::spin_site_error(SpinSiteArgs{6, 3, M, ok, 6, 2}) == nullptr && eigenex::spin_site_error(SpinSiteArgs{6, -1, M, ok, 6, -1}) == nullptr);
    EXPECT(eigenex::spin_site_error(SpinSiteArgs{32, 32, M, ok, 32, 31}) == nullptr && eigenex::spin_site_error(SpinSiteArgs{30, -1, P, ok, 30, -1}) == nullptr);
    EXPECT(refused(SpinSiteArgs{6, 3, 3, ok, 6, 3}, "kind") && refused(SpinSiteArgs{6, 3, -1, ok, 6, 3}, "kind"));
    EXPECT(refused(SpinSiteArgs{6, 3, Z, inf, 6, 3}, "not finite") && refused(SpinSiteArgs{6, -1, P, nan, 6, -1}, "not finite"));
    EXPECT(refused(SpinSiteArgs{6, 3, Z, nullptr, 6, 3}, "NULL"));
    EXPECT(refused(SpinSiteArgs{6, 6, P, ok, 6, 7}, "destination sector") && refused(SpinSiteArgs{6, 0, M, ok, 6, -1}, "destination sector"));
    EXPECT(refused(SpinSiteArgs{6, 3, P, ok, 6, 3}, "belong together") && refused(SpinSiteArgs{6, 3, Z, ok, 6, 4}, "belong together"));
    EXPECT(refused(SpinSiteArgs{6, 3, M, ok, 6, 4}, "belong together") && refused(SpinSiteArgs{6, 3, M, ok, 7, 2}, "belong together"));
    EXPECT(refused(SpinSiteArgs{6, -1, P, ok, 6, 4}, "belong together") && refused(SpinSiteArgs{6, 3, Z, ok, 6, -1}, "belong together"));
    EXPECT(refused(SpinSiteArgs{31, -1, Z, ok, 31, -1}, "n_sites") && refused(SpinSiteArgs{33, 2, Z, ok, 33, 2}, "n_sites") &&
           refused(SpinSiteArgs{1, -1, Z, ok, 1, -1}, "n_sites"));
    EXPECT(refused(SpinSiteArgs{6, 7, Z, ok, 6, 7}, "n_up") && refused(SpinSiteArgs{6, -2, Z, ok, 6, -2}, "n_up"));
    EXPECT(eigenex::spin_site_dst_up(-1, P) == -1 && eigenex::spin_site_dst_up(4, Z) == 4 && eigenex::spin_site_dst_up(4, P) == 5 && eigenex::spin_site_dst_up(4, M) == 3);
  }
  if (fails) return 1;
  std::printf("SPIN SITE OK\n");
  return 0;
}
