// Host code of the site operators of COMPLEX vectors under AddressSanitizer + UBSan (device code cannot be sanitised on the GPU
// pool): csrc/spin_site.hpp -- the argument check with imaginary coefficients, the kernel's table with its imaginary halves and
// real_coef, and spin_site_apply_host_z -- compiled into this program, which links nothing else.  NOT part of the reference.
// For every shape the row loop of k_spin_site_apply<SECTOR, SpinZ> (kernels.hip) runs on that table over every row of the
// destination -- the kernel's own functions (csrc/spin_rows.hpp: spin_site_weights, spin_site_product, spin_site_targets,
// spin_gather, spin_site_add of a SpinZ), every load checked against its array.  y and norm2 must equal spin_site_apply_host_z
// bit for bit: the same operations in the same order.  Each shape runs with complex coefficients, with coef_im = NULL and with an
// all-zero coef_im; the last two must give, part by part, spin_site_apply_host of the real and of the imaginary part of x.
// Sectors: (4,2), (9,4), (11,5), (13,1), (17,8) (three site batches), (6,0) -> PLUS, (6,6) -> MINUS, (32,1) -> MINUS (a one-row
// destination, bit 31), (32,31) -> PLUS; the full space at L = 3 and 8.
// Built and run by tests/test_spin_site_z_host.py; prints SPIN SITE Z OK and exits 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "spin_site.hpp"
#include "spin_rows_checked.hpp"

using eigenex::SpinSiteArgs;
using eigenex::SpinSiteCoefficients;
using eigenex::SpinSiteTable;
using eigenex::SpinZ;

struct CheckedVectorZ {  // an interleaved complex vector, element i
  const std::vector<double>* x;
  SpinZ operator()(std::uint32_t i) const { return SpinZ{x->at(2 * static_cast<std::size_t>(i)), x->at(2 * static_cast<std::size_t>(i) + 1)}; }
};

// k_spin_site_apply<SECTOR, SpinZ> over ascending rows, by the kernel's own functions, every load checked
static void replay(const SpinSiteArgs& a, const std::vector<double>& x, std::vector<double>& y, double* norm2) {
  const int B = eigenex::kSpinBatch;
  const bool sector = a.n_up_src != -1;
  const std::int64_t n = eigenex::spin_site_rows(a.n_sites, a.n_up_dst);
  EXPECT(static_cast<std::int64_t>(x.size()) == 2 * eigenex::spin_site_rows(a.n_sites, a.n_up_src));
  SpinSiteTable tb;
  eigenex::spin_site_build_table(a, tb);
  EXPECT(tb.kind == a.kind && tb.n_sites == a.n_sites);
  bool any_im = false;
  for (int i = 0; i < a.n_sites; ++i) {
    const double ci = a.coef_im ? a.coef_im[i] : 0.0;
    EXPECT(tb.coef[i] == a.coef[i] && tb.half[i] == a.coef[i] * 0.5 && tb.coef_im[i] == ci && tb.half_im[i] == ci * 0.5);
    any_im = any_im || ci != 0.0;
  }
  for (int i = a.n_sites; i < eigenex::kSectorMaxSites; ++i) EXPECT(tb.coef[i] == 0.0 && tb.half[i] == 0.0 && tb.coef_im[i] == 0.0 && tb.half_im[i] == 0.0);
  EXPECT(tb.real_coef == (any_im ? 0 : 1));
  const bool real_coef = tb.real_coef != 0;
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
  const CheckedVectorZ xs_at{&x};
  y.assign(2 * static_cast<std::size_t>(n), -1.0);
  double nrm = 0.0;
  for (std::int64_t r = 0; r < n; ++r) {
    std::uint32_t s = static_cast<std::uint32_t>(r);
    if (sector) {
      const eigenex::SpinUnranked u = eigenex::spin_unrank_row(binom, tb.n_sites, dst->n_up, s);
      EXPECT(u.left == 0 && u.k == 0 && u.s == eigenex::spin_sector_unrank(a.n_sites, a.n_up_dst, r));
      s = u.s;
    }
    SpinZ yr = SpinZ{};
    if (tb.kind == eigenex::kSpinSiteZ) {
      const SpinZ w = eigenex::spin_site_weights(SpinSiteCoefficients{tb.half, tb.half_im, real_coef}, tb.n_sites, s, SpinZ{});
      yr = eigenex::spin_site_product(w, real_coef, xs_at(static_cast<std::uint32_t>(r)));
    } else {
      const std::uint32_t has = tb.kind == eigenex::kSpinSitePlus ? s : ~s & tb.site_mask;
      for (int i0 = 0; i0 < tb.n_sites; i0 += B) {
        EXPECT(i0 + B <= eigenex::kSectorMaxSites);
        bool on[eigenex::kSpinBatch];
        std::uint32_t base[eigenex::kSpinBatch], low[eigenex::kSpinBatch];
        SpinZ xv[eigenex::kSpinBatch];
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
        yr = eigenex::spin_site_add(yr, SpinSiteCoefficients{tb.coef + i0, tb.coef_im + i0, real_coef}, on, xv);
      }
    }
    y.at(2 * static_cast<std::size_t>(r)) = yr.re;
    y.at(2 * static_cast<std::size_t>(r) + 1) = yr.im;
    nrm = eigenex::spin_norm_add(nrm, yr);
  }
  *norm2 = nrm;
}

static std::vector<double> part(const std::vector<double>& z, int which) {
  std::vector<double> out(z.size() / 2);
  for (std::size_t i = 0; i < out.size(); ++i) out[i] = z[2 * i + static_cast<std::size_t>(which)];
  return out;
}

static void check_shape(int L, int n_up, int kind, std::mt19937& rng) {
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  std::vector<double> cr(static_cast<std::size_t>(L)), ci(static_cast<std::size_t>(L));  // exactly sized: one read too many is a heap overflow
  for (auto& c : cr) c = u(rng);
  for (auto& c : ci) c = u(rng);
  cr[static_cast<std::size_t>(L / 2)] = 0.0, ci[0] = 0.0;
  const std::vector<double> zero(static_cast<std::size_t>(L), 0.0);
  const int up = eigenex::spin_site_dst_up(n_up, kind);
  std::vector<double> x(2 * static_cast<std::size_t>(eigenex::spin_site_rows(L, n_up)));
  for (auto& e : x) e = u(rng);
  const std::size_t nd = static_cast<std::size_t>(eigenex::spin_site_rows(L, up));
  const double* forms[3] = {ci.data(), nullptr, zero.data()};
  for (int form = 0; form < 3; ++form) {
    const SpinSiteArgs a{L, n_up, kind, cr.data(), L, up, forms[form]};
    EXPECT(eigenex::spin_site_error(a) == nullptr);
    EXPECT(eigenex::spin_site_real_coef(a) == (form != 0));
    std::vector<double> hy(2 * nd, -1.0), ky;
    double hn = -1.0, kn = -1.0;
    eigenex::spin_site_apply_host_z(a, x.data(), hy.data(), &hn);
    replay(a, x, ky, &kn);
    EXPECT(same_bits(hy, ky) && std::memcmp(&hn, &kn, sizeof(double)) == 0);
    EXPECT(hn > 0.0);
    eigenex::spin_site_apply_host_z(a, x.data(), hy.data(), nullptr);  // norm2 may be absent
    if (kind == eigenex::kSpinSiteZ) {  // in place
      std::vector<double> v = x;
      eigenex::spin_site_apply_host_z(a, v.data(), v.data(), nullptr);
      EXPECT(same_bits(v, ky));
    }
    if (form != 0) {  // no imaginary coefficients: each part is the real call on that part
      const SpinSiteArgs real{L, n_up, kind, cr.data(), L, up};
      for (int which = 0; which < 2; ++which) {
        std::vector<double> ry(nd, -1.0);
        eigenex::spin_site_apply_host(real, part(x, which).data(), ry.data(), nullptr);
        EXPECT(same_bits(ry, part(ky, which)));
      }
    }
  }
}

static bool refused(const SpinSiteArgs& a, const char* word) {
  const char* why = eigenex::spin_site_error(a);
  return why != nullptr && std::strstr(why, word) != nullptr;
}

int main() {
  std::mt19937 rng(29);
  const int Z = eigenex::kSpinSiteZ, P = eigenex::kSpinSitePlus, M = eigenex::kSpinSiteMinus;
  for (int L : {3, 8})
    for (int kind : {Z, P, M}) check_shape(L, -1, kind, rng);
  const int all[5][2] = {{4, 2}, {9, 4}, {11, 5}, {13, 1}, {17, 8}};
  for (const auto& s : all)
    for (int kind : {Z, P, M}) check_shape(s[0], s[1], kind, rng);
  check_shape(6, 0, P, rng), check_shape(6, 0, Z, rng);    // a one-row source
  check_shape(6, 6, M, rng), check_shape(6, 6, Z, rng);
  check_shape(32, 1, M, rng), check_shape(32, 1, Z, rng);  // a one-row destination; bit 31
  check_shape(32, 31, P, rng);
  // the refusals that the imaginary coefficients add; a real coefficient list keeps its own (spin_site_sanitize.cpp)
  {
    const double ok[32] = {1.0, -2.0, 0.0, 4.0, 5.0, 6.0, 7.0, 8.0};
    double inf[7] = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0, INFINITY}, nan[6] = {NAN, 2.0, 3.0, 4.0, 5.0, 6.0};
    EXPECT(eigenex::spin_site_error(SpinSiteArgs{6, 3, Z, ok, 6, 3, ok}) == nullptr && eigenex::spin_site_error(SpinSiteArgs{6, 3, P, ok, 6, 4, nullptr}) == nullptr);
    EXPECT(eigenex::spin_site_error(SpinSiteArgs{6, 3, M, ok, 6, 2, inf}) == nullptr);  // the seventh entry is not read
    inf[5] = INFINITY;
    EXPECT(refused(SpinSiteArgs{6, 3, Z, ok, 6, 3, inf}, "not finite") && refused(SpinSiteArgs{6, -1, P, ok, 6, -1, nan}, "not finite"));
    EXPECT(refused(SpinSiteArgs{6, 3, Z, inf, 6, 3, ok}, "not finite") && refused(SpinSiteArgs{6, 3, Z, nullptr, 6, 3, ok}, "NULL"));
    EXPECT(refused(SpinSiteArgs{6, 3, 3, ok, 6, 3, ok}, "kind") && refused(SpinSiteArgs{6, 6, P, ok, 6, 7, ok}, "destination sector"));
    EXPECT(refused(SpinSiteArgs{6, 3, P, ok, 6, 3, ok}, "belong together"));
    const double negzero[6] = {-0.0, 0.0, -0.0, 0.0, 0.0, -0.0};
    EXPECT(eigenex::spin_site_real_coef(SpinSiteArgs{6, 3, Z, ok, 6, 3, negzero}) && !eigenex::spin_site_real_coef(SpinSiteArgs{6, 3, Z, ok, 6, 3, ok}));
  }
  if (fails) return 1;
  std::printf("SPIN SITE Z OK\n");
  return 0;
}
