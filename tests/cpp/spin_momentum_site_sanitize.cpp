// csrc/spin_momentum_site.hpp and the walk of k_spin_momentum_site_apply<E, Word> (csrc/spin_rows.hpp) under AddressSanitizer +
// UBSan, stand-alone (no library, no GPU), for the state word given as the argument, 32 or 64:
//   g++ -std=c++11 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -pthread -I cmpt-eigenex_amd/csrc spin_momentum_site_sanitize.cpp
// For every shape, every (m, p) with m in {0, 1, N/2} and p in {0, 1, N/2, N-1}, every kind whose two sectors exist and both
// elements (a real vector where the real form applies): the argument check, the table, the definition
// spin_momentum_site_apply_host<Word>, and the kernel's own walk over the destination's rows -- spin_orbit,
// spin_momentum_site_targets, spin_momentum_gather, spin_momentum_site_add, spin_momentum_site_z_row on the source's lookup and
// tables, every load bounds-checked, the fallback lookups included -- whose rows must equal the definition's bit for bit.  A lane
// without a term must have looked up row 0 of the source.  The 64-bit run also evaluates the definition with both words on every
// ring of at most 32 sites and compares the bytes.  32 sites are among the shapes of the 32-bit run and 33, 36 and 48 among those
// of the 64-bit run, so that UBSan sees every shift.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "spin_momentum_site.hpp"
#include "spin_rows_checked.hpp"

using namespace eigenex;

template <class Word>
struct CheckedLookup {
  const SpinMomentumBasisOf<Word>* b;
  Word reps(std::uint32_t i) const { return b->reps.at(i); }
  std::uint32_t bucket(std::uint32_t i) const { return b->bucket.at(i); }
};
template <class Word>
struct CheckedMomentumTables {
  const SpinMomentumTablesOf<Word>* t;
  double ratio(int i) const {
    EXPECT(i >= 0 && i < SpinWord<Word>::kRatioPitch * SpinWord<Word>::kRatioPitch);
    return t->ratio[i];
  }
  double phase_re(int i) const {
    EXPECT(i >= 0 && i < SpinWord<Word>::kMaxPeriod);
    return t->phase_re[i];
  }
  double phase_im(int i) const {
    EXPECT(i >= 0 && i < SpinWord<Word>::kMaxPeriod);
    return t->phase_im[i];
  }
};
struct CheckedVectorZ {
  const std::vector<double>* x;  // interleaved
  SpinZ operator()(std::uint32_t i) const { return SpinZ{x->at(2 * (std::size_t)i), x->at(2 * (std::size_t)i + 1)}; }
};
template <class E>
struct VectorOf;
template <>
struct VectorOf<double> {
  typedef CheckedVector type;
};
template <>
struct VectorOf<SpinZ> {
  typedef CheckedVectorZ type;
};

static void put(std::vector<double>& y, std::size_t r, double v) { y.at(r) = v; }
static void put(std::vector<double>& y, std::size_t r, SpinZ v) { y.at(2 * r) = v.re, y.at(2 * r + 1) = v.im; }

// a deterministic vector with both signs and some spread of magnitudes
static std::vector<double> test_vector(std::size_t n, std::uint64_t seed) {
  std::vector<double> x(n);
  std::uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
  for (std::size_t i = 0; i < n; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    x[i] = ((double)(std::int64_t)(s >> 11) / (double)(1ull << 52) - 1.0) * (1.0 + (double)(i % 7));
  }
  return x;
}

// the kernel's row loop on row r of the destination: y_r
template <class E, class Word>
static E walk_row(const SpinMomentumSiteTable& tb, const SpinMomentumBasisOf<Word>& src, const SpinMomentumTablesOf<Word>& ts,
                  const SpinMomentumBasisOf<Word>& dst, const std::vector<double>& x, std::size_t r, bool real_coef) {
  const CheckedLookup<Word> lk{&src};
  const CheckedMomentumTables<Word> tab{&ts};
  const typename VectorOf<E>::type xs{&x};
  const int n_sites = src.n_sites, cell = src.cell, n_trans = src.n_trans, h = src.h, steps = src.steps;
  const Word site_mask = spin_momentum_site_mask<Word>(n_sites), compatible = (Word)tb.compatible, fallback = (Word)tb.first_rep;
  EXPECT((std::uint64_t)compatible == tb.compatible && (std::uint64_t)fallback == tb.first_rep);
  const Word s = dst.reps.at(r);
  const int period = spin_orbit(s, n_sites, cell, n_trans).period;
  EXPECT(period == dst.period.at(r));
  if (tb.kind == kSpinSiteZ)
    return spin_momentum_site_z_row(s, period, n_sites, compatible, fallback, h, steps, lk, SpinSiteCoefficients{tb.half, tb.half_im, real_coef}, xs, E{});
  E yr = E{};
  const Word has = tb.kind == kSpinSitePlus ? s : Word(~s & site_mask);
  for (int i0 = 0; i0 < n_sites; i0 += kSpinBatch) {
    EXPECT(i0 + kSpinBatch <= kMomentumSiteMaxSites && i0 + kSpinBatch <= SpinWord<Word>::kBits);
    bool on[kSpinBatch];
    std::uint32_t column[kSpinBatch];
    int ri[kSpinBatch], li[kSpinBatch];
    E xv[kSpinBatch];
    spin_momentum_site_targets(i0, s, has, period, n_sites, cell, n_trans, compatible, fallback, h, steps, lk, on, column, ri, li);
    for (int t = 0; t < kSpinBatch; ++t) {
      if (!on[t]) EXPECT(column[t] == 0);  // a lane without the term reads row 0 of the source
      if (i0 + t >= n_sites) EXPECT(!on[t]);
      EXPECT(li[t] >= 0 && li[t] < n_trans);
      EXPECT(column[t] < src.reps.size());
    }
    spin_momentum_gather(xs, column, xv);
    yr = spin_momentum_site_add(yr, SpinSiteCoefficients{tb.coef + i0, tb.coef_im + i0, real_coef}, tab, on, ri, li, xv);
  }
  return yr;
}

// the rows of the sectors of one ring, built once per (n_up, momentum): with the lookup for a source of the walk, without it else
template <class Word>
struct Ring {
  int n_sites, cell;
  std::map<std::pair<int, int>, std::unique_ptr<SpinMomentumBasisOf<Word>>> with_lookup, plain;
  const SpinMomentumBasisOf<Word>& rows(int n_up, int momentum, bool lookup) {
    std::unique_ptr<SpinMomentumBasisOf<Word>>& b = (lookup ? with_lookup : plain)[std::make_pair(n_up, momentum)];
    if (!b) {
      b.reset(new SpinMomentumBasisOf<Word>());
      if (spin_momentum_build_basis<Word>(n_sites, n_up, cell, momentum, b.get(), lookup) == 0) *b = SpinMomentumBasisOf<Word>();
    }
    return *b;
  }
};

template <class Word>
struct Sectors {
  const SpinMomentumBasisOf<Word>*src_p, *dst_p;
  std::unique_ptr<SpinMomentumTablesOf<Word>> ts;
  SpinMomentumSiteTable table;
  bool ok;
  const SpinMomentumBasisOf<Word>& src() const { return *src_p; }
  const SpinMomentumBasisOf<Word>& dst() const { return *dst_p; }
};

// the two sectors, the source's tables and the table of a valid call; ok is false where either sector has no rows
template <class Word>
static void build(Ring<Word>& ring, const SpinMomentumSiteArgs& a, bool with_lookup, Sectors<Word>& s) {
  const int n_trans = a.n_sites / a.cell;
  EXPECT(spin_momentum_site_error<Word>(a).empty());
  s.src_p = &ring.rows(a.n_up, a.momentum, with_lookup);
  s.dst_p = &ring.rows(spin_momentum_site_dst_up(a.n_up, a.kind), spin_momentum_site_dst_momentum(n_trans, a.momentum, a.p), false);
  s.ok = !s.src().reps.empty() && !s.dst().reps.empty();
  if (!s.ok) return;
  s.ts.reset(new SpinMomentumTablesOf<Word>());
  spin_momentum_build_tables(n_trans, a.momentum, *s.ts);
  spin_momentum_site_build_table<Word>(a, s.src().reps[0], s.table);
}

template <class Word>
static std::vector<double> definition(const Sectors<Word>& s, bool is_complex, const std::vector<double>& x, double* norm2) {
  std::vector<double> y((is_complex ? 2 : 1) * s.dst().reps.size(), -1.0);
  spin_momentum_site_apply_host(s.src(), s.dst(), *s.ts, s.table, is_complex, x.data(), y.data(), norm2);
  return y;
}

static long calls = 0, agreed = 0;

template <class Word>
static void run_call(Ring<Word>& ring, Ring<std::uint32_t>* narrow, const SpinMomentumSiteArgs& a) {
  Sectors<Word> s;
  build<Word>(ring, a, true, s);
  if (!s.ok) return;
  const bool real_form = spin_momentum_site_is_real(a);
  EXPECT(!real_form || s.table.real_coef == 1);
  for (int is_complex = real_form ? 0 : 1; is_complex <= 1; ++is_complex) {
    const std::vector<double> x = test_vector((is_complex ? 2 : 1) * s.src().reps.size(), 17 + (std::uint64_t)a.n_sites * 31 + (std::uint64_t)a.p);
    double norm2 = -1.0;
    const std::vector<double> want = definition(s, is_complex != 0, x, &norm2);
    std::vector<double> got(want.size(), -2.0);
    double nrm = 0.0;
    for (std::size_t r = 0; r < s.dst().reps.size(); ++r) {
      if (is_complex) {
        const SpinZ v = walk_row<SpinZ, Word>(s.table, s.src(), *s.ts, s.dst(), x, r, s.table.real_coef != 0);
        put(got, r, v);
        nrm = spin_norm_add(nrm, v);
      } else {
        const double v = walk_row<double, Word>(s.table, s.src(), *s.ts, s.dst(), x, r, true);
        put(got, r, v);
        nrm = spin_norm_add(nrm, v);
      }
    }
    EXPECT(same_bits(got, want));
    EXPECT(std::memcmp(&nrm, &norm2, 8) == 0);
    if (a.kind == kSpinSiteZ && a.p == 0) {  // in place
      std::vector<double> z = x;
      spin_momentum_site_apply_host(s.src(), s.dst(), *s.ts, s.table, is_complex != 0, z.data(), z.data(), nullptr);
      EXPECT(same_bits(z, want));
    }
    if (narrow) {
      Sectors<std::uint32_t> n;
      build<std::uint32_t>(*narrow, a, false, n);
      EXPECT(n.ok);
      double norm32 = -1.0;
      if (n.ok) EXPECT(same_bits(definition(n, is_complex != 0, x, &norm32), want) && std::memcmp(&norm32, &norm2, 8) == 0);
      ++agreed;
    }
    ++calls;
  }
}

template <class Word>
static void run_shape(int L, int n_up, int cell, bool both_words) {
  const int N = L / cell;
  Ring<Word> ring{L, cell, {}, {}};
  Ring<std::uint32_t> narrow{L, cell, {}, {}};
  const int ms[3] = {0, 1 % N, N / 2}, ps[4] = {0, 1 % N, N / 2, N - 1};
  double re[48], im[48], zero[48];
  for (int j = 0; j < 48; ++j) re[j] = 0.75 - 0.25 * j, im[j] = 0.5 + 0.125 * j, zero[j] = 0.0;
  for (int mi = 0; mi < 3; ++mi)
    for (int pi = 0; pi < 4; ++pi) {
      bool repeated = false;
      for (int k = 0; k < mi; ++k) repeated = repeated || ms[k] == ms[mi];
      for (int k = 0; k < pi; ++k) repeated = repeated || ps[k] == ps[pi];
      if (repeated) continue;
      for (int kind = kSpinSiteZ; kind <= kSpinSiteMinus; ++kind) {
        const int up2 = spin_momentum_site_dst_up(n_up, kind);
        if (up2 < 0 || up2 > L) continue;
        const double* forms[3][2] = {{re, im}, {re, nullptr}, {re, zero}};
        for (int f = 0; f < 3; ++f) run_call<Word>(ring, both_words && L <= 32 ? &narrow : nullptr, SpinMomentumSiteArgs{L, n_up, cell, ms[mi], kind, ps[pi], forms[f][0], forms[f][1]});
      }
    }
}

static void check_refusals() {
  const double one[2] = {1.0, 1.0}, bad[2] = {1.0, HUGE_VAL};
  EXPECT(spin_momentum_site_error<std::uint32_t>(SpinMomentumSiteArgs{8, 4, 1, 0, 0, 0, one, nullptr}).empty());
  EXPECT(!spin_momentum_site_error<std::uint32_t>(SpinMomentumSiteArgs{33, 4, 1, 0, 0, 0, one, nullptr}).empty());
  EXPECT(spin_momentum_site_error<std::uint64_t>(SpinMomentumSiteArgs{33, 4, 1, 0, 0, 0, one, nullptr}).empty());
  EXPECT(!spin_momentum_site_error<std::uint64_t>(SpinMomentumSiteArgs{8, 4, 1, 0, 3, 0, one, nullptr}).empty());
  EXPECT(!spin_momentum_site_error<std::uint64_t>(SpinMomentumSiteArgs{8, 4, 1, 0, 0, 8, one, nullptr}).empty());
  EXPECT(!spin_momentum_site_error<std::uint64_t>(SpinMomentumSiteArgs{8, 4, 1, 0, 0, -1, one, nullptr}).empty());
  EXPECT(!spin_momentum_site_error<std::uint64_t>(SpinMomentumSiteArgs{8, 4, 2, 0, 0, 0, bad, nullptr}).empty());
  EXPECT(!spin_momentum_site_error<std::uint64_t>(SpinMomentumSiteArgs{8, 4, 2, 0, 0, 0, one, bad}).empty());
  EXPECT(!spin_momentum_site_error<std::uint64_t>(SpinMomentumSiteArgs{8, 4, 1, 0, 0, 0, nullptr, nullptr}).empty());
  EXPECT(!spin_momentum_site_error<std::uint64_t>(SpinMomentumSiteArgs{8, 8, 1, 0, 1, 0, one, nullptr}).empty());
  EXPECT(!spin_momentum_site_error<std::uint64_t>(SpinMomentumSiteArgs{8, 0, 1, 0, 2, 0, one, nullptr}).empty());
}

int main(int argc, char** argv) {
  const bool wide = argc > 1 && std::strcmp(argv[1], "64") == 0;
  check_refusals();
  if (!wide) {
    const int shapes[][3] = {{2, 1, 1}, {8, 4, 1}, {8, 4, 2}, {12, 5, 2}, {12, 6, 3}, {16, 8, 1}, {20, 3, 1}, {31, 2, 1}, {32, 3, 1}, {32, 30, 2}};
    for (const auto& s : shapes) run_shape<std::uint32_t>(s[0], s[1], s[2], false);
  } else {
    const int shapes[][3] = {{8, 4, 1}, {12, 5, 2}, {16, 6, 1}, {32, 3, 1}, {33, 3, 1}, {36, 3, 1}, {36, 4, 2}, {48, 3, 1}};
    for (const auto& s : shapes) run_shape<std::uint64_t>(s[0], s[1], s[2], true);
    std::printf("words agree on %ld calls\n", agreed);
  }
  std::printf("%ld calls\n", calls);
  if (fails || calls < 100) {
    std::printf("SPIN MOMENTUM SITE FAILED: %d\n", fails);
    return 1;
  }
  std::printf("SPIN MOMENTUM SITE OK\n");
  return 0;
}
