// csrc/spin_momentum.hpp and the momentum part of csrc/spin_rows.hpp under AddressSanitizer + UBSan, stand-alone (no library, no GPU):
//   g++ -std=c++11 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I cmpt-eigenex_amd/csrc spin_momentum_sanitize.cpp
// For every shape: the basis, its buckets and the search's trip count; then the row walk of k_spin_momentum_spmv<E> -- the
// kernel's own functions on the real tables, every load bounds-checked -- whose sum per row must equal, bit for bit, the sum over
// the entries spin_momentum_write_rows wrote for that row (written into exactly-sized arrays), added the way k_spmv / k_spmv_z
// add them; and the walk of k_spin_momentum_expand<E> against spin_momentum_expand_host, bit for bit.  32 sites are among the
// shapes, so that UBSan sees every shift of the rotation.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "spin_momentum.hpp"
#include "spin_rows_checked.hpp"

using namespace eigenex;

struct CheckedLookup {
  const SpinMomentumBasis* b;
  std::uint32_t reps(std::uint32_t i) const { return b->reps.at(i); }
  std::uint32_t bucket(std::uint32_t i) const { return b->bucket.at(i); }
};
struct CheckedMomentumTables {
  const SpinMomentumTables* t;
  double ratio(int i) const {
    EXPECT(i >= 0 && i < kMomentumRatioPitch * kMomentumRatioPitch);
    return t->ratio[i];
  }
  double inv_sqrt(int i) const {
    EXPECT(i >= 1 && i < kMomentumRatioPitch);
    return t->inv_sqrt[i];
  }
  double phase_re(int i) const {
    EXPECT(i >= 0 && i < kMomentumMaxPeriod);
    return t->phase_re[i];
  }
  double phase_im(int i) const {
    EXPECT(i >= 0 && i < kMomentumMaxPeriod);
    return t->phase_im[i];
  }
};
struct CheckedVectorZ {
  const std::vector<double>* x;  // interleaved
  SpinZ operator()(std::uint32_t i) const { return SpinZ{x->at(2 * (std::size_t)i), x->at(2 * (std::size_t)i + 1)}; }
};

static double element_of(const CheckedVector& x, std::uint32_t i) { return x(i); }
static SpinZ element_of(const CheckedVectorZ& x, std::uint32_t i) { return x(i); }
static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }
static bool same(SpinZ a, SpinZ b) { return same(a.re, b.re) && same(a.im, b.im); }

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

// the row walk of k_spin_momentum_spmv<E> on row r, before the shift
template <class E, class Vector>
static E walk_row(const SpinMomentumView& v, const SpinMomentumBasis& b, const Vector& xs, std::int64_t r, double scale) {
  const CheckedLookup lk{&b};
  const CheckedMomentumTables tb{&v.tab};
  const SpinOperatorView& m = v.model;
  const std::uint32_t s = lk.reps((std::uint32_t)r);
  const int period = spin_orbit(s, m.n_sites, v.cell, v.n_trans).period;
  EXPECT(period == b.period.at((std::size_t)r));
  const double d = spin_row_diagonal(m.dmask, m.dval, m.ndiag, s);
  E yr = spin_momentum_add(E{}, SpinZ{d, 0.0}, element_of(xs, (std::uint32_t)r), scale);
  for (int t0 = 0; t0 < m.nflip; t0 += kSpinBatch) {
    EXPECT(t0 + kSpinBatch <= kSpinMaxTerms);
    bool on[kSpinBatch];
    std::uint32_t column[kSpinBatch];
    int ri[kSpinBatch], li[kSpinBatch];
    E xv[kSpinBatch];
    spin_momentum_targets(m.fmask + t0, s, period, m.n_sites, v.cell, v.n_trans, v.compatible, v.h, v.steps, lk, on, column, ri, li);
    for (int t = 0; t < kSpinBatch; ++t) {
      if (!on[t]) EXPECT(column[t] == (std::uint32_t)r);  // a lane without the term reads its own element
      if (m.fmask[t0 + t] == 0) EXPECT(!on[t]);
      EXPECT(li[t] >= 0 && li[t] < v.n_trans);
    }
    spin_momentum_gather(xs, column, xv);
    yr = spin_momentum_add_flips(yr, m.fval + t0, tb, on, ri, li, xv, scale);
  }
  return yr;
}

// the sum over the stored entries of one row as k_spmv (val.re) and k_spmv_z add them
static double csr_row(const std::int32_t* col, const double* val, std::int64_t p0, std::int64_t p1, const CheckedVector& x, double scale) {
  double sum = 0.0;
  for (std::int64_t p = p0; p < p1; ++p) sum = add_product_nofma(sum, val[2 * p], x((std::uint32_t)col[p]) * scale);
  return sum;
}
static SpinZ csr_row(const std::int32_t* col, const double* val, std::int64_t p0, std::int64_t p1, const CheckedVectorZ& x, double scale) {
  SpinZ sum = {0.0, 0.0};
  for (std::int64_t p = p0; p < p1; ++p) {
    const SpinZ xv = x((std::uint32_t)col[p]);
    const double xr = xv.re * scale, xi = xv.im * scale;
    const double a = val[2 * p] * xr, bb = val[2 * p + 1] * xi, c = val[2 * p] * xi, d = val[2 * p + 1] * xr;
    const double pr = a - bb, pi = c + d;
    sum.re = sum.re + pr;
    sum.im = sum.im + pi;
  }
  return sum;
}

struct Model {
  int n_sites;
  std::vector<std::int32_t> si, sj;
  std::vector<double> jz, jxy, hz;
  SpinModelArgs args() const {
    return SpinModelArgs{n_sites, (int)si.size(), si.data(), sj.data(), jz.data(), jxy.data(), hz.empty() ? nullptr : hz.data(), nullptr};
  }
};
// a ring invariant under the translation by `cell` sites: nearest neighbours and, with `far`, bonds of that reach, couplings and hz by place in the cell
static Model ring(int L, int cell, int far) {
  Model m;
  m.n_sites = L;
  for (int i = 0; i < L; ++i) {
    const int p = i % cell;
    if (!(L == 2 && i == 1)) m.si.push_back(i), m.sj.push_back((i + 1) % L), m.jz.push_back(0.7 + 0.25 * p), m.jxy.push_back(1.1 + 0.125 * p);
    if (far > 1) m.si.push_back((i + far) % L), m.sj.push_back(i), m.jz.push_back(0.3 - 0.05 * p), m.jxy.push_back(p == 1 ? 0.0 : 0.2 + 0.0625 * p);
  }
  if (cell > 1)
    for (int i = 0; i < L; ++i) m.hz.push_back(0.1 * (1 + i % cell));
  return m;
}

template <class E, class Vector>
static void check_rows(const SpinModelArgs& a, const SpinMomentumView& v, const SpinMomentumBasis& b, const std::vector<double>& x, double scale) {
  const std::int64_t dim = (std::int64_t)b.reps.size();
  const std::int64_t begin = dim > 3 ? 1 : 0, n_rows = dim - begin;  // a range from the middle
  std::vector<std::int64_t> rowptr((std::size_t)n_rows + 1);
  std::int64_t nnz = 0, again = 0;
  spin_momentum_write_rows(a, b, v.tab, begin, n_rows, rowptr.data(), nullptr, nullptr, &nnz);
  std::vector<std::int32_t> col((std::size_t)nnz);
  std::vector<double> val((std::size_t)(2 * nnz));  // exactly sized: a write behind the count is a heap overflow
  spin_momentum_write_rows(a, b, v.tab, begin, n_rows, rowptr.data(), col.data(), val.data(), &again);
  EXPECT(again == nnz && rowptr.back() == nnz);
  const Vector xs{&x};
  for (std::int64_t k = 0; k < n_rows; ++k) {
    for (std::int64_t p = rowptr[(std::size_t)k]; p < rowptr[(std::size_t)k + 1]; ++p) EXPECT(col[(std::size_t)p] >= 0 && col[(std::size_t)p] < dim);
    EXPECT(col[(std::size_t)rowptr[(std::size_t)k]] == begin + k);  // the diagonal first
    const E walked = walk_row<E>(v, b, xs, begin + k, scale);
    const E stored = csr_row(col.data(), val.data(), rowptr[(std::size_t)k], rowptr[(std::size_t)k + 1], xs, scale);
    EXPECT(same(walked, stored));
  }
  if (spin_momentum_is_real(b.n_trans, b.momentum))
    for (std::int64_t p = 0; p < nnz; ++p) EXPECT(same(val[(std::size_t)(2 * p + 1)], 0.0));
}

template <class E, class Vector>
static void check_expand(const SpinMomentumView& v, const SpinMomentumBasis& b, const std::vector<double>& x, bool is_complex) {
  const int L = b.n_sites, es = is_complex ? 2 : 1;
  const std::int64_t n = spin_sector_dim(L, b.n_up);
  std::vector<double> y((std::size_t)(n * es));  // exactly sized
  spin_momentum_expand_host(b, v.tab, is_complex, x.data(), y.data());
  std::unique_ptr<SpinSectorView> sv(new SpinSectorView());
  Model none = ring(L, 1, 0);
  spin_sector_build_view(none.args(), b.n_up, *sv);
  const CheckedBinomials bin(*sv);
  const CheckedLookup lk{&b};
  const CheckedMomentumTables tb{&v.tab};
  const Vector xs{&x};
  double n2x = 0.0, n2y = 0.0;
  for (double e : x) n2x += e * e;
  for (std::int64_t r = 0; r < n; ++r) {
    const std::uint32_t s = spin_unrank_row(bin, L, b.n_up, (std::uint32_t)r).s;
    EXPECT(s == spin_sector_unrank(L, b.n_up, r));
    const E yr = spin_momentum_expand_row(s, L, v.cell, v.n_trans, v.compatible, v.first_rep, v.h, v.steps, lk, tb, xs, E{});
    E host;
    std::memcpy(&host, &y[(std::size_t)(r * es)], sizeof(E));
    EXPECT(same(yr, host));
    n2y = spin_norm_add(n2y, yr);
  }
  EXPECT(std::fabs(n2y - n2x) <= 1e-12 * n2x);  // expand preserves the norm
}

static void check_shape(int L, int n_up, int cell, int far) {
  const int N = L / cell;
  const Model model = ring(L, cell, far);
  const SpinModelArgs a = model.args();
  EXPECT(spin_momentum_model_error(a, n_up, cell).empty());
  std::int64_t total = 0;
  for (int m = 0; m < N; ++m) {
    EXPECT(spin_momentum_geometry_error(L, n_up, cell, m).empty());
    if (N > 13 && !(m <= 1 || m == N / 2 || m == N - 1)) {  // the dimensions of all, the walks of four
      total += spin_momentum_build_basis(L, n_up, cell, m, nullptr);
      continue;
    }
    SpinMomentumBasis b;
    const std::int64_t dim = spin_momentum_build_basis(L, n_up, cell, m, &b);
    EXPECT(dim == (std::int64_t)b.reps.size() && dim == spin_momentum_build_basis(L, n_up, cell, m, nullptr));
    total += dim;
    if (dim == 0) continue;
    EXPECT(b.bucket.size() == (std::size_t(1) << (L - b.h)) + 1 && b.bucket.front() == 0 && b.bucket.back() == dim);
    std::size_t largest = 0;
    for (std::size_t i = 0; i + 1 < b.bucket.size(); ++i) largest = std::max(largest, (std::size_t)(b.bucket[i + 1] - b.bucket[i]));
    EXPECT((std::size_t(1) << b.steps) >= largest + 1 && (b.steps == 0 || (std::size_t(1) << (b.steps - 1)) < largest + 1));
    const CheckedLookup lk{&b};
    for (std::int64_t r = 0; r < dim; ++r) {
      if (r > 0) EXPECT(b.reps[(std::size_t)r - 1] < b.reps[(std::size_t)r]);
      EXPECT(spin_momentum_index(lk, b.reps[(std::size_t)r], b.h, b.steps) == (std::uint32_t)r);
      const SpinMomentumOrbit o = spin_momentum_orbit_host(b.reps[(std::size_t)r], L, cell);
      const SpinOrbit w = spin_orbit(b.reps[(std::size_t)r], L, cell, N);
      EXPECT(o.rep == b.reps[(std::size_t)r] && o.j == 0 && o.period == b.period[(std::size_t)r] && N % o.period == 0);
      EXPECT(w.rep == o.rep && w.j == o.j && w.period == o.period);
    }
    std::unique_ptr<SpinMomentumView> v(new SpinMomentumView());
    spin_momentum_build_view(a, b, *v);
    EXPECT(v->first_rep == b.reps[0]);
    const std::vector<double> xz = test_vector((std::size_t)(2 * dim), 17 + (std::uint64_t)m);
    check_rows<SpinZ, CheckedVectorZ>(a, *v, b, xz, 1.0);
    check_rows<SpinZ, CheckedVectorZ>(a, *v, b, xz, -0.37);
    check_expand<SpinZ, CheckedVectorZ>(*v, b, xz, true);
    if (spin_momentum_is_real(N, m)) {
      const std::vector<double> x = test_vector((std::size_t)dim, 5 + (std::uint64_t)m);
      check_rows<double, CheckedVector>(a, *v, b, x, 1.0);
      check_rows<double, CheckedVector>(a, *v, b, x, 1.7);
      check_expand<double, CheckedVector>(*v, b, x, false);
    }
  }
  EXPECT(total == spin_sector_dim(L, n_up));  // the momentum sectors tile the Sz sector
}

int main() {
  // every state's orbit by the kernel's walk against the definition's, on a ring where every period occurs
  for (std::uint32_t s = 0; s < (1u << 12); ++s)
    for (int cell = 1; cell <= 6; ++cell) {
      if (12 % cell) continue;
      const SpinMomentumOrbit o = spin_momentum_orbit_host(s, 12, cell);
      const SpinOrbit w = spin_orbit(s, 12, cell, 12 / cell);
      EXPECT(w.rep == o.rep && w.j == o.j && w.period == o.period);
    }
  EXPECT(spin_momentum_translate(0x80000001u, 32, 1) == 0x00000003u && spin_momentum_translate(0xffff0000u, 32, 16) == 0x0000ffffu);
  const int shapes[][4] = {{2, 1, 1, 0},  {4, 2, 1, 0},  {6, 0, 1, 0},  {6, 6, 1, 0},  {6, 3, 3, 2},  {8, 4, 1, 0},  {8, 4, 2, 3},   {8, 3, 2, 3},
                           {9, 4, 1, 0},  {12, 6, 1, 2}, {12, 6, 2, 5}, {12, 4, 3, 5}, {13, 6, 1, 0}, {16, 8, 1, 0}, {31, 2, 1, 0},  {32, 2, 1, 0},
                           {32, 3, 1, 0}, {32, 31, 1, 0}, {32, 2, 16, 0}, {32, 3, 2, 15}};
  for (const auto& s : shapes) check_shape(s[0], s[1], s[2], s[3]);
  // refusals
  {
    const Model open = [] {
      Model m = ring(8, 1, 0);
      m.si.pop_back(), m.sj.pop_back(), m.jz.pop_back(), m.jxy.pop_back();
      return m;
    }();
    EXPECT(spin_momentum_model_error(open.args(), 4, 1).find("bond") != std::string::npos);
    Model altered = ring(8, 1, 0);
    altered.jxy[3] = 1.25;
    EXPECT(spin_momentum_model_error(altered.args(), 4, 1).find("bond 2") != std::string::npos);  // whose image, bond 3, differs
    Model field = ring(8, 2, 0);
    field.hz[5] = 0.5;
    EXPECT(spin_momentum_model_error(field.args(), 4, 2).find("hz at site 3") != std::string::npos);
    EXPECT(!spin_momentum_geometry_error(8, 4, 3, 0).empty() && !spin_momentum_geometry_error(8, 4, 8, 0).empty() &&
           !spin_momentum_geometry_error(8, 4, 1, 8).empty() && !spin_momentum_geometry_error(8, 4, 1, -1).empty() &&
           !spin_momentum_geometry_error(33, 4, 1, 0).empty() && !spin_momentum_geometry_error(8, 9, 1, 0).empty());
    EXPECT(spin_momentum_build_basis(6, 0, 1, 1, nullptr) == 0 && spin_momentum_build_basis(31, 2, 1, 7, nullptr) == 15);
  }
  if (fails) {
    std::fprintf(stderr, "%d check(s) failed\n", fails);
    return 1;
  }
  std::printf("SPIN MOMENTUM OK\n");
  return 0;
}
