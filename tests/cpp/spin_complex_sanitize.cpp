// The row walk of the complex-state spin kernels under AddressSanitizer + UBSan (device code cannot be sanitised on the GPU pool):
// csrc/spin_rows.hpp's functions on complex elements (SpinZ: spin_gather, spin_add_flips, spin_measure_flips,
// spin_measure_diagonals and the element helpers) and csrc/spin_measure.hpp's spin_measure_host_z, compiled into this program,
// which links nothing else.
// For the sectors (4,2), (11,5), (32,2), (31,2) and the full space of L = 2 and 9 sites, on models with bonds across the split of
// the rank tables and on the top sites, longitudinal fields and (full space) a transverse field:
//   - the row sum of k_spin_spmv<SECTOR, SpinZ> -- the kernel's own functions on its tables, every load checked against its array, an
//     element read as the (re, im) pair at 2 i and 2 i + 1 of an exactly-sized interleaved vector -- equals, part by part and bit
//     for bit, the real walk (checked_operator_row, the row sum of k_spin_spmv<SECTOR, double>) on the vector of real parts and on the vector of
//     imaginary parts;
//   - the row loop of k_spin_measure<SECTOR, SpinZ> over ascending rows equals spin_measure_host_z bit for bit, and with every imaginary part
//     +0 both equal spin_measure_host.
// Built and run by tests/test_spin_complex_host.py; prints SPIN COMPLEX OK and exits 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "spin_measure.hpp"
#include "spin_model.hpp"
#include "spin_rows_checked.hpp"
#include "spin_sector.hpp"

using eigenex::SpinMeasureArgs;
using eigenex::SpinMeasureChunk;
using eigenex::SpinZ;

struct CheckedVectorZ {  // interleaved (re, im)
  const std::vector<double>* x;
  SpinZ operator()(std::uint32_t i) const { return SpinZ{x->at(2 * static_cast<std::size_t>(i)), x->at(2 * static_cast<std::size_t>(i) + 1)}; }
};

struct Model {
  int L;
  std::vector<std::int32_t> si, sj;
  std::vector<double> jz, jxy, hz, hx;
  eigenex::SpinModelArgs args() const {
    return eigenex::SpinModelArgs{L, static_cast<int>(si.size()), si.data(), sj.data(), jz.data(), jxy.data(), hz.empty() ? nullptr : hz.data(),
                                  hx.empty() ? nullptr : hx.data()};
  }
};

static Model model_of(int L, bool sector, std::mt19937& rng) {
  std::uniform_real_distribution<double> u(-1.5, 1.5);
  Model m;
  m.L = L;
  for (int i = 0; i + 1 < L; ++i) m.si.push_back(i), m.sj.push_back(i + 1), m.jz.push_back(1.0), m.jxy.push_back(0.7);
  if (L > 2) {
    m.si.push_back(L - 1), m.sj.push_back(0), m.jz.push_back(0.4), m.jxy.push_back(-1.3);  // the top site
    m.si.push_back(L / 2 - 1), m.sj.push_back(L / 2 + 1), m.jz.push_back(0.3), m.jxy.push_back(0.6);  // across the split
    for (int b = 0; b < 9; ++b) {
      const int i = static_cast<int>(rng() % L), j = (i + 1 + static_cast<int>(rng() % (L - 1))) % L;
      m.si.push_back(i), m.sj.push_back(j), m.jz.push_back(b % 5 == 4 ? 0.0 : u(rng)), m.jxy.push_back(b % 3 == 2 ? 0.0 : u(rng));
    }
  }
  for (int i = 0; i < L; ++i) m.hz.push_back(u(rng));
  if (!sector)
    for (int i = 0; i < L; ++i) m.hx.push_back(i % 2 ? u(rng) : 0.0);
  return m;
}

static void check_operator(int L, int n_up, std::mt19937& rng) {
  const bool sector = n_up != -1;
  const Model mod = model_of(L, sector, rng);
  const eigenex::SpinModelArgs a = mod.args();
  EXPECT((sector ? eigenex::spin_sector_error(a, n_up) : eigenex::spin_model_error(a)) == nullptr);
  const std::int64_t n = sector ? eigenex::spin_sector_dim(L, n_up) : std::int64_t(1) << L;
  std::unique_ptr<eigenex::SpinSectorView> v(new eigenex::SpinSectorView());
  eigenex::SpinSectorTables t;
  if (sector) {
    eigenex::spin_sector_build_view(a, n_up, *v);
    eigenex::spin_sector_build_tables(L, n_up, t);
  } else {
    eigenex::spin_build_view(a, v->model);
  }
  const CheckedBinomials binom(*v);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  std::vector<double> xz(2 * static_cast<std::size_t>(n)), re(static_cast<std::size_t>(n)), im(static_cast<std::size_t>(n));  // exactly sized
  for (std::int64_t r = 0; r < n; ++r) {
    re[static_cast<std::size_t>(r)] = xz[2 * static_cast<std::size_t>(r)] = u(rng);
    im[static_cast<std::size_t>(r)] = xz[2 * static_cast<std::size_t>(r) + 1] = u(rng);
  }
  for (double scale : {1.0, 0.73})
    for (std::int64_t r = 0; r < n; ++r) {
      std::uint32_t s = static_cast<std::uint32_t>(r);
      if (sector) {
        const eigenex::SpinUnranked un = eigenex::spin_unrank_row(binom, L, n_up, s);
        EXPECT(un.left == 0 && un.k == 0);
        s = un.s;
      }
      SpinZ z;
      double wr, wi;
      if (sector) {
        z = checked_operator_row_of<true, SpinZ>(v->model, t, v->h, v->lo_mask, CheckedVectorZ{&xz}, r, s, scale);
        wr = checked_operator_row<true>(v->model, t, v->h, v->lo_mask, re, r, s, scale);
        wi = checked_operator_row<true>(v->model, t, v->h, v->lo_mask, im, r, s, scale);
      } else {
        z = checked_operator_row_of<false, SpinZ>(v->model, t, 0, 0u, CheckedVectorZ{&xz}, r, s, scale);
        wr = checked_operator_row<false>(v->model, t, 0, 0u, re, r, s, scale);
        wi = checked_operator_row<false>(v->model, t, 0, 0u, im, r, s, scale);
      }
      EXPECT(std::memcmp(&z.re, &wr, sizeof(double)) == 0 && std::memcmp(&z.im, &wi, sizeof(double)) == 0);
    }
}

// k_spin_measure<SECTOR, SpinZ> (kernels.hip) over ascending rows, by the kernel's own functions: one chunk per pass, every load checked
static void replay_z(const SpinMeasureArgs& a, const std::vector<double>& xz, std::vector<double>& diag, std::vector<double>& flip, double* norm2) {
  const int C = eigenex::kSpinMeasureChunk, B = eigenex::kSpinBatch;
  const bool sector = a.n_up != -1;
  const std::int64_t n = eigenex::spin_measure_rows(a);
  EXPECT(static_cast<std::int64_t>(xz.size()) == 2 * n);
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
  const CheckedVectorZ xs_at{&xz};
  diag.assign(static_cast<std::size_t>(a.n_diag), 0.0);
  flip.assign(static_cast<std::size_t>(a.n_flip), 0.0);
  for (std::size_t k = 0; k < chunks.size(); ++k) {
    const SpinMeasureChunk& ch = chunks[k];
    double nrm = 0.0, dg[eigenex::kSpinMeasureChunk] = {0.0}, fl[eigenex::kSpinMeasureChunk] = {0.0};
    for (std::int64_t r = 0; r < n; ++r) {
      std::uint32_t s = static_cast<std::uint32_t>(r);
      if (sector) s = eigenex::spin_unrank_row(binom, v->model.n_sites, v->n_up, s).s;
      const SpinZ xs = xs_at(static_cast<std::uint32_t>(r));
      nrm = eigenex::spin_norm_add(nrm, xs);
      for (int t0 = 0; t0 < C; t0 += B)
        if (t0 < ch.ndiag) eigenex::spin_measure_diagonals(xs, s, ch.dmask + t0, dg + t0);
      for (int t0 = 0; t0 < C; t0 += B)
        if (t0 < ch.nflip) {
          bool on[eigenex::kSpinBatch];
          std::uint32_t base[eigenex::kSpinBatch], low[eigenex::kSpinBatch];
          SpinZ xv[eigenex::kSpinBatch];
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
}

static void check_measure(int L, int n_up, std::mt19937& rng) {
  const bool sector = n_up != -1;
  std::vector<std::uint32_t> dmask, fmask;
  for (int i = 0; i < L; ++i) dmask.push_back(std::uint32_t(1) << i);
  for (int i = 0; i < L; ++i)
    for (int j = i + 1; j < L; ++j) fmask.push_back((std::uint32_t(1) << i) | (std::uint32_t(1) << j));
  dmask.insert(dmask.end(), fmask.begin(), fmask.end());
  dmask.push_back(L == 32 ? 0xFFFFFFFFu : (std::uint32_t(1) << L) - 1);
  if (!sector)
    for (int i = 0; i < L; ++i) fmask.push_back(std::uint32_t(1) << i);
  const SpinMeasureArgs a{L, n_up, static_cast<int>(dmask.size()), dmask.data(), static_cast<int>(fmask.size()), fmask.data()};
  EXPECT(eigenex::spin_measure_error(a) == nullptr);
  const std::int64_t n = eigenex::spin_measure_rows(a);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  std::vector<double> xz(2 * static_cast<std::size_t>(n)), re(static_cast<std::size_t>(n));
  for (auto& e : xz) e = u(rng);
  for (int pass = 0; pass < 2; ++pass) {  // 0: a complex vector; 1: imaginary parts +0
    if (pass == 1)
      for (std::int64_t r = 0; r < n; ++r) re[static_cast<std::size_t>(r)] = xz[2 * static_cast<std::size_t>(r)], xz[2 * static_cast<std::size_t>(r) + 1] = 0.0;
    std::vector<double> hd(dmask.size(), -7.0), hf(fmask.size(), -7.0), kd, kf;  // exactly sized
    double hn = -7.0, kn = -7.0;
    eigenex::spin_measure_host_z(a, xz.data(), hd.data(), hf.data(), &hn);
    replay_z(a, xz, kd, kf, &kn);
    EXPECT(same_bits(hd, kd) && same_bits(hf, kf) && std::memcmp(&hn, &kn, sizeof(double)) == 0);
    if (pass == 1) {
      std::vector<double> rd(dmask.size(), -7.0), rf(fmask.size(), -7.0);
      double rn = -7.0;
      eigenex::spin_measure_host(a, re.data(), rd.data(), rf.data(), &rn);
      EXPECT(same_bits(hd, rd) && same_bits(hf, rf) && std::memcmp(&hn, &rn, sizeof(double)) == 0);
    }
  }
}

int main() {
  std::mt19937 rng(11);
  const int shapes[6][2] = {{4, 2}, {11, 5}, {32, 2}, {31, 2}, {2, -1}, {9, -1}};
  for (const auto& sh : shapes) {
    check_operator(sh[0], sh[1], rng);
    check_measure(sh[0], sh[1], rng);
  }
  if (fails) return 1;
  std::printf("SPIN COMPLEX OK\n");
  return 0;
}
