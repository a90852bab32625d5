// Host code of the reduced density matrix of a COMPLEX vector under AddressSanitizer + UBSan (device code cannot be sanitised
// on the GPU pool): csrc/spin_rdm.hpp -- the argument check, the layout, the work table and spin_rdm_host_z -- compiled into this
// program, which links nothing else.  Over the shapes of tests/test_gpu_spin_rdm_z.py and three launch grids it replays
// k_spin_rdm<SECTOR, TILE, SpinZ> and k_spin_rdm_reduce<SpinZ> on an interleaved vector (spin_rdm_replay.hpp has the replay and
// what it checks on the way: the panels of CHUNK x (TILE + 1) pairs among it) and checks that the diagonal's imaginary part is
// +0.0 and (j, i) the conjugate of (i, j) bit for bit, and that the result equals spin_rdm_host_z within twice the bound
// 2 n_b eps (|Mr||Mr|^T + |Mi||Mi|^T) resp. 2 n_b eps (|Mi||Mr|^T + |Mr||Mi|^T): each side is within that bound of the true sum
// of 2 n_b products, whatever the grouping.  The plan is spin_rdm_build_plan's, the real call's.
// Built and run by tests/test_spin_rdm_z_host.py; prints SPIN RDM Z OK and exits 0 when every check holds.
#include <cfloat>
#include <cstring>

#include "spin_rdm_replay.hpp"

static void check_shape(int L, int n_up, std::uint32_t mask_a, std::mt19937& rng) {
  const SpinRdmArgs a{L, n_up, mask_a};
  EXPECT(eigenex::spin_rdm_error(a) == nullptr);
  eigenex::SpinRdmLayout l;
  eigenex::spin_rdm_layout(a, l);
  const std::int64_t n = n_up != -1 ? eigenex::spin_sector_dim(L, n_up) : std::int64_t(1) << L;
  std::vector<double> x(static_cast<std::size_t>(2 * n)), ax(x.size());
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  for (std::size_t i = 0; i < x.size(); ++i) x[i] = u(rng), ax[i] = std::fabs(x[i]);
  // the magnitudes of the bound from the real definition on a = |Re x|, b = |Im x| and a + b:
  // |Mr||Mr|^T, |Mi||Mi|^T, and (|Mr| + |Mi|)(|Mr| + |Mi|)^T minus the two = |Mr||Mi|^T + |Mi||Mr|^T
  std::vector<double> ar(static_cast<std::size_t>(n)), ai(ar.size()), sum(ar.size());
  for (std::size_t r = 0; r < ar.size(); ++r) ar[r] = ax[2 * r], ai[r] = ax[2 * r + 1], sum[r] = ar[r] + ai[r];
  const std::size_t total = static_cast<std::size_t>(l.offsets[l.n_blocks]);
  std::vector<double> host_out(2 * total, -1.0);  // exactly sized: one entry too many is a heap overflow
  std::vector<double> mag_rr(total, -1.0), mag_ii(total, -1.0), mag_ss(total, -1.0);
  eigenex::spin_rdm_host_z(a, x.data(), host_out.data());
  const std::vector<double>& host = host_out;
  eigenex::spin_rdm_host(a, ar.data(), mag_rr.data());
  eigenex::spin_rdm_host(a, ai.data(), mag_ii.data());
  eigenex::spin_rdm_host(a, sum.data(), mag_ss.data());
  double trace = 0.0, norm2 = 0.0;
  for (int b = 0; b < l.n_blocks; ++b)
    for (std::int64_t i = 0; i < l.dims[b]; ++i) trace += host[2 * static_cast<std::size_t>(l.offsets[b] + i + i * l.dims[b])];
  for (double e : x) norm2 += e * e;
  EXPECT(std::fabs(trace - norm2) <= 1e-12 * norm2);
  replay_grids<SpinZ>(a, l, x, [&](const std::vector<double>& out) {
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
  });
}

int main() {
  std::mt19937 rng(29);
  for_every_shape([&](int L, int n_up, std::uint32_t mask_a) { check_shape(L, n_up, mask_a, rng); });
  if (fails) return 1;
  std::printf("SPIN RDM Z OK\n");
  return 0;
}
