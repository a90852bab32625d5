// Host code of the reduced density matrix under AddressSanitizer + UBSan (device code cannot be sanitised on the GPU pool):
// csrc/spin_rdm.hpp -- the argument check, the layout, the work table and the host evaluation -- compiled into this program,
// which links nothing else.  Over the shapes of tests/test_gpu_spin_rdm.py and three launch grids it replays
// k_spin_rdm<SECTOR, TILE, double> and k_spin_rdm_reduce<double> (spin_rdm_replay.hpp has the replay and what it checks on the
// way) and checks that the result equals spin_rdm_host within 2 n_b eps (|M| |M|^T): each side is within n_b eps (|M| |M|^T) of
// the true sum, whatever the grouping.
// Built and run by tests/test_spin_rdm_host.py; prints SPIN RDM OK and exits 0 when every check holds.
#include <cfloat>
#include <cstring>

#include "spin_rdm_replay.hpp"

static void check_shape(int L, int n_up, std::uint32_t mask_a, std::mt19937& rng) {
  const SpinRdmArgs a{L, n_up, mask_a};
  EXPECT(eigenex::spin_rdm_error(a) == nullptr);
  eigenex::SpinRdmLayout l;
  eigenex::spin_rdm_layout(a, l);
  const std::int64_t n = n_up != -1 ? eigenex::spin_sector_dim(L, n_up) : std::int64_t(1) << L;
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
  replay_grids<double>(a, l, x, [&](const std::vector<double>& out) {
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
  });
}

static bool refused(const SpinRdmArgs& a, const char* word) {
  const char* why = eigenex::spin_rdm_error(a);
  return why != nullptr && std::strstr(why, word) != nullptr;
}

int main() {
  std::mt19937 rng(23);
  for_every_shape([&](int L, int n_up, std::uint32_t mask_a) { check_shape(L, n_up, mask_a, rng); });
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
