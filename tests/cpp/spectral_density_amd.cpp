// C++11 user program on SpectralDensitySolver<double> and FilteredLanczosEigenSolver<double>: on a 1-D Anderson chain (on-site
// energies read from a file, hopping -1) the density solver says how wide the window around the centre of the spectrum is that
// holds `count` levels; the filtered solver is then asked for exactly that many eigenvalues there.
// usage: spectral_density_amd diagonal.txt moments vectors seed count degree m.  Prints JSON; tests/test_gpu_density.py reads it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <vector>

#include "cmpt/eigen_ex/spectral_density.hpp"

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  using namespace cmpt::EigenEx;
  std::vector<double> diag;
  {
    std::ifstream in(argv[1]);
    double x;
    while (in >> x) diag.push_back(x);
  }
  const int n = static_cast<int>(diag.size());
  const int moments = std::atoi(argv[2]), vectors = std::atoi(argv[3]);
  const std::uint64_t seed = static_cast<std::uint64_t>(std::atoll(argv[4]));
  const int count = std::atoi(argv[5]), degree = std::atoi(argv[6]), m = std::atoi(argv[7]);
  std::vector<std::int32_t> rowptr(1, 0), col;
  std::vector<double> val;
  double lo = 1e300, hi = -1e300;
  for (int i = 0; i < n; ++i) {
    double radius = 0.0;
    if (i > 0) col.push_back(i - 1), val.push_back(-1.0), radius += 1.0;
    col.push_back(i), val.push_back(diag[static_cast<std::size_t>(i)]);
    if (i + 1 < n) col.push_back(i + 1), val.push_back(-1.0), radius += 1.0;
    rowptr.push_back(static_cast<std::int32_t>(col.size()));
    lo = std::min(lo, diag[static_cast<std::size_t>(i)] - radius);
    hi = std::max(hi, diag[static_cast<std::size_t>(i)] + radius);
  }
  auto ctx = std::make_shared<device::Context>(0);
  auto op = std::make_shared<device::CsrOperator>(ctx, n, 0, n, rowptr.data(), col.data(), val.data());
  SpectralDensitySolver<double> sd;
  sd.setDeviceOperator(op).setMoments(moments).setRandomVectors(vectors).setSeed(seed);
  sd.compute();  // no spectral range yet
  const int invalid = static_cast<int>(sd.info());
  sd.setSpectralRange(lo, hi);
  sd.compute();
  const double tau = 0.5 * (lo + hi);
  const double delta = sd.energyWindow(tau, count);
  const double inside = sd.eigenvalueCount(tau - delta, tau + delta), inside_err = sd.eigenvalueCountStandardError(tau - delta, tau + delta);
  sd.continueToCompute();
  const long vectors_after = static_cast<long>(sd.randomVectors());

  FilteredLanczosEigenSolver<double> es;
  es.setDeviceOperator(op);
  es.setNumberOfEigenvalues(count);
  es.setMaxBasisSize(m);
  es.setTarget(tau).setFilterDegree(degree).setSpectralRange(lo, hi);
  es.compute();
  const auto& lam = es.eigenvalues();
  std::printf("{\"info\": %d, \"invalid_without_range\": %d, \"tau\": %.17g, \"delta\": %.17g, \"count_in_window\": %.17g, \"count_error\": %.17g, "
              "\"mu0\": %.17g, \"vectors_after_continue\": %ld, \"applications\": %ld, \"solver_info\": %d, \"eigenvalues\": [",
              static_cast<int>(sd.info()), invalid, tau, delta, inside, inside_err, sd.moments()[0], vectors_after, static_cast<long>(sd.operatorApplications()),
              static_cast<int>(es.info()));
  for (Index e = 0; e < lam.size(); ++e) std::printf("%s%.17g", e ? ", " : "", lam[e]);
  std::printf("]}\n");
  return 0;
}
