// C++11 user program on FilteredLanczosEigenSolver<double>: the eigenpairs of a 1-D Anderson chain (on-site energies read
// from a file, hopping -1) nearest a target energy, with the Gershgorin bounds as the spectral range.
// usage: filtered_lanczos_amd diagonal.txt tau degree m nev.  Prints JSON; tests/test_gpu_filter.py reads it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <vector>

#include "cmpt/eigen_ex/filtered_lanczos.hpp"

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  using namespace cmpt::EigenEx;
  std::vector<double> diag;
  {
    std::ifstream in(argv[1]);
    double x;
    while (in >> x) diag.push_back(x);
  }
  const int n = static_cast<int>(diag.size());
  const double tau = std::atof(argv[2]);
  const int degree = std::atoi(argv[3]), m = std::atoi(argv[4]), nev = std::atoi(argv[5]);
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
  FilteredLanczosEigenSolver<double> es;
  es.setDeviceOperator(op);
  es.setNumberOfEigenvalues(nev);
  es.setMaxBasisSize(m);
  es.setTarget(tau).setFilterDegree(degree);
  es.compute();  // no spectral range yet
  const int invalid = static_cast<int>(es.info());
  es.setSpectralRange(lo, hi);
  es.compute();
  const auto& lam = es.eigenvalues();
  const auto& X = es.eigenvectors();
  std::printf("{\"info\": %d, \"invalid_without_range\": %d, \"restarts\": %d, \"applications\": %ld, \"eigenvalues\": [", static_cast<int>(es.info()), invalid,
              static_cast<int>(es.restarts()), static_cast<long>(es.operatorApplications()));
  for (Index e = 0; e < lam.size(); ++e) std::printf("%s%.17g", e ? ", " : "", lam[e]);
  std::printf("], \"residuals\": [");
  for (Index e = 0; e < lam.size(); ++e) {  // ||A x - lambda x|| formed here, not the solver's own figure
    double r2 = 0.0;
    for (int i = 0; i < n; ++i) {
      double s = diag[static_cast<std::size_t>(i)] * X(i, e) - lam[e] * X(i, e);
      if (i > 0) s -= X(i - 1, e);
      if (i + 1 < n) s -= X(i + 1, e);
      r2 += s * s;
    }
    std::printf("%s%.17g", e ? ", " : "", std::sqrt(r2));
  }
  std::printf("]}\n");
  return 0;
}
