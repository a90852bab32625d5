// C++11 user program: the ground state of the periodic spin-1/2 Heisenberg chain (L sites, default 12) through
// LanczosEigenSolver<double>, once with the matrix-free operator (device::spinHalfOperator) and once with the stored CSR of
// the same model (SpinHalfModel::toCsr) in the same program.  Prints JSON: both energies, and the true residual
// |H x - E x|_2 of the matrix-free solver's vector, taken on the host from the CSR rows.  tests/test_gpu_spin_operator.py reads it.
// usage: spin_chain_amd [L]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "cmpt/eigen_ex/lanczos.hpp"
#include "cmpt/eigen_ex/spin_operator.hpp"

using namespace cmpt::EigenEx;

int main(int argc, char** argv) {
  const int L = argc > 1 ? std::atoi(argv[1]) : 12;
  using Solver = LanczosEigenSolver<double>;
  try {
    const SpinHalfModel model = SpinHalfModel::chain(L, 1.0, 1.0, true);
    const HostCsr<double> csr = model.toCsr();
    const Index n = model.rows();
    std::shared_ptr<device::Context> ctx = std::make_shared<device::Context>(0);
    double energy[2] = {0.0, 0.0}, residual = 0.0, norm = 0.0;
    long iterations[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
      std::shared_ptr<device::CsrOperator> op =
          pass == 0 ? device::spinHalfOperator(ctx, model)
                    : std::make_shared<device::CsrOperator>(ctx, n, 0, n, csr.rowptr.data(), csr.col.data(), csr.val.data());
      std::mt19937 random_engine(1);
      Solver es;
      es.setDeviceOperator(op);
      es.setTolerance(1.0e-13);
      es.setMaxIterations(400);
      es.setComputeEigenvectorsOn(true);
      es.setIndicesForConvergence({0});
      es.setInitialVector(es.lanczosBase().makeRandomVector(random_engine, n));
      es.setMaxEigenvalues(1);
      es.compute();
      energy[pass] = es.eigenvalues()[0];
      iterations[pass] = static_cast<long>(es.iterations());
      if (pass == 0) {
        const double* x = es.eigenvectors().colData(0);
        for (Index r = 0; r < n; ++r) {
          double s = 0.0;
          for (std::int32_t p = csr.rowptr[static_cast<std::size_t>(r)]; p < csr.rowptr[static_cast<std::size_t>(r) + 1]; ++p)
            s += csr.val[static_cast<std::size_t>(p)] * x[csr.col[static_cast<std::size_t>(p)]];
          const double d = s - energy[0] * x[r];
          residual += d * d;
          norm += x[r] * x[r];
        }
      }
    }
    std::printf("{\"sites\": %d, \"rows\": %ld, \"stored_entries\": %ld, \"energy_matrix_free\": %.17g, \"energy_csr\": %.17g, "
                "\"iterations\": [%ld, %ld], \"residual\": %.6g, \"norm\": %.17g}\n",
                L, static_cast<long>(n), static_cast<long>(csr.col.size()), energy[0], energy[1], iterations[0], iterations[1],
                std::sqrt(residual), std::sqrt(norm));
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\"}\n", e.what());
    return 1;
  }
  return 0;
}
