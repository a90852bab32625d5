// C++11 user program: the ground state of the periodic spin-1/2 Heisenberg chain (L sites, default 12) in the sector of n_up
// sites up (default L/2) through LanczosEigenSolver<double>, once with the matrix-free sector operator
// (device::spinHalfSectorOperator) and once with the stored CSR of the same sector (SpinHalfModel::toSectorCsr) in the same
// program.  Prints JSON: both energies, the true residual |H x - E x|_2 of the matrix-free solver's vector, taken on the host
// from the CSR rows, and the first and last state of the sector.  tests/test_gpu_spin_sector.py reads it.
// usage: spin_sector_amd [L [n_up]]
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
  const int nUp = argc > 2 ? std::atoi(argv[2]) : L / 2;
  using Solver = LanczosEigenSolver<double>;
  try {
    const SpinHalfModel model = SpinHalfModel::chain(L, 1.0, 1.0, true);
    const HostCsr<double> csr = model.toSectorCsr(nUp);
    const Index n = model.sectorRows(nUp);
    const std::vector<std::uint32_t> states = model.sectorStates(nUp);
    std::shared_ptr<device::Context> ctx = std::make_shared<device::Context>(0);
    double energy[2] = {0.0, 0.0}, residual = 0.0, norm = 0.0;
    long iterations[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
      std::shared_ptr<device::CsrOperator> op =
          pass == 0 ? device::spinHalfSectorOperator(ctx, model, nUp)
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
    std::printf("{\"sites\": %d, \"n_up\": %d, \"rows\": %ld, \"stored_entries\": %ld, \"first_state\": %lu, \"last_state\": %lu, "
                "\"energy_matrix_free\": %.17g, \"energy_csr\": %.17g, \"iterations\": [%ld, %ld], \"residual\": %.6g, \"norm\": %.17g}\n",
                L, nUp, static_cast<long>(n), static_cast<long>(csr.col.size()), static_cast<unsigned long>(states.front()),
                static_cast<unsigned long>(states.back()), energy[0], energy[1], iterations[0], iterations[1], std::sqrt(residual),
                std::sqrt(norm));
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\"}\n", e.what());
    return 1;
  }
  return 0;
}
