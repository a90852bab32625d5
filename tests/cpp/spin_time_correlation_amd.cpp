// C++11 user program: SpinTimeCorrelationSolver.  (1) Two sites, Heisenberg J, from |up down> in the sector (2,1), A = B = Sz_0:
// <Sz_0(t) Sz_0(0)> = cos(J t) / 4; the Krylov space is the whole sector, so every step is exact and the bound is 0.  (2) The
// Neel state of the open XXZ chain of 10 sites in (10,5), B = S-_4, A_j = S-_j for every site: four calls of evolve(0.25) at
// m = 12, tol = 1e-9.  Prints JSON: the largest deviation and bound of (1); of (2) the values at t = 0 and t = 1 (site 4), the
// sum of |C_j(0)| over the other sites, <B^dagger B>, the bounds, the sub-steps and the operator applications; and whether no
// model, no source operator, a state of the wrong length, a short coefficient list and an operator that leaves the sectors end in
// InvalidInput with an ERROR line in the log.  Exits non-zero if a computation that must succeed does not.
// NOT part of the reference.  tests/test_gpu_spin_time_correlation.py reads it.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "cmpt/eigen_ex/spin_time_correlation.hpp"

using namespace cmpt::EigenEx;
typedef SpinTimeCorrelationSolver::Coefficients Coefficients;
typedef std::complex<double> Complex;

static bool refused(const SpinTimeCorrelationSolver& tc) {
  bool line = false;
  for (const std::string& l : tc.log()) line = line || l.compare(0, SpinTimeCorrelationSolver::headERROR().size(), SpinTimeCorrelationSolver::headERROR()) == 0;
  return tc.info() == InvalidInput && line;
}

static int fail(const SpinTimeCorrelationSolver& tc, int code) {
  for (const std::string& l : tc.log()) std::fprintf(stderr, "%s\n", l.c_str());
  return code;
}

static Coefficients site(int L, int i) {
  Coefficients c(static_cast<std::size_t>(L), Complex(0.0, 0.0));
  c[static_cast<std::size_t>(i)] = Complex(1.0, 0.0);
  return c;
}

int main() {
  try {
    std::shared_ptr<device::Context> ctx = std::make_shared<device::Context>(0);
    // (1)
    const double J = 1.3;
    double worst = 0.0, worst_bound = 0.0;
    {
      SpinTimeCorrelationSolver tc;
      tc.setModel(ctx, SpinHalfModel::chain(2, J, J, false), 1).setProductState(1u);  // site 0 up
      tc.setSourceOperator(EIGENEX_SPIN_SITE_Z, site(2, 0)).addMeasuredOperator(site(2, 0));
      for (int k = 0; k <= 6; ++k) {
        if (k > 0) {
          tc.evolve(k % 3 == 0 ? -0.4 : 0.7);
          if (tc.info() != Success) return fail(tc, 2);
        }
        const std::vector<Complex> c = tc.values();
        if (tc.info() != Success || c.size() != 1) return fail(tc, 3);
        worst = std::max(worst, std::abs(c[0] - Complex(0.25 * std::cos(J * tc.time()), 0.0)));
        worst_bound = std::max(worst_bound, tc.errorBound());
      }
    }
    // (2)
    const int L = 10, nUp = 5;
    const SpinHalfModel model = SpinHalfModel::chain(L, 0.6, 1.0, false);
    std::uint32_t neel = 0;
    for (int i = 0; i < L; i += 2) neel |= std::uint32_t(1) << i;
    SpinTimeCorrelationSolver tc;
    tc.setModel(ctx, model, nUp).setKrylovDimension(12).setTolerance(1e-9).setProductState(neel);
    tc.setSourceOperator(EIGENEX_SPIN_SITE_MINUS, site(L, 4)).setMeasuredSites();
    const std::vector<Complex> c0 = tc.values();
    if (tc.info() != Success || c0.size() != static_cast<std::size_t>(L)) return fail(tc, 4);
    double others = 0.0;
    for (int j = 0; j < L; ++j)
      if (j != 4) others += std::abs(c0[static_cast<std::size_t>(j)]);
    long substeps = 0;
    for (int k = 0; k < 4; ++k) {
      substeps += static_cast<long>(tc.evolve(0.25));
      if (tc.info() != Success) return fail(tc, 5);
    }
    const std::vector<Complex> c1 = tc.values();
    if (tc.info() != Success || c1.size() != static_cast<std::size_t>(L)) return fail(tc, 6);
    double sum1 = 0.0;  // sum_j |<S+_j(t) S-_4(0)>|^2 <= <B^dagger B> |psi|^2: the hole is somewhere, and the Neel state has other terms
    for (const Complex& z : c1) sum1 += std::norm(z);

    SpinTimeCorrelationSolver none, source, length, count, leaves;
    none.evolve(0.1);
    source.setModel(ctx, model, nUp).setProductState(neel);
    source.values();
    length.setModel(ctx, model, nUp).setState(SpinTimeCorrelationSolver::RealVectorType(7, 1.0)).setSourceOperator(EIGENEX_SPIN_SITE_Z, site(L, 0));
    length.evolve(0.1);
    count.setModel(ctx, model, nUp).setProductState(neel).setSourceOperator(EIGENEX_SPIN_SITE_Z, site(L - 1, 0));
    count.evolve(0.1);
    leaves.setModel(ctx, model, L).setState(SpinTimeCorrelationSolver::RealVectorType(1, 1.0)).setSourceOperator(EIGENEX_SPIN_SITE_PLUS, site(L, 0));
    leaves.evolve(0.1);

    std::printf("{\"worst\": %.3e, \"worst_bound\": %.3e, \"c0_re\": %.17g, \"c0_im\": %.17g, \"others0\": %.3e, \"c1_re\": %.17g, \"c1_im\": %.17g, "
                "\"sum1\": %.17g, \"source_norm2\": %.17g, \"time\": %.17g, \"bound\": %.3e, \"eps_state\": %.3e, \"eps_source\": %.3e, "
                "\"substeps\": %ld, \"applications\": %lld, \"refused_no_model\": %d, \"refused_no_source\": %d, \"refused_length\": %d, "
                "\"refused_count\": %d, \"refused_leaves\": %d}\n",
                worst, worst_bound, c0[4].real(), c0[4].imag(), others, c1[4].real(), c1[4].imag(), sum1, tc.sourceNormSquared(), tc.time(),
                tc.errorBound(), tc.stateErrorBound(), tc.sourceErrorBound(), substeps, static_cast<long long>(tc.operatorApplications()),
                refused(none) ? 1 : 0, refused(source) ? 1 : 0, refused(length) ? 1 : 0, refused(count) ? 1 : 0, refused(leaves) ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
}
