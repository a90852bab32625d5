// C++11 user program: SpinTimeEvolutionSolver.  (1) Two sites, Heisenberg J, from |up down> in the sector (2,1): <Sz_0(t)> =
// cos(J t) / 2 and <psi_0|psi(t)> = exp(i J t / 4) cos(J t / 2); the Krylov space is the whole sector, so every step is exact.
// (2) The Neel state of the open XXZ chain of 10 sites in the sector (10,5): four calls of evolve(0.25) and one of evolve(-1.0),
// which returns to the start.  Prints JSON: the largest deviations of (1), and of (2) the norm, the energy before and after, the
// error bounds, the number of sub-steps and operator applications and the distance from the start state after the return; and
// whether no model, a product state outside the sector, a state of the wrong length and a Krylov dimension of 1 end in
// InvalidInput with an ERROR line in the log (the last leaves dimension and state as they were).  Exits non-zero if a
// computation that must succeed does not.
// NOT part of the reference.  tests/test_gpu_spin_evolution.py reads it.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "cmpt/eigen_ex/spin_evolution.hpp"

using namespace cmpt::EigenEx;

static bool refused(const SpinTimeEvolutionSolver& te) {
  bool line = false;
  for (const std::string& l : te.log()) line = line || l.compare(0, SpinTimeEvolutionSolver::headERROR().size(), SpinTimeEvolutionSolver::headERROR()) == 0;
  return te.info() == InvalidInput && line;
}

static int fail(const SpinTimeEvolutionSolver& te, int code) {
  for (const std::string& l : te.log()) std::fprintf(stderr, "%s\n", l.c_str());
  return code;
}

int main() {
  try {
    std::shared_ptr<device::Context> ctx = std::make_shared<device::Context>(0);
    // (1)
    const double J = 1.3;
    double worst_sz = 0.0, worst_overlap = 0.0, worst_bound = 0.0;
    {
      SpinTimeEvolutionSolver te;
      te.setModel(ctx, SpinHalfModel::chain(2, J, J, false), 1).setProductState(1u);  // site 0 up
      if (te.info() != Success) return fail(te, 2);
      for (int k = 1; k <= 6; ++k) {
        const double dt = k % 3 == 0 ? -0.4 : 0.7;
        if (te.evolve(dt) < 1 || te.info() != Success) return fail(te, 3);
        const double t = te.time();
        worst_sz = std::max(worst_sz, std::fabs(te.magnetisation()[0] - 0.5 * std::cos(J * t)));
        const std::complex<double> want = std::exp(std::complex<double>(0.0, J * t / 4)) * std::cos(J * t / 2);
        worst_overlap = std::max(worst_overlap, std::abs(te.overlapWithInitial() - want));
        worst_bound = std::max(worst_bound, te.errorBound());
      }
    }
    // (2)
    const int L = 10, nUp = 5;
    const SpinHalfModel model = SpinHalfModel::chain(L, 0.6, 1.0, false);
    std::uint32_t neel = 0;
    for (int i = 0; i < L; i += 2) neel |= std::uint32_t(1) << i;
    SpinTimeEvolutionSolver te;
    te.setModel(ctx, model, nUp).setKrylovDimension(12).setTolerance(1e-9).setProductState(neel);
    if (te.info() != Success) return fail(te, 4);
    const SpinTimeEvolutionSolver::VectorType start = te.state();
    const double e0 = te.energy();
    const std::complex<double> overlap0 = te.overlapWithInitial();
    long substeps = 0;
    double bounds = 0.0;
    for (int k = 0; k < 4; ++k) {
      substeps += static_cast<long>(te.evolve(0.25));
      if (te.info() != Success) return fail(te, 5);
      bounds += te.errorBound();
    }
    const double t_forward = te.time(), norm2 = te.normSquared(), e1 = te.energy(), overlap1 = std::abs(te.overlapWithInitial());
    substeps += static_cast<long>(te.evolve(-1.0));
    if (te.info() != Success) return fail(te, 6);
    bounds += te.errorBound();
    const SpinTimeEvolutionSolver::VectorType back = te.state();
    double dist = 0.0;
    for (Index r = 0; r < back.size(); ++r) dist += std::norm(back[r] - start[r]);
    double sum_sz = 0.0;
    for (double s : te.magnetisation()) sum_sz += s;

    SpinTimeEvolutionSolver none, outside, length, tiny;
    none.evolve(0.1);
    outside.setModel(ctx, model, nUp).setProductState(1u);
    length.setModel(ctx, model, nUp).setState(SpinTimeEvolutionSolver::RealVectorType(7, 1.0));
    tiny.setModel(ctx, model, nUp).setProductState(neel).setKrylovDimension(1);  // refused: the dimension stays 30, the state stays
    const bool tiny_kept = refused(tiny) && tiny.krylovDimension() == 30 && tiny.normSquared() == 1.0 && tiny.evolve(0.1) >= 1 && tiny.info() == Success;

    std::printf("{\"worst_sz\": %.3e, \"worst_overlap\": %.3e, \"worst_bound\": %.3e, \"rows\": %lld, \"t_forward\": %.17g, \"t_back\": %.17g, "
                "\"norm2\": %.17g, \"e0\": %.17g, \"e1\": %.17g, \"overlap0_re\": %.17g, \"overlap0_im\": %.17g, \"overlap1\": %.17g, "
                "\"substeps\": %ld, \"applications\": %lld, \"bounds\": %.3e, \"total_bound\": %.3e, \"return_distance\": %.3e, \"sum_sz\": %.3e, "
                "\"refused_no_model\": %d, \"refused_outside\": %d, \"refused_length\": %d, \"refused_tiny\": %d}\n",
                worst_sz, worst_overlap, worst_bound, static_cast<long long>(back.size()), t_forward, te.time(), norm2, e0, e1, overlap0.real(),
                overlap0.imag(), overlap1, substeps, static_cast<long long>(te.operatorApplications()), bounds, te.totalErrorBound(), std::sqrt(dist),
                sum_sz, refused(none) ? 1 : 0, refused(outside) ? 1 : 0, refused(length) ? 1 : 0, tiny_kept ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
}
