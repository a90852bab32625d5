// C++11 user program: every log line and info() of the six spin front-end classes (SpinDynamicsSolver, SpinTimeEvolutionSolver,
// SpinTimeCorrelationSolver, SpinEntanglementSolver, SpinCorrelationSolver, SpinMomentumCorrelationSolver) over the outcomes that
// pass through the code they share (spin_frontend.hpp): refusals, zero responses, the restart note and one successful call each,
// on the open chain of 4 sites in the full space and the ring of 6 sites with 3 up.  Prints a JSON list of
// {"case", "info", "log"}.  tests/test_gpu_spin_frontend_logs.py holds the output to tests/golden/spin_frontend_logs.json, which
// scripts/record_spin_frontend_logs.py recorded from the commit before the shared header existed.
// NOT part of the reference.
#include <cmath>
#include <complex>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "cmpt/eigen_ex/spin_correlations.hpp"
#include "cmpt/eigen_ex/spin_dynamics.hpp"
#include "cmpt/eigen_ex/spin_entanglement.hpp"
#include "cmpt/eigen_ex/spin_time_correlation.hpp"

using namespace cmpt::EigenEx;
typedef std::complex<double> Complex;
typedef std::vector<Complex> Coefficients;
typedef DenseVector<double> Real;
typedef DenseVector<Complex> Cplx;

static bool g_first = true;

template <class Solver>
static void record(const std::string& name, const Solver& s) {
  std::printf("%s\n {\"case\": \"%s\", \"info\": %d, \"log\": [", g_first ? "" : ",", name.c_str(), static_cast<int>(s.info()));
  g_first = false;
  for (std::size_t i = 0; i < s.log().size(); ++i) {
    std::string esc;
    for (char c : s.log()[i]) {
      char hex[8];
      if (c == '"' || c == '\\') esc += '\\';
      if (static_cast<unsigned char>(c) < 0x20)
        std::snprintf(hex, sizeof hex, "\\u%04x", static_cast<unsigned>(c)), esc += hex;
      else
        esc += c;
    }
    std::printf("%s\"%s\"", i ? ", " : "", esc.c_str());
  }
  std::printf("]}");
}

static Real ramp(Index n) {
  Real v(n, 0.0);
  for (Index r = 0; r < n; ++r) v[r] = 1.0 + 0.25 * static_cast<double>((r * 7) % 5) - 0.125 * static_cast<double>(r % 3);
  return v;
}
static Cplx rampZ(Index n) {
  Cplx v(n, Complex(0.0, 0.0));
  for (Index r = 0; r < n; ++r) v[r] = Complex(1.0 + 0.25 * static_cast<double>((r * 7) % 5), 0.5 - 0.125 * static_cast<double>(r % 4));
  return v;
}
static Real unit(Index n, Index row) {
  Real v(n, 0.0);
  v[row] = 1.0;
  return v;
}
static std::vector<double> siteR(int L, int i, double value = 1.0) {
  std::vector<double> c(static_cast<std::size_t>(L), 0.0);
  c[static_cast<std::size_t>(i)] = value;
  return c;
}
static Coefficients siteZ(int L, int i, Complex value = Complex(1.0, 0.0)) {
  Coefficients c(static_cast<std::size_t>(L), Complex(0.0, 0.0));
  c[static_cast<std::size_t>(i)] = value;
  return c;
}

struct Geometry {
  std::string name;
  SpinHalfModel model;
  int L, nUp;
  Index rows;
  std::uint32_t inside;  // a product state of the space or sector whose site 0 is up: row `insideRow`
  Index insideRow;
};

static void dynamics(const std::shared_ptr<device::Context>& ctx, const Geometry& g) {
  const std::string p = "dynamics/" + g.name + "/";
  const double nan = std::numeric_limits<double>::quiet_NaN();
  {
    SpinDynamicsSolver s;
    s.setModel(ctx, g.model, g.nUp).setSiteOperator(EIGENEX_SPIN_SITE_Z, siteR(g.L, 0)).setLanczosSteps(8);
    s.compute();
    record(p + "no_state", s);
    s.setState(Real(3, 1.0)).compute();
    record(p + "state_length", s);
    s.setState(Real(g.rows, 0.0)).compute();
    record(p + "state_zero", s);
    s.setState(ramp(g.rows)).setSiteOperator(EIGENEX_SPIN_SITE_Z, siteR(g.L - 1, 0)).compute();
    record(p + "coefficients_length", s);
    s.setSiteOperator(EIGENEX_SPIN_SITE_Z, siteR(g.L, 1, nan)).compute();
    record(p + "coefficients_nan", s);
    s.setSiteOperator(EIGENEX_SPIN_SITE_Z, siteZ(g.L, 1, Complex(0.0, nan))).compute();
    record(p + "coefficients_nan_imaginary", s);
    s.setSiteOperator(7, siteR(g.L, 0)).compute();
    record(p + "kind", s);
    s.setSiteOperator(EIGENEX_SPIN_SITE_Z, siteR(g.L, 0)).setLanczosSteps(0).compute();
    record(p + "steps", s);
    s.setLanczosSteps(8).compute();
    record(p + "success_z", s);
    s.computeStructureFactorZ(1.0);
    record(p + "success_structure_factor", s);
    s.computeStructureFactorZSingleRun(1.0);
    record(p + "success_single_run", s);
    s.setState(rampZ(g.rows)).computeStructureFactorZ(1.0);
    record(p + "structure_factor_of_complex_state", s);
    s.setSiteOperator(EIGENEX_SPIN_SITE_MINUS, siteZ(g.L, 0, Complex(0.5, -0.25))).compute();
    record(p + "success_complex_minus", s);
    // S+_0 of a product state whose site 0 is up: an exact zero
    s.setState(unit(g.rows, g.insideRow)).setSiteOperator(EIGENEX_SPIN_SITE_PLUS, siteR(g.L, 0)).compute();
    record(p + "annihilated", s);
    s.setSiteOperator(EIGENEX_SPIN_SITE_MINUS, siteR(g.L, 0)).compute();
    record(p + "success_minus", s);
  }
  if (g.nUp >= 0) {
    SpinDynamicsSolver up, down;
    up.setModel(ctx, g.model, g.L).setState(Real(1, 1.0)).setSiteOperator(EIGENEX_SPIN_SITE_PLUS, siteR(g.L, 0)).compute();
    record(p + "plus_of_all_up", up);
    down.setModel(ctx, g.model, 0).setState(Real(1, 1.0)).setSiteOperator(EIGENEX_SPIN_SITE_MINUS, siteR(g.L, 0)).compute();
    record(p + "minus_of_none_up", down);
  }
}

static void evolution(const std::shared_ptr<device::Context>& ctx, const Geometry& g) {
  const std::string p = "evolution/" + g.name + "/";
  SpinTimeEvolutionSolver s;
  s.setModel(ctx, g.model, g.nUp);
  s.evolve(0.1);
  record(p + "no_state", s);
  s.entanglementEntropy(std::uint32_t(3));
  record(p + "entanglement_no_state", s);
  s.setState(Real(3, 1.0));
  record(p + "state_length", s);
  s.setState(Real(g.rows, 0.0));
  record(p + "state_zero", s);
  s.setProductState(std::uint32_t(1) << g.L);
  record(p + "product_outside_sites", s);
  if (g.nUp >= 0) {
    s.setProductState(1u);
    record(p + "product_outside_sector", s);
  }
  s.setProductState(g.inside);
  record(p + "product_state", s);
  s.setKrylovDimension(1);
  record(p + "krylov_dimension", s);
  s.evolve(std::numeric_limits<double>::infinity());
  record(p + "dt", s);
  s.setTolerance(0.0).evolve(0.1);
  record(p + "tolerance", s);
  s.setTolerance(1e-10).setKrylovDimension(4).evolve(0.3);
  record(p + "success_evolve", s);
  s.evolve(-0.2);
  record(p + "success_evolve_back", s);
  s.entanglementEntropy(std::uint32_t(3));
  record(p + "success_entanglement", s);
  s.entanglementEntropy(std::vector<int>{0, 0});
  record(p + "entanglement_site_twice", s);
  s.entanglementRenyi2(std::vector<int>{0, 32});
  record(p + "entanglement_site_32", s);
  s.setState(rampZ(g.rows));
  record(p + "success_state", s);
  s.evolve(0.1);
  record(p + "success_evolve_state", s);
}

static void timeCorrelation(const std::shared_ptr<device::Context>& ctx, const Geometry& g) {
  const std::string p = "time_correlation/" + g.name + "/";
  const double nan = std::numeric_limits<double>::quiet_NaN();
  {
    SpinTimeCorrelationSolver s;
    s.setModel(ctx, g.model, g.nUp);
    s.evolve(0.1);
    record(p + "no_state", s);
    s.setProductState(g.inside).values();
    record(p + "no_source", s);
    s.setSourceOperator(7, siteZ(g.L, 0)).values();
    record(p + "kind", s);
    s.setSourceOperator(EIGENEX_SPIN_SITE_Z, siteZ(g.L - 1, 0)).evolve(0.1);
    record(p + "source_length", s);
    s.setSourceOperator(EIGENEX_SPIN_SITE_Z, siteZ(g.L, 0, Complex(nan, 0.0))).evolve(0.1);
    record(p + "source_nan", s);
    s.setSourceOperator(EIGENEX_SPIN_SITE_Z, siteZ(g.L, 0)).addMeasuredOperator(siteZ(g.L + 1, 0)).evolve(0.1);
    record(p + "measured_length", s);
    s.clearMeasuredOperators().addMeasuredOperator(siteZ(g.L, 0, Complex(0.0, nan))).values();
    record(p + "measured_nan", s);
    s.clearMeasuredOperators().setMeasuredSites().setState(Real(3, 1.0)).evolve(0.1);
    record(p + "state_length", s);
    s.setState(Cplx(g.rows, Complex(0.0, 0.0))).evolve(0.1);
    record(p + "state_zero", s);
    s.setProductState(std::uint32_t(1) << g.L).evolve(0.1);
    record(p + "product_outside_sites", s);
    if (g.nUp >= 0) {
      s.setProductState(1u).evolve(0.1);
      record(p + "product_outside_sector", s);
    }
    s.setProductState(g.inside).setKrylovDimension(1).evolve(0.1);
    record(p + "krylov_dimension", s);
    s.setKrylovDimension(4).setEigenstate(nan).evolve(0.1);
    record(p + "eigenstate_energy", s);
    s.setProductState(g.inside).evolve(nan);
    record(p + "dt", s);
    s.setTolerance(-1.0).evolve(0.1);
    record(p + "tolerance", s);
    s.setTolerance(1e-10).values();
    record(p + "success_values_at_0", s);
    s.evolve(0.3);
    record(p + "success_evolve", s);
    s.values();
    record(p + "success_values", s);
    s.addMeasuredOperator(siteZ(g.L, 0, Complex(nan, 0.0))).values();  // added between time points: checked by values() itself
    record(p + "measured_nan_between_time_points", s);
    s.setMeasuredSites().setKrylovDimension(5).evolve(0.2);
    record(p + "restart_note", s);
    s.setState(rampZ(g.rows)).setMomentumZ(1.0).evolve(0.1);
    record(p + "success_momentum_z", s);
    s.values();
    record(p + "success_momentum_z_values", s);
    // S+_0 of a product state whose site 0 is up: an exact zero
    s.setProductState(g.inside).setSourceOperator(EIGENEX_SPIN_SITE_PLUS, siteZ(g.L, 0)).setMeasuredSites().evolve(0.1);
    record(p + "annihilated_evolve", s);
    s.values();
    record(p + "annihilated_values", s);
    s.setSourceOperator(EIGENEX_SPIN_SITE_MINUS, siteZ(g.L, 0)).evolve(0.1);
    record(p + "success_minus", s);
  }
  if (g.nUp >= 0) {
    SpinTimeCorrelationSolver up, down;
    up.setModel(ctx, g.model, g.L).setState(Real(1, 1.0)).setSourceOperator(EIGENEX_SPIN_SITE_PLUS, siteZ(g.L, 0)).evolve(0.1);
    record(p + "plus_of_all_up", up);
    down.setModel(ctx, g.model, 0).setState(Real(1, 1.0)).setSourceOperator(EIGENEX_SPIN_SITE_MINUS, siteZ(g.L, 0)).values();
    record(p + "minus_of_none_up", down);
  }
}

static void measurements(const std::shared_ptr<device::Context>& ctx, const Geometry& g) {
  const std::shared_ptr<device::CsrOperator> op =
      g.nUp < 0 ? device::spinHalfOperator(ctx, g.model) : device::spinHalfSectorOperator(ctx, g.model, g.nUp);
  {
    const std::string p = "entanglement/" + g.name + "/";
    SpinEntanglementSolver s;
    s.setDeviceOperator(op).setSubsystemMask(3u);
    s.compute();
    record(p + "no_state", s);
    s.setState(Real(3, 1.0)).compute();
    record(p + "state_length", s);
    s.setState(Real(g.rows, 0.0)).compute();
    record(p + "state_zero", s);
    s.setState(ramp(g.rows)).setSubsystem(std::vector<int>{1, 1}).compute();
    record(p + "site_twice", s);
    s.setSubsystem(std::vector<int>{0, -1}).compute();
    record(p + "site_negative", s);
    s.setSubsystemMask(std::uint32_t(1) << g.L).compute();
    record(p + "mask_outside_sites", s);
    s.setSubsystem(std::vector<int>{0, 1}).compute();
    record(p + "success", s);
    s.setState(rampZ(g.rows)).compute();
    record(p + "complex_state_of_real_operator", s);
  }
  {
    const std::string p = "correlations/" + g.name + "/";
    SpinCorrelationSolver s;
    s.setDeviceOperator(op);
    s.compute();
    record(p + "no_state", s);
    s.setState(Real(3, 1.0)).compute();
    record(p + "state_length", s);
    s.setState(Real(g.rows, 0.0)).compute();
    record(p + "state_zero", s);
    s.setState(ramp(g.rows)).compute();
    record(p + "success", s);
  }
}

int main() {
  try {
    std::shared_ptr<device::Context> ctx = std::make_shared<device::Context>(0);
    std::printf("[");
    {
      SpinDynamicsSolver d;
      d.compute();
      record("dynamics/no_model", d);
      d.computeStructureFactorZ(1.0);
      record("dynamics/no_model_structure_factor", d);
      SpinTimeEvolutionSolver e;
      e.evolve(0.1);
      record("evolution/no_model_evolve", e);
      e.setState(Real(4, 1.0));
      record("evolution/no_model_state", e);
      e.setProductState(1u);
      record("evolution/no_model_product_state", e);
      SpinTimeCorrelationSolver t;
      t.evolve(0.1);
      record("time_correlation/no_model_evolve", t);
      t.values();
      record("time_correlation/no_model_values", t);
      SpinEntanglementSolver n;
      n.compute();
      record("entanglement/no_operator", n);
      SpinCorrelationSolver c;
      c.compute();
      record("correlations/no_operator", c);
      SpinMomentumCorrelationSolver m;
      m.compute();
      record("momentum_correlations/no_operator", m);
    }
    const Geometry chain = {"chain4", SpinHalfModel::chain(4, 0.7, 1.0, false), 4, -1, 16, 5u, 5};
    const Geometry ring = {"ring6_up3", SpinHalfModel::chain(6, 0.7, 1.0, true), 6, 3, 20, 7u, 0};  // 0b000111 is the sector's first state
    for (const Geometry* g : {&chain, &ring}) {
      dynamics(ctx, *g);
      evolution(ctx, *g);
      timeCorrelation(ctx, *g);
      measurements(ctx, *g);
    }
    {
      const std::string p = "momentum_correlations/ring6_up3/";
      const std::shared_ptr<device::CsrOperator> op = device::spinHalfMomentumOperator(ctx, ring.model, 3, 0);
      const Index rows = static_cast<Index>(op->rows());
      SpinMomentumCorrelationSolver s;
      s.setDeviceOperator(op);
      s.compute();
      record(p + "no_state", s);
      s.setState(Real(rows + 1, 1.0)).compute();
      record(p + "state_length", s);
      s.setState(Real(rows, 0.0)).compute();
      record(p + "state_zero", s);
      s.setState(ramp(rows)).compute();
      record(p + "success", s);
    }
    std::printf("\n]\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
}
