// Real-time evolution |psi(t)> = exp(-i H t) |psi_0> of a state of a spin-1/2 model by Krylov (Lanczos) propagation (T. J. Park
// and J. C. Light, J. Chem. Phys. 85 (1986) 5870), matrix-free and without a vector visiting the host between time steps.
//
// NOT part of the reference.  The state is a complex vector over the rows of a SpinHalfModel (full space, or the sector of nUp
// sites up) and lives in the work vector W of a complex Krylov state on device::spinHalfComplexOperator, the matrix-free operator
// for complex states (eigenex_spin_upload_z / eigenex_spin_sector_upload_z: the same real Hamiltonian).  psi_0 is kept in the
// last basis column of that state.  setState normalises: the device holds psi / |psi_0| and state() multiplies the norm back.
//
// A sub-step.  m + 1 calls of the Lanczos step from W (eigenex_lanczos_enqueue: the complex state takes the two-sweep path, full
// re-orthogonalisation) give the basis V_m, T_m = tridiag(alpha, beta) and beta_m, the coupling to the next vector.  T_m = S theta
// S^T on the host (small_eigen.hpp), the coefficients of the step tau are c(tau) = S exp(-i tau theta) S^T e_1, and
// psi <- V_m c(tau) by eigenex_krylov_combine_to(..., EIGENEX_VEC_W), followed by eigenex_basis_clear.  The Lanczos start divides W
// by its norm, so every sub-step starts from a unit vector.
//
// Step control.  The error e(s) = psi_Krylov(s) - psi(s) of a sub-step obeys e' = -i H e - i beta_m [exp(-i s T_m)]_{m,1} v_{m+1}
// with e(0) = 0 and a unitary propagator, hence
//   |e(tau)| <= B(tau) = beta_m  int_0^tau |[exp(-i s T_m)]_{m,1}| ds,      [exp(-i s T_m)]_{m,1} = sum_j S(m,j) exp(-i s theta_j) S(1,j),
// a bound in exact arithmetic.  B is evaluated on the host by the composite Simpson rule with kQuadPanels = 512 panels (513
// equidistant nodes on [0, tau]).  A sub-step takes the largest tau <= remaining with B(tau) <= tol * tau / |dt|: tau = remaining
// if that passes, else a bisection of [0, remaining] of exactly 60 halvings, keeping the largest passing point; over one
// evolve(dt) the accepted B therefore add up to at most tol.  errorBound() is that sum for the last evolve(dt),
// totalErrorBound() the sum since setState.  A breakdown (the Lanczos run stops on an invariant subspace, or m is at least the
// dimension, then m is the dimension and beta_m is not formed) makes the step exact: B = 0, tau = remaining.  A run stops where a
// coupling beta_k falls to the state's breakdown threshold (the library's default, 1e-12) or below, so "exact" there means up to
// that neglected coupling: by the bound above it adds at most threshold * tau to the error, which errorBound() does not count.
// Coefficients that are not finite end the call with NumericalIssue.  dt may be negative.
//
// Measurements read W where it is: normSquared(), magnetisation(), correlationsZZ() and correlationsXY() through
// eigenex_spin_measure (Hermitian sums of a complex vector), energy() = Re <psi|H|psi> / <psi|psi> through one operator application
// and its dot, overlapWithInitial() = <psi_0|psi(t)> through eigenex_dots with the kept column.  entanglementEntropy(A),
// entanglementSpectrum(A) and entanglementRenyi2(A) of a subsystem A (a site mask or a site list; at most 12 sites in the full
// space, 14 in a sector) form rho_A = M M^H of W through eigenex_spin_rdm_z and take the spectrum on the host with the code of
// SpinEntanglementSolver (spin_entanglement.hpp: detail::EntanglementBlocks); they change no vector, time, bound or counter.
// state() downloads.
//
// The sub-step, its bound and the loop over sub-steps are detail::krylovSubStep, detail::krylovErrorIntegral and
// detail::advanceInSubSteps below, which SpinTimeCorrelationSolver (spin_time_correlation.hpp: unequal-time correlations
// <A(t) B(0)>, through site operators of complex states) shares.
//
// Out of scope: complex couplings (Sy, Dzyaloshinskii-Moriya terms); momentum sectors; time-dependent Hamiltonians; Chebyshev
// propagators; more than one GPU (the matrix-free spin operators are one shard).
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <string>
#include <vector>

#include "lanczos.hpp"
#include "small_eigen.hpp"
#include "spin_entanglement.hpp"
#include "spin_frontend.hpp"
#include "spin_operator.hpp"

namespace cmpt {
namespace EigenEx {

namespace detail {

constexpr int kKrylovQuadPanels = 512;  // composite Simpson: kKrylovQuadPanels + 1 nodes
constexpr int kKrylovBisections = 60;
constexpr Index kKrylovMaxSubSteps = 1000000;

// B(tau) of the header for T = S diag(theta) S^T of dimension k (S column-major): beta_m times the Simpson sum
inline double krylovErrorIntegral(const std::vector<double>& theta, const std::vector<double>& S, int k, double betaM, double tau) {
  std::vector<double> w(static_cast<std::size_t>(k));
  for (int j = 0; j < k; ++j) w[static_cast<std::size_t>(j)] = S[static_cast<std::size_t>(j) * k + (k - 1)] * S[static_cast<std::size_t>(j) * k];
  const double hstep = tau / kKrylovQuadPanels;
  double sum = 0.0;
  for (int q = 0; q <= kKrylovQuadPanels; ++q) {
    const double s = hstep * q;
    double re = 0.0, im = 0.0;
    for (int j = 0; j < k; ++j) {
      re += w[static_cast<std::size_t>(j)] * std::cos(s * theta[static_cast<std::size_t>(j)]);
      im -= w[static_cast<std::size_t>(j)] * std::sin(s * theta[static_cast<std::size_t>(j)]);
    }
    const double weight = (q == 0 || q == kKrylovQuadPanels) ? 1.0 : ((q & 1) ? 4.0 : 2.0);
    sum += weight * std::sqrt(re * re + im * im);
  }
  return betaM * sum * hstep / 3.0;
}

// One sub-step of the header on the work vector W of the complex Krylov state `basis` of n rows, whose capacity is at least m + 2
// columns (m: the Krylov dimension, at most n): W <- exp(-i sign tau H) W for the largest tau <= remaining whose bound passes
// tol * tau / total; the state is cleared afterwards.  failure: null, or what went wrong (a NumericalIssue of the caller);
// applications counts the operator applications of the Lanczos run whether the step failed or not.
struct KrylovSubStep {
  double tau = 0.0, bound = 0.0;
  Index applications = 0;
  const char* failure = nullptr;
};
inline KrylovSubStep krylovSubStep(eigenex_basis_t basis, Index n, Index m, double tol, double remaining, double total, double sign) {
  KrylovSubStep out;
  const auto failed = [&out](const char* what) {
    out.failure = what;
    return out;
  };
  const bool whole = m >= n;  // the Krylov space is the space: exact without beta_m
  const int calls = static_cast<int>(whole ? m : m + 1);
  device::check(eigenex_lanczos_enqueue(basis, calls), "eigenex_lanczos_enqueue");
  eigenex_state_t st;
  std::vector<double> alpha(static_cast<std::size_t>(m) + 4, 0.0), beta(static_cast<std::size_t>(m) + 4, 0.0);
  device::check(eigenex_lanczos_state(basis, &st, alpha.data(), beta.data()), "eigenex_lanczos_state");
  out.applications = st.nalpha;
  const int k = std::min<int>(st.nalpha, static_cast<int>(m));
  if (k < 1) return failed("the state failed the breakdown threshold of the Lanczos run (it is zero or not finite)");
  for (int j = 0; j < k; ++j)
    if (!std::isfinite(alpha[static_cast<std::size_t>(j)]) || (j + 1 < k && !std::isfinite(beta[static_cast<std::size_t>(j)])))
      return failed("the Lanczos coefficients are not finite");
  const bool exact = whole || st.stopped != 0 || st.nbeta < static_cast<int>(m);
  std::vector<double> theta, S;
  if (!small_eigen::tridiagonal(alpha.data(), beta.data(), k, theta, &S)) return failed("the tridiagonal eigenproblem did not converge");
  const double betaM = exact ? 0.0 : beta[static_cast<std::size_t>(m) - 1];
  if (!std::isfinite(betaM)) return failed("the Lanczos coefficients are not finite");
  double tau = remaining, bound = 0.0;
  if (!exact) {
    const auto passes = [&](double t, double& B) {
      B = krylovErrorIntegral(theta, S, k, betaM, t);
      return B <= tol * t / total;
    };
    double B = 0.0;
    if (passes(remaining, B)) {
      bound = B;
    } else {
      double lo = 0.0, hi = remaining, Blo = 0.0;
      for (int it = 0; it < kKrylovBisections; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (passes(mid, B))
          lo = mid, Blo = B;
        else
          hi = mid;
      }
      if (!(lo > 0.0)) return failed("no step passes the tolerance: the Krylov dimension is too small");
      tau = lo, bound = Blo;
    }
  }
  // c = S exp(-i sign tau theta) S^T e_1
  std::vector<double> cre(static_cast<std::size_t>(k), 0.0), cim(static_cast<std::size_t>(k), 0.0);
  for (int j = 0; j < k; ++j) {
    const double ph = sign * tau * theta[static_cast<std::size_t>(j)], s0 = S[static_cast<std::size_t>(j) * k];
    const double fr = std::cos(ph) * s0, fi = -std::sin(ph) * s0;
    for (int r = 0; r < k; ++r) {
      cre[static_cast<std::size_t>(r)] += S[static_cast<std::size_t>(j) * k + r] * fr;
      cim[static_cast<std::size_t>(r)] += S[static_cast<std::size_t>(j) * k + r] * fi;
    }
  }
  device::check(eigenex_krylov_combine_to(basis, k, cre.data(), cim.data(), EIGENEX_VEC_W), "eigenex_krylov_combine_to");
  device::check(eigenex_basis_clear(basis), "eigenex_basis_clear");
  out.tau = tau, out.bound = bound;
  return out;
}

// W <- exp(-i H dt) W in sub-steps of Krylov dimension m until |dt| is used up.  accepted(step, sign) sees every sub-step that
// was taken (the time it covers is sign * step.tau); applications grows by those of every Lanczos run, steps by the sub-steps
// taken.  Null, or what went wrong (a NumericalIssue of the caller), then after the sub-steps completed so far.
template <class Accepted>
inline const char* advanceInSubSteps(eigenex_basis_t basis, Index n, Index m, double tol, double dt, Index& applications, Index& steps, Accepted accepted) {
  const double total = std::fabs(dt), sign = dt < 0.0 ? -1.0 : 1.0;
  double remaining = total;
  for (Index mine = 0; remaining > 0.0; ++mine, ++steps) {
    if (mine >= kKrylovMaxSubSteps) return "more than 10^6 sub-steps: the Krylov dimension is too small for this tolerance";
    const KrylovSubStep step = krylovSubStep(basis, n, m, tol, remaining, total, sign);
    applications += step.applications;
    if (step.failure) return step.failure;
    accepted(step, sign);
    remaining = step.tau >= remaining ? 0.0 : remaining - step.tau;
  }
  return nullptr;
}

}  // namespace detail

class SpinTimeEvolutionSolver {
 public:
  using Index = EigenEx::Index;
  using Complex = std::complex<double>;
  using VectorType = DenseVector<Complex>;
  using RealVectorType = DenseVector<double>;

  static constexpr int kQuadPanels = detail::kKrylovQuadPanels;  // composite Simpson: kQuadPanels + 1 nodes
  static constexpr int kBisections = detail::kKrylovBisections;
  static constexpr Index kMaxSubSteps = detail::kKrylovMaxSubSteps;

  static std::string headERROR() { return detail::CallLog::headERROR(); }
  static std::string headINFO() { return detail::CallLog::headINFO(); }

  // nUp = -1: the full space (up to 30 sites); else the sector of nUp sites up (up to 32 sites, no transverse field)
  SpinTimeEvolutionSolver& setModel(const std::shared_ptr<device::Context>& ctx, const SpinHalfModel& model, int nUp = -1) {
    ctx_ = ctx, model_ = model, nUp_ = nUp, haveModel_ = true, haveState_ = false;
    dev_.release();  // the state goes before its operator
    op_.reset();
    return *this;
  }
  // the Krylov dimension m of a sub-step (default 30, at least 2) and the error budget of one evolve(dt) (default 1e-10)
  SpinTimeEvolutionSolver& setKrylovDimension(Index m) {
    if (m < 2) {  // refused: the dimension and the state stay as they were
      begin_("setKrylovDimension");
      invalid_("invalid input: setKrylovDimension needs at least 2");
      return *this;
    }
    if (m != m_ && dev_.alive()) {  // the state moves to a Krylov state of the new capacity
      const VectorType psi = dev_.download<Complex>(EIGENEX_VEC_W), psi0 = dev_.download<Complex>(EIGENEX_VEC_COL(dev_.capacity() - 1));
      m_ = m;
      place_(psi, psi0);
    }
    m_ = m;
    return *this;
  }
  SpinTimeEvolutionSolver& setTolerance(double tol) {
    tol_ = tol;
    return *this;
  }
  Index krylovDimension() const { return m_; }
  double tolerance() const { return tol_; }

  // a host vector over the rows of the model's space or sector; normalised on upload, the norm is kept (initialNorm())
  SpinTimeEvolutionSolver& setState(const VectorType& v) {
    begin_("setState");
    if (!ready_()) return *this;
    std::string why;
    double nrm = 0.0;
    const VectorType u = detail::normalised(v, rows_(), nrm, why);
    if (!why.empty()) return invalid_(why), *this;
    norm0_ = nrm;
    place_(u, u);
    reset_();
    return *this;
  }
  SpinTimeEvolutionSolver& setState(const RealVectorType& v) {
    VectorType z(v.size());
    for (Index r = 0; r < v.size(); ++r) z[r] = Complex(v[r], 0.0);
    return setState(z);
  }
  // the basis state with site i up where bit i of `bits` is set, e.g. the Neel state 0b0101...; it must lie in the sector
  SpinTimeEvolutionSolver& setProductState(std::uint32_t bits) {
    begin_("setProductState");
    if (!ready_()) return *this;
    std::string why;
    const Index row = detail::productStateRow(model_.sites(), nUp_, rows_(), bits, why);
    if (row < 0) return invalid_(why), *this;
    VectorType u(rows_(), Complex(0.0, 0.0));
    u[row] = Complex(1.0, 0.0);
    norm0_ = 1.0;
    place_(u, u);
    reset_();
    return *this;
  }

  // psi <- exp(-i H dt) psi; returns the number of sub-steps (0 after an error: info(), log())
  Index evolve(double dt) {
    begin_("evolve");
    lastBound_ = 0.0;
    if (!ready_()) return 0;
    if (!haveState_) return invalid_("invalid input: no state (setState, setProductState)");
    if (!std::isfinite(dt)) return invalid_("invalid input: dt is not finite");
    if (!(tol_ > 0.0) || !std::isfinite(tol_)) return invalid_("invalid input: setTolerance needs a positive tolerance");
    Index steps = 0;
    // a failed call leaves the time advanced by the sub-steps that were completed
    const char* failure = detail::advanceInSubSteps(dev_.handle(), rows_(), krylov_(), tol_, dt, applications_, steps, [this](const detail::KrylovSubStep& step, double sign) {
      lastBound_ += step.bound, totalBound_ += step.bound;
      time_ += sign * step.tau;
    });
    if (failure) return failed_(failure);
    log_.note("sub-steps: " + std::to_string(steps) + ", error bound of this call: " + std::to_string(lastBound_));
    return steps;
  }

  double time() const { return time_; }
  double errorBound() const { return lastBound_; }
  double totalErrorBound() const { return totalBound_; }
  Index operatorApplications() const { return applications_; }
  double initialNorm() const { return norm0_; }

  // <psi|psi> of the device vector (1 up to rounding: the kept norm is not in it)
  double normSquared() {
    double n2 = 0.0;
    if (!measurable_()) return 0.0;
    device::check(eigenex_spin_measure(dev_.handle(), EIGENEX_VEC_W, 0, nullptr, 0, nullptr, nullptr, nullptr, &n2), "eigenex_spin_measure");
    return n2;
  }
  // Re <psi|H|psi> / <psi|psi>: one operator application and its dot
  double energy() {
    if (!measurable_()) return 0.0;
    double dot[2] = {0.0, 0.0};
    device::check(eigenex_apply(dev_.handle(), EIGENEX_VEC_W, EIGENEX_VEC_V, 0.0, dot), "eigenex_apply");
    ++applications_;
    return dot[0] / normSquared();
  }
  // <Sz_i>, i < sites
  std::vector<double> magnetisation() {
    if (!measurable_()) return {};
    const std::size_t L = static_cast<std::size_t>(model_.sites());
    std::vector<std::uint32_t> masks;
    detail::appendSiteMasks(L, masks);
    std::vector<double> d(L, 0.0);
    double n2 = 0.0;
    device::check(eigenex_spin_measure(dev_.handle(), EIGENEX_VEC_W, static_cast<int>(L), masks.data(), 0, nullptr, d.data(), nullptr, &n2), "eigenex_spin_measure");
    for (double& x : d) x /= 2.0 * n2;
    return d;
  }
  // <Sz_i Sz_j> and <Sx_i Sx_j + Sy_i Sy_j>, row-major sites x sites (i = j: 1/4 and 1/2)
  std::vector<double> correlationsZZ() { return pairs_(true); }
  std::vector<double> correlationsXY() { return pairs_(false); }
  // <psi_0|psi(t)>, both of unit norm
  Complex overlapWithInitial() {
    if (!measurable_()) return Complex(0.0, 0.0);
    double h[2] = {0.0, 0.0};
    device::check(eigenex_dots(dev_.handle(), EIGENEX_VEC_W, dev_.capacity() - 1, 1, 1, 0, h), "eigenex_dots");
    return Complex(h[0], h[1]);
  }
  // The entanglement of the subsystem `mask` (bit i = site i) with the other sites: the von Neumann entropy, the spectrum of rho_A
  // (descending) and the Renyi-2 entropy -ln ||rho_A||_F^2 (no eigen-solve).  An invalid subsystem is logged (info(), log()) and
  // gives 0 or an empty spectrum.  Nothing of the trajectory changes; log() and info() are those of the call.
  double entanglementEntropy(std::uint32_t mask) {
    detail::EntanglementBlocks e;
    return entangle_(mask, true, e) ? e.entropy() : 0.0;
  }
  std::vector<double> entanglementSpectrum(std::uint32_t mask) {
    detail::EntanglementBlocks e;
    return entangle_(mask, true, e) ? e.spectrum : std::vector<double>();
  }
  double entanglementRenyi2(std::uint32_t mask) {
    detail::EntanglementBlocks e;
    return entangle_(mask, true, e) ? e.renyi2() : 0.0;
  }
  double entanglementEntropy(const std::vector<int>& sites) {
    bool valid = true;
    const std::uint32_t mask = detail::siteMask(sites, valid);
    detail::EntanglementBlocks e;
    return entangle_(mask, valid, e) ? e.entropy() : 0.0;
  }
  std::vector<double> entanglementSpectrum(const std::vector<int>& sites) {
    bool valid = true;
    const std::uint32_t mask = detail::siteMask(sites, valid);
    detail::EntanglementBlocks e;
    return entangle_(mask, valid, e) ? e.spectrum : std::vector<double>();
  }
  double entanglementRenyi2(const std::vector<int>& sites) {
    bool valid = true;
    const std::uint32_t mask = detail::siteMask(sites, valid);
    detail::EntanglementBlocks e;
    return entangle_(mask, valid, e) ? e.renyi2() : 0.0;
  }
  // psi(t) on the host, the kept norm multiplied back
  VectorType state() {
    if (!measurable_()) return VectorType();
    VectorType v = dev_.download<Complex>(EIGENEX_VEC_W);
    if (norm0_ != 1.0)
      for (Index r = 0; r < v.size(); ++r) v[r] *= norm0_;
    return v;
  }

  int sites() const { return haveModel_ ? model_.sites() : 0; }
  int sitesUp() const { return nUp_; }
  ComputationInfo info() const { return log_.info(); }
  const std::vector<std::string>& log() const { return log_.log(); }

  // B(tau) of the header for T = S diag(theta) S^T of dimension k (S column-major): beta_m times the Simpson sum
  static double errorIntegral(const std::vector<double>& theta, const std::vector<double>& S, int k, double betaM, double tau) {
    return detail::krylovErrorIntegral(theta, S, k, betaM, tau);
  }

 private:
  void begin_(const char* who) { log_.begin("SpinTimeEvolutionSolver", who); }
  Index invalid_(const std::string& what) { return log_.invalid(what); }
  Index failed_(const std::string& what) { return log_.failed(what); }
  void reset_() { time_ = 0.0, lastBound_ = 0.0, totalBound_ = 0.0, applications_ = 0, haveState_ = true; }
  Index rows_() const { return static_cast<Index>(op_->rows()); }
  bool measurable_() const { return haveState_ && dev_.alive(); }

  // the model, the settings and the operator; false after invalid_()
  bool ready_() {
    if (!haveModel_ || !ctx_) return invalid_("invalid input: no model (setModel)"), false;
    try {
      if (!op_) op_ = device::spinHalfComplexOperator(ctx_, model_, nUp_);
    } catch (const LanczosException& e) {
      return invalid_(std::string("invalid input: the model has no such operator: ") + e.what()), false;
    }
    return true;
  }
  Index krylov_() const { return std::min<Index>(m_, rows_()); }
  // a complex Krylov state of m + 2 columns: the run's m + 1 and psi_0 in the last
  void place_(const VectorType& psi, const VectorType& psi0) {
    const int cap = static_cast<int>(krylov_() + 2);
    if (!dev_.alive() || dev_.capacity() != cap)
      dev_.create(ctx_, op_, rows_(), cap, 0, true);
    else
      device::check(eigenex_basis_clear(dev_.handle()), "eigenex_basis_clear");
    dev_.upload(EIGENEX_VEC_W, psi);
    dev_.upload(EIGENEX_VEC_COL(cap - 1), psi0);
  }
  // rho_A of W, to unit trace and diagonalised; false (and logged) for an invalid subsystem or without a state
  bool entangle_(std::uint32_t mask, bool sitesValid, detail::EntanglementBlocks& e) {
    begin_("entanglement");  // these calls can be refused: the log and info() are theirs, as for setState and evolve
    if (!measurable_()) return invalid_("invalid input: no state (setState, setProductState)"), false;
    if (!sitesValid) return invalid_("invalid input: the subsystem names a site outside 0..31 or names a site twice"), false;
    int nBlocks = 0, kFirst = 0;
    std::int64_t dims[33], offsets[34];
    if (eigenex_spin_rdm_layout(model_.sites(), nUp_, mask, &nBlocks, &kFirst, dims, offsets) != 0)
      return invalid_(std::string("invalid input: ") + eigenex_last_error()), false;
    std::vector<double> raw(2 * static_cast<std::size_t>(offsets[nBlocks]), 0.0);
    device::check(eigenex_spin_rdm_z(dev_.handle(), EIGENEX_VEC_W, mask, raw.data(), static_cast<std::int64_t>(raw.size())), "eigenex_spin_rdm_z");
    switch (e.assemble(raw, true, nBlocks, kFirst, dims, offsets)) {
      case detail::EntanglementBlocks::ZeroState:
        return failed_("the state is zero (or not finite)"), false;
      case detail::EntanglementBlocks::NoConvergence:
        return failed_("the eigen-solve of a block of the reduced density matrix did not converge"), false;
      case detail::EntanglementBlocks::Ok:
        break;
    }
    return true;
  }

  std::vector<double> pairs_(bool zz) {
    if (!measurable_()) return {};
    const std::size_t L = static_cast<std::size_t>(model_.sites());
    std::vector<std::uint32_t> masks;
    detail::appendPairMasks(L, masks);
    std::vector<double> raw(masks.size(), 0.0);
    double n2 = 0.0;
    device::check(eigenex_spin_measure(dev_.handle(), EIGENEX_VEC_W, zz ? static_cast<int>(masks.size()) : 0, zz ? masks.data() : nullptr,
                                       zz ? 0 : static_cast<int>(masks.size()), zz ? nullptr : masks.data(), zz ? raw.data() : nullptr,
                                       zz ? nullptr : raw.data(), &n2),
                  "eigenex_spin_measure");
    return detail::pairMatrix(raw.data(), L, (zz ? 4.0 : 2.0) * n2, zz ? 0.25 : 0.5);
  }

  std::shared_ptr<device::Context> ctx_;
  SpinHalfModel model_;
  bool haveModel_ = false, haveState_ = false;
  int nUp_ = -1;
  Index m_ = 30;
  double tol_ = 1e-10;
  std::shared_ptr<device::CsrOperator> op_;
  detail::KrylovDevice dev_;
  double norm0_ = 1.0, time_ = 0.0, lastBound_ = 0.0, totalBound_ = 0.0;
  Index applications_ = 0;
  detail::CallLog log_;
};

}  // namespace EigenEx
}  // namespace cmpt
