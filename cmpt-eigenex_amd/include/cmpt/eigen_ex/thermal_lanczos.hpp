// Finite-temperature Lanczos (thermal_sums.hpp has the method, the normalisation and the error estimate): thermodynamics of any
// Hermitian device operator and thermal expectation values of spin observables, from R Lanczos runs of M steps.
//
//   ThermalLanczosSolver<S>   one operator (one symmetry sector).  Per sample: the start vector is uploaded (setSampleVectors) or
//                             drawn as +-1 entries on the device (eigenex_vec_random_signs, stream firstStream + r) and normalised
//                             by the first step; M step calls with full re-orthogonalisation go through the batched enqueue; a
//                             breakdown (the library's threshold) ends the sample there, and the sample is then exact for that
//                             start vector; T is solved on the host (small_eigen); with observables set, one call of
//                             eigenex_spin_measure_columns gives g_ti = <v_i| A_t |v_0> for all columns the sample produced.
//                             Only alpha, beta and g cross to the host, never a vector.  Thermodynamics needs alpha and beta
//                             alone, so it runs on every operator handle, momentum sectors of up to 48 sites included, with real
//                             or complex states; observables need a real state on a handle of eigenex_spin_upload or
//                             eigenex_spin_sector_upload (setSpinObservables returns InvalidInput otherwise).
//   ThermalEnsemble           sums over sectors: Z = sum_k m_k Z_k with multiplicities m_k.
// Not here: complex states with observables, observables on momentum handles, the low-temperature variant (LTLM), dynamical
// quantities at T > 0, more than one GPU.
#pragma once

#include <cmath>
#include <complex>
#include <cstdint>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "lanczos.hpp"
#include "small_eigen.hpp"
#include "thermal_sums.hpp"

namespace cmpt {
namespace EigenEx {

template <class Scalar_>
class ThermalLanczosSolver {
  static_assert(std::is_same<Scalar_, double>::value || std::is_same<Scalar_, std::complex<double>>::value,
                "cmpt-eigenex_amd: ThermalLanczosSolver takes double or std::complex<double>");

 public:
  using Index = EigenEx::Index;
  using Scalar = Scalar_;

  static std::string headERROR() { return std::string("ERROR     "); }
  static std::string headINFO() { return std::string("INFO      "); }

  ThermalLanczosSolver& setDeviceOperator(const std::shared_ptr<device::CsrOperator>& op) {
    op_ = op;
    height_ = op ? static_cast<Index>(op->rows()) : 0;
    diagMasks_.clear(), flipMasks_.clear();
    sitesAndPairs_ = 0;
    return *this;
  }
  ThermalLanczosSolver& setLanczosSteps(Index M) {
    M_ = M;
    return *this;
  }
  ThermalLanczosSolver& setRandomVectors(Index R) {
    R_ = R;
    return *this;
  }
  ThermalLanczosSolver& setSeed(std::uint64_t seed) {
    seed_ = seed;
    return *this;
  }
  ThermalLanczosSolver& setFirstStream(std::uint64_t stream) {
    firstStream_ = stream;
    return *this;
  }
  // R explicit start vectors of N entries each, one after the other (copied; they need not be normalised); a null pointer
  // returns to random vectors
  ThermalLanczosSolver& setSampleVectors(const Scalar* vectors, Index N, Index R) {
    if (vectors && N > 0 && R > 0) {
      given_.assign(vectors, vectors + static_cast<std::size_t>(N) * static_cast<std::size_t>(R));
      givenN_ = N, givenR_ = R;
    } else {
      given_.clear();
      givenN_ = givenR_ = 0;
    }
    return *this;
  }
  // the observables, as the two mask lists of eigenex_spin_measure_columns; empty lists: thermodynamics alone
  ComputationInfo setSpinObservables(const std::vector<std::uint32_t>& diagMasks, const std::vector<std::uint32_t>& flipMasks) {
    diagMasks_.clear(), flipMasks_.clear();
    sitesAndPairs_ = 0;
    if (diagMasks.empty() && flipMasks.empty()) return Success;
    int sites = 0, nUp = 0;
    if (detail::IsComplex<Scalar>::value || !op_ || eigenex_spin_geometry(op_->handle(), &sites, &nUp) != 0) return InvalidInput;
    diagMasks_ = diagMasks, flipMasks_ = flipMasks;
    return Success;
  }
  // sigma_i for every site and sigma_i sigma_j for every pair i < j on the diagonal list, S+_i S-_j + S-_i S+_j for every pair on
  // the flip list: what correlationZZ, correlationXY and correlationSS read
  ComputationInfo setAllSitesAndPairs() {
    int sites = 0, nUp = 0;
    if (detail::IsComplex<Scalar>::value || !op_ || eigenex_spin_geometry(op_->handle(), &sites, &nUp) != 0) return InvalidInput;
    std::vector<std::uint32_t> d, f;
    for (int i = 0; i < sites; ++i) d.push_back(std::uint32_t(1) << i);
    for (int i = 0; i < sites; ++i)
      for (int j = i + 1; j < sites; ++j) f.push_back((std::uint32_t(1) << i) | (std::uint32_t(1) << j));
    d.insert(d.end(), f.begin(), f.end());
    const ComputationInfo r = setSpinObservables(d, f);
    if (r == Success) sitesAndPairs_ = sites;
    return r;
  }

  Index compute() {
    log_.clear();
    log_.push_back(headINFO() + "ThermalLanczosSolver::compute(...) was called");
    sums_.clear();
    matvecs_ = 0;
    info_ = Success;
    const bool given = !given_.empty();
    const Index R = given ? givenR_ : R_;
    if (!op_ || height_ <= 0 || M_ < 1 || M_ > 1000 || R < 1 || (given && givenN_ != height_)) {
      log_.push_back(headERROR() + "invalid input: a device operator, 1..1000 Lanczos steps and at least one vector of the operator's height are required");
      info_ = InvalidInput;
      return 0;
    }
    const int M = static_cast<int>(M_ < height_ ? M_ : height_);
    if (!dev_.alive() || devOp_ != op_.get() || dev_.capacity() < M + 2) {
      dev_.create(op_->context(), op_, height_, M + 2, 0, detail::IsComplex<Scalar>::value);
      devOp_ = op_.get();
    }
    sums_.setDimension(static_cast<double>(height_));
    const int nd = static_cast<int>(diagMasks_.size()), nf = static_cast<int>(flipMasks_.size());
    std::vector<double> alpha(static_cast<std::size_t>(M) + 2), beta(static_cast<std::size_t>(M) + 2), theta, S, gd, gf;
    Index breakdowns = 0;
    for (Index r = 0; r < R; ++r) {
      device::check(eigenex_basis_clear(dev_.handle()), "eigenex_basis_clear");
      if (given)
        device::check(eigenex_vec_upload(dev_.handle(), EIGENEX_VEC_W, reinterpret_cast<const double*>(given_.data() + static_cast<std::size_t>(r) * static_cast<std::size_t>(givenN_))),
                      "eigenex_vec_upload");
      else
        device::check(eigenex_vec_random_signs(dev_.handle(), EIGENEX_VEC_W, seed_, firstStream_ + static_cast<std::uint64_t>(r)), "eigenex_vec_random_signs");
      device::check(eigenex_lanczos_enqueue(dev_.handle(), M), "eigenex_lanczos_enqueue");
      eigenex_state_t st;
      device::check(eigenex_lanczos_state(dev_.handle(), &st, alpha.data(), beta.data()), "eigenex_lanczos_state");
      const int n = st.nalpha < st.nvec ? st.nalpha : st.nvec;
      if (n < 1) {
        log_.push_back(headERROR() + "sample " + std::to_string(r) + ": the start vector is zero");
        info_ = InvalidInput;
        sums_.clear();
        return 0;
      }
      matvecs_ += n;
      if (st.stopped) ++breakdowns;
      if (!small_eigen::tridiagonal(alpha.data(), beta.data(), n, theta, &S)) {
        log_.push_back(headERROR() + "sample " + std::to_string(r) + ": the tridiagonal eigenproblem did not converge");
        info_ = NoConvergence;
        sums_.clear();
        return 0;
      }
      ThermalSample sample;
      sample.theta = theta;
      sample.weight.resize(static_cast<std::size_t>(n));
      for (int j = 0; j < n; ++j) sample.weight[static_cast<std::size_t>(j)] = S[static_cast<std::size_t>(j) * n] * S[static_cast<std::size_t>(j) * n];
      if (nd + nf > 0) {
        gd.assign(static_cast<std::size_t>(nd) * n, 0.0), gf.assign(static_cast<std::size_t>(nf) * n, 0.0);
        device::check(eigenex_spin_measure_columns(dev_.handle(), EIGENEX_VEC_COL(0), 0, n, nd, nd ? diagMasks_.data() : nullptr, nf,
                                                   nf ? flipMasks_.data() : nullptr, nd ? gd.data() : nullptr, nf ? gf.data() : nullptr),
                      "eigenex_spin_measure_columns");
        sample.a.assign(static_cast<std::size_t>(nd + nf), std::vector<double>(static_cast<std::size_t>(n)));
        for (int t = 0; t < nd + nf; ++t) {
          const double* g = t < nd ? gd.data() + static_cast<std::size_t>(t) * n : gf.data() + static_cast<std::size_t>(t - nd) * n;
          for (int j = 0; j < n; ++j) {
            const double* s = S.data() + static_cast<std::size_t>(j) * n;  // Ritz vector j in the Lanczos basis
            double dot = 0.0;
            for (int i = 0; i < n; ++i) dot += s[i] * g[i];
            sample.a[static_cast<std::size_t>(t)][static_cast<std::size_t>(j)] = s[0] * dot;
          }
        }
      }
      sums_.addSample(std::move(sample));
    }
    log_.push_back(headINFO() + "samples: " + std::to_string(R) + (given ? " (given vectors)" : " (random sign vectors)") + ", steps per sample: at most " +
                   std::to_string(M) + ", ended by a breakdown: " + std::to_string(breakdowns) + ", operator applications: " + std::to_string(matvecs_) +
                   ", observables: " + std::to_string(nd) + " diagonal, " + std::to_string(nf) + " flip");
    return 0;
  }

  // ---- results ----
  Index dimension() const { return height_; }
  Index samples() const { return static_cast<Index>(sums_.samples()); }
  Index operatorApplications() const { return matvecs_; }
  Index diagonalTerms() const { return static_cast<Index>(diagMasks_.size()); }
  Index flipTerms() const { return static_cast<Index>(flipMasks_.size()); }
  int sitesWithAllPairs() const { return sitesAndPairs_; }  // 0 unless the masks came from setAllSitesAndPairs
  ComputationInfo info() const { return info_; }
  const std::vector<std::string>& log() const { return log_; }
  const ThermalSums& sums() const { return sums_; }

  double logPartitionFunction(double beta) const { return sums_.logPartitionFunction(beta); }
  double energy(double beta) const { return sums_.energy(beta); }
  double specificHeat(double beta) const { return sums_.specificHeat(beta); }
  double entropy(double beta) const { return sums_.entropy(beta); }
  double freeEnergy(double beta) const { return sums_.freeEnergy(beta); }
  // the raw thermal averages of the mask lists: <prod sigma> and <S+S- + S-S+> (or <2 Sx> of a one-bit flip mask)
  double diagonal(Index t, double beta) const { return sums_.observable(diagIndex_(t), beta); }
  double flip(Index t, double beta) const { return sums_.observable(flipIndex_(t), beta); }
  // <Sz_i Sz_j>, <Sx_i Sx_j + Sy_i Sy_j> and <S_i . S_j> after setAllSitesAndPairs; i = j gives 1/4, 1/2 and 3/4
  double correlationZZ(int i, int j, double beta) const {
    const Index p = pair_(i, j);
    return i == j ? 0.25 : diagonal(sitesAndPairs_ + p, beta) / 4;
  }
  double correlationXY(int i, int j, double beta) const {
    const Index p = pair_(i, j);
    return i == j ? 0.5 : flip(p, beta) / 2;
  }
  double correlationSS(int i, int j, double beta) const { return correlationZZ(i, j, beta) + correlationXY(i, j, beta); }

  // delete-one jackknife over the samples (thermal_sums.hpp says what it covers); t is the index into the diagonal list followed
  // by the flip list, as observableIndexOfZZ and observableIndexOfXY give it
  double standardError(ThermalQuantity q, double beta, Index t = 0) const { return sums_.standardError(q, beta, static_cast<std::size_t>(t)); }
  Index observableIndexOfDiagonal(Index t) const { return static_cast<Index>(diagIndex_(t)); }
  Index observableIndexOfFlip(Index t) const { return static_cast<Index>(flipIndex_(t)); }
  Index observableIndexOfZZ(int i, int j) const { return static_cast<Index>(diagIndex_(sitesAndPairs_ + pair_(i, j))); }
  Index observableIndexOfXY(int i, int j) const { return static_cast<Index>(flipIndex_(pair_(i, j))); }

 private:
  std::size_t diagIndex_(Index t) const {
    if (t < 0 || t >= static_cast<Index>(diagMasks_.size())) throw LanczosException("ThermalLanczosSolver: no such diagonal observable");
    return static_cast<std::size_t>(t);
  }
  std::size_t flipIndex_(Index t) const {
    if (t < 0 || t >= static_cast<Index>(flipMasks_.size())) throw LanczosException("ThermalLanczosSolver: no such flip observable");
    return diagMasks_.size() + static_cast<std::size_t>(t);
  }
  // the place of the pair {i, j} in the list of pairs a < b, a ascending, then b
  Index pair_(int i, int j) const {
    const int L = sitesAndPairs_;
    if (L == 0) throw LanczosException("ThermalLanczosSolver: the correlations need setAllSitesAndPairs()");
    if (i < 0 || j < 0 || i >= L || j >= L) throw LanczosException("ThermalLanczosSolver: a site is outside the model");
    const int a = i < j ? i : j, b = i < j ? j : i;
    return static_cast<Index>(a) * L - static_cast<Index>(a) * (a + 1) / 2 + (b - a - 1);
  }

  std::shared_ptr<device::CsrOperator> op_;
  const device::CsrOperator* devOp_ = nullptr;
  detail::KrylovDevice dev_;
  Index height_ = 0, M_ = 100, R_ = 20, matvecs_ = 0, givenN_ = 0, givenR_ = 0;
  std::uint64_t seed_ = 0, firstStream_ = 0;
  std::vector<Scalar> given_;
  std::vector<std::uint32_t> diagMasks_, flipMasks_;
  int sitesAndPairs_ = 0;
  ThermalSums sums_;
  ComputationInfo info_ = Success;
  std::vector<std::string> log_;
};

// Sectors added up.  A sector enters with a multiplicity m_k and a magnetisation M_k = n_up - L / 2; Z = sum_k m_k Z_k, and every
// average is weighted with p_k = m_k Z_k / Z.  Multiplicity 2 stands for the sector and its image under spin inversion, at +M_k
// and -M_k (what n_up < L / 2 is at hz = 0): it counts twice in Z and M^2 and cancels in <M>.  observable(t, beta) weights the
// sectors' <A_t> the same way, so the caller vouches that the term is invariant under the symmetry behind a multiplicity of 2:
// under spin inversion that holds for diagonal masks with an even number of sites and for pair flips, not for sigma_i.
class ThermalEnsemble {
 public:
  explicit ThermalEnsemble(int sites = 0) : sites_(sites) {}
  void setSites(int sites) { sites_ = sites; }
  void clear() { parts_.clear(); }
  std::size_t sectors() const { return parts_.size(); }

  template <class Solver>
  void add(const Solver& solver, double multiplicity, double magnetisation) {
    add(solver.sums(), multiplicity, magnetisation);
  }
  void add(const ThermalSums& sums, double multiplicity, double magnetisation) {
    if (sums.samples() == 0 || !(multiplicity > 0.0)) throw LanczosException("ThermalEnsemble: a sector needs computed samples and a positive multiplicity");
    parts_.push_back(Part{sums, multiplicity, magnetisation});
  }

  double logPartitionFunction(double beta) const { return weights_(beta, nullptr); }
  double energy(double beta) const {
    std::vector<double> p;
    weights_(beta, &p);
    double e = 0.0;
    for (std::size_t k = 0; k < parts_.size(); ++k) e += p[k] * parts_[k].sums.energy(beta);
    return e;
  }
  double specificHeat(double beta) const {
    std::vector<double> p;
    weights_(beta, &p);
    const double e = energy(beta);
    double var = 0.0;  // sum_k p_k (var_k + (E_k - E)^2)
    for (std::size_t k = 0; k < parts_.size(); ++k) {
      double ek = 0.0, vk = 0.0;
      parts_[k].sums.moments(beta, nullptr, &ek, &vk);
      var += p[k] * (vk + (ek - e) * (ek - e));
    }
    return beta * beta * var;
  }
  double entropy(double beta) const { return beta * energy(beta) + logPartitionFunction(beta); }
  // beta (<M^2> - <M>^2) / L from the sector partition functions alone
  double susceptibility(double beta) const {
    if (sites_ < 1) throw LanczosException("ThermalEnsemble: the susceptibility per site needs the number of sites");
    std::vector<double> p;
    weights_(beta, &p);
    double m1 = 0.0, m2 = 0.0;
    for (std::size_t k = 0; k < parts_.size(); ++k) {
      m2 += p[k] * parts_[k].magnetisation * parts_[k].magnetisation;
      if (parts_[k].multiplicity != 2.0) m1 += p[k] * parts_[k].magnetisation;
    }
    return beta * (m2 - m1 * m1) / sites_;
  }
  double observable(std::size_t t, double beta) const {
    std::vector<double> p;
    weights_(beta, &p);
    double a = 0.0;
    for (std::size_t k = 0; k < parts_.size(); ++k) a += p[k] * parts_[k].sums.observable(t, beta);
    return a;
  }

 private:
  struct Part {
    ThermalSums sums;
    double multiplicity, magnetisation;
  };
  // log Z, and p_k = m_k Z_k / Z if wanted: log-sum-exp over the sectors
  double weights_(double beta, std::vector<double>* p) const {
    if (parts_.empty()) throw LanczosException("ThermalEnsemble: no sector");
    std::vector<double> l(parts_.size());
    double top = -std::numeric_limits<double>::infinity();
    for (std::size_t k = 0; k < parts_.size(); ++k) {
      l[k] = std::log(parts_[k].multiplicity) + parts_[k].sums.logPartitionFunction(beta);
      top = l[k] > top ? l[k] : top;
    }
    double s = 0.0;
    for (double v : l) s += std::exp(v - top);
    if (p) {
      p->resize(l.size());
      for (std::size_t k = 0; k < l.size(); ++k) (*p)[k] = std::exp(l[k] - top) / s;
    }
    return top + std::log(s);
  }
  int sites_;
  std::vector<Part> parts_;
};

}  // namespace EigenEx
}  // namespace cmpt
