// Reduced density matrix and entanglement of a state of a matrix-free spin-1/2 operator (spin_operator.hpp), formed on the
// device in one call.
//
// NOT part of the reference.  For a real vector v over the rows of device::spinHalfOperator (full space) or
// device::spinHalfSectorOperator (nUp sites up) and a subsystem A of at most 12 (full space) or 14 (sector) sites, compute()
// forms rho_A = Tr_B |v><v| / <v|v> without downloading v (eigenex_spin_rdm: rho_A = M M^T with M gathered through the sector's
// rank tables and never stored).  In a sector rho_A is block-diagonal in the number of up sites inside A; the full space has one
// block.  From the blocks follow, on the host,
//   spectrum()       all eigenvalues of rho_A, descending (small_eigen::symmetric per block); values below 0 at rounding level are 0
//   entropy()        S = -sum lambda ln lambda, the von Neumann entanglement entropy
//   renyi(alpha)     ln(sum lambda^alpha) / (1 - alpha), alpha != 1
//   renyi2()         -ln ||rho||_F^2, without an eigen-solve
//   schmidtRank(tol) the number of eigenvalues above tol
// Mutual information and the like are combinations of calls with different subsystems.  The vector is a host vector (e.g. a
// column of a solver's eigenvectors()) and is uploaded by compute().
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "lanczos.hpp"
#include "small_eigen.hpp"
#include "spin_operator.hpp"

namespace cmpt {
namespace EigenEx {

class SpinEntanglementSolver {
 public:
  using Index = EigenEx::Index;
  using VectorType = DenseVector<double>;

  static std::string headERROR() { return std::string("ERROR     "); }
  static std::string headINFO() { return std::string("INFO      "); }

  SpinEntanglementSolver& setDeviceOperator(const std::shared_ptr<device::CsrOperator>& op) {
    op_ = op;
    height_ = op ? static_cast<Index>(op->rows()) : 0;
    return *this;
  }
  SpinEntanglementSolver& setState(const VectorType& v) {
    state_ = v;
    return *this;
  }
  // the sites of the subsystem; a site outside 0..31 or named twice makes compute() report invalid input
  SpinEntanglementSolver& setSubsystem(const std::vector<int>& sites) {
    mask_ = 0, sitesValid_ = true;
    for (int i : sites) {
      if (i < 0 || i > 31 || ((mask_ >> i) & 1u)) sitesValid_ = false;
      else mask_ |= std::uint32_t(1) << i;
    }
    return *this;
  }
  SpinEntanglementSolver& setSubsystemMask(std::uint32_t mask) {
    mask_ = mask, sitesValid_ = true;
    return *this;
  }
  Index matrixHeight() const { return height_; }
  int sites() const { return sites_; }
  int sitesUp() const { return nUp_; }  // -1: the full space
  std::uint32_t subsystemMask() const { return mask_; }
  double normSquared() const { return norm2_; }

  Index compute() {
    log_.clear();
    log_.push_back(headINFO() + "SpinEntanglementSolver::compute(...) was called");
    info_ = Success;
    clear_();
    if (!op_ || height_ <= 0 || eigenex_spin_geometry(op_->handle(), &sites_, &nUp_) != 0) {
      sites_ = 0;
      return invalid_("invalid input: a matrix-free spin operator (device::spinHalfOperator, device::spinHalfSectorOperator) is required");
    }
    if (static_cast<Index>(state_.size()) != height_) return invalid_("invalid input: the state must have one entry per row of the operator");
    if (!sitesValid_) return invalid_("invalid input: the subsystem names a site outside 0..31 or names a site twice");
    int nBlocks = 0, kFirst = 0;
    std::int64_t dims[33], offsets[34];
    if (eigenex_spin_rdm_layout(sites_, nUp_, mask_, &nBlocks, &kFirst, dims, offsets) != 0) return invalid_(std::string("invalid input: ") + eigenex_last_error());
    if (!dev_.alive() || devOp_ != op_.get()) {
      dev_.create(op_->context(), op_, height_, 1, 0, false);
      devOp_ = op_.get();
    }
    dev_.upload(EIGENEX_VEC_COL(0), state_);
    std::vector<double> raw(static_cast<std::size_t>(offsets[nBlocks]), 0.0);
    device::check(eigenex_spin_rdm(dev_.handle(), EIGENEX_VEC_COL(0), mask_, raw.data(), static_cast<std::int64_t>(raw.size())), "eigenex_spin_rdm");
    // the trace, block by block and along the diagonal: sum_s v_s^2
    double trace = 0.0;
    for (int n = 0; n < nBlocks; ++n)
      for (std::int64_t i = 0; i < dims[n]; ++i) trace += raw[static_cast<std::size_t>(offsets[n] + i + i * dims[n])];
    if (!(trace > 0.0) || !std::isfinite(trace)) return invalid_("invalid input: the state is zero (or not finite)");
    norm2_ = trace;
    frob2_ = 0.0;
    for (int n = 0; n < nBlocks; ++n) {
      const std::size_t d = static_cast<std::size_t>(dims[n]);
      std::vector<double> rho(raw.begin() + static_cast<std::ptrdiff_t>(offsets[n]), raw.begin() + static_cast<std::ptrdiff_t>(offsets[n + 1]));
      for (double& e : rho) e /= trace;
      for (double e : rho) frob2_ += e * e;
      std::vector<double> work(rho), values, vectors;
      if (!small_eigen::symmetric(work, static_cast<int>(d), values, vectors)) {
        clear_();
        log_.push_back(headERROR() + "the eigen-solve of a block of the reduced density matrix did not converge");
        info_ = NoConvergence;
        return 0;
      }
      for (double lam : values) spectrum_.push_back(lam > 0.0 ? lam : 0.0);
      blockUp_.push_back(kFirst + n), blockDim_.push_back(static_cast<Index>(d));
      rho_.push_back(std::move(rho));
    }
    std::sort(spectrum_.begin(), spectrum_.end(), std::greater<double>());
    log_.push_back(headINFO() + "sites: " + std::to_string(sites_) + (nUp_ < 0 ? std::string(", full space") : ", sites up: " + std::to_string(nUp_)) +
                   ", subsystem sites: " + std::to_string(__builtin_popcount(mask_)) + ", blocks: " + std::to_string(nBlocks) +
                   ", eigenvalues: " + std::to_string(spectrum_.size()));
    return 0;
  }

  // ---- results (after a successful compute(); a block outside 0..blocks()-1 throws) ----
  Index blocks() const { return static_cast<Index>(rho_.size()); }
  int blockSitesUp(Index n) const { return blockUp_[block_(n)]; }  // up sites inside the subsystem; 0 in the full space
  Index blockDimension(Index n) const { return blockDim_[block_(n)]; }
  // block n of rho_A, normalised to unit trace over all blocks: column-major blockDimension(n)^2, symmetric bit for bit
  const std::vector<double>& reducedDensityMatrix(Index n) const { return rho_[block_(n)]; }
  const std::vector<double>& spectrum() const { return spectrum_; }
  double entropy() const {
    double s = 0.0;
    for (double lam : spectrum_)
      if (lam > 0.0) s -= lam * std::log(lam);
    return s;
  }
  double renyi(double alpha) const {
    if (alpha == 1.0 || spectrum_.empty()) throw LanczosException("SpinEntanglementSolver::renyi: alpha must not be 1 (that is entropy()), and compute() comes first");
    double s = 0.0;
    for (double lam : spectrum_)
      if (lam > 0.0) s += std::pow(lam, alpha);
    return std::log(s) / (1.0 - alpha);
  }
  double renyi2() const {
    if (rho_.empty()) throw LanczosException("SpinEntanglementSolver::renyi2: no result (compute() first)");
    return -std::log(frob2_);
  }
  Index schmidtRank(double tol) const {
    Index r = 0;
    for (double lam : spectrum_) r += lam > tol ? 1 : 0;
    return r;
  }
  ComputationInfo info() const { return info_; }
  const std::vector<std::string>& log() const { return log_; }

 private:
  void clear_() {
    norm2_ = 0.0, frob2_ = 0.0;
    rho_.clear(), spectrum_.clear(), blockUp_.clear(), blockDim_.clear();
  }
  Index invalid_(const std::string& what) {
    log_.push_back(headERROR() + what);
    info_ = InvalidInput;
    clear_();
    return 0;
  }
  std::size_t block_(Index n) const {
    if (n < 0 || n >= static_cast<Index>(rho_.size())) throw LanczosException("SpinEntanglementSolver: no such block (compute() first; blocks are 0..blocks()-1)");
    return static_cast<std::size_t>(n);
  }

  std::shared_ptr<device::CsrOperator> op_;
  const device::CsrOperator* devOp_ = nullptr;
  detail::KrylovDevice dev_;
  Index height_ = 0;
  VectorType state_;
  std::uint32_t mask_ = 0;
  bool sitesValid_ = true;
  int sites_ = 0, nUp_ = -1;
  double norm2_ = 0.0, frob2_ = 0.0;
  std::vector<std::vector<double>> rho_;
  std::vector<int> blockUp_;
  std::vector<Index> blockDim_;
  std::vector<double> spectrum_;
  ComputationInfo info_ = Success;
  std::vector<std::string> log_;
};

}  // namespace EigenEx
}  // namespace cmpt
