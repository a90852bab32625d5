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
//
// A complex state (setState(DenseVector<std::complex<double>>)) needs the operator for complex states
// (device::spinHalfComplexOperator) and goes through eigenex_spin_rdm_z: rho_A = M M^H, Hermitian, its blocks are read with
// reducedDensityMatrixComplex(n) and diagonalised by small_eigen::hermitian; everything that follows from the spectrum is the same
// code (detail::EntanglementBlocks, which SpinTimeEvolutionSolver shares for the state it holds on the device).
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "lanczos.hpp"
#include "small_eigen.hpp"
#include "spin_frontend.hpp"
#include "spin_operator.hpp"

namespace cmpt {
namespace EigenEx {

namespace detail {

// The blocks of a raw reduced density matrix (eigenex_spin_rdm: real entries; eigenex_spin_rdm_z: interleaved pairs) brought to
// unit trace and diagonalised, and the entropies of the spectrum.  One copy for SpinEntanglementSolver and
// SpinTimeEvolutionSolver.
struct EntanglementBlocks {
  enum Status { Ok, ZeroState, NoConvergence };
  bool complexState = false;
  double norm2 = 0.0, frob2 = 0.0;
  std::vector<std::vector<double>> rho;                  // real state: the unit-trace blocks, column-major
  std::vector<std::vector<std::complex<double>>> rhoZ;   // complex state
  std::vector<int> blockUp;
  std::vector<Index> blockDim;
  std::vector<double> spectrum;  // descending, clamped at 0

  void clear() {
    norm2 = 0.0, frob2 = 0.0;
    rho.clear(), rhoZ.clear(), spectrum.clear(), blockUp.clear(), blockDim.clear();
  }
  std::size_t blocks() const { return blockDim.size(); }

  // raw: offsets[nBlocks] doubles (real) or twice as many (complex)
  Status assemble(const std::vector<double>& raw, bool isComplex, int nBlocks, int kFirst, const std::int64_t* dims, const std::int64_t* offsets) {
    clear();
    complexState = isComplex;
    const std::size_t w = isComplex ? 2 : 1;
    // the trace, block by block and along the diagonal: sum_s |v_s|^2
    double trace = 0.0;
    for (int n = 0; n < nBlocks; ++n)
      for (std::int64_t i = 0; i < dims[n]; ++i) trace += raw[w * static_cast<std::size_t>(offsets[n] + i + i * dims[n])];
    if (!(trace > 0.0) || !std::isfinite(trace)) return ZeroState;
    norm2 = trace;
    for (int n = 0; n < nBlocks; ++n) {
      const std::size_t d = static_cast<std::size_t>(dims[n]);
      std::vector<double> values;
      bool ok;
      if (isComplex) {
        std::vector<std::complex<double>> r(d * d);
        for (std::size_t e = 0; e < d * d; ++e) {
          const std::size_t at = 2 * (static_cast<std::size_t>(offsets[n]) + e);
          r[e] = std::complex<double>(raw[at] / trace, raw[at + 1] / trace);
          frob2 += r[e].real() * r[e].real() + r[e].imag() * r[e].imag();
        }
        ok = small_eigen::hermitian(r, static_cast<int>(d), values, nullptr);
        rhoZ.push_back(std::move(r));
      } else {
        std::vector<double> r(raw.begin() + static_cast<std::ptrdiff_t>(offsets[n]), raw.begin() + static_cast<std::ptrdiff_t>(offsets[n + 1]));
        for (double& e : r) e /= trace;
        for (double e : r) frob2 += e * e;
        std::vector<double> work(r), vectors;
        ok = small_eigen::symmetric(work, static_cast<int>(d), values, vectors);
        rho.push_back(std::move(r));
      }
      if (!ok) {
        clear();
        return NoConvergence;
      }
      for (double lam : values) spectrum.push_back(lam > 0.0 ? lam : 0.0);
      blockUp.push_back(kFirst + n), blockDim.push_back(static_cast<Index>(d));
    }
    std::sort(spectrum.begin(), spectrum.end(), std::greater<double>());
    return Ok;
  }
  double entropy() const {
    double s = 0.0;
    for (double lam : spectrum)
      if (lam > 0.0) s -= lam * std::log(lam);
    return s;
  }
  double renyi(double alpha) const {
    double s = 0.0;
    for (double lam : spectrum)
      if (lam > 0.0) s += std::pow(lam, alpha);
    return std::log(s) / (1.0 - alpha);
  }
  double renyi2() const { return -std::log(frob2); }  // -ln ||rho||_F^2: no eigen-solve in it
};

}  // namespace detail

class SpinEntanglementSolver {
 public:
  using Index = EigenEx::Index;
  using VectorType = DenseVector<double>;
  using Complex = std::complex<double>;
  using ComplexVectorType = DenseVector<Complex>;

  static std::string headERROR() { return detail::CallLog::headERROR(); }
  static std::string headINFO() { return detail::CallLog::headINFO(); }

  SpinEntanglementSolver& setDeviceOperator(const std::shared_ptr<device::CsrOperator>& op) {
    op_ = op;
    height_ = op ? static_cast<Index>(op->rows()) : 0;
    return *this;
  }
  SpinEntanglementSolver& setState(const VectorType& v) {
    state_ = v, stateZ_ = ComplexVectorType(), complex_ = false;
    return *this;
  }
  // a complex state: the operator must then be one for complex states (device::spinHalfComplexOperator)
  SpinEntanglementSolver& setState(const ComplexVectorType& v) {
    stateZ_ = v, state_ = VectorType(), complex_ = true;
    return *this;
  }
  bool stateIsComplex() const { return complex_; }
  // the sites of the subsystem; a site outside 0..31 or named twice makes compute() report invalid input
  SpinEntanglementSolver& setSubsystem(const std::vector<int>& sites) {
    sitesValid_ = true;
    mask_ = detail::siteMask(sites, sitesValid_);
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
  double normSquared() const { return r_.norm2; }

  Index compute() {
    log_.begin("SpinEntanglementSolver", "compute");
    clear_();
    if (!op_ || height_ <= 0 || eigenex_spin_geometry(op_->handle(), &sites_, &nUp_) != 0) {
      sites_ = 0;
      return invalid_("invalid input: a matrix-free spin operator (device::spinHalfOperator, device::spinHalfSectorOperator) is required");
    }
    if (static_cast<Index>(complex_ ? stateZ_.size() : state_.size()) != height_) return invalid_("invalid input: the state must have one entry per row of the operator");
    if (!sitesValid_) return invalid_("invalid input: the subsystem names a site outside 0..31 or names a site twice");
    int nBlocks = 0, kFirst = 0;
    std::int64_t dims[33], offsets[34];
    if (eigenex_spin_rdm_layout(sites_, nUp_, mask_, &nBlocks, &kFirst, dims, offsets) != 0) return invalid_(std::string("invalid input: ") + eigenex_last_error());
    if (!dev_.alive() || devOp_ != op_.get() || devComplex_ != complex_) {
      if (complex_) {
        // a complex state is refused by an operator for real states (the library's scalar-type check)
        try {
          dev_.create(op_->context(), op_, height_, 1, 0, true);
        } catch (const LanczosException&) {
          devOp_ = nullptr;
          return invalid_("invalid input: a complex state needs the matrix-free spin operator for complex states (device::spinHalfComplexOperator: eigenex_spin_upload_z, eigenex_spin_sector_upload_z)");
        }
      } else {
        dev_.create(op_->context(), op_, height_, 1, 0, false);
      }
      devOp_ = op_.get(), devComplex_ = complex_;
    }
    std::vector<double> raw(static_cast<std::size_t>(offsets[nBlocks]) * (complex_ ? 2 : 1), 0.0);
    if (complex_) {
      dev_.upload(EIGENEX_VEC_COL(0), stateZ_);
      device::check(eigenex_spin_rdm_z(dev_.handle(), EIGENEX_VEC_COL(0), mask_, raw.data(), static_cast<std::int64_t>(raw.size())), "eigenex_spin_rdm_z");
    } else {
      dev_.upload(EIGENEX_VEC_COL(0), state_);
      device::check(eigenex_spin_rdm(dev_.handle(), EIGENEX_VEC_COL(0), mask_, raw.data(), static_cast<std::int64_t>(raw.size())), "eigenex_spin_rdm");
    }
    switch (r_.assemble(raw, complex_, nBlocks, kFirst, dims, offsets)) {
      case detail::EntanglementBlocks::ZeroState:
        return invalid_("invalid input: the state is zero (or not finite)");
      case detail::EntanglementBlocks::NoConvergence:
        return log_.failed("the eigen-solve of a block of the reduced density matrix did not converge", NoConvergence);
      case detail::EntanglementBlocks::Ok:
        break;
    }
    log_.note("sites: " + std::to_string(sites_) + (nUp_ < 0 ? std::string(", full space") : ", sites up: " + std::to_string(nUp_)) +
                   ", subsystem sites: " + std::to_string(detail::popcount(mask_)) + ", blocks: " + std::to_string(nBlocks) +
                   ", eigenvalues: " + std::to_string(r_.spectrum.size()));
    return 0;
  }

  // ---- results (after a successful compute(); a block outside 0..blocks()-1 throws) ----
  Index blocks() const { return static_cast<Index>(r_.blocks()); }
  int blockSitesUp(Index n) const { return r_.blockUp[block_(n)]; }  // up sites inside the subsystem; 0 in the full space
  Index blockDimension(Index n) const { return r_.blockDim[block_(n)]; }
  // block n of rho_A, normalised to unit trace over all blocks: column-major blockDimension(n)^2, symmetric bit for bit.  Real
  // states only: for a complex state it throws (the real part alone is not the block), see reducedDensityMatrixComplex
  const std::vector<double>& reducedDensityMatrix(Index n) const {
    const std::size_t at = block_(n);
    if (r_.complexState) throw LanczosException("SpinEntanglementSolver::reducedDensityMatrix: the state is complex (reducedDensityMatrixComplex)");
    return r_.rho[at];
  }
  // the same of a complex state: Hermitian bit for bit, the diagonal's imaginary parts +0.0; throws for a real state
  const std::vector<Complex>& reducedDensityMatrixComplex(Index n) const {
    const std::size_t at = block_(n);
    if (!r_.complexState) throw LanczosException("SpinEntanglementSolver::reducedDensityMatrixComplex: the state is real (reducedDensityMatrix)");
    return r_.rhoZ[at];
  }
  const std::vector<double>& spectrum() const { return r_.spectrum; }
  double entropy() const { return r_.entropy(); }
  double renyi(double alpha) const {
    if (alpha == 1.0 || r_.spectrum.empty()) throw LanczosException("SpinEntanglementSolver::renyi: alpha must not be 1 (that is entropy()), and compute() comes first");
    return r_.renyi(alpha);
  }
  double renyi2() const {
    if (r_.blocks() == 0) throw LanczosException("SpinEntanglementSolver::renyi2: no result (compute() first)");
    return r_.renyi2();
  }
  Index schmidtRank(double tol) const {
    Index r = 0;
    for (double lam : r_.spectrum) r += lam > tol ? 1 : 0;
    return r;
  }
  ComputationInfo info() const { return log_.info(); }
  const std::vector<std::string>& log() const { return log_.log(); }

 private:
  void clear_() { r_.clear(); }
  Index invalid_(const std::string& what) {
    clear_();
    return log_.invalid(what);
  }
  std::size_t block_(Index n) const {
    if (n < 0 || n >= static_cast<Index>(r_.blocks())) throw LanczosException("SpinEntanglementSolver: no such block (compute() first; blocks are 0..blocks()-1)");
    return static_cast<std::size_t>(n);
  }

  std::shared_ptr<device::CsrOperator> op_;
  const device::CsrOperator* devOp_ = nullptr;
  detail::KrylovDevice dev_;
  Index height_ = 0;
  VectorType state_;
  ComplexVectorType stateZ_;
  bool complex_ = false, devComplex_ = false;
  std::uint32_t mask_ = 0;
  bool sitesValid_ = true;
  int sites_ = 0, nUp_ = -1;
  detail::EntanglementBlocks r_;
  detail::CallLog log_;
};

}  // namespace EigenEx
}  // namespace cmpt
