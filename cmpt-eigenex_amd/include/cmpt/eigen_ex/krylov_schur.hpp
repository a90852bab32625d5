// Krylov-Schur (thick-restart Arnoldi) eigensolver: the eigenvalues of largest magnitude of a general operator from a
// basis of fixed size, on the device Krylov state of arnoldi.hpp.
//
// NOT part of the reference: versmc/cmpt-eigenex has no restart of any kind, and its ArnoldiEigenSolver
// grows the basis by one column per step until it converges or memory ends.  Built from the reference's own
// ingredients -- the Arnoldi step with full orthogonalisation (arnoldi.hpp:312-392), the Ritz back-transform
// (:841-865), the same setters -- plus the Krylov-Schur restart of Stewart (SIAM J. Matrix Anal. Appl. 23 (2001) 601):
// after m steps  A V_m = V_m H_m + w e_m^T;  keep an orthonormal basis Q of the invariant subspace of H_m that belongs
// to the `keep` Ritz values of largest magnitude; then  A (V_m Q) = (V_m Q) (Q^H H_m Q) + w (e_m^T Q),  a Krylov
// decomposition whose projected matrix is full in its leading block.  The Arnoldi step needs nothing else: it
// orthogonalises against all columns anyway, so the run continues from column `keep` with w as the next vector.
// Memory stays bounded at (m + keep + 1) basis columns however long the run is.
//
// Convergence: residual estimate residue * |s_i[m-1]| <= tolerance * |theta_first - theta_last| for the first
// numberOfEigenvalues() Ritz pairs, the scale ArnoldiEigenSolver and the thick-restart Lanczos use.
#pragma once

#include "arnoldi.hpp"

namespace cmpt {
namespace EigenEx {

template <class Scalar_>
class KrylovSchurEigenSolver {
  static_assert(detail::SupportedScalar<Scalar_>::value, "cmpt-eigenex_amd: Scalar must be double, std::complex<double>, float or std::complex<float>");

 public:
  using Index = EigenEx::Index;
  using Scalar = Scalar_;
  using RealScalar = typename RealOf<Scalar_>::type;
  using ComplexScalar = std::complex<RealScalar>;
  using VectorType = DenseVector<Scalar>;
  using RealVectorType = DenseVector<RealScalar>;
  using ComplexVectorType = DenseVector<ComplexScalar>;
  using ComplexMatrixType = DenseMatrix<ComplexScalar>;
  using MatMulFunction = std::function<void(const Scalar*, Scalar*)>;

  static std::string headERROR() { return std::string("ERROR     "); }
  static std::string headWARN() { return std::string("WARN      "); }
  static std::string headINFO() { return std::string("INFO      "); }

  // ---- operator and start vector: same meaning as in ArnoldiEigenSolver ----
  KrylovSchurEigenSolver& setMatrixMultiplication(const MatMulFunction& matmul, Index height) {
    matmul_ = matmul;
    height_ = height;
    op_.reset();
    return *this;
  }
  KrylovSchurEigenSolver& setDeviceOperator(const std::shared_ptr<device::CsrOperator>& op) {
    op_ = op;
    matmul_ = nullptr;
    height_ = op ? static_cast<Index>(op->rows()) : 0;
    if (op) ctx_ = op->context();
    return *this;
  }
  KrylovSchurEigenSolver& setDeviceContext(const std::shared_ptr<device::Context>& ctx) {
    ctx_ = ctx;
    return *this;
  }
  KrylovSchurEigenSolver& setInitialVector(const VectorType& v) {
    initial_ = v;
    return *this;
  }
  KrylovSchurEigenSolver& setInitialVector() {
    std::mt19937 rengine;
    initial_ = ArnoldiBase<Scalar>::makeRandomVector(rengine, height_);
    return *this;
  }
  KrylovSchurEigenSolver& setEigenvalueShift(Scalar s) {  // a Scalar, as in ArnoldiBase (arnoldi.hpp:108)
    shift_ = s;
    return *this;
  }
  KrylovSchurEigenSolver& setThreshold(RealScalar t) {
    threshold_ = t;
    return *this;
  }
  // ---- restart control ----
  KrylovSchurEigenSolver& setNumberOfEigenvalues(Index nev) {
    nev_ = nev;
    return *this;
  }
  KrylovSchurEigenSolver& setMaxBasisSize(Index m) {  // Arnoldi vectors per cycle (default 128)
    m_ = m;
    return *this;
  }
  KrylovSchurEigenSolver& setKeepSize(Index keep) {  // dimension kept at a restart; -1: nev + (m - nev)/2
    keep_ = keep;
    return *this;
  }
  KrylovSchurEigenSolver& setTolerance(RealScalar tol) {
    tolerance_ = tol;
    return *this;
  }
  KrylovSchurEigenSolver& setMaxRestarts(Index r) {
    maxRestarts_ = r;
    return *this;
  }
  KrylovSchurEigenSolver& setComputeEigenvectorsOn(bool on) {
    vectorsOn_ = on;
    return *this;
  }
  Index matrixHeight() const { return height_; }
  Index numberOfEigenvalues() const { return nev_; }
  Index maxBasisSize() const { return m_; }
  RealScalar tolerance() const { return tolerance_; }

  // ---- results ----
  const ComplexVectorType& eigenvalues() const { return eigenvalues_; }    // |lambda| descending, shift removed
  const ComplexMatrixType& eigenvectors() const { return eigenvectors_; }  // normalised, phase-fixed (arnoldi.hpp:854-865)
  const RealVectorType& residuals() const { return residuals_; }           // residue |s_i[m-1]| of the returned pairs
  Index restarts() const { return restarts_; }
  Index operatorApplications() const { return matvecs_; }
  const std::vector<std::string>& log() const { return log_; }
  ComputationInfo info() const { return info_; }

  Index compute() {
    using W = typename detail::Wide<Scalar>::type;  // the device's scalar: fp64, real or complex
    log_.clear();
    log_.push_back(headINFO() + "KrylovSchurEigenSolver::compute(...) was called");
    eigenvalues_.resize(0);
    eigenvectors_.resize(0, 0);
    residuals_.resize(0);
    restarts_ = matvecs_ = 0;
    info_ = Success;
    if (height_ <= 0 || (!op_ && !matmul_) || nev_ < 1) {
      log_.push_back(headERROR() + "invalid input: matrix height, operator or number of eigenvalues");
      info_ = InvalidInput;
      return 0;
    }
    if (initial_.size() != height_) setInitialVector();
    const Index m = std::max<Index>(1, std::min<Index>(m_, height_));
    const Index nev = std::min<Index>(nev_, m);
    Index keep = keep_ >= 0 ? keep_ : nev + (m - nev) / 2;
    keep = std::max<Index>(1, std::min<Index>(keep, m - 1));
    if (!ctx_) ctx_ = op_ ? op_->context() : device::defaultContext();

    // the slab (m + keep + 1 columns: the basis, the scratch columns of the restart, one more when a conjugate pair makes
    // keep grow) is kept from one compute() to the next
    const int cap = static_cast<int>(m + keep + 1);
    if (!dev_.alive() || devHeight_ != height_ || devOp_ != op_.get() || devCtx_ != ctx_.get() || dev_.capacity() < cap) {
      dev_.create(ctx_, op_, height_, cap, 0, detail::IsComplex<Scalar>::value);
      devHeight_ = height_;
      devOp_ = op_.get();
      devCtx_ = ctx_.get();
    } else {
      device::check(eigenex_basis_clear(dev_.handle()), "eigenex_basis_clear");
    }
    if (!op_) {
      thunk_.fn = matmul_;
      thunk_.n = height_;
      device::check(eigenex_basis_set_host_operator(dev_.handle(), &detail::HostOperatorThunk<Scalar>::call, &thunk_), "eigenex_basis_set_host_operator");
    }
    const std::complex<double> sh(shift_);
    // the Arnoldi vector A q_k has O(1) components along the basis: the adaptive second pass keeps it orthogonal (eigenex_hip.h)
    device::check(eigenex_basis_configure_z(dev_.handle(), sh.real(), sh.imag(), threshold_, 1, EIGENEX_ORTHO_BATCHED_ADAPTIVE),
                  "eigenex_basis_configure_z");
    dev_.upload(EIGENEX_VEC_W, initial_);

    const int ldh = static_cast<int>(m + 1);
    std::vector<W> H(static_cast<std::size_t>(ldh) * m), Q, B;
    std::vector<small_eigen::cplx> theta, S;
    Index k = 0;     // dimension kept at the head of the basis
    Index meff = m;  // size of the projected matrix of this cycle (smaller after a breakdown)
    while (true) {
      device::check(eigenex_arnoldi_enqueue(dev_.handle(), static_cast<int>(m - k)), "eigenex_arnoldi_enqueue");
      matvecs_ += m - k;
      eigenex_state_t st;
      device::check(eigenex_arnoldi_state(dev_.handle(), &st, reinterpret_cast<double*>(H.data()), ldh), "eigenex_arnoldi_state");
      if (st.nvec == 0) {
        log_.push_back(headINFO() + "initial arnoldivector generation fail");
        info_ = NumericalIssue;
        break;
      }
      // a breakdown (residue <= threshold) leaves nvec <= m vectors spanning an invariant subspace
      const bool broke = st.stopped != 0;
      meff = st.nvec;
      if (!small_eigen::ritz_pairs_by_magnitude(H.data(), ldh, static_cast<int>(meff), theta, S))
        log_.push_back(headWARN() + "QR iteration of the projected matrix did not converge");
      const Index nw = std::min(nev, meff);
      const double scale = std::abs(theta.front() - theta.back());
      bool converged = true;
      residuals_.resize(nw);
      for (Index i = 0; i < nw; ++i) {
        const double r = st.residue * std::abs(S[static_cast<std::size_t>(meff - 1 + i * meff)]);
        residuals_[i] = static_cast<RealScalar>(r);
        if (r > tolerance_ * scale) converged = false;
      }
      if (broke) {
        log_.push_back(headINFO() + "arnoldi steps finished with threshold");
        converged = true;
      }
      if (converged) {
        log_.push_back(headINFO() + "krylov-schur converged with tolerance");
        break;
      }
      if (restarts_ == maxRestarts_ || meff < 2) {
        log_.push_back(headWARN() + "krylov-schur achieved maxRestarts");
        info_ = NoConvergence;
        break;
      }
      k = small_eigen::krylov_schur_basis<W>(H.data(), ldh, static_cast<int>(meff), static_cast<int>(keep), st.residue, theta, S, Q, B);
      if (k < 1) {  // two vectors and one conjugate pair: a real basis cannot keep half of it
        log_.push_back(headWARN() + "krylov-schur cannot restart: the basis holds one complex-conjugate pair only");
        info_ = NoConvergence;
        break;
      }
      device::check(eigenex_arnoldi_restart(dev_.handle(), static_cast<int>(k), reinterpret_cast<const double*>(Q.data()), static_cast<int>(meff),
                                            reinterpret_cast<const double*>(B.data()), static_cast<int>(k + 1)),
                    "eigenex_arnoldi_restart");
      ++restarts_;
    }

    if (info_ != NumericalIssue) {
      const Index nw = std::min(nev, meff);
      eigenvalues_.resize(nw);
      for (Index i = 0; i < nw; ++i) eigenvalues_[i] = static_cast<ComplexScalar>(theta[static_cast<std::size_t>(i)] - sh);
      if (vectorsOn_) {
        std::vector<double> sr(static_cast<std::size_t>(meff * nw)), si(sr.size());
        for (std::size_t i = 0; i < sr.size(); ++i) sr[i] = S[i].real(), si[i] = S[i].imag();
        eigenvectors_ = ComplexMatrixType(dev_.localRows(), nw);
        detail::WideOut<ComplexScalar> x(eigenvectors_.data(), eigenvectors_.size());
        device::check(eigenex_ritz_vectors_complex(dev_.handle(), static_cast<int>(meff), static_cast<int>(nw), sr.data(), si.data(),
                                                   static_cast<int>(meff), x.data(), eigenvectors_.rows()),
                      "eigenex_ritz_vectors_complex");
      }
    }
    log_.push_back(headINFO() + "KrylovSchurEigenSolver::compute(...) finish computing");
    return 0;
  }

 protected:
  MatMulFunction matmul_;
  std::shared_ptr<device::CsrOperator> op_;
  std::shared_ptr<device::Context> ctx_;
  Index height_ = 0;
  VectorType initial_;
  Scalar shift_ = Scalar(0.0);
  RealScalar threshold_ = 1e-12, tolerance_ = 1e-10;
  Index nev_ = 1, m_ = 128, keep_ = -1, maxRestarts_ = 1000;
  bool vectorsOn_ = true;

  ComplexVectorType eigenvalues_;
  RealVectorType residuals_;
  ComplexMatrixType eigenvectors_;
  Index restarts_ = 0, matvecs_ = 0;
  std::vector<std::string> log_;
  ComputationInfo info_ = Success;

  detail::KrylovDevice dev_;
  Index devHeight_ = -1;
  const device::CsrOperator* devOp_ = nullptr;
  const device::Context* devCtx_ = nullptr;
  detail::HostOperatorThunk<Scalar> thunk_;
};

}  // namespace EigenEx
}  // namespace cmpt
