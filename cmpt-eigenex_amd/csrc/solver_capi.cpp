// Flat C view of the header-only C++ solver classes
// (cmpt-eigenex_amd/include/cmpt/eigen_ex/{lanczos,arnoldi}.hpp) so that hosts
// without a C++ front-end (ctypes in tests/ and bench.py, cgo, JNI ...) can drive
// the same code a C++ user of the reference API would compile.  Host-only code:
// all device work goes through libeigenex_hip.so.
//
// Four families of entry points, one per instantiation:
//   eigenex_lanczos_solver_*   LanczosEigenSolver<double>
//   eigenex_zlanczos_solver_*  LanczosEigenSolver<std::complex<double>>
//   eigenex_arnoldi_solver_*   ArnoldiEigenSolver<double>
//   eigenex_zarnoldi_solver_*  ArnoldiEigenSolver<std::complex<double>>
// plus eigenex_[z]trlanczos_solver_* (ThickRestartLanczosEigenSolver), eigenex_[z]kschur_solver_* (KrylovSchurEigenSolver) and
// eigenex_[z]flanczos_solver_* (FilteredLanczosEigenSolver); eigenex_[z]density_solver_* (SpectralDensitySolver);
// eigenex_[z]thermal_solver_* (ThermalLanczosSolver) and eigenex_thermal_ensemble_* (ThermalEnsemble);
// eigenex_spin_dynamics_solver_* (SpinDynamicsSolver); eigenex_spin_momentum_dynamics_solver_* (SpinMomentumDynamicsSolver);
// eigenex_spin_entanglement_solver_* (SpinEntanglementSolver);
// eigenex_spin_evolution_solver_* (SpinTimeEvolutionSolver); eigenex_spin_time_correlation_solver_* (SpinTimeCorrelationSolver).
// Complex data cross this boundary as interleaved (re, im) doubles.
#include <complex>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "cmpt/eigen_ex/arnoldi.hpp"
#include "cmpt/eigen_ex/block_operator.hpp"
#include "cmpt/eigen_ex/filtered_lanczos.hpp"
#include "cmpt/eigen_ex/krylov_schur.hpp"
#include "cmpt/eigen_ex/lanczos.hpp"
#include "cmpt/eigen_ex/lanczos_function.hpp"
#include "cmpt/eigen_ex/spectral_density.hpp"
#include "cmpt/eigen_ex/spin_correlations.hpp"
#include "cmpt/eigen_ex/spin_dynamics.hpp"
#include "cmpt/eigen_ex/spin_momentum_dynamics.hpp"
#include "cmpt/eigen_ex/spin_entanglement.hpp"
#include "cmpt/eigen_ex/spin_evolution.hpp"
#include "cmpt/eigen_ex/spin_time_correlation.hpp"
#include "cmpt/eigen_ex/thermal_lanczos.hpp"
#include "cmpt/eigen_ex/thick_restart_lanczos.hpp"
#include "cmpt/eigen_ex/triplets_operator.hpp"

using namespace cmpt::EigenEx;

namespace {
thread_local std::string g_serr;

template <class Solver>
struct Box {
  std::shared_ptr<device::Context> ctx;
  std::shared_ptr<device::CsrOperator> op;
  Solver es;
};

template <class F>
int guard(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_serr = e.what();
    return -1;
  }
}

template <class S>
constexpr int es_of() {
  return detail::IsComplex<S>::value ? 2 : 1;
}

template <class S>
DenseVector<S> make_vector(const double* p, int64_t n) {
  return DenseVector<S>(reinterpret_cast<const S*>(p), (Index)n);
}

template <class Solver>
void set_common(Solver& es, const std::string& k, double v) {
  if (k == "minIterations") es.setMinIterations((Index)v);
  else if (k == "maxIterations") es.setMaxIterations((Index)v);
  else if (k == "tolerance") es.setTolerance(v);
  else if (k == "maxEigenvalues") es.setMaxEigenvalues((Index)v);
  else if (k == "computeEigenvectorsOn") es.setComputeEigenvectorsOn(v != 0.0);
  else if (k == "reserveSize") es.setReserveSize((Index)v);
  else if (k == "threshold") es.setThreshold(v);
  else if (k == "speculativeLookahead") es.setSpeculativeLookahead(v != 0.0);
  else if (k == "orthogonalization") {  // 0 batched, 1 sequential (reference order), 2 batched twice, 3 batched adaptive
    if (v < 0.0 || v > 3.0) throw LanczosException("orthogonalization must be 0..3");
    es.setOrthogonalization(static_cast<Orthogonalization>(static_cast<int>(v)));
  }
  else throw LanczosException("unknown setting: " + k);
}

inline void assign_shift(double& dst, double re, double) { dst = re; }
inline void assign_shift(std::complex<double>& dst, double re, double im) { dst = std::complex<double>(re, im); }

template <class Solver>
int sv_set_device_operator(void* p, eigenex_context_t ctx, eigenex_csr_t csr) {
  return guard([&] {
    auto* b = static_cast<Box<Solver>*>(p);
    b->ctx = device::Context::borrow(ctx);
    b->op = device::CsrOperator::borrow(b->ctx, csr);
    b->es.setDeviceOperator(b->op);
  });
}

template <class Solver>
int sv_set_host_operator(void* p, eigenex_context_t ctx, eigenex_matvec_fn fn, void* user, int64_t height) {
  using S = typename Solver::Scalar;
  return guard([&] {
    auto* b = static_cast<Box<Solver>*>(p);
    if (ctx) {
      b->ctx = device::Context::borrow(ctx);
      b->es.setDeviceContext(b->ctx);
    }
    b->es.setMatrixMultiplication(
        [fn, user](const S* in, S* out) { fn(reinterpret_cast<const double*>(in), reinterpret_cast<double*>(out), user); }, (Index)height);
  });
}

template <class Solver>
int sv_set_vectors(void* p, const double* vecs, int64_t n, int count) {
  using S = typename Solver::Scalar;
  return guard([&] {
    std::vector<DenseVector<S>> q;
    for (int i = 0; i < count; ++i) q.push_back(make_vector<S>(vecs + (size_t)i * n * es_of<S>(), n));
    static_cast<Box<Solver>*>(p)->es.setOrthogonalizingVectors(std::move(q));
  });
}

template <class Solver>
const char* sv_log_line(void* p, int64_t i) {
  auto& lg = static_cast<Box<Solver>*>(p)->es.log();
  return (i >= 0 && i < (int64_t)lg.size()) ? lg[(size_t)i].c_str() : "";
}

// ---- Lanczos ---------------------------------------------------------------------------
template <class S>
int lz_set(void* p, const char* key, double v, double v_im) {
  using Solver = LanczosEigenSolver<S>;
  (void)v_im;
  return guard([&] {
    auto& es = static_cast<Box<Solver>*>(p)->es;
    const std::string k(key);
    if (k == "reorthogonalizeInterval") es.setReorthogonalizeInterval((Index)v);
    else if (k == "eigenvalueShift") es.setEigenvalueShift(v);
    else set_common(es, k, v);
  });
}

// sizes: [iterations, nvec, nalpha, nbeta, neigenvalues, eigvec_rows, eigvec_cols, nlog, info, hasWARN, hasERROR]
template <class S>
int lz_sizes(void* p, int64_t* out) {
  return guard([&] {
    auto& es = static_cast<Box<LanczosEigenSolver<S>>*>(p)->es;
    out[0] = es.iterations();
    out[1] = es.lanczosBase().lanczosvectorsSize();
    out[2] = (int64_t)es.alpha().size();
    out[3] = (int64_t)es.beta().size();
    out[4] = es.eigenvalues().size();
    out[5] = es.eigenvectors().rows();
    out[6] = es.eigenvectors().cols();
    out[7] = (int64_t)es.log().size();
    out[8] = (int64_t)es.info();
    out[9] = es.hasWARN();
    out[10] = es.hasERROR();
  });
}

template <class S>
int lz_get(void* p, double* alpha, double* beta, double* eigenvalues, double* eigenvectors) {
  return guard([&] {
    auto& es = static_cast<Box<LanczosEigenSolver<S>>*>(p)->es;
    if (alpha) std::copy(es.alpha().begin(), es.alpha().end(), alpha);
    if (beta) std::copy(es.beta().begin(), es.beta().end(), beta);
    if (eigenvalues) std::copy(es.eigenvalues().begin(), es.eigenvalues().end(), eigenvalues);
    if (eigenvectors && es.eigenvectors().size())
      std::memcpy(eigenvectors, es.eigenvectors().data(), sizeof(S) * (size_t)es.eigenvectors().size());
  });
}

template <class S>
int lz_vector(void* p, int64_t k, double* out) {
  return guard([&] {
    const auto& v = static_cast<Box<LanczosEigenSolver<S>>*>(p)->es.lanczosvectors();
    if (k < 0 || k >= (int64_t)v.size()) throw LanczosException("vector index out of range");
    std::memcpy(out, v[(size_t)k].data(), sizeof(S) * (size_t)v[(size_t)k].size());
  });
}

template <class S>
int64_t lz_convergence_log(void* p, int64_t index, double* out, int64_t cap) {
  auto& cl = static_cast<Box<LanczosEigenSolver<S>>*>(p)->es.convergenceLog();
  auto it = cl.find((Index)index);
  if (it == cl.end()) return 0;
  for (int64_t i = 0; i < (int64_t)it->second.size() && i < cap; ++i) out[i] = it->second[(size_t)i];
  return (int64_t)it->second.size();
}

// ---- Arnoldi ------------------------------------------------------------------------------
template <class S>
int ar_set(void* p, const char* key, double v, double v_im) {
  using Solver = ArnoldiEigenSolver<S>;
  return guard([&] {
    auto& es = static_cast<Box<Solver>*>(p)->es;
    const std::string k(key);
    if (k == "eigenvalueShift") {
      S sh;
      assign_shift(sh, v, v_im);
      es.setEigenvalueShift(sh);
    } else {
      set_common(es, k, v);
    }
  });
}

// convergence log of index `index`: (re, im) pairs; returns the number of entries
template <class S>
int64_t ar_convergence_log(void* p, int64_t index, double* out, int64_t cap) {
  auto& cl = static_cast<Box<ArnoldiEigenSolver<S>>*>(p)->es.convergenceLog();
  auto it = cl.find((Index)index);
  if (it == cl.end()) return 0;
  for (int64_t i = 0; i < (int64_t)it->second.size() && i < cap; ++i) out[2 * i] = it->second[(size_t)i].real(), out[2 * i + 1] = it->second[(size_t)i].imag();
  return (int64_t)it->second.size();
}

// sizes: [iterations, nvec, hess_rows, neigenvalues, eigvec_rows, eigvec_cols, nlog, info, hasWARN, hasERROR]
template <class S>
int ar_sizes(void* p, int64_t* out) {
  return guard([&] {
    auto& es = static_cast<Box<ArnoldiEigenSolver<S>>*>(p)->es;
    out[0] = es.iterations();
    out[1] = es.arnoldiBase().arnoldivectorsSize();
    out[2] = es.hessenbergMatrix().rows();
    out[3] = es.eigenvalues().size();
    out[4] = es.eigenvectors().rows();
    out[5] = es.eigenvectors().cols();
    out[6] = (int64_t)es.log().size();
    out[7] = (int64_t)es.info();
    out[8] = es.hasWARN();
    out[9] = es.hasERROR();
  });
}

// hess: column-major Scalar; eigenvalues / eigenvectors complex (interleaved)
template <class S>
int ar_get(void* p, double* hess, double* eigenvalues, double* eigenvectors, double* residue) {
  return guard([&] {
    auto& es = static_cast<Box<ArnoldiEigenSolver<S>>*>(p)->es;
    if (hess && es.hessenbergMatrix().size())
      std::memcpy(hess, es.hessenbergMatrix().data(), sizeof(S) * (size_t)es.hessenbergMatrix().size());
    if (eigenvalues && es.eigenvalues().size())
      std::memcpy(eigenvalues, es.eigenvalues().data(), sizeof(double) * 2 * (size_t)es.eigenvalues().size());
    if (eigenvectors && es.eigenvectors().size())
      std::memcpy(eigenvectors, es.eigenvectors().data(), sizeof(double) * 2 * (size_t)es.eigenvectors().size());
    if (residue) *residue = es.arnoldiBase().residue();
  });
}

// ---- thick-restart Lanczos -----------------------------------------------------------------
inline bool tr_set_extra(ThickRestartLanczosEigenSolver<double>&, const std::string&, double, double) { return false; }
inline bool tr_set_extra(ThickRestartLanczosEigenSolver<std::complex<double>>&, const std::string&, double, double) { return false; }
template <class S>
bool tr_set_extra(FilteredLanczosEigenSolver<S>& es, const std::string& k, double v, double v2) {
  if (k == "target") es.setTarget(v);
  else if (k == "filterDegree") es.setFilterDegree((Index)v);
  else if (k == "spectralRange") es.setSpectralRange(v, v2);  // (lo, hi) travel as the (re, im) pair of the value
  else return false;
  return true;
}
template <class Solver>
int tr_set(void* p, const char* key, double v, double v2) {
  return guard([&] {
    auto& es = static_cast<Box<Solver>*>(p)->es;
    const std::string k(key);
    if (tr_set_extra(es, k, v, v2)) return;
    if (k == "numberOfEigenvalues") es.setNumberOfEigenvalues((Index)v);
    else if (k == "maxBasisSize") es.setMaxBasisSize((Index)v);
    else if (k == "keepSize") es.setKeepSize((Index)v);
    else if (k == "tolerance") es.setTolerance(v);
    else if (k == "maxRestarts") es.setMaxRestarts((Index)v);
    else if (k == "computeEigenvectorsOn") es.setComputeEigenvectorsOn(v != 0.0);
    else if (k == "eigenvalueShift") es.setEigenvalueShift(v);
    else if (k == "threshold") es.setThreshold(v);
    else throw LanczosException("unknown setting: " + k);
  });
}
// sizes: [neigenvalues, eigvec_rows, eigvec_cols, restarts, operatorApplications, nlog, info]
template <class Solver>
int tr_sizes(void* p, int64_t* out) {
  return guard([&] {
    auto& es = static_cast<Box<Solver>*>(p)->es;
    out[0] = es.eigenvalues().size();
    out[1] = es.eigenvectors().rows();
    out[2] = es.eigenvectors().cols();
    out[3] = es.restarts();
    out[4] = es.operatorApplications();
    out[5] = (int64_t)es.log().size();
    out[6] = (int64_t)es.info();
  });
}
template <class Solver>
int tr_get(void* p, double* eigenvalues, double* residuals, double* eigenvectors) {
  using S = typename Solver::Scalar;
  return guard([&] {
    auto& es = static_cast<Box<Solver>*>(p)->es;
    if (eigenvalues) std::copy(es.eigenvalues().begin(), es.eigenvalues().end(), eigenvalues);
    if (residuals) std::copy(es.residuals().begin(), es.residuals().end(), residuals);
    if (eigenvectors && es.eigenvectors().size())
      std::memcpy(eigenvectors, es.eigenvectors().data(), sizeof(S) * (size_t)es.eigenvectors().size());
  });
}

// ---- Krylov-Schur (krylov_schur.hpp) ---------------------------------------------------------------
template <class S>
int ks_set(void* p, const char* key, double v, double v_im) {
  return guard([&] {
    auto& es = static_cast<Box<KrylovSchurEigenSolver<S>>*>(p)->es;
    const std::string k(key);
    if (k == "numberOfEigenvalues") es.setNumberOfEigenvalues((Index)v);
    else if (k == "maxBasisSize") es.setMaxBasisSize((Index)v);
    else if (k == "keepSize") es.setKeepSize((Index)v);
    else if (k == "tolerance") es.setTolerance(v);
    else if (k == "maxRestarts") es.setMaxRestarts((Index)v);
    else if (k == "computeEigenvectorsOn") es.setComputeEigenvectorsOn(v != 0.0);
    else if (k == "eigenvalueShift") {
      S sh;
      assign_shift(sh, v, v_im);
      es.setEigenvalueShift(sh);
    }
    else if (k == "threshold") es.setThreshold(v);
    else throw LanczosException("unknown setting: " + k);
  });
}
// sizes: [neigenvalues, eigvec_rows, eigvec_cols, restarts, operatorApplications, nlog, info]
template <class S>
int ks_sizes(void* p, int64_t* out) {
  return guard([&] {
    auto& es = static_cast<Box<KrylovSchurEigenSolver<S>>*>(p)->es;
    out[0] = es.eigenvalues().size();
    out[1] = es.eigenvectors().rows();
    out[2] = es.eigenvectors().cols();
    out[3] = es.restarts();
    out[4] = es.operatorApplications();
    out[5] = (int64_t)es.log().size();
    out[6] = (int64_t)es.info();
  });
}
// eigenvalues and eigenvectors: (re, im) pairs for either instantiation
template <class S>
int ks_get(void* p, double* eigenvalues, double* residuals, double* eigenvectors) {
  return guard([&] {
    auto& es = static_cast<Box<KrylovSchurEigenSolver<S>>*>(p)->es;
    if (eigenvalues && es.eigenvalues().size())
      std::memcpy(eigenvalues, es.eigenvalues().data(), sizeof(std::complex<double>) * (size_t)es.eigenvalues().size());
    if (residuals) std::copy(es.residuals().begin(), es.residuals().end(), residuals);
    if (eigenvectors && es.eigenvectors().size())
      std::memcpy(eigenvectors, es.eigenvectors().data(), sizeof(std::complex<double>) * (size_t)es.eigenvectors().size());
  });
}
// the host part of one restart on its own (no GPU): see eigenex_solver_krylov_schur_basis
template <class T>
int ks_basis(const double* H, int ldh, int m, int keep, double residue, int* keep_out, double* Q, double* B, double* theta) {
  return guard([&] {
    if (m < 2 || ldh < m || keep < 1) throw LanczosException("krylov_schur_basis: m >= 2, ldh >= m and keep >= 1 are required");
    const T* h = reinterpret_cast<const T*>(H);
    std::vector<small_eigen::cplx> th, S;
    if (!small_eigen::ritz_pairs_by_magnitude(h, ldh, m, th, S)) throw LanczosException("QR iteration did not converge");
    std::vector<T> q, b;
    const int k = small_eigen::krylov_schur_basis<T>(h, ldh, m, keep, residue, th, S, q, b);
    *keep_out = k;
    std::memcpy(Q, q.data(), sizeof(T) * q.size());
    std::memcpy(B, b.data(), sizeof(T) * b.size());
    if (theta) std::memcpy(theta, th.data(), sizeof(small_eigen::cplx) * th.size());
  });
}

// ---- f(H)v / exp(xH)v (lanczos_function.hpp) -----------------------------------------------------
// kind 0: f(t) = exp(a t); 1: f(t) = 1/(t - a); 2: f(t) = t*t + a
template <class S>
std::function<S(S)> make_function(int kind, double a_re, double a_im) {
  S a;
  assign_shift(a, a_re, a_im);
  if (kind == 0) return [a](S t) { return std::exp(a * t); };
  if (kind == 1) return [a](S t) { return S(1.0) / (t - a); };
  if (kind == 2) return [a](S t) { return t * t + a; };
  throw LanczosException("unknown function kind");
}
template <class S>
int lz_exp_with_lanczos(void* p, double x_re, double x_im, double* out) {
  return guard([&] {
    auto& es = static_cast<Box<LanczosEigenSolver<S>>*>(p)->es;
    S x;
    assign_shift(x, x_re, x_im);
    DenseVector<S> o;
    LanczosExponentialSolver<S>::solveWithLanczos(x, es, o);
    std::memcpy(out, o.data(), sizeof(S) * (size_t)o.size());
  });
}
template <class S>
int lz_function_of(void* p, int kind, double a_re, double a_im, double* out) {
  return guard([&] {
    auto& es = static_cast<Box<LanczosEigenSolver<S>>*>(p)->es;
    const DenseVector<S> o = LanczosFunctionSolver<S>::solve(make_function<S>(kind, a_re, a_im), es);
    std::memcpy(out, o.data(), sizeof(S) * (size_t)o.size());
  });
}
template <class S>
int fn_exp_eigens(double x_re, double x_im, int64_t n, int64_t nev, const double* eivals, const double* eivecs, int64_t max_expand,
                  const double* in, double* out) {
  return guard([&] {
    S x;
    assign_shift(x, x_re, x_im);
    DenseVector<double> ev(eivals, (Index)nev);
    DenseMatrix<S> X((Index)n, (Index)nev);
    std::memcpy(reinterpret_cast<double*>(X.data()), eivecs, sizeof(S) * (size_t)(n * nev));
    DenseVector<S> o;
    LanczosExponentialSolver<S>::solveWithEigens(x, ev, X, (Index)max_expand, make_vector<S>(in, n), o);
    std::memcpy(out, o.data(), sizeof(S) * (size_t)o.size());
  });
}
template <class S>
int fn_exp_taylor(eigenex_context_t ctx, eigenex_csr_t csr, eigenex_matvec_fn fn, void* user, int64_t height, double x_re, double x_im,
                  double radius, const double* in, int64_t n_in, double* out, double error, int64_t max_expansion, int auto_division) {
  return guard([&] {
    S x;
    assign_shift(x, x_re, x_im);
    auto c = device::Context::borrow(ctx);
    DenseVector<S> o;
    const DenseVector<S> v = make_vector<S>(in, n_in);
    if (csr) {
      auto op = device::CsrOperator::borrow(c, csr);
      if (auto_division)
        LanczosExponentialSolver<S>::solveWithTaylorAutoDivision(x, op, radius, v, o, error, (Index)max_expansion);
      else
        LanczosExponentialSolver<S>::solveWithTaylorNoDivision(x, op, radius, v, o, error, (Index)max_expansion);
    } else {
      typename LanczosExponentialSolver<S>::MatMulFunction mm = [fn, user](const S* a, S* b) {
        fn(reinterpret_cast<const double*>(a), reinterpret_cast<double*>(b), user);
      };
      if (auto_division)
        LanczosExponentialSolver<S>::solveWithTaylorAutoDivision(x, std::make_pair(mm, (Index)height), radius, v, o, error, (Index)max_expansion);
      else
        LanczosExponentialSolver<S>::solveWithTaylorNoDivision(x, mm, (Index)height, radius, v, o, error, (Index)max_expansion, c);
    }
    std::memcpy(out, o.data(), sizeof(S) * (size_t)o.size());
  });
}

// ---- spectral density (spectral_density.hpp) -----------------------------------------------------
template <class Solver>
int sd_set(void* p, const char* key, double v, double v2) {
  return guard([&] {
    auto& es = static_cast<Box<Solver>*>(p)->es;
    const std::string k(key);
    if (k == "spectralRange") es.setSpectralRange(v, v2);
    else if (k == "moments") es.setMoments((Index)v);
    else if (k == "randomVectors") es.setRandomVectors((Index)v);
    else throw LanczosException("unknown setting: " + k);
  });
}
template <class Solver>
int sd_sizes(void* p, int64_t* out) {
  return guard([&] {
    auto& es = static_cast<Box<Solver>*>(p)->es;
    out[0] = (int64_t)es.moments().size();
    out[1] = (int64_t)es.randomVectors();
    out[2] = (int64_t)es.operatorApplications();
    out[3] = (int64_t)es.log().size();
    out[4] = (int64_t)es.info();
  });
}
// mean[M], standard error[M], each[R*M] (any may be NULL); range[2] = (center, halfwidth)
template <class Solver>
int sd_get(void* p, double* mean, double* se, double* each, double* range) {
  return guard([&] {
    auto& es = static_cast<Box<Solver>*>(p)->es;
    if (mean) std::copy(es.moments().begin(), es.moments().end(), mean);
    if (se) std::copy(es.momentsStandardError().begin(), es.momentsStandardError().end(), se);
    if (each)
      for (const auto& m : es.momentsOfEachVector()) each = std::copy(m.begin(), m.end(), each);
    if (range) range[0] = es.center(), range[1] = es.halfwidth();
  });
}

}  // namespace

extern "C" {

const char* eigenex_solver_last_error(void) { return g_serr.c_str(); }

// ---- host helpers exposed for CPU tests ------------------------------------------------
// reference default start vector: std::mt19937 (default seed) + std::normal_distribution, normalised
int eigenex_solver_default_start_vector(int64_t n, double* out) {
  return guard([&] {
    std::mt19937 g;
    auto v = LanczosBase<double>::makeRandomVector(g, (Index)n);
    std::copy(v.begin(), v.end(), out);
  });
}
int eigenex_solver_random_vector(uint32_t seed, int64_t n, double* out) {
  return guard([&] {
    std::mt19937 g(seed);
    auto v = LanczosBase<double>::makeRandomVector(g, (Index)n);
    std::copy(v.begin(), v.end(), out);
  });
}
// complex: real part then imaginary part per entry (util.hpp:76-97); out interleaved
int eigenex_solver_random_vector_z(uint32_t seed, int64_t n, double* out) {
  return guard([&] {
    std::mt19937 g(seed);
    auto v = LanczosBase<std::complex<double>>::makeRandomVector(g, (Index)n);
    std::memcpy(out, v.data(), sizeof(double) * 2 * (size_t)n);
  });
}
// ---- SURVEY 8d's synthetic inputs, from the host STL's engines (the engines are specified by the standard; of the
// distributions only std::normal_distribution is used, as the reference's own samples use it) ------------------------
// Dense512 (BASELINE config 1): n draws of std::normal_distribution<double>(0, 1) from std::mt19937(seed), in order
int eigenex_solver_stl_normal(uint32_t seed, int64_t n, double* out) {
  return guard([&] {
    std::mt19937 g(seed);
    std::normal_distribution<double> d(0.0, 1.0);
    for (int64_t i = 0; i < n; ++i) out[i] = d(g);
  });
}
// RandomCSR (BASELINE config 3): std::mt19937_64(seed) drawn row by row -- first the row's `per` distinct columns
// (engine() % n, a repeated column is drawn again), stored ascending; then its `per` values in that order, each
// 2 * ((engine() >> 11) * 2^-53) - 1, i.e. U(-1, 1) from the top 53 bits.  Raw engine output only: the same numbers on any STL.
int eigenex_solver_random_csr(int64_t n, int per, uint64_t seed, int32_t* rowptr, int32_t* col, double* val) {
  return guard([&] {
    if (n <= 0 || per <= 0 || per > n || n > 2147483647 || n * (int64_t)per > 2147483647) throw LanczosException("random_csr: bad size");
    std::mt19937_64 g(seed);
    std::vector<int32_t> c((size_t)per);
    for (int64_t r = 0; r < n; ++r) {
      rowptr[r] = (int32_t)(r * per);
      int have = 0;
      while (have < per) {
        const int32_t x = (int32_t)(g() % (uint64_t)n);
        bool seen = false;
        for (int i = 0; i < have; ++i) seen |= c[(size_t)i] == x;
        if (!seen) c[(size_t)have++] = x;
      }
      std::sort(c.begin(), c.end());
      std::copy(c.begin(), c.end(), col + r * per);
      for (int i = 0; i < per; ++i) val[r * per + i] = 2.0 * ((double)(g() >> 11) * 0x1p-53) - 1.0;
    }
    rowptr[n] = (int32_t)(n * per);
  });
}
// small dense solvers (small_eigen.hpp); vectors may be NULL
int eigenex_solver_tridiagonal_eigen(int n, const double* diag, const double* sub, double* values, double* vectors) {
  return guard([&] {
    std::vector<double> vals, vecs;
    if (!small_eigen::tridiagonal(diag, sub, n, vals, vectors ? &vecs : nullptr)) throw LanczosException("QL iteration did not converge");
    std::copy(vals.begin(), vals.end(), values);
    if (vectors) std::copy(vecs.begin(), vecs.end(), vectors);
  });
}
// COO -> CSR (TripletsMatrix::shrink semantics); out arrays sized count / n+1; returns nnz in *nnz
int eigenex_solver_triplets_to_csr(int64_t n, int64_t count, const int64_t* rows, const int64_t* cols, const double* vals,
                                   int is_complex, int32_t* rowptr, int32_t* col, double* val, int64_t* nnz) {
  return guard([&] {
    std::vector<Index> r(rows, rows + count), c(cols, cols + count);
    if (is_complex) {
      auto m = triplets_to_csr<std::complex<double>>((Index)n, (Index)count, r.data(), c.data(), reinterpret_cast<const std::complex<double>*>(vals));
      std::copy(m.rowptr.begin(), m.rowptr.end(), rowptr);
      std::copy(m.col.begin(), m.col.end(), col);
      std::memcpy(val, m.val.data(), sizeof(double) * 2 * m.val.size());
      *nnz = (int64_t)m.val.size();
    } else {
      auto m = triplets_to_csr<double>((Index)n, (Index)count, r.data(), c.data(), vals);
      std::copy(m.rowptr.begin(), m.rowptr.end(), rowptr);
      std::copy(m.col.begin(), m.col.end(), col);
      std::copy(m.val.begin(), m.val.end(), val);
      *nnz = (int64_t)m.val.size();
    }
  });
}
// Block-sparse matrix (BlockTensor<double,2> layout: partitions + dense column-major blocks) -> CSR.
// blocks: nblocks entries (qr, qc) with values concatenated column-major in `vals`; outputs sized by the caller
// (nnz = sum of block sizes).
int eigenex_solver_blocks_to_csr(int nbr, const int64_t* row_sizes, int nbc, const int64_t* col_sizes, int nblocks,
                                 const int64_t* qr, const int64_t* qc, const double* vals, int32_t* rowptr, int32_t* col,
                                 double* val, int64_t* nnz) {
  return guard([&] {
    BlockSparseMatrix<double> H(std::vector<Index>(row_sizes, row_sizes + nbr), std::vector<Index>(col_sizes, col_sizes + nbc));
    const double* p = vals;
    for (int b = 0; b < nblocks; ++b) {
      if (qr[b] < 0 || qr[b] >= nbr || qc[b] < 0 || qc[b] >= nbc) throw LanczosException("block index out of range");
      DenseMatrix<double> B((Index)row_sizes[qr[b]], (Index)col_sizes[qc[b]]);
      std::copy(p, p + B.size(), B.data());
      p += B.size();
      H.addBlock((Index)qr[b], (Index)qc[b], B);
    }
    const auto m = H.toCsr();
    std::copy(m.rowptr.begin(), m.rowptr.end(), rowptr);
    std::copy(m.col.begin(), m.col.end(), col);
    std::copy(m.val.begin(), m.val.end(), val);
    *nnz = (int64_t)m.val.size();
  });
}
int eigenex_solver_gershgorin_range(int64_t n, int64_t count, const int64_t* rows, const int64_t* cols, const double* vals,
                                    int is_complex, double* lo_hi) {
  return guard([&] {
    std::vector<Index> r(rows, rows + count), c(cols, cols + count);
    const auto b = is_complex ? estimateEigenvalueRange<std::complex<double>>((Index)n, (Index)count, r.data(), c.data(),
                                                                             reinterpret_cast<const std::complex<double>*>(vals))
                              : estimateEigenvalueRange<double>((Index)n, (Index)count, r.data(), c.data(), vals);
    lo_hi[0] = b[0];
    lo_hi[1] = b[1];
  });
}
// dense symmetric (column-major n x n); vectors column-major
int eigenex_solver_symmetric_eigen(int n, const double* A, double* values, double* vectors) {
  return guard([&] {
    std::vector<double> a(A, A + (size_t)n * n), vals, vecs;
    if (!small_eigen::symmetric(a, n, vals, vecs)) throw LanczosException("QL iteration did not converge");
    std::copy(vals.begin(), vals.end(), values);
    std::copy(vecs.begin(), vecs.end(), vectors);
  });
}
// H: column-major n x n complex (interleaved re,im); values/vectors interleaved
int eigenex_solver_hessenberg_eigen(int n, const double* H_interleaved, double* values, double* vectors) {
  return guard([&] {
    std::vector<small_eigen::cplx> H((size_t)n * n), vals, vecs;
    std::memcpy(static_cast<void*>(H.data()), H_interleaved, sizeof(double) * 2 * (size_t)n * n);
    if (!small_eigen::hessenberg(H, n, vals, vectors ? &vecs : nullptr)) throw LanczosException("QR iteration did not converge");
    std::memcpy(values, vals.data(), sizeof(double) * 2 * (size_t)n);
    if (vectors) std::memcpy(vectors, vecs.data(), sizeof(double) * 2 * (size_t)n * n);
  });
}

// eigenvalues only of a REAL upper-Hessenberg matrix (column-major), Francis double-shift QR; values: (re, im) pairs
int eigenex_solver_hessenberg_values_real(int n, const double* H, double* values) {
  return guard([&] {
    std::vector<double> A(H, H + (size_t)n * n);
    std::vector<small_eigen::cplx> vals;
    if (!small_eigen::hessenberg_real_values(A, n, vals)) throw LanczosException("QR iteration did not converge");
    std::memcpy(values, vals.data(), sizeof(double) * 2 * (size_t)n);
  });
}

#define EIGENEX_SOLVER_COMMON(PFX, SOLVER)                                                                              \
  void* PFX##create(void) {                                                                                             \
    try {                                                                                                               \
      return new Box<SOLVER>();                                                                                         \
    } catch (const std::exception& e) {                                                                                 \
      g_serr = e.what();                                                                                                \
      return nullptr;                                                                                                   \
    }                                                                                                                   \
  }                                                                                                                     \
  void PFX##destroy(void* p) { delete static_cast<Box<SOLVER>*>(p); }                                                   \
  int PFX##set_device_operator(void* p, eigenex_context_t ctx, eigenex_csr_t csr) {                                     \
    return sv_set_device_operator<SOLVER>(p, ctx, csr);                                                                 \
  }                                                                                                                     \
  int PFX##set_host_operator(void* p, eigenex_context_t ctx, eigenex_matvec_fn fn, void* user, int64_t height) {        \
    return sv_set_host_operator<SOLVER>(p, ctx, fn, user, height);                                                      \
  }                                                                                                                     \
  int PFX##set_indices_for_convergence(void* p, const int64_t* idx, int n) {                                            \
    return guard([&] { static_cast<Box<SOLVER>*>(p)->es.setIndicesForConvergence(std::vector<Index>(idx, idx + n)); }); \
  }                                                                                                                     \
  int PFX##set_initial_vector(void* p, const double* v, int64_t n) {                                                    \
    return guard([&] { static_cast<Box<SOLVER>*>(p)->es.setInitialVector(make_vector<SOLVER::Scalar>(v, n)); });        \
  }                                                                                                                     \
  int PFX##set_orthogonalizing_vectors(void* p, const double* vecs, int64_t n, int count) {                             \
    return sv_set_vectors<SOLVER>(p, vecs, n, count);                                                                   \
  }                                                                                                                     \
  int PFX##compute(void* p) { return guard([&] { static_cast<Box<SOLVER>*>(p)->es.compute(); }); }                      \
  int PFX##continue(void* p) { return guard([&] { static_cast<Box<SOLVER>*>(p)->es.continueToCompute(); }); }           \
  const char* PFX##log_line(void* p, int64_t i) { return sv_log_line<SOLVER>(p, i); }

#define EIGENEX_LANCZOS_FAMILY(PFX, S)                                                                                  \
  EIGENEX_SOLVER_COMMON(PFX, LanczosEigenSolver<S>)                                                                     \
  int PFX##set(void* p, const char* key, double v, double v_im) { return lz_set<S>(p, key, v, v_im); }                  \
  int PFX##sizes(void* p, int64_t* out) { return lz_sizes<S>(p, out); }                                                 \
  int PFX##get(void* p, double* a, double* b, double* ev, double* X) { return lz_get<S>(p, a, b, ev, X); }              \
  int PFX##lanczosvector(void* p, int64_t k, double* out) { return lz_vector<S>(p, k, out); }                           \
  int64_t PFX##convergence_log(void* p, int64_t i, double* out, int64_t cap) { return lz_convergence_log<S>(p, i, out, cap); } \
  int PFX##exp_with_lanczos(void* p, double x_re, double x_im, double* out) { return lz_exp_with_lanczos<S>(p, x_re, x_im, out); } \
  int PFX##function_of(void* p, int kind, double a_re, double a_im, double* out) { return lz_function_of<S>(p, kind, a_re, a_im, out); }

#define EIGENEX_ARNOLDI_FAMILY(PFX, S)                                                                                  \
  EIGENEX_SOLVER_COMMON(PFX, ArnoldiEigenSolver<S>)                                                                     \
  int PFX##set(void* p, const char* key, double v, double v_im) { return ar_set<S>(p, key, v, v_im); }                  \
  int PFX##sizes(void* p, int64_t* out) { return ar_sizes<S>(p, out); }                                                 \
  int PFX##get(void* p, double* H, double* ev, double* X, double* res) { return ar_get<S>(p, H, ev, X, res); }              \
  int64_t PFX##convergence_log(void* p, int64_t i, double* out, int64_t cap) { return ar_convergence_log<S>(p, i, out, cap); }

#define EIGENEX_TRLANCZOS_FAMILY(PFX, SOLVER)                                                                           \
  void* PFX##create(void) {                                                                                             \
    try {                                                                                                               \
      return new Box<SOLVER>();                                                                                         \
    } catch (const std::exception& e) {                                                                                 \
      g_serr = e.what();                                                                                                \
      return nullptr;                                                                                                   \
    }                                                                                                                   \
  }                                                                                                                     \
  void PFX##destroy(void* p) { delete static_cast<Box<SOLVER>*>(p); }                                                   \
  int PFX##set_device_operator(void* p, eigenex_context_t ctx, eigenex_csr_t csr) {                                     \
    return sv_set_device_operator<SOLVER>(p, ctx, csr);                                                                 \
  }                                                                                                                     \
  int PFX##set_host_operator(void* p, eigenex_context_t ctx, eigenex_matvec_fn fn, void* user, int64_t height) {        \
    return sv_set_host_operator<SOLVER>(p, ctx, fn, user, height);                                                      \
  }                                                                                                                     \
  int PFX##set_initial_vector(void* p, const double* v, int64_t n) {                                                    \
    return guard([&] { static_cast<Box<SOLVER>*>(p)->es.setInitialVector(make_vector<SOLVER::Scalar>(v, n)); });        \
  }                                                                                                                     \
  int PFX##set(void* p, const char* key, double v, double v2) { return tr_set<SOLVER>(p, key, v, v2); }                 \
  int PFX##compute(void* p) { return guard([&] { static_cast<Box<SOLVER>*>(p)->es.compute(); }); }                      \
  int PFX##sizes(void* p, int64_t* out) { return tr_sizes<SOLVER>(p, out); }                                            \
  int PFX##get(void* p, double* ev, double* res, double* X) { return tr_get<SOLVER>(p, ev, res, X); }                   \
  const char* PFX##log_line(void* p, int64_t i) { return sv_log_line<SOLVER>(p, i); }

#define EIGENEX_KSCHUR_FAMILY(PFX, S)                                                                                   \
  void* PFX##create(void) {                                                                                             \
    try {                                                                                                               \
      return new Box<KrylovSchurEigenSolver<S>>();                                                                      \
    } catch (const std::exception& e) {                                                                                 \
      g_serr = e.what();                                                                                                \
      return nullptr;                                                                                                   \
    }                                                                                                                   \
  }                                                                                                                     \
  void PFX##destroy(void* p) { delete static_cast<Box<KrylovSchurEigenSolver<S>>*>(p); }                                \
  int PFX##set_device_operator(void* p, eigenex_context_t ctx, eigenex_csr_t csr) {                                     \
    return sv_set_device_operator<KrylovSchurEigenSolver<S>>(p, ctx, csr);                                              \
  }                                                                                                                     \
  int PFX##set_host_operator(void* p, eigenex_context_t ctx, eigenex_matvec_fn fn, void* user, int64_t height) {        \
    return sv_set_host_operator<KrylovSchurEigenSolver<S>>(p, ctx, fn, user, height);                                   \
  }                                                                                                                     \
  int PFX##set_initial_vector(void* p, const double* v, int64_t n) {                                                    \
    return guard([&] { static_cast<Box<KrylovSchurEigenSolver<S>>*>(p)->es.setInitialVector(make_vector<S>(v, n)); });  \
  }                                                                                                                     \
  int PFX##set(void* p, const char* key, double v, double v_im) { return ks_set<S>(p, key, v, v_im); }                  \
  int PFX##compute(void* p) { return guard([&] { static_cast<Box<KrylovSchurEigenSolver<S>>*>(p)->es.compute(); }); }   \
  int PFX##sizes(void* p, int64_t* out) { return ks_sizes<S>(p, out); }                                                 \
  int PFX##get(void* p, double* ev, double* res, double* X) { return ks_get<S>(p, ev, res, X); }                        \
  const char* PFX##log_line(void* p, int64_t i) { return sv_log_line<KrylovSchurEigenSolver<S>>(p, i); }

// The dense host part of one Krylov-Schur restart (small_eigen::krylov_schur_basis), callable without a GPU.  H: the projected
// matrix, column-major m x m with leading dimension ldh (is_complex: (re, im) pairs), Hessenberg or with a full leading block.
// Out: *keep_out (keep, or keep + 1 when a real matrix's conjugate pair would have been split), Q (m x *keep_out, leading
// dimension m), B ((*keep_out + 1) x *keep_out, leading dimension *keep_out + 1; last row = residue * Q[m-1, :]) -- room for
// keep + 1 columns each -- and theta (optional): all m Ritz values as (re, im) pairs, |theta| descending.
int eigenex_solver_krylov_schur_basis(int is_complex, const double* H, int ldh, int m, int keep, double residue, int* keep_out,
                                      double* Q, double* B, double* theta) {
  return is_complex ? ks_basis<std::complex<double>>(H, ldh, m, keep, residue, keep_out, Q, B, theta)
                    : ks_basis<double>(H, ldh, m, keep, residue, keep_out, Q, B, theta);
}

// Coefficients of FilteredLanczosEigenSolver's filter (chebyshevDeltaCoefficients): mu[degree + 1] of the Jackson-damped delta
// peak at tau on [center - halfwidth, center + halfwidth], p(tau) = 1.  Host only.
int eigenex_solver_chebyshev_delta(double tau, double center, double halfwidth, int degree, double* mu) {
  return guard([&] {
    if (degree < 0 || !mu || !(halfwidth > 0.0)) throw LanczosException("chebyshev_delta: degree >= 0, halfwidth > 0 and mu are required");
    const std::vector<double> c = chebyshevDeltaCoefficients(tau, center, halfwidth, degree);
    std::copy(c.begin(), c.end(), mu);
  });
}

int eigenex_solver_exp_eigens(int is_complex, double x_re, double x_im, int64_t n, int64_t nev, const double* eivals,
                              const double* eivecs, int64_t max_expand, const double* in, double* out) {
  return is_complex ? fn_exp_eigens<std::complex<double>>(x_re, x_im, n, nev, eivals, eivecs, max_expand, in, out)
                    : fn_exp_eigens<double>(x_re, x_im, n, nev, eivals, eivecs, max_expand, in, out);
}
// operator: csr handle, or (csr == NULL) the host callback fn/user of `height` rows
int eigenex_solver_exp_taylor(int is_complex, eigenex_context_t ctx, eigenex_csr_t csr, eigenex_matvec_fn fn, void* user, int64_t height,
                              double x_re, double x_im, double radius, const double* in, int64_t n_in, double* out, double error,
                              int64_t max_expansion, int auto_division) {
  return is_complex ? fn_exp_taylor<std::complex<double>>(ctx, csr, fn, user, height, x_re, x_im, radius, in, n_in, out, error, max_expansion, auto_division)
                    : fn_exp_taylor<double>(ctx, csr, fn, user, height, x_re, x_im, radius, in, n_in, out, error, max_expansion, auto_division);
}

// SpectralDensitySolver: the entry points of the family above as far as they apply (no host operator, no eigenpairs); _set takes
// "spectralRange" (lo, hi), "moments", "randomVectors"; the results are moments and functions of an energy
#define EIGENEX_DENSITY_FAMILY(PFX, SOLVER)                                                                             \
  void* PFX##create(void) {                                                                                             \
    try {                                                                                                               \
      return new Box<SOLVER>();                                                                                         \
    } catch (const std::exception& e) {                                                                                 \
      g_serr = e.what();                                                                                                \
      return nullptr;                                                                                                   \
    }                                                                                                                   \
  }                                                                                                                     \
  void PFX##destroy(void* p) { delete static_cast<Box<SOLVER>*>(p); }                                                   \
  int PFX##set_device_operator(void* p, eigenex_context_t ctx, eigenex_csr_t csr) {                                     \
    return sv_set_device_operator<SOLVER>(p, ctx, csr);                                                                 \
  }                                                                                                                     \
  int PFX##set_initial_vector(void* p, const double* v, int64_t n) {                                                    \
    return guard([&] {                                                                                                  \
      if (v) static_cast<Box<SOLVER>*>(p)->es.setInitialVector(make_vector<SOLVER::Scalar>(v, n));                      \
      else static_cast<Box<SOLVER>*>(p)->es.setInitialVector();                                                         \
    });                                                                                                                 \
  }                                                                                                                     \
  int PFX##set(void* p, const char* key, double v, double v2) { return sd_set<SOLVER>(p, key, v, v2); }                 \
  int PFX##set_seed(void* p, uint64_t seed) { return guard([&] { static_cast<Box<SOLVER>*>(p)->es.setSeed(seed); }); }  \
  int PFX##compute(void* p) { return guard([&] { static_cast<Box<SOLVER>*>(p)->es.compute(); }); }                      \
  int PFX##continue(void* p) { return guard([&] { static_cast<Box<SOLVER>*>(p)->es.continueToCompute(); }); }           \
  int PFX##sizes(void* p, int64_t* out) { return sd_sizes<SOLVER>(p, out); }                                            \
  int PFX##get(void* p, double* mean, double* se, double* each, double* range) { return sd_get<SOLVER>(p, mean, se, each, range); } \
  int PFX##density(void* p, const double* E, int64_t n, double* out) {                                                  \
    return guard([&] {                                                                                                  \
      for (int64_t i = 0; i < n; ++i) out[i] = static_cast<Box<SOLVER>*>(p)->es.density(E[i]);                          \
    });                                                                                                                 \
  }                                                                                                                     \
  int PFX##eigenvalue_count(void* p, double a, double b, double* count, double* standard_error) {                       \
    return guard([&] {                                                                                                  \
      if (count) *count = static_cast<Box<SOLVER>*>(p)->es.eigenvalueCount(a, b);                                       \
      if (standard_error) *standard_error = static_cast<Box<SOLVER>*>(p)->es.eigenvalueCountStandardError(a, b);        \
    });                                                                                                                 \
  }                                                                                                                     \
  int PFX##energy_window(void* p, double tau, double count, double* halfwidth) {                                        \
    return guard([&] { *halfwidth = static_cast<Box<SOLVER>*>(p)->es.energyWindow(tau, count); });                      \
  }                                                                                                                     \
  const char* PFX##log_line(void* p, int64_t i) { return sv_log_line<SOLVER>(p, i); }

// The host arithmetic behind SpectralDensitySolver's results (kpmDensity, kpmCount, kpmWindow, jacksonFactor) for given
// normalised moments mu[M].  Host only.
int eigenex_solver_jackson_factors(int M, double* g) {
  return guard([&] {
    if (M < 1 || !g) throw LanczosException("jackson_factors: M >= 1 and g are required");
    for (int k = 0; k < M; ++k) g[k] = jacksonFactor(k, M);
  });
}
int eigenex_solver_kpm_density(const double* mu, int M, double center, double halfwidth, const double* E, int64_t n, double* out) {
  return guard([&] {
    if (M < 1 || !mu || !(halfwidth > 0.0)) throw LanczosException("kpm_density: mu[M], M >= 1 and halfwidth > 0 are required");
    for (int64_t i = 0; i < n; ++i) out[i] = kpmDensity(mu, M, center, halfwidth, E[i]);
  });
}
int eigenex_solver_kpm_count(const double* mu, int M, double center, double halfwidth, double a, double b, double N, double* out) {
  return guard([&] {
    if (M < 1 || !mu || !(halfwidth > 0.0)) throw LanczosException("kpm_count: mu[M], M >= 1 and halfwidth > 0 are required");
    *out = kpmCount(mu, M, center, halfwidth, a, b, N);
  });
}
int eigenex_solver_kpm_window(const double* mu, int M, double center, double halfwidth, double tau, double count, double N, double* out) {
  return guard([&] {
    if (M < 1 || !mu || !(halfwidth > 0.0)) throw LanczosException("kpm_window: mu[M], M >= 1 and halfwidth > 0 are required");
    *out = kpmWindow(mu, M, center, halfwidth, tau, count, N);
  });
}

// ThermalLanczosSolver (thermal_lanczos.hpp): _set takes "lanczosSteps" and "randomVectors"; _set_seed the seed and the first
// stream; _set_sample_vectors R vectors of n entries (NULL: random vectors again); _set_spin_observables the two mask lists
// (n_diag = -1: setAllSitesAndPairs) and writes the returned ComputationInfo to *info.  _sizes: dimension, samples, operator
// applications, log lines, info, diagonal terms, flip terms, sites of setAllSitesAndPairs (0: other masks).  _value: quantity
// 0 log Z, 1 E, 2 C, 3 S, 4 F, 5 observable t (diagonal list, then flip list); value and its jackknife error (either may be NULL).
// _correlation: kind 0 ZZ, 1 XY, 2 SS of sites i, j.  _sample: theta and weight of sample r (*n entries; pointers may be NULL).
#define EIGENEX_THERMAL_FAMILY(PFX, SOLVER)                                                                                              \
  void* PFX##create(void) {                                                                                                              \
    try {                                                                                                                                \
      return new Box<SOLVER>();                                                                                                          \
    } catch (const std::exception& e) {                                                                                                  \
      g_serr = e.what();                                                                                                                 \
      return nullptr;                                                                                                                    \
    }                                                                                                                                    \
  }                                                                                                                                      \
  void PFX##destroy(void* p) { delete static_cast<Box<SOLVER>*>(p); }                                                                    \
  int PFX##set_device_operator(void* p, eigenex_context_t ctx, eigenex_csr_t csr) { return sv_set_device_operator<SOLVER>(p, ctx, csr); } \
  int PFX##set(void* p, const char* key, double v, double) {                                                                             \
    return guard([&] {                                                                                                                   \
      auto& es = static_cast<Box<SOLVER>*>(p)->es;                                                                                       \
      const std::string k(key);                                                                                                          \
      if (k == "lanczosSteps") es.setLanczosSteps((Index)v);                                                                             \
      else if (k == "randomVectors") es.setRandomVectors((Index)v);                                                                      \
      else throw LanczosException("unknown setting: " + k);                                                                              \
    });                                                                                                                                  \
  }                                                                                                                                      \
  int PFX##set_seed(void* p, uint64_t seed, uint64_t first_stream) {                                                                     \
    return guard([&] { static_cast<Box<SOLVER>*>(p)->es.setSeed(seed).setFirstStream(first_stream); });                                  \
  }                                                                                                                                      \
  int PFX##set_sample_vectors(void* p, const double* v, int64_t n, int64_t count) {                                                      \
    return guard([&] { static_cast<Box<SOLVER>*>(p)->es.setSampleVectors(reinterpret_cast<const SOLVER::Scalar*>(v), (Index)n, (Index)count); }); \
  }                                                                                                                                      \
  int PFX##set_spin_observables(void* p, int n_diag, const uint32_t* diag, int n_flip, const uint32_t* flip, int* info) {                \
    return guard([&] {                                                                                                                   \
      auto& es = static_cast<Box<SOLVER>*>(p)->es;                                                                                       \
      const ComputationInfo r = n_diag < 0 ? es.setAllSitesAndPairs()                                                                    \
                                           : es.setSpinObservables(std::vector<uint32_t>(diag, diag + n_diag), std::vector<uint32_t>(flip, flip + n_flip)); \
      if (info) *info = (int)r;                                                                                                          \
    });                                                                                                                                  \
  }                                                                                                                                      \
  int PFX##compute(void* p) { return guard([&] { static_cast<Box<SOLVER>*>(p)->es.compute(); }); }                                       \
  int PFX##sizes(void* p, int64_t* out) {                                                                                                \
    return guard([&] {                                                                                                                   \
      auto& es = static_cast<Box<SOLVER>*>(p)->es;                                                                                       \
      out[0] = (int64_t)es.dimension(), out[1] = (int64_t)es.samples(), out[2] = (int64_t)es.operatorApplications();                     \
      out[3] = (int64_t)es.log().size(), out[4] = (int64_t)es.info(), out[5] = (int64_t)es.diagonalTerms();                              \
      out[6] = (int64_t)es.flipTerms(), out[7] = (int64_t)es.sitesWithAllPairs();                                                        \
    });                                                                                                                                  \
  }                                                                                                                                      \
  int PFX##value(void* p, int quantity, int64_t t, double beta, double* value, double* standard_error) {                                 \
    return guard([&] {                                                                                                                   \
      if (quantity < 0 || quantity > 5) throw LanczosException("thermal solver: quantity must be 0..5");                                 \
      auto& es = static_cast<Box<SOLVER>*>(p)->es;                                                                                       \
      if (value) *value = es.sums().value((ThermalQuantity)quantity, beta, (std::size_t)t);                                              \
      if (standard_error) *standard_error = es.standardError((ThermalQuantity)quantity, beta, (Index)t);                                 \
    });                                                                                                                                  \
  }                                                                                                                                      \
  int PFX##correlation(void* p, int kind, int i, int j, double beta, double* value) {                                                    \
    return guard([&] {                                                                                                                   \
      auto& es = static_cast<Box<SOLVER>*>(p)->es;                                                                                       \
      *value = kind == 0 ? es.correlationZZ(i, j, beta) : kind == 1 ? es.correlationXY(i, j, beta) : es.correlationSS(i, j, beta);       \
    });                                                                                                                                  \
  }                                                                                                                                      \
  int PFX##sample(void* p, int64_t r, int64_t* n, double* theta, double* weight) {                                                       \
    return guard([&] {                                                                                                                   \
      const ThermalSample& s = static_cast<Box<SOLVER>*>(p)->es.sums().sample((std::size_t)r);                                           \
      if (n) *n = (int64_t)s.theta.size();                                                                                               \
      if (theta) std::copy(s.theta.begin(), s.theta.end(), theta);                                                                       \
      if (weight) std::copy(s.weight.begin(), s.weight.end(), weight);                                                                   \
    });                                                                                                                                  \
  }                                                                                                                                      \
  int PFX##add_to_ensemble(void* p, void* ensemble, double multiplicity, double magnetisation) {                                         \
    return guard([&] { static_cast<ThermalEnsemble*>(ensemble)->add(static_cast<Box<SOLVER>*>(p)->es, multiplicity, magnetisation); });  \
  }                                                                                                                                      \
  const char* PFX##log_line(void* p, int64_t i) { return sv_log_line<SOLVER>(p, i); }

EIGENEX_THERMAL_FAMILY(eigenex_thermal_solver_, ThermalLanczosSolver<double>)
EIGENEX_THERMAL_FAMILY(eigenex_zthermal_solver_, ThermalLanczosSolver<std::complex<double>>)

// ThermalEnsemble (thermal_lanczos.hpp); sectors are added by eigenex_[z]thermal_solver_add_to_ensemble.  _value: quantity 0 log Z,
// 1 E, 2 C, 3 S, 4 susceptibility per site, 5 observable t.
void* eigenex_thermal_ensemble_create(int sites) {
  try {
    return new ThermalEnsemble(sites);
  } catch (const std::exception& e) {
    g_serr = e.what();
    return nullptr;
  }
}
void eigenex_thermal_ensemble_destroy(void* e) { delete static_cast<ThermalEnsemble*>(e); }
int eigenex_thermal_ensemble_value(void* e, int quantity, int64_t t, double beta, double* value) {
  return guard([&] {
    const ThermalEnsemble& en = *static_cast<ThermalEnsemble*>(e);
    switch (quantity) {
      case 0: *value = en.logPartitionFunction(beta); break;
      case 1: *value = en.energy(beta); break;
      case 2: *value = en.specificHeat(beta); break;
      case 3: *value = en.entropy(beta); break;
      case 4: *value = en.susceptibility(beta); break;
      case 5: *value = en.observable((std::size_t)t, beta); break;
      default: throw LanczosException("thermal ensemble: quantity must be 0..5");
    }
  });
}

EIGENEX_DENSITY_FAMILY(eigenex_density_solver_, SpectralDensitySolver<double>)
EIGENEX_DENSITY_FAMILY(eigenex_zdensity_solver_, SpectralDensitySolver<std::complex<double>>)
EIGENEX_TRLANCZOS_FAMILY(eigenex_trlanczos_solver_, ThickRestartLanczosEigenSolver<double>)
EIGENEX_TRLANCZOS_FAMILY(eigenex_ztrlanczos_solver_, ThickRestartLanczosEigenSolver<std::complex<double>>)
// FilteredLanczosEigenSolver: the same entry points; _set also takes "target", "filterDegree" and "spectralRange" (lo, hi)
EIGENEX_TRLANCZOS_FAMILY(eigenex_flanczos_solver_, FilteredLanczosEigenSolver<double>)
EIGENEX_TRLANCZOS_FAMILY(eigenex_zflanczos_solver_, FilteredLanczosEigenSolver<std::complex<double>>)
EIGENEX_KSCHUR_FAMILY(eigenex_kschur_solver_, double)
EIGENEX_KSCHUR_FAMILY(eigenex_zkschur_solver_, std::complex<double>)
EIGENEX_LANCZOS_FAMILY(eigenex_lanczos_solver_, double)
EIGENEX_LANCZOS_FAMILY(eigenex_zlanczos_solver_, std::complex<double>)
EIGENEX_ARNOLDI_FAMILY(eigenex_arnoldi_solver_, double)
EIGENEX_ARNOLDI_FAMILY(eigenex_zarnoldi_solver_, std::complex<double>)

// ---- The spin front-ends (spin_dynamics.hpp, spin_evolution.hpp, spin_time_correlation.hpp, spin_entanglement.hpp).  What their
// entry points share is written once here, over the box type; the families below name it per prefix.
}  // extern "C"

namespace {

// a solver that takes a model: the context it borrowed, the model and sector it was given (n_up = -1: the full space)
template <class Solver>
struct SpinBox {
  std::shared_ptr<device::Context> ctx;
  SpinHalfModel model;
  int n_up = -1;
  Solver es;
};
struct SpinDynamicsBox : SpinBox<SpinDynamicsSolver> {
  DenseVector<double> state;  // for static_structure_factor_z
};
typedef SpinBox<SpinMomentumDynamicsSolver> SpinMomentumDynamicsBox;
struct SpinEvolutionBox : SpinBox<SpinTimeEvolutionSolver> {
  std::vector<double> out;  // the last vector-valued result, until the next one
};
struct SpinTimeCorrelationBox : SpinBox<SpinTimeCorrelationSolver> {
  std::vector<std::complex<double>> out;  // the last values()
};
struct SpinEntanglementBox : Box<SpinEntanglementSolver> {
  DenseVector<double> state;
  DenseVector<std::complex<double>> stateZ;
};

// the model from the arrays of eigenex_spin_upload
SpinHalfModel spin_model_from_arrays(int n_sites, int n_bonds, const int32_t* site_i, const int32_t* site_j, const double* jz, const double* jxy,
                                     const double* hz_or_null, const double* hx_or_null) {
  SpinHalfModel model(n_sites);
  for (int k = 0; k < n_bonds; ++k) model.addBond(site_i[k], site_j[k], jz[k], jxy[k]);
  for (int i = 0; i < n_sites; ++i) {
    if (hz_or_null) model.setFieldZ(i, hz_or_null[i]);
    if (hx_or_null) model.setFieldX(i, hx_or_null[i]);
  }
  return model;
}
std::vector<std::complex<double>> complex_coefficients(const double* c, int n) {
  std::vector<std::complex<double>> out((size_t)(n > 0 ? n : 0));
  for (size_t i = 0; i < out.size(); ++i) out[i] = std::complex<double>(c[2 * i], c[2 * i + 1]);
  return out;
}

template <class B>
void* sp_create() {
  try {
    return new B();
  } catch (const std::exception& e) {
    g_serr = e.what();
    return nullptr;
  }
}
template <class B>
const char* sp_log_line(void* p, int64_t i) {
  auto& log = static_cast<B*>(p)->es.log();
  return i >= 0 && i < (int64_t)log.size() ? log[(size_t)i].c_str() : "";
}
template <class B>
int sp_set_model(void* p, eigenex_context_t ctx, int n_sites, int n_bonds, const int32_t* site_i, const int32_t* site_j, const double* jz,
                 const double* jxy, const double* hz_or_null, const double* hx_or_null, int n_up) {
  return guard([&] {
    auto* b = static_cast<B*>(p);
    b->ctx = device::Context::borrow(ctx);
    b->model = spin_model_from_arrays(n_sites, n_bonds, site_i, site_j, jz, jxy, hz_or_null, hx_or_null);
    b->n_up = n_up;
    b->es.setModel(b->ctx, b->model, n_up);
  });
}
// v: n entries, interleaved (re, im) if is_complex, else real
template <class B>
int sp_set_state(void* p, const double* v, int64_t n, int is_complex) {
  return guard([&] {
    auto& es = static_cast<B*>(p)->es;
    if (is_complex)
      es.setState(make_vector<std::complex<double>>(v, n));
    else
      es.setState(make_vector<double>(v, n));
  });
}
template <class B>
int sp_evolve(void* p, double dt, int64_t* substeps) {
  return guard([&] {
    const Index s = static_cast<B*>(p)->es.evolve(dt);
    if (substeps) *substeps = (int64_t)s;
  });
}

}  // namespace

extern "C" {

#define EIGENEX_SPIN_COMMON(PFX, BOX)                       \
  void* PFX##create(void) { return sp_create<BOX>(); }      \
  void PFX##destroy(void* p) { delete static_cast<BOX*>(p); } \
  const char* PFX##log_line(void* p, int64_t i) { return sp_log_line<BOX>(p, i); }

// ... of a solver that takes a model, which crosses as the arrays of eigenex_spin_upload; n_up = -1: the full space
#define EIGENEX_SPIN_MODEL_COMMON(PFX, BOX)                                                                                              \
  EIGENEX_SPIN_COMMON(PFX, BOX)                                                                                                          \
  int PFX##set_model(void* p, eigenex_context_t ctx, int n_sites, int n_bonds, const int32_t* site_i, const int32_t* site_j, const double* jz, \
                     const double* jxy, const double* hz_or_null, const double* hx_or_null, int n_up) {                                 \
    return sp_set_model<BOX>(p, ctx, n_sites, n_bonds, site_i, site_j, jz, jxy, hz_or_null, hx_or_null, n_up);                           \
  }

// ... of a solver that evolves a state; vectors are interleaved (re, im) if is_complex, else real
#define EIGENEX_SPIN_EVOLVING_FAMILY(PFX, BOX)                                                                                           \
  EIGENEX_SPIN_MODEL_COMMON(PFX, BOX)                                                                                                    \
  int PFX##set_state(void* p, const double* v, int64_t n, int is_complex) { return sp_set_state<BOX>(p, v, n, is_complex); }            \
  int PFX##set_product_state(void* p, uint32_t bits) { return guard([&] { static_cast<BOX*>(p)->es.setProductState(bits); }); }         \
  int PFX##set_krylov_dimension(void* p, int64_t m) { return guard([&] { static_cast<BOX*>(p)->es.setKrylovDimension((Index)m); }); }   \
  int PFX##set_tolerance(void* p, double tol) { return guard([&] { static_cast<BOX*>(p)->es.setTolerance(tol); }); }                    \
  int PFX##evolve(void* p, double dt, int64_t* substeps) { return sp_evolve<BOX>(p, dt, substeps); }

// ---- SpinDynamicsSolver
EIGENEX_SPIN_MODEL_COMMON(eigenex_spin_dynamics_solver_, SpinDynamicsBox)
int eigenex_spin_dynamics_solver_set_state(void* p, const double* v, int64_t n) {
  return guard([&] {
    auto* b = static_cast<SpinDynamicsBox*>(p);
    b->state = make_vector<double>(v, n);
    b->es.setState(b->state);
  });
}
// a complex state (n entries, interleaved) and complex coefficients (two arrays): the run becomes a complex one
int eigenex_spin_dynamics_solver_set_state_z(void* p, const double* v, int64_t n) { return sp_set_state<SpinDynamicsBox>(p, v, n, 1); }
int eigenex_spin_dynamics_solver_set_state_energy(void* p, double E0) {
  return guard([&] { static_cast<SpinDynamicsBox*>(p)->es.setStateEnergy(E0); });
}
int eigenex_spin_dynamics_solver_set_site_operator(void* p, int kind, const double* coef, int n) {
  return guard([&] { static_cast<SpinDynamicsBox*>(p)->es.setSiteOperator(kind, std::vector<double>(coef, coef + (n > 0 ? n : 0))); });
}
int eigenex_spin_dynamics_solver_set_site_operator_z(void* p, int kind, const double* coef_re, const double* coef_im, int n) {
  return guard([&] {
    std::vector<std::complex<double>> c((size_t)(n > 0 ? n : 0));
    for (size_t i = 0; i < c.size(); ++i) c[i] = std::complex<double>(coef_re[i], coef_im ? coef_im[i] : 0.0);
    static_cast<SpinDynamicsBox*>(p)->es.setSiteOperator(kind, c);
  });
}
int eigenex_spin_dynamics_solver_set_lanczos_steps(void* p, int64_t m) {
  return guard([&] { static_cast<SpinDynamicsBox*>(p)->es.setLanczosSteps((Index)m); });
}
int eigenex_spin_dynamics_solver_compute(void* p) { return guard([&] { static_cast<SpinDynamicsBox*>(p)->es.compute(); }); }
int eigenex_spin_dynamics_solver_compute_structure_factor_z(void* p, double q) {
  return guard([&] { static_cast<SpinDynamicsBox*>(p)->es.computeStructureFactorZ(q); });
}
int eigenex_spin_dynamics_solver_compute_structure_factor_z_single_run(void* p, double q) {
  return guard([&] { static_cast<SpinDynamicsBox*>(p)->es.computeStructureFactorZSingleRun(q); });
}
// out[5]: poles, alpha, beta, log lines, info
int eigenex_spin_dynamics_solver_sizes(void* p, int64_t* out) {
  return guard([&] {
    auto& es = static_cast<SpinDynamicsBox*>(p)->es;
    out[0] = (int64_t)es.poles().size(), out[1] = (int64_t)es.lanczosAlpha().size(), out[2] = (int64_t)es.lanczosBeta().size();
    out[3] = (int64_t)es.log().size(), out[4] = (int64_t)es.info();
  });
}
// any pointer may be NULL; scalars[3] = (totalWeight, stateEnergy, stateNormSquared)
int eigenex_spin_dynamics_solver_get(void* p, double* poles, double* weights, double* alpha, double* beta, double* scalars) {
  return guard([&] {
    auto& es = static_cast<SpinDynamicsBox*>(p)->es;
    if (poles) std::copy(es.poles().begin(), es.poles().end(), poles);
    if (weights) std::copy(es.weights().begin(), es.weights().end(), weights);
    if (alpha) std::copy(es.lanczosAlpha().begin(), es.lanczosAlpha().end(), alpha);
    if (beta) std::copy(es.lanczosBeta().begin(), es.lanczosBeta().end(), beta);
    if (scalars) scalars[0] = es.totalWeight(), scalars[1] = es.stateEnergy(), scalars[2] = es.stateNormSquared();
  });
}
int eigenex_spin_dynamics_solver_spectrum(void* p, const double* omega, int64_t n, double eta, double* out) {
  return guard([&] {
    for (int64_t i = 0; i < n; ++i) out[i] = static_cast<SpinDynamicsBox*>(p)->es.spectrum(omega[i], eta);
  });
}
int eigenex_spin_dynamics_solver_moment(void* p, int k, double* out) {
  return guard([&] { *out = static_cast<SpinDynamicsBox*>(p)->es.moment(k); });
}
// SpinCorrelationSolver::structureFactorZ(q) of the same model and state: the sum rule of computeStructureFactorZ(q)
int eigenex_spin_dynamics_solver_static_structure_factor_z(void* p, double q, double* out) {
  return guard([&] {
    auto* b = static_cast<SpinDynamicsBox*>(p);
    if (!b->ctx) throw LanczosException("static_structure_factor_z: no model");
    SpinCorrelationSolver sc;
    sc.setDeviceOperator(b->n_up < 0 ? device::spinHalfOperator(b->ctx, b->model) : device::spinHalfSectorOperator(b->ctx, b->model, b->n_up));
    sc.setState(b->state);
    sc.compute();
    if (sc.info() != Success) throw LanczosException("static_structure_factor_z: " + (sc.log().empty() ? std::string("failed") : sc.log().back()));
    *out = sc.structureFactorZ(q);
  });
}

// ---- SpinMomentumDynamicsSolver: the model crosses as the arrays of eigenex_spin_momentum_upload
EIGENEX_SPIN_COMMON(eigenex_spin_momentum_dynamics_solver_, SpinMomentumDynamicsBox)
int eigenex_spin_momentum_dynamics_solver_set_model(void* p, eigenex_context_t ctx, int n_sites, int n_bonds, const int32_t* site_i, const int32_t* site_j,
                                                    const double* jz, const double* jxy, const double* hz_or_null, int n_up, int momentum, int cell) {
  return guard([&] {
    auto* b = static_cast<SpinMomentumDynamicsBox*>(p);
    b->ctx = device::Context::borrow(ctx);
    b->model = spin_model_from_arrays(n_sites, n_bonds, site_i, site_j, jz, jxy, hz_or_null, nullptr);
    b->n_up = n_up;
    b->es.setModel(b->ctx, b->model, n_up, momentum, cell);
  });
}
int eigenex_spin_momentum_dynamics_solver_set_state(void* p, const double* v, int64_t n, int is_complex) {
  return sp_set_state<SpinMomentumDynamicsBox>(p, v, n, is_complex);
}
int eigenex_spin_momentum_dynamics_solver_set_state_energy(void* p, double E0) {
  return guard([&] { static_cast<SpinMomentumDynamicsBox*>(p)->es.setStateEnergy(E0); });
}
int eigenex_spin_momentum_dynamics_solver_set_site_operator(void* p, int kind, const double* cell_re, const double* cell_im, int n, int mp) {
  return guard([&] {
    std::vector<std::complex<double>> c((size_t)(n > 0 ? n : 0));
    for (size_t i = 0; i < c.size(); ++i) c[i] = std::complex<double>(cell_re[i], cell_im ? cell_im[i] : 0.0);
    static_cast<SpinMomentumDynamicsBox*>(p)->es.setSiteOperator(kind, c, mp);
  });
}
int eigenex_spin_momentum_dynamics_solver_set_lanczos_steps(void* p, int64_t m) {
  return guard([&] { static_cast<SpinMomentumDynamicsBox*>(p)->es.setLanczosSteps((Index)m); });
}
int eigenex_spin_momentum_dynamics_solver_compute(void* p) { return guard([&] { static_cast<SpinMomentumDynamicsBox*>(p)->es.compute(); }); }
int eigenex_spin_momentum_dynamics_solver_compute_structure_factor_z(void* p, int q_index) {
  return guard([&] { static_cast<SpinMomentumDynamicsBox*>(p)->es.computeStructureFactorZ(q_index); });
}
// out[9]: poles, alpha, beta, log lines, info, destination n_up, destination momentum, destination dimension, complex run
int eigenex_spin_momentum_dynamics_solver_sizes(void* p, int64_t* out) {
  return guard([&] {
    auto& es = static_cast<SpinMomentumDynamicsBox*>(p)->es;
    out[0] = (int64_t)es.poles().size(), out[1] = (int64_t)es.lanczosAlpha().size(), out[2] = (int64_t)es.lanczosBeta().size();
    out[3] = (int64_t)es.log().size(), out[4] = (int64_t)es.info();
    out[5] = es.destinationSitesUp(), out[6] = es.destinationMomentum(), out[7] = (int64_t)es.destinationDimension(), out[8] = es.complexRun() ? 1 : 0;
  });
}
// any pointer may be NULL; scalars[3] = (totalWeight, stateEnergy, stateNormSquared)
int eigenex_spin_momentum_dynamics_solver_get(void* p, double* poles, double* weights, double* alpha, double* beta, double* scalars) {
  return guard([&] {
    auto& es = static_cast<SpinMomentumDynamicsBox*>(p)->es;
    if (poles) std::copy(es.poles().begin(), es.poles().end(), poles);
    if (weights) std::copy(es.weights().begin(), es.weights().end(), weights);
    if (alpha) std::copy(es.lanczosAlpha().begin(), es.lanczosAlpha().end(), alpha);
    if (beta) std::copy(es.lanczosBeta().begin(), es.lanczosBeta().end(), beta);
    if (scalars) scalars[0] = es.totalWeight(), scalars[1] = es.stateEnergy(), scalars[2] = es.stateNormSquared();
  });
}
int eigenex_spin_momentum_dynamics_solver_spectrum(void* p, const double* omega, int64_t n, double eta, double* out) {
  return guard([&] {
    for (int64_t i = 0; i < n; ++i) out[i] = static_cast<SpinMomentumDynamicsBox*>(p)->es.spectrum(omega[i], eta);
  });
}
int eigenex_spin_momentum_dynamics_solver_moment(void* p, int k, double* out) {
  return guard([&] { *out = static_cast<SpinMomentumDynamicsBox*>(p)->es.moment(k); });
}

// ---- SpinTimeEvolutionSolver
EIGENEX_SPIN_EVOLVING_FAMILY(eigenex_spin_evolution_solver_, SpinEvolutionBox)
// scalars[5] = (time, errorBound, totalErrorBound, initialNorm, operatorApplications); counts[4] = (log lines, info, sites, rows of out)
int eigenex_spin_evolution_solver_status(void* p, double* scalars, int64_t* counts) {
  return guard([&] {
    auto* b = static_cast<SpinEvolutionBox*>(p);
    auto& es = b->es;
    if (scalars)
      scalars[0] = es.time(), scalars[1] = es.errorBound(), scalars[2] = es.totalErrorBound(), scalars[3] = es.initialNorm(),
      scalars[4] = (double)es.operatorApplications();
    if (counts) counts[0] = (int64_t)es.log().size(), counts[1] = (int64_t)es.info(), counts[2] = es.sites(), counts[3] = (int64_t)b->out.size();
  });
}
// what: 0 normSquared, 1 energy, 2 overlapWithInitial (re, im); out[2]
int eigenex_spin_evolution_solver_scalar(void* p, int what, double* out) {
  return guard([&] {
    auto& es = static_cast<SpinEvolutionBox*>(p)->es;
    out[0] = out[1] = 0.0;
    if (what == 0) out[0] = es.normSquared();
    else if (what == 1) out[0] = es.energy();
    else if (what == 2) {
      const std::complex<double> z = es.overlapWithInitial();
      out[0] = z.real(), out[1] = z.imag();
    } else throw LanczosException("eigenex_spin_evolution_solver_scalar: what must be 0..2");
  });
}
// what: 0 magnetisation (sites), 1 correlationsZZ, 2 correlationsXY (sites^2, row-major), 3 state (2 * rows, interleaved).  Forms the
// result and returns its length in doubles; eigenex_spin_evolution_solver_fetch copies it out.
int eigenex_spin_evolution_solver_measure(void* p, int what, int64_t* len) {
  return guard([&] {
    auto* b = static_cast<SpinEvolutionBox*>(p);
    auto& es = b->es;
    if (what == 0) b->out = es.magnetisation();
    else if (what == 1) b->out = es.correlationsZZ();
    else if (what == 2) b->out = es.correlationsXY();
    else if (what == 3) {
      const auto v = es.state();
      b->out.assign(reinterpret_cast<const double*>(v.data()), reinterpret_cast<const double*>(v.data()) + 2 * v.size());
    } else throw LanczosException("eigenex_spin_evolution_solver_measure: what must be 0..3");
    if (len) *len = (int64_t)b->out.size();
  });
}
// The entanglement of a subsystem of the state (SpinTimeEvolutionSolver::entanglementEntropy, entanglementRenyi2,
// entanglementSpectrum), given as a mask (sites = NULL) or as n_sites_listed sites.  what: 0 entropy, 1 renyi2 (one double each), 2 the
// spectrum.  Forms the result and returns its length; eigenex_spin_evolution_solver_fetch copies it out.
int eigenex_spin_evolution_solver_entanglement(void* p, uint32_t mask, const int32_t* sites, int n_sites_listed, int what, int64_t* len) {
  return guard([&] {
    auto* b = static_cast<SpinEvolutionBox*>(p);
    auto& es = b->es;
    const std::vector<int> list(sites, sites + (sites && n_sites_listed > 0 ? n_sites_listed : 0));
    if (what == 0) b->out.assign(1, sites ? es.entanglementEntropy(list) : es.entanglementEntropy(mask));
    else if (what == 1) b->out.assign(1, sites ? es.entanglementRenyi2(list) : es.entanglementRenyi2(mask));
    else if (what == 2) b->out = sites ? es.entanglementSpectrum(list) : es.entanglementSpectrum(mask);
    else throw LanczosException("eigenex_spin_evolution_solver_entanglement: what must be 0..2");
    if (len) *len = (int64_t)b->out.size();
  });
}
int eigenex_spin_evolution_solver_fetch(void* p, double* out) {
  return guard([&] {
    auto* b = static_cast<SpinEvolutionBox*>(p);
    std::copy(b->out.begin(), b->out.end(), out);
    std::vector<double>().swap(b->out);
  });
}

// ---- SpinTimeCorrelationSolver.  Complex coefficients are interleaved (re, im).
EIGENEX_SPIN_EVOLVING_FAMILY(eigenex_spin_time_correlation_solver_, SpinTimeCorrelationBox)
int eigenex_spin_time_correlation_solver_set_eigenstate(void* p, double E0) {
  return guard([&] { static_cast<SpinTimeCorrelationBox*>(p)->es.setEigenstate(E0); });
}
// coef: n complex coefficients, interleaved
int eigenex_spin_time_correlation_solver_set_source_operator(void* p, int kind, const double* coef, int n) {
  return guard([&] { static_cast<SpinTimeCorrelationBox*>(p)->es.setSourceOperator(kind, complex_coefficients(coef, n)); });
}
int eigenex_spin_time_correlation_solver_add_measured_operator(void* p, const double* coef, int n) {
  return guard([&] { static_cast<SpinTimeCorrelationBox*>(p)->es.addMeasuredOperator(complex_coefficients(coef, n)); });
}
int eigenex_spin_time_correlation_solver_clear_measured_operators(void* p) {
  return guard([&] { static_cast<SpinTimeCorrelationBox*>(p)->es.clearMeasuredOperators(); });
}
int eigenex_spin_time_correlation_solver_set_measured_sites(void* p) {
  return guard([&] { static_cast<SpinTimeCorrelationBox*>(p)->es.setMeasuredSites(); });
}
int eigenex_spin_time_correlation_solver_set_momentum_z(void* p, double q) {
  return guard([&] { static_cast<SpinTimeCorrelationBox*>(p)->es.setMomentumZ(q); });
}
// forms values() and returns their number; eigenex_spin_time_correlation_solver_fetch copies them out, interleaved
int eigenex_spin_time_correlation_solver_values(void* p, int64_t* count) {
  return guard([&] {
    auto* b = static_cast<SpinTimeCorrelationBox*>(p);
    b->out = b->es.values();
    if (count) *count = (int64_t)b->out.size();
  });
}
int eigenex_spin_time_correlation_solver_fetch(void* p, double* out) {
  return guard([&] {
    auto* b = static_cast<SpinTimeCorrelationBox*>(p);
    for (size_t i = 0; i < b->out.size(); ++i) out[2 * i] = b->out[i].real(), out[2 * i + 1] = b->out[i].imag();
  });
}
// scalars[6] = (time, sourceNormSquared, errorBound, stateErrorBound, sourceErrorBound, operatorApplications);
// counts[3] = (log lines, info, measured operators)
int eigenex_spin_time_correlation_solver_status(void* p, double* scalars, int64_t* counts) {
  return guard([&] {
    auto& es = static_cast<SpinTimeCorrelationBox*>(p)->es;
    if (scalars)
      scalars[0] = es.time(), scalars[1] = es.sourceNormSquared(), scalars[2] = es.errorBound(), scalars[3] = es.stateErrorBound(),
      scalars[4] = es.sourceErrorBound(), scalars[5] = (double)es.operatorApplications();
    if (counts) counts[0] = (int64_t)es.log().size(), counts[1] = (int64_t)es.info(), counts[2] = (int64_t)es.measuredOperators();
  });
}
// errorBound(n) and operatorNormBound(n) of measured operator n; out[2]
int eigenex_spin_time_correlation_solver_operator_bounds(void* p, int64_t n, double* out) {
  return guard([&] {
    auto& es = static_cast<SpinTimeCorrelationBox*>(p)->es;
    out[0] = es.errorBound((size_t)n), out[1] = es.operatorNormBound((size_t)n);
  });
}

// ---- SpinEntanglementSolver.  The operator crosses as a handle of eigenex_spin_upload / eigenex_spin_sector_upload.
EIGENEX_SPIN_COMMON(eigenex_spin_entanglement_solver_, SpinEntanglementBox)
int eigenex_spin_entanglement_solver_set_device_operator(void* p, eigenex_context_t ctx, eigenex_csr_t csr) {
  return guard([&] {
    auto* b = static_cast<SpinEntanglementBox*>(p);
    b->ctx = device::Context::borrow(ctx);
    b->op = device::CsrOperator::borrow(b->ctx, csr);
    b->es.setDeviceOperator(b->op);
  });
}
int eigenex_spin_entanglement_solver_set_state(void* p, const double* v, int64_t n) {
  return guard([&] {
    auto* b = static_cast<SpinEntanglementBox*>(p);
    b->state = make_vector<double>(v, n);
    b->es.setState(b->state);
  });
}
// a complex state: n interleaved (re, im) pairs
int eigenex_spin_entanglement_solver_set_state_z(void* p, const double* v, int64_t n) {
  return guard([&] {
    auto* b = static_cast<SpinEntanglementBox*>(p);
    b->stateZ = make_vector<std::complex<double>>(v, n);
    b->es.setState(b->stateZ);
  });
}
int eigenex_spin_entanglement_solver_set_subsystem(void* p, const int32_t* sites, int n) {
  return guard([&] { static_cast<SpinEntanglementBox*>(p)->es.setSubsystem(std::vector<int>(sites, sites + (n > 0 ? n : 0))); });
}
int eigenex_spin_entanglement_solver_set_subsystem_mask(void* p, uint32_t mask) {
  return guard([&] { static_cast<SpinEntanglementBox*>(p)->es.setSubsystemMask(mask); });
}
int eigenex_spin_entanglement_solver_compute(void* p) { return guard([&] { static_cast<SpinEntanglementBox*>(p)->es.compute(); }); }
// out[4]: blocks, eigenvalues, log lines, info
int eigenex_spin_entanglement_solver_sizes(void* p, int64_t* out) {
  return guard([&] {
    auto& es = static_cast<SpinEntanglementBox*>(p)->es;
    out[0] = (int64_t)es.blocks(), out[1] = (int64_t)es.spectrum().size(), out[2] = (int64_t)es.log().size(), out[3] = (int64_t)es.info();
  });
}
// block n: sites up inside the subsystem, dimension and, unless NULL, the dimension^2 column-major entries of unit-trace rho_A
int eigenex_spin_entanglement_solver_block(void* p, int64_t n, int* sites_up, int64_t* dim, double* rho) {
  return guard([&] {
    auto& es = static_cast<SpinEntanglementBox*>(p)->es;
    if (sites_up) *sites_up = es.blockSitesUp((Index)n);
    if (dim) *dim = (int64_t)es.blockDimension((Index)n);
    if (rho) std::copy(es.reducedDensityMatrix((Index)n).begin(), es.reducedDensityMatrix((Index)n).end(), rho);
  });
}
// the same of a complex state: rho takes 2 * dimension^2 doubles, interleaved (re, im); *is_complex (may be NULL) says which of
// the two calls has the entries (the other one throws)
int eigenex_spin_entanglement_solver_block_z(void* p, int64_t n, int* is_complex, double* rho) {
  return guard([&] {
    auto& es = static_cast<SpinEntanglementBox*>(p)->es;
    if (is_complex) *is_complex = es.stateIsComplex() ? 1 : 0;
    if (rho) {
      const auto& z = es.reducedDensityMatrixComplex((Index)n);
      std::copy(reinterpret_cast<const double*>(z.data()), reinterpret_cast<const double*>(z.data()) + 2 * z.size(), rho);
    }
  });
}
// any pointer may be NULL; scalars[3] = (normSquared, entropy, renyi2), the last two only after a successful compute()
int eigenex_spin_entanglement_solver_get(void* p, double* spectrum, double* scalars) {
  return guard([&] {
    auto& es = static_cast<SpinEntanglementBox*>(p)->es;
    if (spectrum) std::copy(es.spectrum().begin(), es.spectrum().end(), spectrum);
    if (scalars) scalars[0] = es.normSquared(), scalars[1] = es.entropy(), scalars[2] = es.blocks() > 0 ? es.renyi2() : 0.0;
  });
}
int eigenex_spin_entanglement_solver_renyi(void* p, double alpha, double* out) {
  return guard([&] { *out = static_cast<SpinEntanglementBox*>(p)->es.renyi(alpha); });
}
int eigenex_spin_entanglement_solver_schmidt_rank(void* p, double tol, int64_t* out) {
  return guard([&] { *out = (int64_t)static_cast<SpinEntanglementBox*>(p)->es.schmidtRank(tol); });
}

}  // extern "C"
