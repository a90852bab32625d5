// small_eigen::hermitian (small_eigen.hpp) in a stand-alone C++11 program: a random 7 x 7 Hermitian matrix, one with a
// degenerate pair (and a degenerate triple), and the 1 x 1 and 2 x 2 cases.  Prints one line of JSON per matrix with
//   residual       ||A V - V Lambda||_F / ||A||_F
//   orthogonality  ||V^H V - I||_F
//   values         the eigenvalues, ascending
// tests/test_spin_rdm_z_host.py holds them to the bound it states.
#include <complex>
#include <cstdio>
#include <random>
#include <vector>

#include "cmpt/eigen_ex/small_eigen.hpp"

using cplx = std::complex<double>;
namespace se = cmpt::EigenEx::small_eigen;

static void report(const char* name, const std::vector<cplx>& A, int n) {
  std::vector<double> values, only;
  std::vector<cplx> V;
  const bool ok = se::hermitian(A, n, values, &V), ok2 = se::hermitian(A, n, only, nullptr);
  double a2 = 0.0, r2 = 0.0, o2 = 0.0;
  for (const cplx& e : A) a2 += std::norm(e);
  for (int c = 0; c < n; ++c)
    for (int r = 0; r < n; ++r) {
      cplx av(0.0, 0.0), g(0.0, 0.0);
      for (int k = 0; k < n; ++k) {
        av += A[static_cast<std::size_t>(r + k * n)] * V[static_cast<std::size_t>(k + c * n)];
        g += std::conj(V[static_cast<std::size_t>(k + r * n)]) * V[static_cast<std::size_t>(k + c * n)];
      }
      r2 += std::norm(av - V[static_cast<std::size_t>(r + c * n)] * values[static_cast<std::size_t>(c)]);
      o2 += std::norm(g - (r == c ? 1.0 : 0.0));
    }
  bool same = values.size() == only.size();
  for (std::size_t k = 0; same && k < values.size(); ++k) same = values[k] == only[k];
  std::printf("{\"name\": \"%s\", \"n\": %d, \"ok\": %d, \"values_alone_equal\": %d, \"residual\": %.17g, \"orthogonality\": %.17g, \"values\": [", name, n,
              ok && ok2 ? 1 : 0, same ? 1 : 0, std::sqrt(r2 / a2), std::sqrt(o2));
  for (int k = 0; k < n; ++k) std::printf("%s%.17g", k ? ", " : "", values[static_cast<std::size_t>(k)]);
  std::printf("]}\n");
}

// U diag(lam) U^H with U from the Gram-Schmidt of a random complex matrix; both triangles are filled, the result is made
// exactly Hermitian (the routine reads the lower triangle)
static std::vector<cplx> with_spectrum(const std::vector<double>& lam, std::mt19937& rng) {
  const int n = static_cast<int>(lam.size());
  std::normal_distribution<double> g(0.0, 1.0);
  std::vector<cplx> U(static_cast<std::size_t>(n * n));
  for (cplx& e : U) e = cplx(g(rng), g(rng));
  for (int c = 0; c < n; ++c) {
    for (int pass = 0; pass < 2; ++pass)
      for (int q = 0; q < c; ++q) {
        cplx dot(0.0, 0.0);
        for (int r = 0; r < n; ++r) dot += std::conj(U[static_cast<std::size_t>(r + q * n)]) * U[static_cast<std::size_t>(r + c * n)];
        for (int r = 0; r < n; ++r) U[static_cast<std::size_t>(r + c * n)] -= dot * U[static_cast<std::size_t>(r + q * n)];
      }
    double nrm = 0.0;
    for (int r = 0; r < n; ++r) nrm += std::norm(U[static_cast<std::size_t>(r + c * n)]);
    for (int r = 0; r < n; ++r) U[static_cast<std::size_t>(r + c * n)] /= std::sqrt(nrm);
  }
  std::vector<cplx> A(static_cast<std::size_t>(n * n), cplx(0.0, 0.0));
  for (int c = 0; c < n; ++c)
    for (int r = c; r < n; ++r) {
      cplx s(0.0, 0.0);
      for (int k = 0; k < n; ++k) s += U[static_cast<std::size_t>(r + k * n)] * lam[static_cast<std::size_t>(k)] * std::conj(U[static_cast<std::size_t>(c + k * n)]);
      if (r == c) s = cplx(s.real(), 0.0);
      A[static_cast<std::size_t>(r + c * n)] = s, A[static_cast<std::size_t>(c + r * n)] = std::conj(s);
    }
  return A;
}

int main() {
  std::mt19937 rng(41);
  std::normal_distribution<double> g(0.0, 1.0);
  const int n = 7;
  std::vector<cplx> A(static_cast<std::size_t>(n * n));
  for (int c = 0; c < n; ++c)
    for (int r = c; r < n; ++r) {
      const cplx e = r == c ? cplx(g(rng), 0.0) : cplx(g(rng), g(rng));
      A[static_cast<std::size_t>(r + c * n)] = e, A[static_cast<std::size_t>(c + r * n)] = std::conj(e);
    }
  report("random7", A, n);
  report("degenerate_pair7", with_spectrum({-1.5, -0.25, 0.5, 0.5, 1.0, 2.0, 3.5}, rng), n);
  report("degenerate_triple7", with_spectrum({0.0, 0.0, 0.0, 0.125, 0.25, 0.25, 0.375}, rng), n);
  report("one", std::vector<cplx>{cplx(0.75, 0.0)}, 1);
  report("two", std::vector<cplx>{cplx(1.0, 0.0), cplx(0.0, -2.0), cplx(0.0, 2.0), cplx(1.0, 0.0)}, 2);
  return 0;
}
