// Small dense eigen-solvers that run on the host, once per Krylov step, on the
// j x j projected matrix (j <= a few hundred).  They stand in for the Eigen3 calls
// the reference makes at these call sites:
//   Eigen::SelfAdjointEigenSolver::computeFromTridiagonal   lanczos.hpp:741, :781
//   Eigen::EigenSolver / Eigen::ComplexEigenSolver::compute  arnoldi.hpp:488-494, :811
// Eigen3 is not vendored by the reference (version unpinned); only the
// mathematical contract is reproduced: ascending eigenvalues + orthonormal
// eigenvectors for the symmetric tridiagonal case; eigenvalues + unit-norm right
// eigenvectors for the Hessenberg case.  O(j^2) per step for values only, which is
// what the convergence test consumes (lanczos.hpp:853-896); vectors are computed
// once at the end ("per-iteration dense eigen-solve").
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <limits>
#include <type_traits>
#include <vector>

namespace cmpt {
namespace EigenEx {
namespace small_eigen {

using cplx = std::complex<double>;

// What the dense routines below look at before they square an entry.  A NaN or an infinite entry makes the routine return
// false: it still runs to its (bounded) end on the entries as they are, so a caller that ignores the return sees what it saw
// before.  Entries whose largest magnitude lies outside [2^-300, 2^300] have squares and products that overflow, or underflow
// below the bits that count; they are multiplied by the power of two that brings the largest into [1/2, 1) -- exact -- and
// the eigenvalues are multiplied back; the vectors do not depend on the scale.  Inside the range nothing is touched, so every
// result there keeps its bits.
struct EntryRange {
  double largest = 0.0;
  bool finite = true;
  void see(double x) {
    if (!std::isfinite(x))
      finite = false;
    else
      largest = std::max(largest, std::fabs(x));
  }
  void see(const cplx& x) { see(x.real()), see(x.imag()); }
  // e != 0: multiply the entries by 2^-e and the eigenvalues by 2^e
  int exponent() const {
    if (!finite || largest == 0.0 || (largest >= std::ldexp(1.0, -300) && largest <= std::ldexp(1.0, 300))) return 0;
    int e = 0;
    std::frexp(largest, &e);
    return e;
  }
};
inline double times_two_to(double x, int e) { return std::ldexp(x, e); }
inline cplx times_two_to(const cplx& x, int e) { return cplx(std::ldexp(x.real(), e), std::ldexp(x.imag(), e)); }
// the eigenvalues of the scaled problem back at the caller's scale; false if one of them is beyond the largest double
template <class T>
bool values_times_two_to(std::vector<T>& values, int e) {
  EntryRange after;
  for (T& v : values) after.see(v = times_two_to(v, e));
  return after.finite;
}

// Symmetric tridiagonal eigenproblem by the implicit-shift QL iteration.
// diag[n], sub[n-1] (extra entries of `sub` are ignored, cf. the surplus beta the
// reference leaves behind on breakdown, lanczos.hpp:433-436).
// values: ascending.  vectors (optional): column-major n x n, column k belongs to values[k].
// Returns false if an eigenvalue failed to converge in 60 sweeps, or if an entry is not finite.
inline bool tridiagonal(const double* diag, const double* sub, int n, std::vector<double>& values,
                        std::vector<double>* vectors) {
  values.assign(diag, diag + n);
  if (vectors) {
    vectors->assign(static_cast<std::size_t>(n) * n, 0.0);
    for (int i = 0; i < n; ++i) (*vectors)[static_cast<std::size_t>(i) * n + i] = 1.0;
  }
  EntryRange seen;
  for (int i = 0; i < n; ++i) seen.see(diag[i]);
  for (int i = 0; i + 1 < n; ++i) seen.see(sub[i]);
  if (n <= 1) return seen.finite;
  std::vector<double> e(sub, sub + (n - 1));
  e.push_back(0.0);
  double* d = values.data();
  double* z = vectors ? vectors->data() : nullptr;  // z[row + col*n]
  const double eps = std::numeric_limits<double>::epsilon();
  bool ok = seen.finite;
  for (int l = 0; l < n; ++l) {
    int iter = 0;
    for (;;) {
      int m = l;
      for (; m < n - 1; ++m) {
        const double dd = std::fabs(d[m]) + std::fabs(d[m + 1]);
        if (std::fabs(e[m]) <= eps * dd) break;
      }
      if (m == l) break;
      if (++iter > 60) {
        ok = false;
        break;
      }
      // Wilkinson-type shift from the leading 2x2 of the unreduced block
      double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
      double r = std::hypot(g, 1.0);
      g = d[m] - d[l] + e[l] / (g + (g >= 0.0 ? std::fabs(r) : -std::fabs(r)));
      double s = 1.0, c = 1.0, p = 0.0;
      int i = m - 1;
      for (; i >= l; --i) {
        double f = s * e[i];
        const double b = c * e[i];
        r = std::hypot(f, g);
        e[i + 1] = r;
        if (r == 0.0) {  // recover from underflow
          d[i + 1] -= p;
          e[m] = 0.0;
          break;
        }
        s = f / r;
        c = g / r;
        g = d[i + 1] - p;
        r = (d[i] - g) * s + 2.0 * c * b;
        p = s * r;
        d[i + 1] = g + p;
        g = c * r - b;
        if (z) {
          double* zi = z + static_cast<std::size_t>(i) * n;
          double* zi1 = zi + n;
          for (int k = 0; k < n; ++k) {
            f = zi1[k];
            zi1[k] = s * zi[k] + c * f;
            zi[k] = c * zi[k] - s * f;
          }
        }
      }
      if (r == 0.0 && i >= l) continue;
      d[l] -= p;
      e[l] = g;
      e[m] = 0.0;
    }
  }
  // ascending order (selection sort keeps the column moves at O(n^2))
  for (int i = 0; i < n - 1; ++i) {
    int k = i;
    for (int j = i + 1; j < n; ++j)
      if (d[j] < d[k]) k = j;
    if (k != i) {
      std::swap(d[i], d[k]);
      if (z) std::swap_ranges(z + static_cast<std::size_t>(i) * n, z + static_cast<std::size_t>(i + 1) * n,
                              z + static_cast<std::size_t>(k) * n);
    }
  }
  return ok;
}

// Dense real symmetric eigenproblem (column-major n x n in A, destroyed): Householder reduction to
// tridiagonal form with accumulated reflectors, then the QL iteration above; eigenvectors = Q * Z.
// Used by the thick-restart solver, whose projected matrix is diag(theta) bordered by one row of
// couplings plus a tridiagonal tail.  values ascending; vectors column-major n x n.  Returns false if the QL iteration did
// not converge, if an entry is not finite, or if an eigenvalue is beyond the largest double (EntryRange above).
inline bool symmetric(std::vector<double>& A, int n, std::vector<double>& values, std::vector<double>& vectors) {
  auto a = [&](int r, int c) -> double& { return A[static_cast<std::size_t>(r) + static_cast<std::size_t>(c) * n]; };
  EntryRange seen;
  for (std::size_t i = 0; i < static_cast<std::size_t>(n) * n; ++i) seen.see(A[i]);
  const int scale = seen.exponent();
  if (scale != 0)
    for (std::size_t i = 0; i < static_cast<std::size_t>(n) * n; ++i) A[i] = times_two_to(A[i], -scale);
  std::vector<double> Q(static_cast<std::size_t>(n) * n, 0.0);
  auto q = [&](int r, int c) -> double& { return Q[static_cast<std::size_t>(r) + static_cast<std::size_t>(c) * n]; };
  for (int i = 0; i < n; ++i) q(i, i) = 1.0;
  std::vector<double> v(static_cast<std::size_t>(n)), p(static_cast<std::size_t>(n));
  for (int k = 0; k + 2 < n; ++k) {
    double nrm2 = 0.0;
    for (int i = k + 1; i < n; ++i) nrm2 += a(i, k) * a(i, k);
    // the entries below the sub-diagonal, summed on their own: nrm2 - a(k+1,k)^2 cancels to 0 once they are below 1.5e-8
    // |a(k+1,k)|, and a column skipped on that account kept entries that nothing looked at again
    double tail2 = 0.0;
    for (int i = k + 2; i < n; ++i) tail2 += a(i, k) * a(i, k);
    if (tail2 <= 0.0) continue;  // column already tridiagonal
    const double nrm = std::sqrt(nrm2);
    const double alpha = a(k + 1, k) > 0.0 ? -nrm : nrm;
    for (int i = k + 1; i < n; ++i) v[static_cast<std::size_t>(i)] = a(i, k);
    v[static_cast<std::size_t>(k + 1)] -= alpha;
    double vn = 0.0;
    for (int i = k + 1; i < n; ++i) vn += v[static_cast<std::size_t>(i)] * v[static_cast<std::size_t>(i)];
    vn = std::sqrt(vn);
    for (int i = k + 1; i < n; ++i) v[static_cast<std::size_t>(i)] /= vn;
    // p = A22 v ; K = v.p ; A22 -= 2 (v w^T + w v^T) with w = p - K v
    double K = 0.0;
    for (int i = k + 1; i < n; ++i) {
      double s = 0.0;
      for (int j = k + 1; j < n; ++j) s += a(i, j) * v[static_cast<std::size_t>(j)];
      p[static_cast<std::size_t>(i)] = s;
      K += s * v[static_cast<std::size_t>(i)];
    }
    for (int i = k + 1; i < n; ++i) p[static_cast<std::size_t>(i)] -= K * v[static_cast<std::size_t>(i)];
    for (int j = k + 1; j < n; ++j)
      for (int i = k + 1; i < n; ++i)
        a(i, j) -= 2.0 * (v[static_cast<std::size_t>(i)] * p[static_cast<std::size_t>(j)] + p[static_cast<std::size_t>(i)] * v[static_cast<std::size_t>(j)]);
    a(k + 1, k) = a(k, k + 1) = alpha;
    for (int i = k + 2; i < n; ++i) a(i, k) = a(k, i) = 0.0;
    // Q <- Q (I - 2 v v^T)
    for (int r = 0; r < n; ++r) {
      double s = 0.0;
      for (int j = k + 1; j < n; ++j) s += q(r, j) * v[static_cast<std::size_t>(j)];
      s *= 2.0;
      for (int j = k + 1; j < n; ++j) q(r, j) -= s * v[static_cast<std::size_t>(j)];
    }
  }
  std::vector<double> d(static_cast<std::size_t>(n)), e(static_cast<std::size_t>(n > 0 ? n : 1), 0.0), Z;
  for (int i = 0; i < n; ++i) d[static_cast<std::size_t>(i)] = a(i, i);
  for (int i = 0; i + 1 < n; ++i) e[static_cast<std::size_t>(i)] = a(i + 1, i);
  bool ok = tridiagonal(d.data(), e.data(), n, values, &Z) && seen.finite;
  if (scale != 0) ok = values_times_two_to(values, scale) && ok;
  vectors.assign(static_cast<std::size_t>(n) * n, 0.0);
  for (int c = 0; c < n; ++c)
    for (int j = 0; j < n; ++j) {
      const double z = Z[static_cast<std::size_t>(j) + static_cast<std::size_t>(c) * n];
      if (z == 0.0) continue;
      for (int r = 0; r < n; ++r) vectors[static_cast<std::size_t>(r) + static_cast<std::size_t>(c) * n] += q(r, j) * z;
    }
  return ok;
}

// Complex Hermitian eigenproblem (column-major n x n in A, read only; the strict upper triangle is not looked at), in the
// simple form: the real symmetric embedding B = [[Re A, -Im A], [Im A, Re A]] of order 2n goes through symmetric() above.
// Every eigenvalue of A is a double eigenvalue of B, with the eigenvectors (Re z; Im z) and (-Im z; Re z) of z and of i z, so
// values[k] = the (2k)-th of B's ascending eigenvalues.  Cost: one dense solve of order 2n, eight times the arithmetic and four
// times the memory of a complex Householder + QL solve of order n; it runs on blocks of a few thousand rows at most, once per
// measurement.  vectors (column-major n x n, column k belongs to values[k]; may be NULL): B's eigenvectors are taken in
// ascending order as z = u + i v and orthogonalised against the columns already accepted by modified Gram-Schmidt, twice; one
// that keeps less than 1 / (4n) of its squared norm is a combination of accepted ones (the partner i z, or a mix of them inside
// a degenerate eigenvalue) and is skipped.  The squared residuals of all 2n candidates against p accepted columns add up to
// 2 (n - p), so until n columns are accepted a candidate above that threshold is still to come: exactly n are kept.
// Normalising an accepted column amplifies its rounding error by at most 2 sqrt(n).
inline bool hermitian(const std::vector<cplx>& A, int n, std::vector<double>& values, std::vector<cplx>* vectors) {
  const int m = 2 * n;
  std::vector<double> B(static_cast<std::size_t>(m) * m, 0.0), w, Z;
  for (int c = 0; c < n; ++c)
    for (int r = c; r < n; ++r) {
      const cplx e = A[static_cast<std::size_t>(r) + static_cast<std::size_t>(c) * n];
      const double re = e.real(), im = r == c ? 0.0 : e.imag();
      const auto put = [&](int i, int j, double v) { B[static_cast<std::size_t>(i) + static_cast<std::size_t>(j) * m] = v, B[static_cast<std::size_t>(j) + static_cast<std::size_t>(i) * m] = v; };
      put(r, c, re), put(n + r, n + c, re);  // Re A on both diagonal blocks
      put(n + r, c, im);                     // Im A below: B[n + r, c] = Im A[r, c], and its mirror B[c, n + r] = -Im A[c, r]
      if (r != c) put(n + c, r, -im);        // Im A[c, r] = -Im A[r, c]
    }
  const bool ok = symmetric(B, m, w, Z);
  values.resize(static_cast<std::size_t>(n));
  for (int k = 0; k < n; ++k) values[static_cast<std::size_t>(k)] = w[static_cast<std::size_t>(2 * k)];
  if (!vectors) return ok;
  vectors->assign(static_cast<std::size_t>(n) * n, cplx(0.0, 0.0));
  int kept = 0;
  std::vector<cplx> z(static_cast<std::size_t>(n));
  for (int c = 0; c < m && kept < n; ++c) {
    for (int r = 0; r < n; ++r) z[static_cast<std::size_t>(r)] = cplx(Z[static_cast<std::size_t>(r) + static_cast<std::size_t>(c) * m], Z[static_cast<std::size_t>(n + r) + static_cast<std::size_t>(c) * m]);
    for (int pass = 0; pass < 2; ++pass)
      for (int q = 0; q < kept; ++q) {
        const cplx* col = vectors->data() + static_cast<std::size_t>(q) * n;
        cplx dot(0.0, 0.0);
        for (int r = 0; r < n; ++r) dot += std::conj(col[r]) * z[static_cast<std::size_t>(r)];
        for (int r = 0; r < n; ++r) z[static_cast<std::size_t>(r)] -= dot * col[r];
      }
    double nrm2 = 0.0;
    for (int r = 0; r < n; ++r) nrm2 += std::norm(z[static_cast<std::size_t>(r)]);
    if (!(nrm2 >= 1.0 / (4.0 * n))) continue;
    const double inv = 1.0 / std::sqrt(nrm2);
    for (int r = 0; r < n; ++r) (*vectors)[static_cast<std::size_t>(r) + static_cast<std::size_t>(kept) * n] = z[static_cast<std::size_t>(r)] * inv;
    ++kept;
  }
  return ok && kept == n;
}

// Eigen-decomposition of a complex upper-Hessenberg matrix H (column-major n x n,
// overwritten) by the single-shift QR iteration to Schur form T = Z^H H Z, then
// back-substitution for the eigenvectors of T and X = Z*Y with unit-norm columns.
// values[k] = T_kk in Schur order (the caller sorts, arnoldi.hpp:813-822).
// vectors (optional): column-major n x n.  Returns false if the iteration did not converge, if an entry on or above the
// sub-diagonal is not finite, or if an eigenvalue is beyond the largest double (EntryRange above).
inline bool hessenberg(std::vector<cplx>& H, int n, std::vector<cplx>& values, std::vector<cplx>* vectors) {
  values.assign(static_cast<std::size_t>(n), cplx(0.0));
  auto h = [&](int r, int c) -> cplx& { return H[static_cast<std::size_t>(r) + static_cast<std::size_t>(c) * n]; };
  EntryRange seen;
  for (int c = 0; c < n; ++c)
    for (int r = 0; r <= std::min(c + 1, n - 1); ++r) seen.see(h(r, c));
  const int scale = seen.exponent();
  if (scale != 0)
    for (int c = 0; c < n; ++c)
      for (int r = 0; r <= std::min(c + 1, n - 1); ++r) h(r, c) = times_two_to(h(r, c), -scale);
  std::vector<cplx> Z;
  const bool wantz = vectors != nullptr;
  if (wantz) {
    Z.assign(static_cast<std::size_t>(n) * n, cplx(0.0));
    for (int i = 0; i < n; ++i) Z[static_cast<std::size_t>(i) * n + i] = 1.0;
  }
  auto zz = [&](int r, int c) -> cplx& { return Z[static_cast<std::size_t>(r) + static_cast<std::size_t>(c) * n]; };
  const double eps = std::numeric_limits<double>::epsilon();
  double hnorm = 0.0;
  for (int c = 0; c < n; ++c)
    for (int r = 0; r <= std::min(c + 1, n - 1); ++r) hnorm = std::max(hnorm, std::abs(h(r, c)));
  if (hnorm == 0.0) hnorm = 1.0;
  bool ok = seen.finite;
  int iu = n - 1, iter = 0, total = 0;
  while (iu > 0) {
    // look for a negligible sub-diagonal entry
    int il = iu;
    while (il > 0) {
      double s = std::abs(h(il - 1, il - 1)) + std::abs(h(il, il));
      if (s == 0.0) s = hnorm;
      if (std::abs(h(il, il - 1)) <= eps * s) break;
      --il;
    }
    if (il > 0) h(il, il - 1) = 0.0;
    if (il == iu) {
      --iu;
      iter = 0;
      continue;
    }
    ++iter;
    if (++total > 60 * n + 200) {
      ok = false;
      break;
    }
    // shift: eigenvalue of the trailing 2x2 closer to its last diagonal entry
    cplx mu;
    if (iter % 11 == 10) {
      mu = h(iu, iu) + cplx(std::abs(h(iu, iu - 1).real()) + std::abs(h(iu - 1, iu - 2 >= 0 ? iu - 2 : 0).real()), 0.0);
    } else {
      const cplx a = h(iu - 1, iu - 1), b = h(iu - 1, iu), c = h(iu, iu - 1), d = h(iu, iu);
      const cplx tr2 = 0.5 * (a + d);
      const cplx disc = std::sqrt(0.25 * (a - d) * (a - d) + b * c);
      const cplx e1 = tr2 + disc, e2 = tr2 - disc;
      mu = std::abs(e1 - d) < std::abs(e2 - d) ? e1 : e2;
    }
    // one QR sweep on rows/cols il..iu by Givens rotations, applied to the whole matrix (Schur form)
    cplx x = h(il, il) - mu, y = h(il + 1, il);
    for (int k = il; k < iu; ++k) {
      const double ax = std::abs(x), ay = std::abs(y);
      double c = 1.0;
      cplx s = 0.0;
      if (ay != 0.0) {
        if (ax == 0.0) {
          c = 0.0;
          s = std::conj(y) / ay;
        } else {
          const double r = std::hypot(ax, ay);
          c = ax / r;
          s = (x / ax) * std::conj(y) / r;
        }
      }
      // rows k, k+1  <-  G * rows,  G = [c s; -conj(s) c]
      for (int j = std::max(k - 1, 0); j < n; ++j) {
        const cplx t1 = h(k, j), t2 = h(k + 1, j);
        h(k, j) = c * t1 + s * t2;
        h(k + 1, j) = -std::conj(s) * t1 + c * t2;
      }
      // cols k, k+1  <-  cols * G^H
      const int rmax = std::min(k + 2, iu);
      for (int i = 0; i <= rmax; ++i) {
        const cplx t1 = h(i, k), t2 = h(i, k + 1);
        h(i, k) = c * t1 + std::conj(s) * t2;
        h(i, k + 1) = -s * t1 + c * t2;
      }
      if (wantz) {
        for (int i = 0; i < n; ++i) {
          const cplx t1 = zz(i, k), t2 = zz(i, k + 1);
          zz(i, k) = c * t1 + std::conj(s) * t2;
          zz(i, k + 1) = -s * t1 + c * t2;
        }
      }
      if (k > il) h(k + 1, k - 1) = 0.0;
      if (k < iu - 1) {
        x = h(k + 1, k);
        y = h(k + 2, k);
      }
    }
  }
  for (int i = 0; i < n; ++i) values[static_cast<std::size_t>(i)] = h(i, i);
  if (scale != 0) ok = values_times_two_to(values, scale) && ok;
  if (!wantz) return ok;
  // eigenvectors of the triangular factor, column by column
  vectors->assign(static_cast<std::size_t>(n) * n, cplx(0.0));
  std::vector<cplx> yv(static_cast<std::size_t>(n));
  const double smallnum = std::numeric_limits<double>::min() / eps;
  for (int k = n - 1; k >= 0; --k) {
    std::fill(yv.begin(), yv.end(), cplx(0.0));
    yv[static_cast<std::size_t>(k)] = 1.0;
    const cplx lam = h(k, k);
    for (int i = k - 1; i >= 0; --i) {
      cplx acc = 0.0;
      for (int j = i + 1; j <= k; ++j) acc += h(i, j) * yv[static_cast<std::size_t>(j)];
      cplx den = h(i, i) - lam;
      const double floor_ = std::max(eps * hnorm, smallnum);
      if (std::abs(den) < floor_) den = floor_;
      yv[static_cast<std::size_t>(i)] = -acc / den;
      // guard against overflow in long back-substitutions
      const double big = std::abs(yv[static_cast<std::size_t>(i)]);
      if (big > 1e150) {
        for (int j = i; j <= k; ++j) yv[static_cast<std::size_t>(j)] /= big;
      }
    }
    double nrm = 0.0;
    cplx* xk = vectors->data() + static_cast<std::size_t>(k) * n;
    for (int i = 0; i < n; ++i) {
      cplx acc = 0.0;
      for (int j = 0; j <= k; ++j) acc += zz(i, j) * yv[static_cast<std::size_t>(j)];
      xk[i] = acc;
      nrm += std::norm(acc);
    }
    nrm = std::sqrt(nrm);
    if (nrm > 0.0)
      for (int i = 0; i < n; ++i) xk[i] /= nrm;
  }
  return ok;
}

// Eigenvalues only of a REAL upper-Hessenberg matrix (column-major n x n, overwritten): Francis' implicit
// double-shift QR with deflation, rotations confined to the active block (no Schur vectors) -- the classical
// EISPACK hqr scheme, a quarter of the arithmetic of the complex single-shift iteration above.  Complex pairs
// come out with the positive imaginary part first (the order LAPACK and Eigen's EigenSolver use).  This is what
// the Arnoldi front-end needs after every step of a real operator (arnoldi.hpp:811).
inline bool hessenberg_real_values(std::vector<double>& H, int n, std::vector<cplx>& values) {
  values.assign(static_cast<std::size_t>(n), cplx(0.0));
  if (n == 0) return true;
  auto a = [&](int r, int c) -> double& { return H[static_cast<std::size_t>(r) + static_cast<std::size_t>(c) * n]; };
  auto sign = [](double x, double y) { return y >= 0.0 ? std::abs(x) : -std::abs(x); };
  EntryRange seen;  // false on an entry that is not finite, a power of two outside the safe range: as in hessenberg()
  for (int c = 0; c < n; ++c)
    for (int r = 0; r <= std::min(c + 1, n - 1); ++r) seen.see(a(r, c));
  const int scale = seen.exponent();
  if (scale != 0)
    for (int c = 0; c < n; ++c)
      for (int r = 0; r <= std::min(c + 1, n - 1); ++r) a(r, c) = times_two_to(a(r, c), -scale);
  double anorm = 0.0;
  for (int i = 0; i < n; ++i)
    for (int j = std::max(i - 1, 0); j < n; ++j) anorm += std::abs(a(i, j));
  int nn = n - 1;
  double t = 0.0, p = 0.0, q = 0.0, r = 0.0, s = 0.0, w, x, y, z;
  bool ok = seen.finite;
  while (nn >= 0) {
    int its = 0, l;
    do {
      for (l = nn; l >= 1; --l) {  // a negligible sub-diagonal entry splits the problem
        s = std::abs(a(l - 1, l - 1)) + std::abs(a(l, l));
        if (s == 0.0) s = anorm;
        if (std::abs(a(l, l - 1)) + s == s) {
          a(l, l - 1) = 0.0;
          break;
        }
      }
      x = a(nn, nn);
      if (l == nn) {  // one real root
        values[static_cast<std::size_t>(nn)] = cplx(x + t, 0.0);
        --nn;
      } else {
        y = a(nn - 1, nn - 1);
        w = a(nn, nn - 1) * a(nn - 1, nn);
        if (l == nn - 1) {  // a 2 x 2 block: two real roots or a complex pair
          p = 0.5 * (y - x);
          q = p * p + w;
          z = std::sqrt(std::abs(q));
          x += t;
          if (q >= 0.0) {
            z = p + sign(z, p);
            double r0 = x + z, r1 = r0;
            if (z != 0.0) r1 = x - w / z;
            values[static_cast<std::size_t>(nn - 1)] = cplx(r0, 0.0);
            values[static_cast<std::size_t>(nn)] = cplx(r1, 0.0);
          } else {
            values[static_cast<std::size_t>(nn - 1)] = cplx(x + p, z);
            values[static_cast<std::size_t>(nn)] = cplx(x + p, -z);
          }
          nn -= 2;
        } else {  // no root yet: one more double-shift sweep
          if (its == 90) {
            ok = false;  // give up on this block: report its diagonal
            for (int i = l; i <= nn; ++i) values[static_cast<std::size_t>(i)] = cplx(a(i, i) + t, 0.0);
            nn = l - 1;
            break;
          }
          if (its == 10 || its == 20 || its == 40) {  // exceptional shift
            t += x;
            for (int i = 0; i <= nn; ++i) a(i, i) -= x;
            s = std::abs(a(nn, nn - 1)) + std::abs(a(nn - 1, nn - 2));
            y = x = 0.75 * s;
            w = -0.4375 * s * s;
          }
          ++its;
          int m;
          for (m = nn - 2; m >= l; --m) {  // two consecutive small sub-diagonal entries let the sweep start at m
            z = a(m, m);
            r = x - z;
            s = y - z;
            p = (r * s - w) / a(m + 1, m) + a(m, m + 1);
            q = a(m + 1, m + 1) - z - r - s;
            r = a(m + 2, m + 1);
            s = std::abs(p) + std::abs(q) + std::abs(r);
            p /= s;
            q /= s;
            r /= s;
            if (m == l) break;
            const double u = std::abs(a(m, m - 1)) * (std::abs(q) + std::abs(r));
            const double v = std::abs(p) * (std::abs(a(m - 1, m - 1)) + std::abs(z) + std::abs(a(m + 1, m + 1)));
            if (u + v == v) break;
          }
          for (int i = m + 2; i <= nn; ++i) {
            a(i, i - 2) = 0.0;
            if (i != m + 2) a(i, i - 3) = 0.0;
          }
          for (int k = m; k <= nn - 1; ++k) {  // Householder reflections of order 3 chase the bulge down
            if (k != m) {
              p = a(k, k - 1);
              q = a(k + 1, k - 1);
              r = 0.0;
              if (k != nn - 1) r = a(k + 2, k - 1);
              if ((x = std::abs(p) + std::abs(q) + std::abs(r)) != 0.0) {
                p /= x;
                q /= x;
                r /= x;
              }
            }
            if ((s = sign(std::sqrt(p * p + q * q + r * r), p)) != 0.0) {
              if (k == m) {
                if (l != m) a(k, k - 1) = -a(k, k - 1);
              } else {
                a(k, k - 1) = -s * x;
              }
              p += s;
              x = p / s;
              y = q / s;
              z = r / s;
              q /= p;
              r /= p;
              for (int j = k; j <= nn; ++j) {  // rows k, k+1, k+2
                p = a(k, j) + q * a(k + 1, j);
                if (k != nn - 1) {
                  p += r * a(k + 2, j);
                  a(k + 2, j) -= p * z;
                }
                a(k + 1, j) -= p * y;
                a(k, j) -= p * x;
              }
              const int mmin = nn < k + 3 ? nn : k + 3;
              for (int i = l; i <= mmin; ++i) {  // columns k, k+1, k+2
                p = x * a(i, k) + y * a(i, k + 1);
                if (k != nn - 1) {
                  p += z * a(i, k + 2);
                  a(i, k + 2) -= p * r;
                }
                a(i, k + 1) -= p * q;
                a(i, k) -= p;
              }
            }
          }
        }
      }
    } while (l < nn - 1);
  }
  if (scale != 0) ok = values_times_two_to(values, scale) && ok;
  return ok;
}

// Eigen-decomposition of a GENERAL complex matrix A (column-major n x n, overwritten): Householder reduction to
// Hessenberg form U^H A U, the QR iteration above, vectors = U X (unit-norm columns).  A matrix that is already
// Hessenberg passes through untouched (no reflector is applied), so this is hessenberg() for the first cycle of a
// Krylov-Schur run and the general case for the later ones, whose leading block is full.
inline bool general(std::vector<cplx>& A, int n, std::vector<cplx>& values, std::vector<cplx>* vectors) {
  auto a = [&](int r, int c) -> cplx& { return A[static_cast<std::size_t>(r) + static_cast<std::size_t>(c) * n]; };
  EntryRange seen;  // false on an entry that is not finite, a power of two outside the safe range: hessenberg() then finds
  for (std::size_t i = 0; i < static_cast<std::size_t>(n) * n; ++i) seen.see(A[i]);  // its input inside the range
  const int scale = seen.exponent();
  if (scale != 0)
    for (std::size_t i = 0; i < static_cast<std::size_t>(n) * n; ++i) A[i] = times_two_to(A[i], -scale);
  std::vector<cplx> U;
  bool reflected = false;
  std::vector<cplx> v(static_cast<std::size_t>(n));
  for (int k = 0; k + 2 < n; ++k) {
    double tail2 = 0.0;
    for (int i = k + 2; i < n; ++i) tail2 += std::norm(a(i, k));
    if (tail2 == 0.0) continue;  // column already Hessenberg
    const double nrm = std::sqrt(tail2 + std::norm(a(k + 1, k)));
    const double a0 = std::abs(a(k + 1, k));
    const cplx alpha = a0 > 0.0 ? -(a(k + 1, k) / a0) * nrm : cplx(-nrm);
    double vn = 0.0;
    for (int i = k + 1; i < n; ++i) {
      v[static_cast<std::size_t>(i)] = a(i, k) - (i == k + 1 ? alpha : cplx(0.0));
      vn += std::norm(v[static_cast<std::size_t>(i)]);
    }
    vn = std::sqrt(vn);
    for (int i = k + 1; i < n; ++i) v[static_cast<std::size_t>(i)] /= vn;
    // A <- P A P with P = I - 2 v v^H (Hermitian, unitary)
    for (int c = k; c < n; ++c) {
      cplx d = 0.0;
      for (int i = k + 1; i < n; ++i) d += std::conj(v[static_cast<std::size_t>(i)]) * a(i, c);
      d *= 2.0;
      for (int i = k + 1; i < n; ++i) a(i, c) -= d * v[static_cast<std::size_t>(i)];
    }
    for (int r = 0; r < n; ++r) {
      cplx d = 0.0;
      for (int j = k + 1; j < n; ++j) d += a(r, j) * v[static_cast<std::size_t>(j)];
      d *= 2.0;
      for (int j = k + 1; j < n; ++j) a(r, j) -= d * std::conj(v[static_cast<std::size_t>(j)]);
    }
    a(k + 1, k) = alpha;
    for (int i = k + 2; i < n; ++i) a(i, k) = 0.0;
    if (vectors) {  // U <- U P
      if (!reflected) {
        U.assign(static_cast<std::size_t>(n) * n, cplx(0.0));
        for (int i = 0; i < n; ++i) U[static_cast<std::size_t>(i) * n + i] = 1.0;
      }
      for (int r = 0; r < n; ++r) {
        cplx d = 0.0;
        for (int j = k + 1; j < n; ++j) d += U[static_cast<std::size_t>(r) + static_cast<std::size_t>(j) * n] * v[static_cast<std::size_t>(j)];
        d *= 2.0;
        for (int j = k + 1; j < n; ++j) U[static_cast<std::size_t>(r) + static_cast<std::size_t>(j) * n] -= d * std::conj(v[static_cast<std::size_t>(j)]);
      }
    }
    reflected = true;
  }
  std::vector<cplx> X;
  bool ok = hessenberg(A, n, values, vectors ? &X : nullptr) && seen.finite;
  if (scale != 0) ok = values_times_two_to(values, scale) && ok;
  if (!vectors) return ok;
  if (!reflected) {
    vectors->swap(X);
    return ok;
  }
  vectors->assign(static_cast<std::size_t>(n) * n, cplx(0.0));
  for (int c = 0; c < n; ++c)
    for (int j = 0; j < n; ++j) {
      const cplx x = X[static_cast<std::size_t>(j) + static_cast<std::size_t>(c) * n];
      for (int r = 0; r < n; ++r) (*vectors)[static_cast<std::size_t>(r) + static_cast<std::size_t>(c) * n] += U[static_cast<std::size_t>(r) + static_cast<std::size_t>(j) * n] * x;
    }
  return ok;
}

// Ritz pairs of a projected matrix H (column-major m x m, leading dimension ldh, T = double or cplx; Hessenberg or with a full
// leading block), ordered by |theta| descending with the stable sort of arnoldi.hpp:813-822.  S: column-major m x m.
template <class T>
bool ritz_pairs_by_magnitude(const T* H, int ldh, int m, std::vector<cplx>& theta, std::vector<cplx>& S) {
  std::vector<cplx> A(static_cast<std::size_t>(m) * m), vals, vecs;
  for (int c = 0; c < m; ++c)
    for (int r = 0; r < m; ++r) A[static_cast<std::size_t>(r) + static_cast<std::size_t>(c) * m] = H[static_cast<std::size_t>(r) + static_cast<std::size_t>(c) * ldh];
  const bool ok = general(A, m, vals, &vecs);
  std::vector<std::size_t> order(static_cast<std::size_t>(m));
  for (std::size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&vals](std::size_t x, std::size_t y) { return std::abs(vals[x]) > std::abs(vals[y]); });
  theta.resize(static_cast<std::size_t>(m));
  S.resize(static_cast<std::size_t>(m) * m);
  for (int i = 0; i < m; ++i) {
    theta[static_cast<std::size_t>(i)] = vals[order[static_cast<std::size_t>(i)]];
    std::copy(vecs.begin() + static_cast<std::ptrdiff_t>(order[static_cast<std::size_t>(i)] * m),
              vecs.begin() + static_cast<std::ptrdiff_t>((order[static_cast<std::size_t>(i)] + 1) * m), S.begin() + static_cast<std::ptrdiff_t>(i) * m);
  }
  return ok;
}

namespace ks_detail {
inline double conj_of(double x) { return x; }
inline cplx conj_of(const cplx& x) { return std::conj(x); }
template <class T>
struct Candidate {
  std::vector<T> v, fallback;  // fallback (may be empty): tried when v adds no new direction
};
// T = double: s is multiplied by the phase that makes Re s and Im s orthogonal with |Re s| >= |Im s| (any phase spans the same
// plane; this one is the best conditioned for the Gram-Schmidt that follows).  A conjugate pair adds both as directions of their
// own; a real Ritz value adds Re s and keeps Im s (rounding noise, or the missing direction if the value was half of an
// unrecognised pair) as the fallback.
inline void push_candidates(const cplx* s, int m, bool pair, std::vector<Candidate<double>>& out) {
  double aa = 0.0, bb = 0.0, ab = 0.0;
  for (int i = 0; i < m; ++i) aa += s[i].real() * s[i].real(), bb += s[i].imag() * s[i].imag(), ab += s[i].real() * s[i].imag();
  const double phi = 0.5 * std::atan2(-2.0 * ab, aa - bb);  // Re(e^{i phi} s) . Im(e^{i phi} s) = 0, |Re| maximal
  const cplx ph = std::polar(1.0, phi);
  std::vector<double> re(static_cast<std::size_t>(m)), im(static_cast<std::size_t>(m));
  for (int i = 0; i < m; ++i) re[static_cast<std::size_t>(i)] = (s[i] * ph).real(), im[static_cast<std::size_t>(i)] = (s[i] * ph).imag();
  if (pair) {
    out.push_back({re, {}});
    out.push_back({im, {}});
  } else {
    out.push_back({re, im});
  }
}
inline void push_candidates(const cplx* s, int m, bool, std::vector<Candidate<cplx>>& out) { out.push_back({std::vector<cplx>(s, s + m), {}}); }
}  // namespace ks_detail

// Restart basis of a Krylov-Schur cycle (Stewart 2001) from the sorted Ritz pairs of H (ritz_pairs_by_magnitude): an
// orthonormal Q (m x keep) spanning the invariant subspace of the first `keep` Ritz values, B_top = Q^H H Q formed
// explicitly (it is not assumed triangular) and the coupling row residue * Q[m-1, :] below it: B is (keep+1) x keep.
// T = double: Q must be real, so a complex-conjugate pair is never split -- `keep` grows by one if the cut falls
// between the two (shrinks by one if that would reach m) -- and a pair contributes Re s and Im s, a real Ritz value
// its (real) vector.  Orthonormalisation: modified Gram-Schmidt applied twice; a direction that vanishes against the ones
// before it (the second member of an unrecognised pair) is replaced by its imaginary part or dropped.  Returns the final keep
// (0 only for m = 2 holding one conjugate pair: nothing real can be kept).
template <class T>
int krylov_schur_basis(const T* H, int ldh, int m, int keep, double residue, const std::vector<cplx>& theta,
                       const std::vector<cplx>& S, std::vector<T>& Q, std::vector<T>& B) {
  constexpr bool real = std::is_same<T, double>::value;
  keep = std::max(1, std::min(keep, m - 1));
  double tmax = 0.0;
  for (int i = 0; i < m; ++i) tmax = std::max(tmax, std::abs(theta[static_cast<std::size_t>(i)]));
  auto paired = [&](int i) { return real && std::abs(theta[static_cast<std::size_t>(i)].imag()) > 1e-10 * tmax; };
  std::vector<int> partner(static_cast<std::size_t>(m), -1);
  std::vector<char> taken(static_cast<std::size_t>(m), 0);
  for (int i = 0; i < keep; ++i) taken[static_cast<std::size_t>(i)] = 1;
  int count = keep;
  for (int i = 0; i < m; ++i) {
    if (!paired(i)) continue;
    const cplx want = std::conj(theta[static_cast<std::size_t>(i)]);
    int best = -1;
    for (int j = 0; j < m; ++j)
      if (j != i && paired(j) && (best < 0 || std::abs(theta[static_cast<std::size_t>(j)] - want) < std::abs(theta[static_cast<std::size_t>(best)] - want))) best = j;
    partner[static_cast<std::size_t>(i)] = best;
  }
  for (int i = 0; i < keep; ++i) {
    const int j = partner[static_cast<std::size_t>(i)];
    if (j < 0 || taken[static_cast<std::size_t>(j)] || !taken[static_cast<std::size_t>(i)]) continue;
    if (count + 1 <= m - 1)
      taken[static_cast<std::size_t>(j)] = 1, ++count;
    else
      taken[static_cast<std::size_t>(i)] = 0, --count;
  }
  std::vector<ks_detail::Candidate<T>> cand;
  for (int i = 0; i < m; ++i) {
    if (!taken[static_cast<std::size_t>(i)]) continue;
    const int j = partner[static_cast<std::size_t>(i)];
    if (j >= 0 && j < i && taken[static_cast<std::size_t>(j)]) continue;  // Re s and Im s of the pair are there already
    ks_detail::push_candidates(S.data() + static_cast<std::size_t>(i) * m, m, j >= 0, cand);
  }
  Q.clear();
  int nq = 0;
  auto orthonormalise = [&](std::vector<T> v) {
    double n0 = 0.0;
    for (const T& x : v) n0 += std::norm(x);
    for (int pass = 0; pass < 2; ++pass)
      for (int c = 0; c < nq; ++c) {
        const T* q = Q.data() + static_cast<std::size_t>(c) * m;
        T d = T(0.0);
        for (int r = 0; r < m; ++r) d += ks_detail::conj_of(q[r]) * v[static_cast<std::size_t>(r)];
        for (int r = 0; r < m; ++r) v[static_cast<std::size_t>(r)] -= d * q[r];
      }
    double n1 = 0.0;
    for (const T& x : v) n1 += std::norm(x);
    if (!(n1 > 1e-16 * n0) || n1 == 0.0) return false;  // |v| fell by 1e-8: no new direction
    const double inv = 1.0 / std::sqrt(n1);
    for (const T& x : v) Q.push_back(x * inv);
    ++nq;
    return true;
  };
  for (const auto& c : cand) {
    if (nq == m - 1) break;
    if (!orthonormalise(c.v) && !c.fallback.empty()) orthonormalise(c.fallback);
  }
  keep = nq;
  B.assign(static_cast<std::size_t>(keep + 1) * keep, T(0.0));
  std::vector<T> HQ(static_cast<std::size_t>(m));
  for (int c = 0; c < keep; ++c) {
    const T* qc = Q.data() + static_cast<std::size_t>(c) * m;
    for (int r = 0; r < m; ++r) {
      T acc = T(0.0);
      for (int j = 0; j < m; ++j) acc += H[static_cast<std::size_t>(r) + static_cast<std::size_t>(j) * ldh] * qc[j];
      HQ[static_cast<std::size_t>(r)] = acc;
    }
    for (int r = 0; r < keep; ++r) {
      const T* qr = Q.data() + static_cast<std::size_t>(r) * m;
      T acc = T(0.0);
      for (int j = 0; j < m; ++j) acc += ks_detail::conj_of(qr[j]) * HQ[static_cast<std::size_t>(j)];
      B[static_cast<std::size_t>(r) + static_cast<std::size_t>(c) * (keep + 1)] = acc;
    }
    B[static_cast<std::size_t>(keep) + static_cast<std::size_t>(c) * (keep + 1)] = residue * qc[m - 1];
  }
  return keep;
}

}  // namespace small_eigen
}  // namespace EigenEx
}  // namespace cmpt
