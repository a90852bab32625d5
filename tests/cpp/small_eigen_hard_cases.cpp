// small_eigen::hermitian, general and hessenberg (small_eigen.hpp) on a matrix read from a file, in a stand-alone C++11 program:
// the two routines that have no Python wrapper, and hessenberg for the bytes general must reproduce on a matrix that is already
// Hessenberg.  The file holds
//   mode n
//   re im          n * n pairs, column-major (strtod's spellings: nan and inf included)
// with mode one of hermitian, hermitian_values (vectors = NULL), general, general_values, hessenberg.  It prints
//   ok 0|1
//   values  ...    n numbers (hermitian) or n pairs re im, %.17g
//   vectors ...    n * n pairs re im, column-major; empty for the _values modes
// and returns 0 whatever the routine returned (2: the file could not be read).  tests/test_small_eigen_hard_cases_host.py
// writes the matrices and holds the output to its bounds; it builds this file a second time with AddressSanitizer + UBSan.
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cmpt/eigen_ex/small_eigen.hpp"

using cplx = std::complex<double>;
namespace se = cmpt::EigenEx::small_eigen;

static void print_complex(const char* name, const std::vector<cplx>& v) {
  std::printf("%s", name);
  for (const cplx& e : v) std::printf(" %.17g %.17g", e.real(), e.imag());
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char mode[32];
  int n = -1;
  if (std::fscanf(f, "%31s %d", mode, &n) != 2 || n < 0 || n > 4096) return 2;
  std::vector<cplx> A(static_cast<std::size_t>(n) * n);
  for (cplx& e : A) {
    double re, im;
    if (std::fscanf(f, "%lf %lf", &re, &im) != 2) return 2;
    e = cplx(re, im);
  }
  std::fclose(f);
  const bool values_only = std::strstr(mode, "_values") != nullptr;
  std::vector<cplx> V;
  bool ok;
  if (std::strncmp(mode, "hermitian", 9) == 0) {
    std::vector<double> values;
    ok = se::hermitian(A, n, values, values_only ? nullptr : &V);
    std::printf("ok %d\nvalues", ok ? 1 : 0);
    for (double v : values) std::printf(" %.17g", v);
    std::printf("\n");
  } else {
    std::vector<cplx> values;
    if (std::strncmp(mode, "general", 7) == 0)
      ok = se::general(A, n, values, values_only ? nullptr : &V);
    else if (std::strcmp(mode, "hessenberg") == 0)
      ok = se::hessenberg(A, n, values, &V);
    else
      return 2;
    std::printf("ok %d\n", ok ? 1 : 0);
    print_complex("values", values);
  }
  print_complex("vectors", V);
  return 0;
}
