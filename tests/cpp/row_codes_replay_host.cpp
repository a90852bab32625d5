// Host replay of the row-code encoding (cmpt-eigenex_amd/csrc/row_codes.hpp) and of k_spmv_rows' row loop, built with
// AddressSanitizer + UBSan and -ffp-contract=off by tests/test_row_codes_host.py.
//
// Per matrix (files passed by the test: the seeded structures of tests/structures.py, and corner cases generated here):
//   * detection accepts exactly the shards that fit (<= 16 offsets, <= 255 bitwise-distinct values, stored orders without a
//     cycle, no column twice in a row) and the slot order is a linear extension of every row's stored order;
//   * decoding every record gives back the row's (column, value) sequence exactly, bit for bit (also -0.0 and NaN payloads);
//     records behind the last row (whole 256-row tiles) are all absent;
//   * the kernel's row loop (every slot, absent ones gathering x[0] and dropped by a select) equals the stored-order row loop
//     of oracle/krylov_ref.c bit for bit, and every gather stays inside the operator input.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <random>
#include <vector>

#include "row_codes.hpp"

using namespace eigenex;

static int g_fail = 0;
#define REQUIRE(cond, ...)                  \
  do {                                      \
    if (!(cond)) {                          \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);             \
      std::printf("\n");                    \
      ++g_fail;                             \
      return false;                         \
    }                                       \
  } while (0)

static uint64_t bits(double v) { return row_code_bits(v); }

// rows [0, n) in local numbering (columns in [0, ncols)); expect: whether detection must accept
static bool check(const char* name, int64_t n, int64_t ncols, const std::vector<int32_t>& rp, const std::vector<int32_t>& col,
                  const std::vector<double>& val, int expect, int nthreads) {
  RowCodeTables T;
  const bool ok = row_codes_detect(n, rp.data(), col.data(), val.data(), nthreads, T);
  if (expect >= 0) REQUIRE(ok == (expect == 1), "%s: detection %d, expected %d", name, (int)ok, expect);
  if (!ok) {
    std::printf("%s: plain (as expected)\n", name);
    return true;
  }
  REQUIRE(T.nslots <= kRowCodeMaxSlots && (int)T.pal.size() <= kRowCodeMaxValues, "%s: tables too large", name);
  for (size_t i = 1; i < T.pal_bits.size(); ++i) REQUIRE(T.pal_bits[i - 1] < T.pal_bits[i], "%s: palette not ascending", name);
  const int rb = T.record_bytes();
  const int64_t nrec = (n + kSpmvRows - 1) / kSpmvRows * kSpmvRows;
  std::vector<uint8_t> rec((size_t)(nrec * rb));
  REQUIRE(row_codes_encode(n, nrec, rp.data(), col.data(), val.data(), T, nthreads, rec.data()), "%s: encoding failed", name);
  std::vector<double> x((size_t)ncols);
  std::mt19937_64 eng(7);
  for (auto& v : x) v = std::ldexp((double)(eng() >> 11), -53) * 2.0 - 1.0;
  const double scale = 0.8125;
  double pal[kRowCodeMaxValues] = {};  // the kernel's LDS copy (entries behind the palette: read for absent slots, dropped)
  for (size_t i = 0; i < T.pal.size(); ++i) pal[i] = T.pal[i];
  for (int64_t r = 0; r < nrec; ++r) {
    uint64_t w[2] = {0, 0};
    memcpy(w, &rec[(size_t)(r * rb)], (size_t)rb);
    if (r >= n) {
      for (int s = 0; s < rb; ++s) REQUIRE(row_code_byte(w, s) == kRowCodeAbsent, "%s: padded row %" PRId64 " not absent", name, r);
      continue;
    }
    // decode: the row's entries in stored order
    int64_t p = rp[(size_t)r];
    for (int s = 0; s < rb; ++s) {
      const unsigned c = row_code_byte(w, s);
      if (c == kRowCodeAbsent) continue;
      REQUIRE(s < T.nslots && c < T.pal.size(), "%s: row %" PRId64 " slot %d code %u out of the tables", name, r, s, c);
      REQUIRE(p < rp[(size_t)r + 1], "%s: row %" PRId64 " decodes to more entries than it stores", name, r);
      REQUIRE(r + T.off[s] == col[(size_t)p], "%s: row %" PRId64 " entry %" PRId64 ": column", name, r, p);
      REQUIRE(T.pal_bits[c] == bits(val[(size_t)p]), "%s: row %" PRId64 " entry %" PRId64 ": value bits", name, r, p);
      ++p;
    }
    REQUIRE(p == rp[(size_t)r + 1], "%s: row %" PRId64 " decodes to fewer entries than it stores", name, r);
    // the kernel's loop against the row loop
    double xs[kRowCodeMaxSlots], sum = 0.0, ref = 0.0;
    for (int s = 0; s < rb; ++s) {
      const int64_t idx = row_code_byte(w, s) != kRowCodeAbsent ? r + T.off[s] : 0;
      REQUIRE(idx >= 0 && idx < ncols, "%s: row %" PRId64 " gathers outside the input", name, r);
      xs[s] = x[(size_t)idx];
    }
    for (int s = 0; s < rb; ++s) {
      const unsigned c = row_code_byte(w, s);
      const bool here = c != kRowCodeAbsent;
      const double prod = pal[here ? c : 0] * (xs[s] * scale);
      const double t = sum + prod;
      sum = here ? t : sum;
    }
    for (int64_t q = rp[(size_t)r]; q < rp[(size_t)r + 1]; ++q) ref = ref + val[(size_t)q] * (x[(size_t)col[(size_t)q]] * scale);
    REQUIRE(bits(sum) == bits(ref) || (std::isnan(sum) && std::isnan(ref)), "%s: row %" PRId64 ": %.17g vs %.17g", name, r, sum, ref);
  }
  std::printf("%s: %d slots, %zu values, %d-byte records, %" PRId64 " rows ok\n", name, T.nslots, T.pal.size(), rb, n);
  return true;
}

struct Csr {
  int64_t n = 0, ncols = 0;
  std::vector<int32_t> rp{0}, col;
  std::vector<double> val;
  void add(int64_t c, double v) { col.push_back((int32_t)c), val.push_back(v); }
  void end_row() { rp.push_back((int32_t)col.size()), ++n; }
};

// a shard of the 7-point Laplacian on n^3 split into P row shards, in the library's local numbering (halo columns at
// npad + slot, below the shard first): the offsets of a loopback shard
static Csr laplacian_shard(int64_t n, int P, int g) {
  const int64_t N = n * n * n, n2 = n * n;
  const int64_t rb = N * g / P, re = N * (g + 1) / P, nloc = re - rb, npad = (nloc + 63) / 64 * 64;
  std::vector<int64_t> halo;
  for (int64_t r = rb; r < re; ++r)
    for (int64_t c : {r - n2, r + n2})
      if (c >= 0 && c < N && (c < rb || c >= re)) halo.push_back(c);
  std::sort(halo.begin(), halo.end());
  halo.erase(std::unique(halo.begin(), halo.end()), halo.end());
  Csr a;
  a.ncols = npad + (int64_t)halo.size();
  for (int64_t r = rb; r < re; ++r) {
    const int64_t x = r % n, y = (r / n) % n, z = r / n2;
    auto emit = [&](int64_t c, double v) {
      a.add(c >= rb && c < re ? c - rb : npad + (std::lower_bound(halo.begin(), halo.end(), c) - halo.begin()), v);
    };
    if (z > 0) emit(r - n2, -1.0);
    if (y > 0) emit(r - n, -1.0);
    if (x > 0) emit(r - 1, -1.0);
    emit(r, 6.0);
    if (x < n - 1) emit(r + 1, -1.0);
    if (y < n - 1) emit(r + n, -1.0);
    if (z < n - 1) emit(r + n2, -1.0);
    a.end_row();
  }
  return a;
}

static bool corner_cases() {
  bool ok = true;
  char name[96];
  for (int P : {1, 2, 3, 8})
    for (int g = 0; g < P; ++g) {
      const Csr a = laplacian_shard(9, P, g);
      std::snprintf(name, sizeof name, "laplacian 9^3 shard %d of %d", g, P);
      ok &= check(name, a.n, a.ncols, a.rp, a.col, a.val, 1, 3);
    }
  {  // empty matrix rows, explicit zeros, +-0.0, NaN payloads: all distinct values
    Csr a;
    a.ncols = 700;
    double nan1, nan2;
    const uint64_t b1 = 0x7ff8000000000001ull, b2 = 0xfff8000000000abcull;
    memcpy(&nan1, &b1, 8), memcpy(&nan2, &b2, 8);
    const double pal[] = {0.0, -0.0, 1.0, nan1, nan2};
    for (int64_t r = 0; r < 700; ++r) {
      if (r % 7 != 3)
        for (int d : {-1, 0, 2})
          if (r + d >= 0 && r + d < 700) a.add(r + d, pal[(r * 3 + d + 1) % 5]);
      a.end_row();
    }
    ok &= check("zeros, signed zeros, NaN payloads, empty rows", a.n, a.ncols, a.rp, a.col, a.val, 1, 2);
  }
  for (int nv : {255, 256}) {  // palette limit
    Csr a;
    a.ncols = 1000;
    for (int64_t r = 0; r < 1000; ++r) {
      a.add(r, 1.0 + (double)(r % nv));
      a.end_row();
    }
    std::snprintf(name, sizeof name, "%d values", nv);
    ok &= check(name, a.n, a.ncols, a.rp, a.col, a.val, nv <= 255 ? 1 : 0, 4);
  }
  for (int no : {8, 9, 16, 17}) {  // slot limit and the two record sizes
    Csr a;
    a.ncols = 600 + 2 * no;
    for (int64_t r = 0; r < 600; ++r) {
      for (int d = 0; d < no; ++d)
        if ((r + d) % 5 != 0) a.add(r + 2 * d, -0.5);
      a.end_row();
    }
    std::snprintf(name, sizeof name, "%d offsets", no);
    ok &= check(name, a.n, a.ncols, a.rp, a.col, a.val, no <= 16 ? 1 : 0, 2);
  }
  {  // two rows store two offsets in opposite orders: no linear extension
    Csr a;
    a.ncols = 10;
    a.add(1, 1.0), a.add(0, 1.0), a.end_row();  // row 0: offsets 1, 0
    a.add(1, 1.0), a.add(2, 1.0), a.end_row();  // row 1: offsets 0, 1
    ok &= check("conflicting stored orders", a.n, a.ncols, a.rp, a.col, a.val, 0, 1);
  }
  {  // descending columns in every row: a consistent order that is not ascending
    Csr a;
    a.ncols = 300;
    for (int64_t r = 0; r < 300; ++r) {
      for (int d : {3, 1, 0, -2})
        if (r + d >= 0 && r + d < 300) a.add(r + d, (double)d);
      a.end_row();
    }
    ok &= check("descending stored order", a.n, a.ncols, a.rp, a.col, a.val, 1, 3);
  }
  {  // a column twice in a row
    Csr a;
    a.ncols = 4;
    a.add(0, 1.0), a.add(0, 2.0), a.end_row();
    ok &= check("column twice in a row", a.n, a.ncols, a.rp, a.col, a.val, 0, 1);
  }
  {  // only empty rows
    Csr a;
    a.ncols = 300;
    for (int r = 0; r < 300; ++r) a.end_row();
    ok &= check("empty rows only", a.n, a.ncols, a.rp, a.col, a.val, 1, 2);
  }
  return ok;
}

int main(int argc, char** argv) {
  bool ok = corner_cases();
  for (int i = 1; i < argc; ++i) {  // header [n, nnz, ...], rowptr (int32), col (int32), val: one shard, global = local columns
    FILE* f = std::fopen(argv[i], "rb");
    if (!f) return 2;
    int64_t hdr[7];
    if (std::fread(hdr, 8, 7, f) != 7) return 2;
    const int64_t n = hdr[0], nnz = hdr[1];
    std::vector<int32_t> rp((size_t)n + 1), col((size_t)nnz);
    std::vector<double> val((size_t)nnz);
    if (std::fread(rp.data(), 4, rp.size(), f) != rp.size() || std::fread(col.data(), 4, col.size(), f) != col.size() ||
        std::fread(val.data(), 8, val.size(), f) != val.size())
      return 2;
    std::fclose(f);
    ok &= check(argv[i], n, n, rp, col, val, -1, 4);
  }
  if (!ok || g_fail) return 1;
  std::printf("ROW CODES REPLAY OK\n");
  return 0;
}
