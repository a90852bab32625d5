// Row codes: a real fp64 CSR shard whose rows use few column offsets (col - row) and few distinct values -- any
// constant-coefficient stencil, graph Laplacian, adjacency matrix, uniform-hopping lattice Hamiltonian -- stored as one
// record per row instead of rowptr / col / val (kernels.hip: k_spmv_rows).
//
//   slot table: at most kRowCodeMaxSlots offsets d_s; the entry of row r in slot s reads local column r + d_s (halo columns are
//               ordinary offsets: local numbering puts the halo at npad + i, a constant distance from the rows that read it)
//   palette:    at most kRowCodeMaxValues bitwise-distinct values (0.0 and -0.0 are two values, NaN payloads are kept),
//               in ascending order of their bit patterns
//   record:     8 bytes (<= 8 slots) or 16 bytes (<= 16 slots) per row, byte s = palette index of the row's entry in slot s,
//               or kRowCodeAbsent; rows behind the shard's last (padding up to whole 256-row tiles) are all kRowCodeAbsent
//
// The slot order is a linear extension of every row's stored entry order, so that a row walked slot by slot adds its
// products in stored order -- bit-identical to the plain kernel and the oracle's row loop.  Among the linear extensions the
// one taken is canonical (Kahn's algorithm, the smallest ready offset first): it depends only on the set of offsets and
// the order constraints the rows impose, so a shard encoded on the host and the same shard written by the device generator
// (library.hip: eigenex_csr_laplacian3d) end in the same tables and the same records.
//
// Shared by the kernel (decode), the library (detection on the host, encoding on the host and on the device) and the host
// replay tests/cpp/row_codes_replay_host.cpp.
#pragma once
#include <stdint.h>
#include <string.h>

#include "spmv_index.hpp"

#include <algorithm>
#include <thread>
#include <vector>

namespace eigenex {

constexpr int kRowCodeMaxSlots = 16;
constexpr int kRowCodeMaxValues = 255;
constexpr unsigned kRowCodeAbsent = 0xFF;

struct RowCodeSlots {  // kernel argument: local column of slot s of row r = r + off[s]
  int64_t off[kRowCodeMaxSlots];
};

EIGENEX_HD uint64_t row_code_bits(double v) {
  uint64_t u;
  memcpy(&u, &v, sizeof u);
  return u;
}
EIGENEX_HD int row_code_record_bytes(int nslots) { return nslots <= 8 ? 8 : 16; }
// byte s of a record held as 64-bit words (little-endian: byte s of the record in memory)
EIGENEX_HD unsigned row_code_byte(const uint64_t* rec, int s) { return (unsigned)(rec[s >> 3] >> (8 * (s & 7))) & 0xFFu; }

// The record of local row r from its stored entries cols[0 .. len), vals[0 .. len): bytes[0 .. rec_bytes).  False if an
// entry's offset is not in the table, its value not in the palette, or the row's entries do not take strictly ascending slots
// (out of slot order, or two entries on one column).
EIGENEX_HD bool row_code_encode(int64_t r, const int32_t* cols, const double* vals, int64_t len, const int64_t* off, int nslots,
                                const uint64_t* pal_bits, int npal, uint8_t* bytes, int rec_bytes) {
  for (int s = 0; s < rec_bytes; ++s) bytes[s] = (uint8_t)kRowCodeAbsent;
  int prev = -1;
  for (int64_t p = 0; p < len; ++p) {
    const int64_t d = (int64_t)cols[p] - r;
    int s = prev + 1;  // slots ascend along the row: search only behind the previous one
    while (s < nslots && off[s] != d) ++s;
    if (s >= nslots) return false;
    const uint64_t b = row_code_bits(vals[p]);
    int v = 0;
    while (v < npal && pal_bits[v] != b) ++v;
    if (v >= npal) return false;
    bytes[s] = (uint8_t)v;
    prev = s;
  }
  return true;
}

// ---- host only ----

struct RowCodeTables {
  int nslots = 0;
  int64_t off[kRowCodeMaxSlots] = {};
  std::vector<double> pal;                 // ascending bit pattern
  std::vector<uint64_t> pal_bits;
  int record_bytes() const { return row_code_record_bytes(nslots); }
};

// What the rows of one range impose: the offsets they use, the values they hold, and for every two consecutive entries of a
// row the constraint "offset a comes before offset b".  Limits exceeded (more offsets or values than a record can name):
// ok = false.
struct RowCodeScan {
  bool ok = true;
  std::vector<int64_t> off;         // discovery order, <= kRowCodeMaxSlots
  std::vector<uint64_t> vals;       // discovery order, <= kRowCodeMaxValues
  uint32_t succ[kRowCodeMaxSlots] = {};  // bit j of succ[i]: off[i] directly precedes off[j] in some row

  int offset_index(int64_t d) {
    for (int i = 0; i < (int)off.size(); ++i)
      if (off[(size_t)i] == d) return i;
    if ((int)off.size() >= kRowCodeMaxSlots) return -1;
    off.push_back(d);
    return (int)off.size() - 1;
  }
  bool add_value(uint64_t b, int& last) {  // last: index of the value found last (rows repeat values), -1: none
    if (last >= 0 && vals[(size_t)last] == b) return true;
    for (size_t v = 0; v < vals.size(); ++v)
      if (vals[v] == b) return last = (int)v, true;
    if ((int)vals.size() >= kRowCodeMaxValues) return false;
    vals.push_back(b);
    last = (int)vals.size() - 1;
    return true;
  }
  void row(int64_t r, const int32_t* cols, const double* vals, int64_t len, int& last) {  // one row, entries in stored order
    int prev = -1;
    for (int64_t p = 0; p < len && ok; ++p) {
      const int i = offset_index((int64_t)cols[p] - r);
      if (i < 0 || !add_value(row_code_bits(vals[p]), last)) {
        ok = false;
        return;
      }
      if (prev >= 0) succ[prev] |= 1u << i;
      prev = i;
    }
  }
  template <class OFF>
  void rows(int64_t r0, int64_t r1, const OFF* lrp, const int32_t* lcol, const double* val) {
    int last = -1;
    for (int64_t r = r0; r < r1 && ok; ++r) row(r, lcol + lrp[r], val + lrp[r], (int64_t)(lrp[r + 1] - lrp[r]), last);
  }
  void merge(const RowCodeScan& o) {
    if (!o.ok) ok = false;
    if (!ok) return;
    int map[kRowCodeMaxSlots];
    for (size_t i = 0; i < o.off.size(); ++i)
      if ((map[i] = offset_index(o.off[i])) < 0) return void(ok = false);
    for (size_t i = 0; i < o.off.size(); ++i)
      for (size_t j = 0; j < o.off.size(); ++j)
        if (o.succ[i] >> j & 1u) succ[map[i]] |= 1u << map[j];
    int last = -1;
    for (uint64_t v : o.vals)
      if (!add_value(v, last)) return void(ok = false);
  }
};

// The canonical tables of a scan: slots by Kahn's algorithm, smallest ready offset first (a cycle -- two rows that store
// two offsets in opposite orders, or one row that stores a column twice -- has no linear extension: false); palette
// ascending by bit pattern.
inline bool row_code_tables(const RowCodeScan& sc, RowCodeTables& T) {
  if (!sc.ok) return false;
  const int m = (int)sc.off.size();
  int indeg[kRowCodeMaxSlots] = {};
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j)
      if (sc.succ[i] >> j & 1u) ++indeg[j];
  bool done[kRowCodeMaxSlots] = {};
  T.nslots = 0;
  for (int k = 0; k < m; ++k) {
    int pick = -1;
    for (int i = 0; i < m; ++i)
      if (!done[i] && indeg[i] == 0 && (pick < 0 || sc.off[(size_t)i] < sc.off[(size_t)pick])) pick = i;
    if (pick < 0) return false;  // cycle
    done[pick] = true;
    T.off[T.nslots++] = sc.off[(size_t)pick];
    for (int j = 0; j < m; ++j)
      if (sc.succ[pick] >> j & 1u) --indeg[j];
  }
  T.pal_bits = sc.vals;
  std::sort(T.pal_bits.begin(), T.pal_bits.end());
  T.pal.resize(T.pal_bits.size());
  for (size_t i = 0; i < T.pal.size(); ++i) memcpy(&T.pal[i], &T.pal_bits[i], sizeof(double));
  return true;
}

// Row ranges of `nthreads` host threads (the caller's pool size); f(th, r0, r1) must not throw.
template <class F>
void row_code_parallel(int64_t nrows, int nthreads, F f) {
  std::vector<std::thread> pool;
  for (int th = 1; th < nthreads; ++th) {
    try {
      pool.emplace_back(f, th, nrows * th / nthreads, nrows * (th + 1) / nthreads);
    } catch (...) {  // no more threads to be had: do the range here
      f(th, nrows * th / nthreads, nrows * (th + 1) / nthreads);
    }
  }
  f(0, (int64_t)0, nrows / nthreads);
  for (auto& t : pool) t.join();
}

// Detection on the host: the tables of rows [0, nloc) of a shard in local numbering, or false if the shard does not fit them.
template <class OFF>
bool row_codes_detect(int64_t nloc, const OFF* lrp, const int32_t* lcol, const double* val, int nthreads, RowCodeTables& T) {
  nthreads = (int)std::max<int64_t>(1, std::min<int64_t>(nthreads, nloc / 65536 + 1));
  std::vector<RowCodeScan> part((size_t)nthreads);
  row_code_parallel(nloc, nthreads, [&](int th, int64_t r0, int64_t r1) {
    try {
      part[(size_t)th].rows(r0, r1, lrp, lcol, val);
    } catch (...) {
      part[(size_t)th].ok = false;
    }
  });
  for (int th = 1; th < nthreads; ++th) part[0].merge(part[(size_t)th]);
  return row_code_tables(part[0], T);
}

// Encoding on the host: nrec_rows records of T.record_bytes() bytes (rows >= nloc: all absent).  False if a row does not fit
// (it cannot after a successful detection on the same rows).
template <class OFF>
bool row_codes_encode(int64_t nloc, int64_t nrec_rows, const OFF* lrp, const int32_t* lcol, const double* val, const RowCodeTables& T,
                      int nthreads, uint8_t* rec) {
  const int rb = T.record_bytes();
  nthreads = (int)std::max<int64_t>(1, std::min<int64_t>(nthreads, nrec_rows / 65536 + 1));
  std::vector<char> ok((size_t)nthreads, 1);
  row_code_parallel(nrec_rows, nthreads, [&](int th, int64_t r0, int64_t r1) {
    for (int64_t r = r0; r < r1; ++r) {
      uint8_t* b = rec + (size_t)r * rb;
      if (r >= nloc) {
        memset(b, (int)kRowCodeAbsent, (size_t)rb);
      } else if (!row_code_encode(r, lcol + lrp[r], val + lrp[r], (int64_t)(lrp[r + 1] - lrp[r]), T.off, T.nslots, T.pal_bits.data(),
                                  (int)T.pal_bits.size(), b, rb)) {
        ok[(size_t)th] = 0;
        return;
      }
    }
  });
  for (char o : ok)
    if (!o) return false;
  return true;
}

}  // namespace eigenex
