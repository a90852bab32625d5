// What do k_sweep's two stores cost, and is it the instructions or the HBM writes?  A pass with the sweep's stream shape (512 persistent
// workgroups of 256 threads over 2048-row tiles, four 512-row slices per lane; two vectors loaded plainly at the tile start, ncols
// columns of 1 GiB in groups of four non-temporal 16-byte loads with one FMA use per value, two vectors written at the tile end, one
// of them in place), with the stores done in different ways.  All variants run in one process on the same allocations, alternately.
//   hipcc --offload-arch=gfx950 -O3 scripts/microbench/sweep_stores.hip -o scripts/microbench/sweep_stores
//   scripts/microbench/sweep_stores [rounds=12]          (runs ncols = 16, 48 and 96; needs 100 GiB of device memory: 96 + 3 vectors of 1 GiB)
//
//   A   no stores: the values feed a branch that is never taken
//   B   direct non-temporal stores at the tile end, as k_sweep issues them
//   C   the same instructions into 32 KB of scratch per workgroup, which stays in L2; Cp: plain stores there
//   D   results parked in LDS at the tile end and stored from the next tile, directly behind its first column group's loads
//   E   parked as in D, released at the first boundary of a chip-wide clock slot that passes (slots of 10.24 us times 1, 2, 4, 8, 16)
//   E2  two parked tiles per workgroup (64 KB of LDS, a queue, oldest first): a boundary releases both, a tile that finds the queue
//       full releases the oldest at its end (slots of 10.24 us times 2, 4, 8, 16)
//   Ef  E with the clock read behind every column's loads instead of every fourth column's;  E2f  both together
//   Fu  only the column, Fw only the in-place vector, stored directly
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

constexpr int kBlock = 256, kTileRows = 2048, kGrid = 512;
enum Mode { kNone, kDirect, kScratch, kParkNext, kParkSlot, kOnlyU, kOnlyW, kScratchPlain, kParkSlot2, kParkSlotF, kParkSlot2F };
constexpr int kParkBytes = 8 * kBlock * (int)sizeof(double2);  // 32 KB: both results of one tile

typedef double v2d_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 ld2(const double* p) { return *reinterpret_cast<const double2*>(p); }
__device__ __forceinline__ double2 nt_ld2(const double* p) {
  const v2d_t v = __builtin_nontemporal_load(reinterpret_cast<const v2d_t*>(p));
  return make_double2(v.x, v.y);
}
__device__ __forceinline__ void nt_st2(double* p, double2 v) {
  v2d_t t;
  t.x = v.x, t.y = v.y;
  __builtin_nontemporal_store(t, reinterpret_cast<v2d_t*>(p));
}
__device__ __forceinline__ void load_col(double2 (&x)[4], const double* p, int64_t base) {
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = nt_ld2(p + base + i * (2 * kBlock));
}
__device__ __forceinline__ void use_col(double2 (&u)[4], double c, const double2 (&x)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u[i].x = fma(-c, x[i].x, u[i].x);
    u[i].y = fma(-c, x[i].y, u[i].y);
  }
}
// the parked tile of this lane: its own eight 16-byte values, so no barrier stands between parking and release
__device__ __forceinline__ void release(const double2* park, double* ucol, double* w, int64_t pbase) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    nt_st2(ucol + pbase + i * (2 * kBlock), park[i * kBlock + threadIdx.x]);
    nt_st2(w + pbase + i * (2 * kBlock), park[(4 + i) * kBlock + threadIdx.x]);
  }
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void k_stream(const double* V, int64_t ldv, int ncols, const double* v, double* w, double* ucol,
                                                   double* scratch, int64_t ntiles, int slot_shift, double* never) {
  constexpr bool SLOT = MODE == kParkSlot || MODE == kParkSlot2 || MODE == kParkSlotF || MODE == kParkSlot2F;
  constexpr bool PARK = SLOT || MODE == kParkNext;
  constexpr int DEPTH = (MODE == kParkSlot2 || MODE == kParkSlot2F) ? 2 : 1;
  constexpr bool FINE = MODE == kParkSlotF || MODE == kParkSlot2F;
  extern __shared__ __align__(16) double2 park[];  // PARK: DEPTH tiles of kParkBytes
  const double scale = 0.5, a = 0.25, c = 1e-3, f = 0.125;
  // the queue, wave-uniform: the oldest tile lies at place `head`, the newer one (DEPTH 2) at the other place; base < 0 = none
  int64_t obase = -1, nbase = -1;
  uint64_t oslot = 0, nslot = 0;
  int head = 0;
  auto release_oldest = [&] {
    release(park + head * (8 * kBlock), ucol, w, obase + 2 * threadIdx.x);
    obase = nbase, oslot = nslot, nbase = -1;
    if (DEPTH == 2) head ^= 1;
  };
  auto release_all = [&] {
    if (obase >= 0) release_oldest();
    if (DEPTH == 2 && obase >= 0) release_oldest();
  };
  auto at_boundary = [&] {  // the slot of the oldest decides for all that is parked
    if (obase >= 0 && (wall_clock64() >> slot_shift) != oslot) release_all();
  };
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * kTileRows + 2 * threadIdx.x;
    double2 u[4], s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = base + i * (2 * kBlock);
      const double2 t = ld2(w + row);
      u[i] = make_double2(t.x * scale, t.y * scale);
      s[i] = ld2(v + row);
      s[i].x = fma(-a, u[i].x, s[i].x);
      s[i].y = fma(-a, u[i].y, s[i].y);
    }
    for (int ci = 0; ci + 4 <= ncols; ci += 4) {
      double2 x0[4], x1[4], x2[4], x3[4];
      load_col(x0, V + (int64_t)(ci + 0) * ldv, base);
      if (FINE) at_boundary();
      load_col(x1, V + (int64_t)(ci + 1) * ldv, base);
      if (FINE) at_boundary();
      load_col(x2, V + (int64_t)(ci + 2) * ldv, base);
      if (FINE) at_boundary();
      load_col(x3, V + (int64_t)(ci + 3) * ldv, base);
      if (MODE == kParkNext && ci == 0) release_all();
      if (SLOT) at_boundary();
      use_col(u, c, x0);
      use_col(u, c, x1);
      use_col(u, c, x2);
      use_col(u, c, x3);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s[i].x = fma(-f, u[i].x, s[i].x);
      s[i].y = fma(-f, u[i].y, s[i].y);
    }
    if (MODE == kNone) {
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) t += (u[i].x + u[i].y) + (s[i].x + s[i].y);
      if (t == 1.2345e300) never[threadIdx.x] = t;
    } else if (PARK) {
      // never waits: with the queue full the oldest goes out before its place is taken
      if (DEPTH == 2 ? nbase >= 0 : obase >= 0) release_oldest();
      double2* place = park + (obase < 0 ? head : head ^ 1) * (8 * kBlock);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        place[i * kBlock + threadIdx.x] = u[i];
        place[(4 + i) * kBlock + threadIdx.x] = s[i];
      }
      const uint64_t now = SLOT ? wall_clock64() >> slot_shift : 0;
      if (obase < 0)
        obase = tile * kTileRows, oslot = now;
      else
        nbase = tile * kTileRows, nslot = now;
    } else {
      double* du = (MODE == kScratch || MODE == kScratchPlain) ? scratch + (int64_t)blockIdx.x * (2 * kTileRows) + 2 * threadIdx.x : ucol + base;
      double* dw = (MODE == kScratch || MODE == kScratchPlain) ? du + kTileRows : w + base;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (MODE == kScratchPlain) {
          *reinterpret_cast<double2*>(du + i * (2 * kBlock)) = u[i];
          *reinterpret_cast<double2*>(dw + i * (2 * kBlock)) = s[i];
          continue;
        }
        if (MODE != kOnlyW) nt_st2(du + i * (2 * kBlock), u[i]);
        if (MODE != kOnlyU) nt_st2(dw + i * (2 * kBlock), s[i]);
      }
      if (MODE == kOnlyU || MODE == kOnlyW) {  // the vector that is not stored stays alive, with its loads
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) t += MODE == kOnlyU ? s[i].x + s[i].y : u[i].x + u[i].y;
        if (t == 1.2345e300) never[threadIdx.x] = t;
      }
    }
  }
  if (PARK) release_all();
}

__global__ void k_fill(double* p, size_t n, double amp) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    p[i] = amp * (double)((i * 2654435761u >> 7) % 1021) / 1021.0;
}

struct Variant {
  const char* name;
  int mode, shift;
  std::vector<float> ms;
};

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 12;
  const int maxcols = 96;
  const size_t col_bytes = (size_t)1 << 30;
  const int64_t n = col_bytes / 8, ntiles = n / kTileRows;
  int clock_khz = 0;
  CHK(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, 0));
  printf("wall clock %d kHz\n", clock_khz);
  double *V, *v, *w, *ucol, *scratch, *never;
  CHK(hipMalloc(&V, col_bytes * maxcols));
  CHK(hipMalloc(&v, col_bytes));
  CHK(hipMalloc(&w, col_bytes));
  CHK(hipMalloc(&ucol, col_bytes));
  CHK(hipMalloc(&scratch, (size_t)kGrid * 2 * kTileRows * 8));
  CHK(hipMalloc(&never, kBlock * 8));
  hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, V, (size_t)n * maxcols, 1.0);
  hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, v, (size_t)n, 1.0);
  hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, w, (size_t)n, 1.0);
  CHK(hipMemset(ucol, 0, col_bytes));
  CHK(hipDeviceSynchronize());
  // slots of about 10, 20 and 40 us as powers of two of the clock's ticks
  int sh10 = 0;
  while ((1 << sh10) < clock_khz / 100) ++sh10;
  std::vector<Variant> vs = {{"A  none", kNone, 0, {}},          {"B  direct (k_sweep)", kDirect, 0, {}},
                             {"C  to L2 scratch", kScratch, 0, {}}, {"D  parked, next tile", kParkNext, 0, {}},
                             {"E  parked, slot 1x", kParkSlot, sh10, {}}, {"E  parked, slot 2x", kParkSlot, sh10 + 1, {}},
                             {"E  parked, slot 4x", kParkSlot, sh10 + 2, {}}, {"E  parked, slot 8x", kParkSlot, sh10 + 3, {}},
                             {"E  parked, slot 16x", kParkSlot, sh10 + 4, {}},
                             {"Cp plain stores to L2 scratch", kScratchPlain, 0, {}}, {"Fu column only", kOnlyU, 0, {}},
                             {"Fw in-place only", kOnlyW, 0, {}}};
  for (int m : {(int)kParkSlot2, (int)kParkSlotF, (int)kParkSlot2F})
    for (int x = 1; x <= 4; ++x) {
      static char names[12][40];
      static int used = 0;
      snprintf(names[used], sizeof names[used], "%s parked, slot %dx", m == kParkSlot2 ? "E2 two" : m == kParkSlotF ? "Ef" : "E2f two", 1 << x);
      vs.push_back({names[used++], m, sh10 + x, {}});
    }
  for (const void* fn : {(const void*)&k_stream<kParkSlot2>, (const void*)&k_stream<kParkSlot2F>})  // 64 KB of dynamic LDS is asked for
    CHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kParkBytes));
  printf("slot 1x = %.2f us\n", (double)(1 << sh10) / clock_khz * 1e3);
  hipEvent_t e0, e1;
  CHK(hipEventCreate(&e0));
  CHK(hipEventCreate(&e1));
  for (int ncols : {16, 48, 96}) {
    for (auto& x : vs) x.ms.clear();
    for (int r = -2; r < rounds; ++r)  // two warm-up rounds
      for (auto& x : vs) {
        (void)hipEventRecord(e0);
#define LAUNCH(M)                                                                                                               \
  hipLaunchKernelGGL(k_stream<M>, dim3(kGrid), dim3(kBlock),                                                                    \
                     (M == kParkSlot2 || M == kParkSlot2F) ? 2 * kParkBytes : (M == kParkNext || M == kParkSlot || M == kParkSlotF) ? kParkBytes : 0, \
                     0, V, n, ncols, v, w, ucol, scratch, ntiles, x.shift, never)
        switch (x.mode) {
          case kNone: LAUNCH(kNone); break;
          case kDirect: LAUNCH(kDirect); break;
          case kScratch: LAUNCH(kScratch); break;
          case kParkNext: LAUNCH(kParkNext); break;
          case kParkSlot: LAUNCH(kParkSlot); break;
          case kParkSlot2: LAUNCH(kParkSlot2); break;
          case kParkSlotF: LAUNCH(kParkSlotF); break;
          case kParkSlot2F: LAUNCH(kParkSlot2F); break;
          case kOnlyU: LAUNCH(kOnlyU); break;
          case kScratchPlain: LAUNCH(kScratchPlain); break;
          default: LAUNCH(kOnlyW); break;
        }
#undef LAUNCH
        (void)hipEventRecord(e1);
        CHK(hipEventSynchronize(e1));
        CHK(hipGetLastError());
        float ms;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (r >= 0) x.ms.push_back(ms);
      }
    printf("ncols = %d, %d timings each, read %.1f GB\n", ncols, rounds, (double)(ncols + 2) * col_bytes / 1e9);
    printf("| variant | fastest ms | median ms | slowest ms |\n|---|---|---|---|\n");
    for (auto& x : vs) {
      std::sort(x.ms.begin(), x.ms.end());
      printf("| %s | %.3f | %.3f | %.3f |\n", x.name, x.ms.front(), x.ms[x.ms.size() / 2], x.ms.back());
    }
    fflush(stdout);
  }
  return 0;
}
