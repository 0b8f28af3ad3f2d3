// Per-instance statistics of id maps on the device: for every id of a (B, H, W) map its pixel count,
// its bounding box and the coordinate sums its centroid is made of, in ONE read of the map.  The semantics are written
// out in include/wm2f.h; tests/instance_stats_reference.py restates them with one np.nonzero per id.
//
//   init_stats     : stats (B, N, 8) <- the empty instance [0, W, H, -1, -1, 0, 0, 0].
//   instance_stats : grid (strips, B), 256 threads.  A workgroup owns a strip of whole rows, so y is uniform per row and
//                    sum_y is y x count.  A wave takes 256 consecutive pixels of one row per load (4 per lane: one 16-byte
//                    load of a 4-byte map, one dword of a uint8 map), kIsUnroll loads in flight.
//                    - A wave whose pixels all carry one value (background, or the inside of an instance: nearly every
//                      wave) needs no per-lane work: count, box and sum_x of a run of consecutive x are closed forms,
//                      and lane 0 alone accumulates them (nothing at all for a value that is no listed id).
//                    - Otherwise a lane folds its own runs of equal values and accumulates once per run.
//                    Accumulators live in LDS while N <= kIsLdsMaxIds (32 B each: count and the strip-relative sum_y
//                    share one 64-bit add, sum_x is the other; the four box bounds are read first and touched by an
//                    atomic only when they move, which after a wave's first rows they hardly do).  A workgroup then
//                    flushes the ids it saw, and only those, with 64-bit integer atomics.  Above the cap the same code
//                    accumulates straight into the result.
// Everything is integer -- a float map's ids are decoded from the bits -- so the result does not depend on the order of
// accumulation.
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kIsThreads = 256;
constexpr int kIsWaves = kIsThreads / 64;
constexpr int kIsPix = 4;               // pixels per lane per load (load_map4)
constexpr int kIsSeg = 64 * kIsPix;     // pixels of one row per wave-instruction
constexpr int kIsUnroll = 4;
constexpr int kIsLdsMaxIds = 1024;      // 32 B of accumulators + 4 B of id list each: 36 KiB, four workgroups per CU
constexpr int kIsMaxStripRows = 256;    // keeps a strip's relative sum_y (< 2^29 at W = 16384) in the packed word's half

struct IsAcc {
  unsigned long long pk;  // count | strip-relative sum_y << 32
  unsigned long long sx;
  int xmin, xmax, ymin, ymax;
};
static_assert(sizeof(IsAcc) == 32, "IsAcc layout");

// result row of a raw map value, -1 for none.  ids == nullptr: the value itself when in [0, N); else its position in
// the image's ascending list (n of them, in LDS)
template <int DT>
__device__ __forceinline__ int row_of(uint32_t raw, const int32_t* ids, int n, int N) {
  int v;
  if (!map_int<DT>(raw, v)) return -1;
  if (ids == nullptr) return (v >= 0 && v < N) ? v : -1;
  return list_row(v, ids, n);
}

// a run of len pixels x0 .. x1 of row y with result row r.  The bounds only ever move one way, so a stale read can at
// worst ask for an atomic that changes nothing.
template <bool kLds>
__device__ __forceinline__ void accumulate(IsAcc* acc, long long* st, int r, int len, int x0, int x1, int y, int y0) {
  const unsigned long long sx = (unsigned long long)len * (unsigned)x0 + (unsigned long long)(len * (len - 1) / 2);
  if (kLds) {
    IsAcc* a = acc + r;
    atomicAdd(&a->pk, (unsigned long long)len | ((unsigned long long)((y - y0) * len) << 32));
    atomicAdd(&a->sx, sx);
    if (x0 < a->xmin) atomicMin(&a->xmin, x0);
    if (x1 > a->xmax) atomicMax(&a->xmax, x1);
    if (y < a->ymin) atomicMin(&a->ymin, y);
    if (y > a->ymax) atomicMax(&a->ymax, y);
  } else {
    long long* s = st + (int64_t)r * 8;
    atomicAdd(reinterpret_cast<unsigned long long*>(s), (unsigned long long)len);
    if (x0 < s[1]) atomicMin(s + 1, (long long)x0);
    if (y < s[2]) atomicMin(s + 2, (long long)y);
    if (x1 > s[3]) atomicMax(s + 3, (long long)x1);
    if (y > s[4]) atomicMax(s + 4, (long long)y);
    atomicAdd(reinterpret_cast<unsigned long long*>(s + 5), sx);
    atomicAdd(reinterpret_cast<unsigned long long*>(s + 6), (unsigned long long)y * (unsigned)len);
  }
}

__global__ __launch_bounds__(kIsThreads) void init_stats_kernel(long long* __restrict__ stats, int total, int H, int W) {
  const int i = blockIdx.x * kIsThreads + threadIdx.x;
  if (i >= total) return;
  long long* s = stats + (int64_t)i * 8;
  s[0] = 0;
  s[1] = W;
  s[2] = H;
  s[3] = -1;
  s[4] = -1;
  s[5] = 0;
  s[6] = 0;
  s[7] = 0;
}

// kVec: W % 4 == 0 and an aligned map, so a lane's four pixels are one load and valid or invalid together
template <int DT, bool kVec, bool kLds>
__global__ __launch_bounds__(kIsThreads) void instance_stats_kernel(const void* __restrict__ map,
                                                                    const int32_t* __restrict__ ids,
                                                                    const int32_t* __restrict__ n_ids,
                                                                    long long* __restrict__ stats, int H, int W, int N,
                                                                    int strip_rows) {
  using E = typename MapElem<DT>::type;
  extern __shared__ __align__(8) unsigned char ismem[];
  IsAcc* acc = reinterpret_cast<IsAcc*>(ismem);
  int32_t* sids = reinterpret_cast<int32_t*>(ismem + (kLds ? (size_t)N * sizeof(IsAcc) : 0));
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int y0 = blockIdx.x * strip_rows;
  const int y1 = y0 + strip_rows < H ? y0 + strip_rows : H;
  int n = 0;
  if (ids != nullptr) {
    n = n_ids[b];
    n = n < 0 ? 0 : (n > N ? N : n);
    for (int j = tid; j < n; j += kIsThreads) sids[j] = ids[(int64_t)b * N + j];
  }
  if (kLds)
    for (int j = tid; j < N; j += kIsThreads) acc[j] = IsAcc{0ull, 0ull, W, -1, H, -1};
  __syncthreads();
  const int32_t* idl = ids != nullptr ? sids : nullptr;
  long long* st = stats + (int64_t)b * N * 8;
  const E* base = reinterpret_cast<const E*>(map) + (int64_t)b * H * W;
  const int segs = (W + kIsSeg - 1) / kIsSeg;

  // this wave's items: (row, 256-pixel segment) pairs of the strip, every kIsWaves-th one
  int y = y0, seg = wave;
  while (seg >= segs) {
    seg -= segs;
    ++y;
  }
  while (y < y1) {  // wave-uniform
    int iy[kIsUnroll], ix[kIsUnroll];
    uint32_t v[kIsUnroll][kIsPix];
#pragma unroll
    for (int u = 0; u < kIsUnroll; ++u) {
      iy[u] = y;
      ix[u] = seg * kIsSeg;
      seg += kIsWaves;
      while (seg >= segs) {
        seg -= segs;
        ++y;
      }
    }
#pragma unroll
    for (int u = 0; u < kIsUnroll; ++u) {
      const int x = ix[u] + lane * kIsPix;
#pragma unroll
      for (int j = 0; j < kIsPix; ++j) v[u][j] = 0u;
      if (iy[u] < y1) {
        const E* p = base + (int64_t)iy[u] * W + x;
        if (kVec) {
          if (x < W) load_map4<DT>(p, v[u]);
        } else {
#pragma unroll
          for (int j = 0; j < kIsPix; ++j)
            if (x + j < W) v[u][j] = (uint32_t)p[j];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kIsUnroll; ++u) {
      if (iy[u] >= y1) break;  // wave-uniform; later items of the batch are past the strip too
      const int yy = iy[u], xs = ix[u], x = xs + lane * kIsPix;
      const int nv = W - x < 0 ? 0 : (W - x < kIsPix ? W - x : kIsPix);  // this lane's pixels inside the row
      const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)v[u][0]);  // lane 0's first pixel is inside
      bool same = true;
#pragma unroll
      for (int j = 0; j < kIsPix; ++j) same = same && (j >= nv || v[u][j] == first);
      if (__ballot(same) == ~0ull) {
        const int r = row_of<DT>(first, idl, n, N);
        if (r >= 0 && lane == 0) {
          const int len = W - xs < kIsSeg ? W - xs : kIsSeg;
          accumulate<kLds>(acc, st, r, len, xs, xs + len - 1, yy, y0);
        }
        continue;
      }
      int j = 0;
      while (j < nv) {
        const uint32_t raw = v[u][j];
        int k = j + 1;
        while (k < nv && v[u][k] == raw) ++k;
        const int r = row_of<DT>(raw, idl, n, N);
        if (r >= 0) accumulate<kLds>(acc, st, r, k - j, x + j, x + k - 1, yy, y0);
        j = k;
      }
    }
  }
  if (kLds) {
    __syncthreads();
    for (int j = tid; j < N; j += kIsThreads) {
      const IsAcc a = acc[j];
      const unsigned long long area = a.pk & 0xffffffffull;
      if (area == 0ull) continue;  // flush only what this strip saw
      long long* s = st + (int64_t)j * 8;
      atomicAdd(reinterpret_cast<unsigned long long*>(s), area);
      atomicMin(s + 1, (long long)a.xmin);
      atomicMin(s + 2, (long long)a.ymin);
      atomicMax(s + 3, (long long)a.xmax);
      atomicMax(s + 4, (long long)a.ymax);
      atomicAdd(reinterpret_cast<unsigned long long*>(s + 5), a.sx);
      atomicAdd(reinterpret_cast<unsigned long long*>(s + 6), (a.pk >> 32) + (unsigned long long)y0 * area);
    }
  }
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_labelmap_instance_stats(const void* map, int dtype, const int32_t* ids, const int32_t* n_ids,
                                            int64_t* stats, int B, int H, int W, int N, void* stream) {
  const char* who = "wm2f_labelmap_instance_stats";
  WM2F_REQUIRE(map && stats, "%s: null pointer", who);
  WM2F_REQUIRE((ids == nullptr) == (n_ids == nullptr), "%s: ids and n_ids go together", who);
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N > 0, "%s: bad size", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  if (H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch || N > kMapMaxIds) {
    set_error("%s: sides <= %d, B <= %d, N <= %d (got %d x %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch, kMapMaxIds, H, W,
              B, N);
    return WM2F_EUNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  long long* out = reinterpret_cast<long long*>(stats);
  hipLaunchKernelGGL(init_stats_kernel, dim3(ceil_div(B * N, kIsThreads)), dim3(kIsThreads), 0, s, out, B * N, H, W);
  // about 1024 strips in all, at least 4096 pixels and at most kIsMaxStripRows rows each
  int rows = ceil_div(H, ceil_div(1024, B));
  const int min_rows = ceil_div(4096, W);
  rows = rows < min_rows ? min_rows : rows;
  rows = rows > kIsMaxStripRows ? kIsMaxStripRows : rows;
  rows = rows > H ? H : rows;
  const dim3 grid(ceil_div(H, rows), B);
  const bool lds = N <= kIsLdsMaxIds;
  const bool vec = map_vec4_ok(map, dtype, W);
  const size_t shm = (lds ? (size_t)N * sizeof(IsAcc) : 0) + (ids ? (size_t)N * sizeof(int32_t) : 0);
  for_map_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kIsThreads), shm, s, map, ids, n_ids, out, H, W, N, rows);
    };
    if (vec && lds) launch(instance_stats_kernel<DT, true, true>);
    else if (vec) launch(instance_stats_kernel<DT, true, false>);
    else if (lds) launch(instance_stats_kernel<DT, false, true>);
    else launch(instance_stats_kernel<DT, false, false>);
  });
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
