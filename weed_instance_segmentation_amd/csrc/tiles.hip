// Merging the instances of overlapping tiles into one id map (the contract is in include/wm2f.h,
// tests/tile_merge_reference.py restates it in numpy).
//
//   tile_pairs   : joint histogram (N+1) x (N+1) of two tiles' ids over the rectangle they share, one grid row per pair,
//                  the tiles read in place.  labelmap_pairs_kernel's fast path (coco_eval.hip): a wave inside one id pair
//                  adds its ballot count once, the (none, none) bin is counted once per workgroup.
//   tile_owned   : pixels of every id inside its tile's own cell.
//   tile_link    : every bin of every pair against the link rule, labelling.h's lock-free union (the root of a set
//                  is its smallest node, whatever the arrival order); then, each its own launch: flatten and mark
//                  the sets that own a pixel, number the surviving roots in ascending order by a scan, write remap.
//   tile_compose : out = remap[owner tile][local id], one workgroup per strip of rows of one cell.
// All integer; no float takes part; every result is independent of the schedule.  Every index read from a device table
// is clamped to the array it addresses before use.
#include "labelling.h"
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kTmThreads = 256;
constexpr int kTmMaxSide = WM2F_TILE_MAX_SIDE;
constexpr int kTmMaxIds = WM2F_TILE_MAX_IDS;
constexpr int kTmMaxTiles = WM2F_TILE_MAX_TILES;
constexpr int kTmMaxPairs = WM2F_TILE_MAX_PAIRS;
constexpr int kTmLdsBins = 16384;       // 64 KiB of LDS bins: N <= 127; larger histograms take global atomics
constexpr int kTmPairPixels = 65536;    // pixels of a rectangle per workgroup (its LDS bins are flushed once)
constexpr int kTmCellPixels = 16384;    // pixels of a cell per workgroup
constexpr int kTmScanThreads = 1024;

// slot of a map value: 0 "no id", id + 1 for an id in [0, n)
template <bool kF32>
__device__ __forceinline__ int tile_slot(uint32_t raw, int n) {
  int v;
  if (!map_int<kF32 ? WM2F_F32 : WM2F_I32>(raw, v)) return 0;
  return (v >= 0 && v < n) ? v + 1 : 0;  // map_id_below's ids, one up
}

__device__ __forceinline__ int clamp_n(int n, int N) { return n < 0 ? 0 : (n > N ? N : n); }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// One add per wave when all its lanes hit the bin of lane 0, one atomic per lane otherwise; bin <= 0 counts nothing.
// Called by all 64 lanes of a wave (inactive pixels pass -1).
__device__ __forceinline__ void wave_count(int32_t* tgt, int bin, int lane) {
  const int first = __shfl(bin, 0, 64);
  const bool same = bin == first;
  const unsigned long long m = __ballot(same);
  if (same) {
    if (lane == 0 && first > 0) atomicAdd(tgt + first, (int)__popcll(m));
  } else if (bin > 0) {
    atomicAdd(tgt + bin, 1);
  }
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// grid (row strips, P), 256 threads.  hist (P, N+1, N+1) cleared by the host side.
template <bool kF32, bool kLds>
__global__ __launch_bounds__(kTmThreads) void tile_pairs_kernel(const uint32_t* __restrict__ tiles,
                                                               const int32_t* __restrict__ n_ids,
                                                               const int32_t* __restrict__ pairs,
                                                               int32_t* __restrict__ hist, int T, int th, int tw, int N) {
  extern __shared__ int32_t bins[];
  const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int32_t* pr = pairs + (int64_t)p * 8;
  const int a = pr[0], b = pr[1], ay = pr[2], ax = pr[3], by = pr[4], bx = pr[5];
  int h = pr[6], w = pr[7];
  if (a < 0 || a >= T || b < 0 || b >= T || ay < 0 || ax < 0 || by < 0 || bx < 0) return;  // uniform in the workgroup
  h = imin(h, th - imax(ay, by));
  w = imin(w, tw - imax(ax, bx));
  if (h <= 0 || w <= 0) return;
  const int rpb = imax(1, kTmPairPixels / w);
  const int r0 = blockIdx.x * rpb;
  if (r0 >= h) return;
  const int rows = imin(h, r0 + rpb) - r0;
  const int NB = N + 1, nb = NB * NB;
  const int na = clamp_n(n_ids[a], N), nbn = clamp_n(n_ids[b], N);
  int32_t* hb = hist + (int64_t)p * nb;
  int32_t* tgt = kLds ? bins : hb;
  if (kLds) {
    for (int j = tid; j < nb; j += kTmThreads) bins[j] = 0;
    __syncthreads();
  }
  const uint32_t* pa = tiles + ((int64_t)a * th + ay + r0) * tw + ax;
  const uint32_t* pb = tiles + ((int64_t)b * th + by + r0) * tw + bx;
  int skipped = 0;
  const bool vec = (w & 3) == 0 && (tw & 3) == 0 && aligned16(pa) && aligned16(pb);
  if (vec) {
    const int wq = w >> 2, total = rows * wq;
    for (int base = 0; base < total; base += kTmThreads) {  // uniform trip count: ballots below
      const int i = base + tid;
      const bool valid = i < total;
      uint4 va = make_uint4(0, 0, 0, 0), vb = va;
      if (valid) {
        const int r = i / wq, q = i - r * wq;
        va = *(const uint4*)(pa + (int64_t)r * tw + 4 * q);
        vb = *(const uint4*)(pb + (int64_t)r * tw + 4 * q);
      }
      const uint32_t ra[4] = {va.x, va.y, va.z, va.w}, rb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        int bin = -1;
        if (valid) {
          bin = tile_slot<kF32>(ra[u], na) * NB + tile_slot<kF32>(rb[u], nbn);
          if (bin == 0) {
            ++skipped;
            bin = -1;
          }
        }
        wave_count(tgt, bin, lane);
      }
    }
  } else {
    const int total = rows * w;
    for (int base = 0; base < total; base += kTmThreads) {
      const int i = base + tid;
      int bin = -1;
      if (i < total) {
        const int r = i / w, x = i - r * w;
        bin = tile_slot<kF32>(pa[(int64_t)r * tw + x], na) * NB + tile_slot<kF32>(pb[(int64_t)r * tw + x], nbn);
        if (bin == 0) {
          ++skipped;
          bin = -1;
        }
      }
      wave_count(tgt, bin, lane);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) skipped += __shfl_xor(skipped, o, 64);
  if (lane == 0 && skipped) atomicAdd(hb, skipped);
  if (kLds) {
    __syncthreads();
    for (int j = tid; j < nb; j += kTmThreads)
      if (bins[j]) atomicAdd(hb + j, bins[j]);
  }
}

// The cell of tile t in the tile's local coordinates, clipped to the tile: geom row (oy, ox, cy0, cy1, cx0, cx1).
struct Cell {
  int oy, ox, y0, y1, x0, x1;  // origin (global); local half-open ranges
};
__device__ __forceinline__ Cell load_cell(const int32_t* __restrict__ geom, int t, int th, int tw) {
  const int32_t* g = geom + (int64_t)t * 6;
  Cell c;
  c.oy = g[0];
  c.ox = g[1];
  // differences of two table words: take them in 64 bits, then clamp
  const int64_t y0 = (int64_t)g[2] - c.oy, y1 = (int64_t)g[3] - c.oy, x0 = (int64_t)g[4] - c.ox, x1 = (int64_t)g[5] - c.ox;
  c.y0 = (int)(y0 < 0 ? 0 : (y0 > th ? th : y0));
  c.y1 = (int)(y1 < 0 ? 0 : (y1 > th ? th : y1));
  c.x0 = (int)(x0 < 0 ? 0 : (x0 > tw ? tw : x0));
  c.x1 = (int)(x1 < 0 ? 0 : (x1 > tw ? tw : x1));
  return c;
}

// grid (row strips, T), 256 threads.  owned (T, N) cleared by the host side.
template <bool kF32>
__global__ __launch_bounds__(kTmThreads) void tile_owned_kernel(const uint32_t* __restrict__ tiles,
                                                               const int32_t* __restrict__ n_ids,
                                                               const int32_t* __restrict__ geom,
                                                               int32_t* __restrict__ owned, int th, int tw, int N) {
  __shared__ int32_t acc[kTmMaxIds + 1];
  const int t = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const Cell c = load_cell(geom, t, th, tw);
  const int h = c.y1 - c.y0, w = c.x1 - c.x0;
  if (h <= 0 || w <= 0) return;
  const int rpb = imax(1, kTmCellPixels / w);
  const int r0 = blockIdx.x * rpb;
  if (r0 >= h) return;
  const int rows = imin(h, r0 + rpb) - r0;
  const int n = clamp_n(n_ids[t], N);
  for (int j = tid; j <= N; j += kTmThreads) acc[j] = 0;
  __syncthreads();
  const uint32_t* pt = tiles + ((int64_t)t * th + c.y0 + r0) * tw + c.x0;
  const bool vec = (w & 3) == 0 && (tw & 3) == 0 && aligned16(pt);
  if (vec) {
    const int wq = w >> 2, total = rows * wq;
    for (int base = 0; base < total; base += kTmThreads) {
      const int i = base + tid;
      const bool valid = i < total;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (valid) {
        const int r = i / wq, q = i - r * wq;
        v = *(const uint4*)(pt + (int64_t)r * tw + 4 * q);
      }
      const uint32_t rv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) wave_count(acc, valid ? tile_slot<kF32>(rv[u], n) : -1, lane);
    }
  } else {
    const int total = rows * w;
    for (int base = 0; base < total; base += kTmThreads) {
      const int i = base + tid;
      int bin = -1;
      if (i < total) {
        const int r = i / w, x = i - r * w;
        bin = tile_slot<kF32>(pt[(int64_t)r * tw + x], n);
      }
      wave_count(acc, bin, lane);
    }
  }
  __syncthreads();
  for (int j = tid; j < n; j += kTmThreads)
    if (acc[j + 1]) atomicAdd(owned + (int64_t)t * N + j, acc[j + 1]);
}

// grid (row strips, T), 256 threads.
template <bool kF32>
__global__ __launch_bounds__(kTmThreads) void tile_compose_kernel(const uint32_t* __restrict__ tiles,
                                                                 const int32_t* __restrict__ n_ids,
                                                                 const int32_t* __restrict__ geom,
                                                                 const int32_t* __restrict__ remap,
                                                                 int32_t* __restrict__ out, int th, int tw, int N, int H,
                                                                 int W) {
  __shared__ int32_t map[kTmMaxIds + 1];  // by slot: map[0] = -1
  const int t = blockIdx.y, tid = threadIdx.x;
  Cell c = load_cell(geom, t, th, tw);
  // the cell inside the output as well: 0 <= oy + y < H, 0 <= ox + x < W
  const int64_t ylo = -(int64_t)c.oy, yhi = (int64_t)H - c.oy, xlo = -(int64_t)c.ox, xhi = (int64_t)W - c.ox;
  if (c.y0 < ylo) c.y0 = (int)(ylo > th ? th : ylo);
  if (c.y1 > yhi) c.y1 = (int)(yhi < 0 ? 0 : yhi);
  if (c.x0 < xlo) c.x0 = (int)(xlo > tw ? tw : xlo);
  if (c.x1 > xhi) c.x1 = (int)(xhi < 0 ? 0 : xhi);
  const int h = c.y1 - c.y0, w = c.x1 - c.x0;
  if (h <= 0 || w <= 0) return;
  const int rpb = imax(1, kTmCellPixels / w);
  const int r0 = blockIdx.x * rpb;
  if (r0 >= h) return;
  const int rows = imin(h, r0 + rpb) - r0;
  const int n = clamp_n(n_ids[t], N);
  for (int j = tid; j <= n; j += kTmThreads) map[j] = j == 0 ? -1 : remap[(int64_t)t * N + j - 1];
  __syncthreads();
  const uint32_t* pt = tiles + ((int64_t)t * th + c.y0 + r0) * tw + c.x0;
  int32_t* po = out + ((int64_t)c.oy + c.y0 + r0) * W + c.ox + c.x0;
  const bool vec = (w & 3) == 0 && (tw & 3) == 0 && (W & 3) == 0 && aligned16(pt) && aligned16(po);
  if (vec) {
    const int wq = w >> 2, total = rows * wq;
    for (int i = tid; i < total; i += kTmThreads) {
      const int r = i / wq, q = i - r * wq;
      const uint4 v = *(const uint4*)(pt + (int64_t)r * tw + 4 * q);
      int4 o;
      o.x = map[tile_slot<kF32>(v.x, n)];
      o.y = map[tile_slot<kF32>(v.y, n)];
      o.z = map[tile_slot<kF32>(v.z, n)];
      o.w = map[tile_slot<kF32>(v.w, n)];
      *(int4*)(po + (int64_t)r * W + 4 * q) = o;
    }
  } else {
    const int total = rows * w;
    for (int i = tid; i < total; i += kTmThreads) {
      const int r = i / w, x = i - r * w;
      po[(int64_t)r * W + x] = map[tile_slot<kF32>(pt[(int64_t)r * tw + x], n)];
    }
  }
}

// ---- linking: labelling.h's union-find over the nodes g = t * N + i, at device scope  -------------------------------
constexpr int kTmScope = __HIP_MEMORY_SCOPE_AGENT;

struct LinkWs {
  int32_t* parent;  // (M) union-find forest
  int32_t* root;    // (M) the flattened root of every node
  int32_t* owns;    // (M) at a root: non-zero when a member of the set owns a pixel
  int32_t* newid;   // (M) at a surviving root: its merged id; -1 elsewhere
};
__host__ __device__ inline LinkWs carve(void* ws, int64_t M) {
  int32_t* b = (int32_t*)ws;
  return LinkWs{b, b + M, b + 2 * M, b + 3 * M};
}

__global__ __launch_bounds__(kTmThreads) void tile_link_init_kernel(LinkWs ws, int M) {
  const int g = blockIdx.x * kTmThreads + threadIdx.x;
  if (g < M) {
    ws.parent[g] = g;
    ws.owns[g] = 0;
  }
}

// grid (P), 256 threads: areas of the pair's ids inside its rectangle (row and column sums), then every inner bin
// against the link rule.
__global__ __launch_bounds__(kTmThreads) void tile_link_kernel(const int32_t* __restrict__ hist,
                                                              const int32_t* __restrict__ pairs,
                                                              const int32_t* __restrict__ labels,
                                                              const int32_t* __restrict__ n_ids, LinkWs ws, int T, int N,
                                                              int num, int den) {
  __shared__ int32_t area_a[kTmMaxIds + 1];
  __shared__ int32_t area_b[kTmMaxIds + 1];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = pairs[(int64_t)p * 8], b = pairs[(int64_t)p * 8 + 1];
  if (a < 0 || a >= T || b < 0 || b >= T || a == b) return;
  const int NB = N + 1;
  const int32_t* hp = hist + (int64_t)p * NB * NB;
  for (int i = wave; i < NB; i += kTmThreads / 64) {
    int s = 0;
    for (int j = lane; j < NB; j += 64) s += hp[i * NB + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) area_a[i] = s;
  }
  for (int j = tid; j < NB; j += kTmThreads) {
    int s = 0;
    for (int i = 0; i < NB; ++i) s += hp[i * NB + j];
    area_b[j] = s;
  }
  __syncthreads();
  const int na = clamp_n(n_ids[a], N), nbn = clamp_n(n_ids[b], N);
  const int32_t* la = labels + (int64_t)a * N;
  const int32_t* lb = labels + (int64_t)b * N;
  for (int idx = tid; idx < na * nbn; idx += kTmThreads) {
    const int i = idx / nbn, j = idx - i * nbn;
    const int inter = hp[(i + 1) * NB + j + 1];
    if (inter <= 0 || la[i] != lb[j]) continue;
    const int smaller = imin(area_a[i + 1], area_b[j + 1]);
    if ((int64_t)inter * den >= (int64_t)num * smaller) unite<kTmScope>(ws.parent, a * N + i, b * N + j);
  }
}

__global__ __launch_bounds__(kTmThreads) void tile_flatten_kernel(const int32_t* __restrict__ n_ids,
                                                                 const int32_t* __restrict__ owned, LinkWs ws, int M,
                                                                 int N) {
  const int g = blockIdx.x * kTmThreads + threadIdx.x;
  if (g >= M) return;
  const int r = find_root<kTmScope>(ws.parent, g);
  ws.root[g] = r;
  const int t = g / N, i = g - t * N;
  if (i < clamp_n(n_ids[t], N) && owned[g] > 0) atomicOr(ws.owns + r, 1);
}

// one workgroup of 1024 threads: surviving roots numbered in ascending node order by a scan of per-thread counts
__global__ __launch_bounds__(kTmScanThreads) void tile_number_kernel(LinkWs ws, int32_t* __restrict__ n_merged, int M) {
  __shared__ int32_t part[kTmScanThreads];
  const int tid = threadIdx.x;
  const int per = ceil_div(M, kTmScanThreads);
  const int g0 = imin(M, tid * per), g1 = imin(M, g0 + per);
  int cnt = 0;
  for (int g = g0; g < g1; ++g) cnt += (ws.root[g] == g && ws.owns[g] != 0);
  part[tid] = cnt;
  __syncthreads();
  for (int o = 1; o < kTmScanThreads; o <<= 1) {  // inclusive scan
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int next = part[tid] - cnt;
  for (int g = g0; g < g1; ++g) ws.newid[g] = (ws.root[g] == g && ws.owns[g] != 0) ? next++ : -1;
  if (tid == kTmScanThreads - 1) n_merged[0] = part[tid];
}

__global__ __launch_bounds__(kTmThreads) void tile_remap_kernel(const int32_t* __restrict__ n_ids, LinkWs ws,
                                                               int32_t* __restrict__ remap, int M, int N) {
  const int g = blockIdx.x * kTmThreads + threadIdx.x;
  if (g >= M) return;
  const int t = g / N, i = g - t * N;
  const int r = ws.root[g];
  remap[g] = (i < clamp_n(n_ids[t], N) && r >= 0 && r < M) ? ws.newid[r] : -1;
}

int check_caps(const char* who, int T, int th, int tw, int N, int P) {
  WM2F_REQUIRE(T > 0 && th > 0 && tw > 0 && N >= 0 && P >= 0, "%s: bad size", who);
  if (T > kTmMaxTiles || th > kTmMaxSide || tw > kTmMaxSide || N > kTmMaxIds || P > kTmMaxPairs) {
    set_error("%s: T = %d, tile %d x %d, N = %d, P = %d: at most %d tiles of side %d, %d ids, %d pairs", who, T, th, tw,
              N, P, kTmMaxTiles, kTmMaxSide, kTmMaxIds, kTmMaxPairs);
    return WM2F_EUNSUPPORTED;
  }
  return WM2F_OK;
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_tile_merge_workspace(int T, int N, int P) {
  if (T <= 0 || N < 0 || P < 0 || T > kTmMaxTiles || N > kTmMaxIds || P > kTmMaxPairs) return -1;
  const int64_t M = (int64_t)T * N;
  return M ? 4 * M * (int64_t)sizeof(int32_t) : 16;
}

extern "C" int wm2f_tile_pair_counts(const void* tiles, int dtype, const int32_t* n_ids, const int32_t* pairs,
                                     int32_t* hist, int T, int th, int tw, int N, int P, void* stream) {
  const char* who = "wm2f_tile_pair_counts";
  const int rc = check_caps(who, T, th, tw, N, P);
  if (rc != WM2F_OK) return rc;
  WM2F_REQUIRE(dtype == WM2F_F32 || dtype == WM2F_I32, "%s: tiles must be fp32 or int32", who);
  if (P == 0) return WM2F_OK;
  WM2F_REQUIRE(tiles && n_ids && pairs && hist, "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  const int nb = (N + 1) * (N + 1);
  if (hipMemsetAsync(hist, 0, (size_t)P * nb * sizeof(int32_t), s) != hipSuccess) {
    set_error("%s: clearing the histograms failed", who);
    return WM2F_ELAUNCH;
  }
  const int rpb = kTmPairPixels / tw > 1 ? kTmPairPixels / tw : 1;  // the widest rectangle: the fewest rows per workgroup
  const dim3 grid(ceil_div(th, rpb), P);
  const bool lds = nb <= kTmLdsBins;
  const size_t shm = lds ? (size_t)nb * sizeof(int32_t) : 0;
  const uint32_t* tp = (const uint32_t*)tiles;
  for_map_dtype_f32_i32(dtype, [&](auto dt) {
    constexpr bool kF32 = decltype(dt)::value == WM2F_F32;
    if (lds)
      hipLaunchKernelGGL((tile_pairs_kernel<kF32, true>), grid, dim3(kTmThreads), shm, s, tp, n_ids, pairs, hist, T, th, tw, N);
    else
      hipLaunchKernelGGL((tile_pairs_kernel<kF32, false>), grid, dim3(kTmThreads), shm, s, tp, n_ids, pairs, hist, T, th, tw, N);
  });
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_tile_owned_counts(const void* tiles, int dtype, const int32_t* n_ids, const int32_t* geom,
                                      int32_t* owned, int T, int th, int tw, int N, void* stream) {
  const char* who = "wm2f_tile_owned_counts";
  const int rc = check_caps(who, T, th, tw, N, 0);
  if (rc != WM2F_OK) return rc;
  WM2F_REQUIRE(dtype == WM2F_F32 || dtype == WM2F_I32, "%s: tiles must be fp32 or int32", who);
  if (N == 0) return WM2F_OK;
  WM2F_REQUIRE(tiles && n_ids && geom && owned, "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(owned, 0, (size_t)T * N * sizeof(int32_t), s) != hipSuccess) {
    set_error("%s: clearing the counts failed", who);
    return WM2F_ELAUNCH;
  }
  const int rpb = kTmCellPixels / tw > 1 ? kTmCellPixels / tw : 1;
  const dim3 grid(ceil_div(th, rpb), T);
  const uint32_t* tp = (const uint32_t*)tiles;
  for_map_dtype_f32_i32(dtype, [&](auto dt) {
    hipLaunchKernelGGL(tile_owned_kernel<decltype(dt)::value == WM2F_F32>, grid, dim3(kTmThreads), 0, s, tp, n_ids, geom,
                       owned, th, tw, N);
  });
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_tile_link(const int32_t* hist, const int32_t* pairs, const int32_t* labels, const int32_t* n_ids,
                              const int32_t* owned, int32_t* remap, int32_t* n_merged, void* workspace, int T, int N,
                              int P, int num, int den, void* stream) {
  const char* who = "wm2f_tile_link";
  const int rc = check_caps(who, T, 1, 1, N, P);
  if (rc != WM2F_OK) return rc;
  WM2F_REQUIRE(num >= 0 && den >= 1, "%s: the threshold num / den needs num >= 0 and den >= 1", who);
  WM2F_REQUIRE(n_merged, "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  const int M = T * N;
  if (M == 0) {
    if (hipMemsetAsync(n_merged, 0, sizeof(int32_t), s) != hipSuccess) {
      set_error("%s: clearing the count failed", who);
      return WM2F_ELAUNCH;
    }
    return WM2F_OK;
  }
  WM2F_REQUIRE(labels && n_ids && owned && remap && workspace && (P == 0 || (hist && pairs)), "%s: null pointer", who);
  const LinkWs ws = carve(workspace, M);
  const dim3 nodes(ceil_div(M, kTmThreads));
  hipLaunchKernelGGL(tile_link_init_kernel, nodes, dim3(kTmThreads), 0, s, ws, M);
  if (P > 0)
    hipLaunchKernelGGL(tile_link_kernel, dim3(P), dim3(kTmThreads), 0, s, hist, pairs, labels, n_ids, ws, T, N, num, den);
  hipLaunchKernelGGL(tile_flatten_kernel, nodes, dim3(kTmThreads), 0, s, n_ids, owned, ws, M, N);
  hipLaunchKernelGGL(tile_number_kernel, dim3(1), dim3(kTmScanThreads), 0, s, ws, n_merged, M);
  hipLaunchKernelGGL(tile_remap_kernel, nodes, dim3(kTmThreads), 0, s, n_ids, ws, remap, M, N);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_tile_compose(const void* tiles, int dtype, const int32_t* n_ids, const int32_t* geom,
                                 const int32_t* remap, int32_t* out, int T, int th, int tw, int N, int H, int W,
                                 void* stream) {
  const char* who = "wm2f_tile_compose";
  const int rc = check_caps(who, T, th, tw, N, 0);
  if (rc != WM2F_OK) return rc;
  WM2F_REQUIRE(H > 0 && W > 0, "%s: bad size", who);
  if (H > kTmMaxSide || W > kTmMaxSide) {
    set_error("%s: output %d x %d, sides at most %d", who, H, W, kTmMaxSide);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(dtype == WM2F_F32 || dtype == WM2F_I32, "%s: tiles must be fp32 or int32", who);
  WM2F_REQUIRE(tiles && n_ids && geom && out && (N == 0 || remap), "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  const int rpb = kTmCellPixels / tw > 1 ? kTmCellPixels / tw : 1;
  const dim3 grid(ceil_div(th, rpb), T);
  const uint32_t* tp = (const uint32_t*)tiles;
  for_map_dtype_f32_i32(dtype, [&](auto dt) {
    hipLaunchKernelGGL(tile_compose_kernel<decltype(dt)::value == WM2F_F32>, grid, dim3(kTmThreads), 0, s, tp, n_ids, geom,
                       remap, out, th, tw, N, H, W);
  });
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
