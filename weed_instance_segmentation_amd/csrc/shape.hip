// Per-instance shape sums of id maps on the device: raw second moments, pixel sides and the border
// counts of the 4-neighbourhood perimeter, and the exact convex hull of every instance's pixel squares.  The semantics
// are written out in include/wm2f.h; tests/shape_reference.py restates them with numpy and scipy, one id at a time.
//
//   wm2f_labelmap_shape_stats (3 launches)
//     clear          : shape (B, N, 10) <- 0.
//     shape_moments  : instance_stats.hip's walk -- a workgroup owns a strip of whole rows, a wave takes 256 consecutive
//                      pixels of one row per load, a wave of one value is one run for lane 0, otherwise a lane folds its
//                      own runs -- with six 64-bit sums per run: len, sum x, y len, sum x^2 (closed form), y^2 len,
//                      y sum x.  Accumulators in LDS while N <= kShLdsMaxIds (48 B each), flushed for the ids the strip
//                      saw by 64-bit integer atomics; above the cap the same code adds straight into the result.
//     shape_border   : a 64 x 32 tile with a halo of 2 in LDS, as result rows (-1: no listed id, or outside the image).
//                      A tile whose 68 x 36 rows are all equal -- background, the inside of a plant -- returns after the
//                      load.  Otherwise a lane looks at its pixel's four neighbours, and only a border pixel goes on to
//                      the 21 cells its code 1 + 2a + 10b is made of.  Four 32-bit counters per id in LDS under the same
//                      cap, flushed for the ids the tile touched.
//   wm2f_labelmap_hull (4 launches), from the boxes of wm2f_labelmap_instance_stats
//     hull_scan      : one workgroup: the exclusive scan of the box heights -> every instance's first row in the table.
//     hull_init      : the table's used rows <- (INT32_MAX, -1).
//     hull_rows      : the same walk; a run folds its first and last x into its (instance, row) entry with atomicMin /
//                      atomicMax, after a look at the entry.
//     hull_chain     : a wave per instance.  The hull of the pixel squares is the hull of the leftmost and rightmost
//                      corner on every corner line y' in [ymin, ymax + 1] (from the rows above and below the line).  The
//                      wave stages 64 lines at a time in LDS; lane 0 runs the monotone chain of the right side, lane 1
//                      that of the left side, in one instruction stream (the side only flips a sign), each with its stack
//                      in the instance's vertex slot and the two top entries in registers.  The wave then closes the
//                      polygon in place, sums the shoelace terms and takes the largest squared distance by brute force.
//   wm2f_labelmap_hull_vertices (1 launch): the slots -> a padded (B, N, K, 2) block.
// Everything is integer, atomics are integer min / max / add: results are bit-identical from run to run.
#include <climits>

#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kShThreads = 256;
constexpr int kShWaves = kShThreads / 64;
constexpr int kShPix = 4;
constexpr int kShSeg = 64 * kShPix;
constexpr int kShUnroll = 4;
constexpr int kShLdsMaxIds = 1024;  // moments: 48 B + 4 B of id list each, 52 KiB; border: 16 B + 4 B and a 9.6 KiB tile
constexpr int kShMaxStripRows = 256;
constexpr int kShCols = 10;

constexpr int kBdW = 64, kBdH = 32, kBdHalo = 2;
constexpr int kBdLW = kBdW + 2 * kBdHalo, kBdLH = kBdH + 2 * kBdHalo;

constexpr int kHullThreads = 64;
constexpr int kScanThreads = 1024;

template <int DT>
__device__ __forceinline__ int sh_row_of(uint32_t raw, const int32_t* ids, int n, int N) {
  int v;
  if (!map_int<DT>(raw, v)) return -1;
  if (ids == nullptr) return (v >= 0 && v < N) ? v : -1;
  return list_row(v, ids, n);
}

// the image's id list into LDS (n of them, clamped to [0, N]); returns n.  The caller synchronises.
__device__ __forceinline__ int load_id_list(const int32_t* ids, const int32_t* n_ids, int32_t* sids, int b, int N, int tid,
                                            int threads) {
  if (ids == nullptr) return 0;
  int n = n_ids[b];
  n = n < 0 ? 0 : (n > N ? N : n);
  for (int j = tid; j < n; j += threads) sids[j] = ids[(int64_t)b * N + j];
  return n;
}

// rows [y0, y1) of one image, a wave per (row, 256-pixel segment): f(r, len, x0, y) for every run of len pixels from x0
// of row y that carry the listed id of result row r.  A run never crosses a lane's four pixels unless the whole wave's
// pixels are equal; then it is the wave's segment, reported by lane 0.
template <int DT, bool kVec, class F>
__device__ __forceinline__ void walk_runs(const typename MapElem<DT>::type* base, int W, int y0, int y1,
                                          const int32_t* idl, int n, int N, F&& f) {
  using E = typename MapElem<DT>::type;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int segs = (W + kShSeg - 1) / kShSeg;
  int y = y0, seg = wave;
  while (seg >= segs) {
    seg -= segs;
    ++y;
  }
  while (y < y1) {  // wave-uniform
    int iy[kShUnroll], ix[kShUnroll];
    uint32_t v[kShUnroll][kShPix];
#pragma unroll
    for (int u = 0; u < kShUnroll; ++u) {
      iy[u] = y;
      ix[u] = seg * kShSeg;
      seg += kShWaves;
      while (seg >= segs) {
        seg -= segs;
        ++y;
      }
    }
#pragma unroll
    for (int u = 0; u < kShUnroll; ++u) {
      const int x = ix[u] + lane * kShPix;
#pragma unroll
      for (int j = 0; j < kShPix; ++j) v[u][j] = 0u;
      if (iy[u] < y1) {
        const E* p = base + (int64_t)iy[u] * W + x;
        if (kVec) {
          if (x < W) load_map4<DT>(p, v[u]);
        } else {
#pragma unroll
          for (int j = 0; j < kShPix; ++j)
            if (x + j < W) v[u][j] = (uint32_t)p[j];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kShUnroll; ++u) {
      if (iy[u] >= y1) break;  // wave-uniform
      const int yy = iy[u], xs = ix[u], x = xs + lane * kShPix;
      const int nv = W - x < 0 ? 0 : (W - x < kShPix ? W - x : kShPix);
      const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)v[u][0]);
      bool same = true;
#pragma unroll
      for (int j = 0; j < kShPix; ++j) same = same && (j >= nv || v[u][j] == first);
      if (__ballot(same) == ~0ull) {
        const int r = sh_row_of<DT>(first, idl, n, N);
        if (r >= 0 && lane == 0) f(r, W - xs < kShSeg ? W - xs : kShSeg, xs, yy);
        continue;
      }
      int j = 0;
      while (j < nv) {
        const uint32_t raw = v[u][j];
        int k = j + 1;
        while (k < nv && v[u][k] == raw) ++k;
        const int r = sh_row_of<DT>(raw, idl, n, N);
        if (r >= 0) f(r, k - j, x + j, yy);
        j = k;
      }
    }
  }
}

// ---- moments -----------------------------------------------------------------------------------------------------------
struct ShAcc {
  unsigned long long s[6];  // area, sum x, sum y, sum x^2, sum y^2, sum xy
};
static_assert(sizeof(ShAcc) == 48, "ShAcc layout");

template <int DT, bool kVec, bool kLds>
__global__ __launch_bounds__(kShThreads) void shape_moments_kernel(const void* __restrict__ map,
                                                                   const int32_t* __restrict__ ids,
                                                                   const int32_t* __restrict__ n_ids,
                                                                   long long* __restrict__ shape, int H, int W, int N,
                                                                   int strip_rows) {
  using E = typename MapElem<DT>::type;
  extern __shared__ __align__(8) unsigned char shmem[];
  ShAcc* acc = reinterpret_cast<ShAcc*>(shmem);
  int32_t* sids = reinterpret_cast<int32_t*>(shmem + (kLds ? (size_t)N * sizeof(ShAcc) : 0));
  const int b = blockIdx.y, tid = threadIdx.x;
  const int y0 = blockIdx.x * strip_rows;
  const int y1 = y0 + strip_rows < H ? y0 + strip_rows : H;
  const int n = load_id_list(ids, n_ids, sids, b, N, tid, kShThreads);
  if (kLds)
    for (int j = tid; j < N * 6; j += kShThreads) reinterpret_cast<unsigned long long*>(acc)[j] = 0ull;
  __syncthreads();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(shape) + (int64_t)b * N * kShCols;
  const E* base = reinterpret_cast<const E*>(map) + (int64_t)b * H * W;
  walk_runs<DT, kVec>(base, W, y0, y1, ids != nullptr ? sids : nullptr, n, N, [&](int r, int len, int x0, int y) {
    const unsigned long long l = (unsigned)len, x = (unsigned)x0, yy = (unsigned)y;
    const unsigned long long tri = l * (l - 1) / 2;                  // sum of 0 .. len-1
    const unsigned long long sq = (l - 1) * l * (2 * l - 1) / 6;     // sum of their squares
    const unsigned long long sx = l * x + tri;
    unsigned long long* a = kLds ? acc[r].s : out + (int64_t)r * kShCols;
    atomicAdd(a + 0, l);
    atomicAdd(a + 1, sx);
    atomicAdd(a + 2, yy * l);
    atomicAdd(a + 3, l * x * x + 2 * x * tri + sq);
    atomicAdd(a + 4, yy * yy * l);
    atomicAdd(a + 5, yy * sx);
  });
  if (kLds) {
    __syncthreads();
    for (int j = tid; j < N; j += kShThreads) {
      if (acc[j].s[0] == 0ull) continue;  // flush only what this strip saw
      unsigned long long* o = out + (int64_t)j * kShCols;
#pragma unroll
      for (int k = 0; k < 6; ++k) atomicAdd(o + k, acc[j].s[k]);
    }
  }
}

// ---- sides and border counts -------------------------------------------------------------------------------------------
// 0: straight, 1: diagonal, 2: mixed, -1: counts nowhere
__device__ __forceinline__ int perimeter_class(int code) {
  switch (code) {
    case 5: case 7: case 15: case 17: case 25: case 27: return 0;
    case 21: case 33: return 1;
    case 13: case 23: return 2;
    default: return -1;
  }
}

template <int DT, bool kLds>
__global__ __launch_bounds__(kShThreads) void shape_border_kernel(const void* __restrict__ map,
                                                                  const int32_t* __restrict__ ids,
                                                                  const int32_t* __restrict__ n_ids,
                                                                  long long* __restrict__ shape, int H, int W, int N) {
  using E = typename MapElem<DT>::type;
  extern __shared__ __align__(8) unsigned char shmem[];
  int* tile = reinterpret_cast<int*>(shmem);
  int32_t* sids = reinterpret_cast<int32_t*>(tile + kBdLW * kBdLH);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(sids + (ids != nullptr ? N : 0));
  const int b = blockIdx.z, tid = threadIdx.x;
  const int bx = blockIdx.x * kBdW, by = blockIdx.y * kBdH;
  const int n = load_id_list(ids, n_ids, sids, b, N, tid, kShThreads);
  __syncthreads();
  const int32_t* idl = ids != nullptr ? sids : nullptr;
  const E* base = reinterpret_cast<const E*>(map) + (int64_t)b * H * W;
  int lo = INT_MAX, hi = INT_MIN;
  for (int i = tid; i < kBdLW * kBdLH; i += kShThreads) {
    const int ly = i / kBdLW, lx = i - ly * kBdLW;
    const int y = by + ly - kBdHalo, x = bx + lx - kBdHalo;
    int r = -1;
    if (y >= 0 && y < H && x >= 0 && x < W) r = sh_row_of<DT>((uint32_t)base[(int64_t)y * W + x], idl, n, N);
    tile[i] = r;
    lo = r < lo ? r : lo;
    hi = r > hi ? r : hi;
  }
  __syncthreads();
  const int ref = tile[0];
  if (!__syncthreads_or(lo != ref || hi != ref)) return;  // one value all over: no border pixel
  if (kLds) {
    for (int j = tid; j < N * 4; j += kShThreads) cnt[j] = 0u;
    __syncthreads();
  }
  unsigned long long* out = reinterpret_cast<unsigned long long*>(shape) + (int64_t)b * N * kShCols;
  const int col = tid & 63;
  for (int ry = tid >> 6; ry < kBdH; ry += kShWaves) {
    const int* t = tile + (ry + kBdHalo) * kBdLW + col + kBdHalo;
    const int c = t[0];
    // a pixel outside the image holds -1 and is skipped with the background
    const int sides = (t[-kBdLW] != c) + (t[kBdLW] != c) + (t[-1] != c) + (t[1] != c);
    if (c < 0 || sides == 0) continue;
    const auto is = [&](int dy, int dx) { return t[dy * kBdLW + dx] == c; };
    // is the neighbour at (dy, dx) a border pixel of c
    const auto border = [&](int dy, int dx) {
      return is(dy, dx) && !(is(dy - 1, dx) && is(dy + 1, dx) && is(dy, dx - 1) && is(dy, dx + 1));
    };
    const int a = border(-1, 0) + border(1, 0) + border(0, -1) + border(0, 1);
    const int d = border(-1, -1) + border(-1, 1) + border(1, -1) + border(1, 1);
    const int k = perimeter_class(1 + 2 * a + 10 * d);
    if (kLds) {
      atomicAdd(cnt + c * 4, (uint32_t)sides);
      if (k >= 0) atomicAdd(cnt + c * 4 + 1 + k, 1u);
    } else {
      atomicAdd(out + (int64_t)c * kShCols + 6, (unsigned long long)sides);
      if (k >= 0) atomicAdd(out + (int64_t)c * kShCols + 7 + k, 1ull);
    }
  }
  if (kLds) {
    __syncthreads();
    for (int j = tid; j < N; j += kShThreads) {
      if (cnt[j * 4] == 0u) continue;  // every border pixel has a side
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (cnt[j * 4 + k]) atomicAdd(out + (int64_t)j * kShCols + 6 + k, (unsigned long long)cnt[j * 4 + k]);
    }
  }
}

// ---- hull ----------------------------------------------------------------------------------------------------------------
// workspace: first (B N + 1) int64 (an instance's first table row, -1 when the table is too short for it; the last entry
// is the rows in use), then the row table, `rows` int2 (xmin, xmax), then the vertex slots, 2 rows + 4 B N int2: instance i
// owns 2 (h + 2) of them from 2 (first[i] + 2 i).
struct HullWs {
  long long* first;
  int2* table;
  int2* slots;
};

__host__ __device__ __forceinline__ HullWs hull_ws(void* workspace, int total, int64_t rows) {
  HullWs w;
  w.first = reinterpret_cast<long long*>(workspace);
  w.table = reinterpret_cast<int2*>(w.first + total + 1);
  w.slots = w.table + rows;
  return w;
}

// box height of instance i, 0 for an empty or impossible row of stats
__device__ __forceinline__ int box_height(const long long* __restrict__ stats, int i, int H) {
  const long long* s = stats + (int64_t)i * 8;
  const long long ymin = s[2], ymax = s[4];
  if (s[0] <= 0 || ymin < 0 || ymax >= H || ymax < ymin) return 0;
  return (int)(ymax - ymin + 1);
}

__global__ __launch_bounds__(kScanThreads) void hull_scan_kernel(const long long* __restrict__ stats,
                                                                 long long* __restrict__ first, int total, int H,
                                                                 long long rows) {
  __shared__ long long part[kScanThreads];
  const int tid = threadIdx.x;
  const int per = ceil_div(total, kScanThreads);
  const int i0 = tid * per, i1 = i0 + per < total ? i0 + per : total;
  long long sum = 0;
  for (int i = i0; i < i1; ++i) sum += box_height(stats, i, H);
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {  // inclusive scan
    const long long v = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  long long off = part[tid] - sum;
  for (int i = i0; i < i1; ++i) {
    const int h = box_height(stats, i, H);
    first[i] = off + h <= rows ? off : -1;
    off += h;
  }
  if (tid == kScanThreads - 1) {
    const long long all = part[tid];
    first[total] = all < rows ? all : rows;
  }
}

__global__ __launch_bounds__(kShThreads) void hull_init_kernel(const long long* __restrict__ first, int2* __restrict__ table,
                                                               int total) {
  const long long used = first[total];
  for (long long i = (long long)blockIdx.x * kShThreads + threadIdx.x; i < used; i += (long long)gridDim.x * kShThreads)
    table[i] = make_int2(INT_MAX, -1);
}

template <int DT, bool kVec>
__global__ __launch_bounds__(kShThreads) void hull_rows_kernel(const void* __restrict__ map, const int32_t* __restrict__ ids,
                                                               const int32_t* __restrict__ n_ids,
                                                               const long long* __restrict__ stats,
                                                               const long long* __restrict__ first, int2* table, int H,
                                                               int W, int N, int strip_rows) {
  using E = typename MapElem<DT>::type;
  extern __shared__ __align__(8) unsigned char shmem[];
  int32_t* sids = reinterpret_cast<int32_t*>(shmem);
  const int b = blockIdx.y, tid = threadIdx.x;
  const int y0 = blockIdx.x * strip_rows;
  const int y1 = y0 + strip_rows < H ? y0 + strip_rows : H;
  const int n = load_id_list(ids, n_ids, sids, b, N, tid, kShThreads);
  __syncthreads();
  const E* base = reinterpret_cast<const E*>(map) + (int64_t)b * H * W;
  walk_runs<DT, kVec>(base, W, y0, y1, ids != nullptr ? sids : nullptr, n, N, [&](int r, int len, int x0, int y) {
    const int i = b * N + r;
    const long long f = first[i];
    const int h = box_height(stats, i, H);
    const long long dy = (long long)y - stats[(int64_t)i * 8 + 2];
    if (f < 0 || dy < 0 || dy >= h) return;  // stats of another map: nothing is written outside the instance's rows
    int2* e = table + f + dy;
    const int x1 = x0 + len - 1;
    if (x0 < e->x) atomicMin(&e->x, x0);
    if (x1 > e->y) atomicMax(&e->y, x1);
  });
}

__device__ __forceinline__ long long cross3(int2 a, int2 b, int2 p) {
  return (long long)(b.x - a.x) * (p.y - b.y) - (long long)(b.y - a.y) * (p.x - b.x);
}

__global__ __launch_bounds__(kHullThreads) void hull_chain_kernel(const long long* __restrict__ stats,
                                                                  const long long* __restrict__ first,
                                                                  const int2* __restrict__ table, int2* slots,
                                                                  long long* __restrict__ hull, int H) {
  __shared__ int2 rows[kHullThreads + 1];  // rows[k]: table row base + k - 1
  __shared__ int2 moved[kHullThreads];
  const int i = blockIdx.x, lane = threadIdx.x;
  const int h = box_height(stats, i, H);
  const long long f = first[i];
  long long* out = hull + (int64_t)i * 3;
  if (h == 0 || f < 0) {
    if (lane == 0) {
      out[0] = (h != 0) ? -1 : 0;  // -1: the table was too short for this instance
      out[1] = 0;
      out[2] = 0;
    }
    return;
  }
  const int ymin = (int)stats[(int64_t)i * 8 + 2];
  const int2* t = table + f;
  int2* slot = slots + 2 * (f + 2 * (long long)i);
  const int cap = 2 * (h + 2);
  const int2 none = make_int2(INT_MAX, -1);
  // the two chains over the corner lines 0 .. h, lane 0 the right side and lane 1 the left
  const bool right = lane == 0;
  int cnt = 0;
  int2 top = none, second = none;
  if (lane == 0) rows[kHullThreads] = none;
  for (int l0 = 0; l0 <= h; l0 += kHullThreads) {
    __syncthreads();
    const int2 carry = rows[kHullThreads];
    __syncthreads();
    rows[lane + 1] = l0 + lane < h ? t[l0 + lane] : none;
    if (lane == 0) rows[0] = carry;
    __syncthreads();
    if (lane < 2) {
      const int lines = h + 1 - l0 < kHullThreads ? h + 1 - l0 : kHullThreads;
      for (int k = 0; k < lines; ++k) {
        const int2 up = rows[k], dn = rows[k + 1];
        int x;
        if (right) {
          x = (up.y > dn.y ? up.y : dn.y) + 1;
          if (x <= 0) continue;  // no pixel on either side of the line
        } else {
          x = up.x < dn.x ? up.x : dn.x;
          if (x == INT_MAX) continue;
        }
        const int2 p = make_int2(x, ymin + l0 + k);
        while (cnt >= 2) {
          const long long c = cross3(second, top, p);
          if (right ? c > 0 : c < 0) break;
          --cnt;
          top = second;
          if (cnt >= 2) second = right ? slot[1 + cnt - 2] : slot[cap - 1 - (cnt - 2)];
        }
        if (right) slot[1 + cnt] = p; else slot[cap - 1 - cnt] = p;
        second = top;
        top = p;
        ++cnt;
      }
    }
  }
  __syncthreads();
  const int nr = __shfl(cnt, 0), nl = __shfl(cnt, 1);
  const int nv = nr + nl;
  // close the polygon: [left 0] [right 0 .. nr-1] [left nl-1 .. 1].  The left stack lies reversed at the slot's end.
  if (lane == 0) slot[0] = slot[cap - 1];
  for (int j0 = 0; j0 < nl - 1; j0 += kHullThreads) {  // the target lies below the source: ascending blocks never collide
    const int j = j0 + lane;
    if (j < nl - 1) moved[lane] = slot[cap - nl + j];
    __syncthreads();
    if (j < nl - 1) slot[nr + 1 + j] = moved[lane];
    __syncthreads();
  }
  __syncthreads();
  long long area2 = 0, feret2 = 0;
  for (int j = lane; j < nv; j += kHullThreads) {
    const int2 a = slot[j], c = slot[j + 1 < nv ? j + 1 : 0];
    area2 += (long long)a.x * c.y - (long long)c.x * a.y;
    for (int k = j + 1; k < nv; ++k) {
      const int2 q = slot[k];
      const long long dx = q.x - a.x, dy = q.y - a.y, d2 = dx * dx + dy * dy;
      feret2 = d2 > feret2 ? d2 : feret2;
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    area2 += __shfl_down(area2, d);
    const long long o = __shfl_down(feret2, d);
    feret2 = o > feret2 ? o : feret2;
  }
  if (lane == 0) {
    out[0] = nv;
    out[1] = area2;
    out[2] = feret2;
  }
}

__global__ __launch_bounds__(kShThreads) void hull_vertices_kernel(const long long* __restrict__ stats,
                                                                   const long long* __restrict__ first,
                                                                   const int2* __restrict__ slots,
                                                                   const long long* __restrict__ hull,
                                                                   int2* __restrict__ vertices, int total, int K, int H) {
  const long long idx = (long long)blockIdx.x * kShThreads + threadIdx.x;
  if (idx >= (long long)total * K) return;
  const int i = (int)(idx / K), k = (int)(idx - (long long)i * K);
  const long long nv = hull[(int64_t)i * 3], f = first[i];
  int2 p = make_int2(-1, -1);
  if (f >= 0 && k < nv && k < 2 * (box_height(stats, i, H) + 2)) p = slots[2 * (f + 2 * (long long)i) + k];
  vertices[idx] = p;
}

constexpr int64_t kHullMaxRows = (int64_t)1 << 30;

int strip_rows_for(int B, int H, int W) {
  // about 1024 strips in all, at least 4096 pixels and at most kShMaxStripRows rows each
  int rows = ceil_div(H, ceil_div(1024, B));
  const int min_rows = ceil_div(4096, W);
  rows = rows < min_rows ? min_rows : rows;
  rows = rows > kShMaxStripRows ? kShMaxStripRows : rows;
  return rows > H ? H : rows;
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_labelmap_shape_stats(const void* map, int dtype, const int32_t* ids, const int32_t* n_ids,
                                         int64_t* shape, int B, int H, int W, int N, void* stream) {
  const char* who = "wm2f_labelmap_shape_stats";
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N > 0, "%s: bad size", who);
  if (H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch || N > kMapMaxIds) {
    set_error("%s: sides <= %d, B <= %d, N <= %d (got %d x %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch, kMapMaxIds, H, W,
              B, N);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(map && shape, "%s: null pointer", who);
  WM2F_REQUIRE((ids == nullptr) == (n_ids == nullptr), "%s: ids and n_ids go together", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  hipStream_t s = (hipStream_t)stream;
  long long* out = reinterpret_cast<long long*>(shape);
  if (hipMemsetAsync(out, 0, (size_t)B * N * kShCols * sizeof(long long), s) != hipSuccess) {
    set_error("%s: clearing the result failed", who);
    return WM2F_ELAUNCH;
  }
  const int rows = strip_rows_for(B, H, W);
  const dim3 grid(ceil_div(H, rows), B);
  const bool lds = N <= kShLdsMaxIds;
  const bool vec = map_vec4_ok(map, dtype, W);
  const size_t idl = ids ? (size_t)N * sizeof(int32_t) : 0;
  const size_t shm = (lds ? (size_t)N * sizeof(ShAcc) : 0) + idl;
  const dim3 bgrid(ceil_div(W, kBdW), ceil_div(H, kBdH), B);
  const size_t bshm = (size_t)kBdLW * kBdLH * sizeof(int) + idl + (lds ? (size_t)N * 4 * sizeof(uint32_t) : 0);
  for_map_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kShThreads), shm, s, map, ids, n_ids, out, H, W, N, rows);
    };
    if (vec && lds) launch(shape_moments_kernel<DT, true, true>);
    else if (vec) launch(shape_moments_kernel<DT, true, false>);
    else if (lds) launch(shape_moments_kernel<DT, false, true>);
    else launch(shape_moments_kernel<DT, false, false>);
    if (lds) hipLaunchKernelGGL((shape_border_kernel<DT, true>), bgrid, dim3(kShThreads), bshm, s, map, ids, n_ids, out, H, W, N);
    else hipLaunchKernelGGL((shape_border_kernel<DT, false>), bgrid, dim3(kShThreads), bshm, s, map, ids, n_ids, out, H, W, N);
  });
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int64_t wm2f_labelmap_hull_workspace(int B, int N, int64_t rows) {
  if (B <= 0 || N <= 0 || rows < 0 || B > kMapMaxBatch || N > kMapMaxIds || rows > kHullMaxRows) return -1;
  const int64_t total = (int64_t)B * N;
  return (total + 1) * 8 + rows * 8 + (2 * rows + 4 * total) * 8;
}

extern "C" int wm2f_labelmap_hull(const void* map, int dtype, const int32_t* ids, const int32_t* n_ids,
                                  const int64_t* stats, int64_t* hull, void* workspace, int64_t rows, int B, int H, int W,
                                  int N, void* stream) {
  const char* who = "wm2f_labelmap_hull";
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N > 0 && rows >= 0, "%s: bad size", who);
  if (H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch || N > kMapMaxIds || rows > kHullMaxRows) {
    set_error("%s: sides <= %d, B <= %d, N <= %d, rows <= 2^30 (got %d x %d, %d, %d, %lld)", who, kMapMaxSide, kMapMaxBatch,
              kMapMaxIds, H, W, B, N, (long long)rows);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(map && stats && hull && workspace, "%s: null pointer", who);
  WM2F_REQUIRE((ids == nullptr) == (n_ids == nullptr), "%s: ids and n_ids go together", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  WM2F_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "%s: the workspace must be 8-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const int total = B * N;
  const HullWs w = hull_ws(workspace, total, rows);
  const long long* st = reinterpret_cast<const long long*>(stats);
  hipLaunchKernelGGL(hull_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, st, w.first, total, H, (long long)rows);
  const int iblocks = (int)(ceil_div64(rows, kShThreads) < 4096 ? ceil_div64(rows, kShThreads) : 4096);
  hipLaunchKernelGGL(hull_init_kernel, dim3(iblocks < 1 ? 1 : iblocks), dim3(kShThreads), 0, s, w.first, w.table, total);
  const int strip = strip_rows_for(B, H, W);
  const dim3 grid(ceil_div(H, strip), B);
  const bool vec = map_vec4_ok(map, dtype, W);
  const size_t shm = ids ? (size_t)N * sizeof(int32_t) : 0;
  for_map_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (vec) hipLaunchKernelGGL((hull_rows_kernel<DT, true>), grid, dim3(kShThreads), shm, s, map, ids, n_ids, st, w.first, w.table, H, W, N, strip);
    else hipLaunchKernelGGL((hull_rows_kernel<DT, false>), grid, dim3(kShThreads), shm, s, map, ids, n_ids, st, w.first, w.table, H, W, N, strip);
  });
  hipLaunchKernelGGL(hull_chain_kernel, dim3(total), dim3(kHullThreads), 0, s, st, w.first, w.table, w.slots,
                     reinterpret_cast<long long*>(hull), H);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_labelmap_hull_vertices(const int64_t* stats, const int64_t* hull, const void* workspace, int64_t rows,
                                           int32_t* vertices, int B, int H, int N, int K, void* stream) {
  const char* who = "wm2f_labelmap_hull_vertices";
  WM2F_REQUIRE(B > 0 && H > 0 && N > 0 && K > 0 && rows >= 0, "%s: bad size", who);
  if (H > kMapMaxSide || B > kMapMaxBatch || N > kMapMaxIds || rows > kHullMaxRows || K > 2 * (kMapMaxSide + 2)) {
    set_error("%s: H <= %d, B <= %d, N <= %d, rows <= 2^30, K <= %d (got %d, %d, %d, %lld, %d)", who, kMapMaxSide,
              kMapMaxBatch, kMapMaxIds, 2 * (kMapMaxSide + 2), H, B, N, (long long)rows, K);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(stats && hull && workspace && vertices, "%s: null pointer", who);
  WM2F_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0 && reinterpret_cast<uintptr_t>(vertices) % 8 == 0,
               "%s: the workspace and vertices must be 8-byte aligned", who);
  const int total = B * N;
  const HullWs w = hull_ws(const_cast<void*>(workspace), total, rows);
  const int64_t cells = (int64_t)total * K;  // < 2^17 * 2^15.1
  WM2F_REQUIRE(ceil_div64(cells, kShThreads) <= INT_MAX, "%s: B N K too large", who);
  hipLaunchKernelGGL(hull_vertices_kernel, dim3((unsigned)ceil_div64(cells, kShThreads)), dim3(kShThreads), 0,
                     (hipStream_t)stream, reinterpret_cast<const long long*>(stats), w.first, w.slots,
                     reinterpret_cast<const long long*>(hull), reinterpret_cast<int2*>(vertices), total, K, H);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
