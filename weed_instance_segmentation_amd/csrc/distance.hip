// Interior distance maps and per-instance aim points of id maps on the device: for every pixel of
// a (B, H, W) map the squared Euclidean distance to the nearest position that does not carry the pixel's own id, and for
// every instance the pixel where that distance is largest.  The semantics are written out in include/wm2f.h;
// tests/distance_reference.py restates them with brute force and with scipy's distance transform per id.
//
// The distance is separable and exact in integers:
//   distance_summary : a lane per column marching down a chunk of rows: the id and length of the run of equal ids at the
//                      chunk's top and at its bottom (16 B per chunk and column).  A chunk whose top run is the whole
//                      chunk is one id throughout.
//   distance_cols    : the same grid.  A lane first takes its carry from the summaries of the chunks above (the run that
//                      ends just over its chunk: it walks up while chunks are one id and that id is the run's), marches
//                      down writing the distance up, takes the carry from below and marches back up writing
//                      g(x, y) = min(up, down), uint16: the vertical distance to the nearest position of column x that
//                      does not carry the pixel's id (0 for a pixel without an id, 0xffff where there is none, which
//                      only border-inside mode knows).
//   distance_rows    : a workgroup stages whole rows -- ids and g -- in LDS.  A wave per row then finds every pixel's
//                      run of equal ids (ballot and bit scan, a carry across 64-pixel steps) and from it h(x), the
//                      horizontal distance to the nearest position off the pixel's id.  A pixel starts from
//                      min(g, h)^2 and walks outwards, both sides at once, while step^2 is below its best, offering
//                      step^2 + min(g(x - step), g(x + step))^2.  The walk ends before it reaches the end of the run
//                      (step^2 >= h^2), so it never needs to look at an id and never goes further than the answer.
// aim points: init (rounded centroids from the stats rows), an atomicMax of d2 per instance, an unsigned 64-bit atomicMin
// of (centroid distance^2 << 32 | y * W + x) over the pixels that attain it, and a pass that writes the rows.
// Everything is integer and no result depends on an order of accumulation.
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kDtThreads = 256;
constexpr int kDtMinChunkRows = 32;   // columns pass: a chunk owns at least this many rows
constexpr int kDtUnroll = 8;          // rows of one column in flight
constexpr int kDtRowPixels = 1024;    // rows pass: short rows share a workgroup up to this many pixels (8 KiB of LDS)
constexpr int kDtWideRow = 4096;      // rows pass: a longer row gets a workgroup of kDtRowThreadsWide threads
constexpr int kDtWalk = 4;            // rows pass: steps of a walk whose LDS reads are in flight together
constexpr int kDtRowThreadsWide = 1024;  // rows pass: threads of a workgroup that holds one long row
constexpr int kDtLdsMaxIds = 1024;    // aim points: per-instance accumulators in LDS up to this N
constexpr int kDtNone = 0xffff;       // g: no position of the column is off the pixel's id
constexpr int kDtNoKey = -2;          // equals no pixel's key, not even "no id" (-1)

// result row of a key, -1 for none: the key itself when in [0, N), or its position in the image's ascending list
__device__ __forceinline__ int row_of_key(int v, const int32_t* ids, int n, int N) {
  if (v < 0) return -1;
  if (ids == nullptr) return v < N ? v : -1;
  return list_row(v, ids, n);
}

// grid (ceil(W / 256), chunks, B), 256 threads: a lane per column, the chunk's rows top to bottom.
// sum[(b * chunks + c) * W + x] = (key_top, run_top, key_bot, run_bot)
template <int DT>
__global__ __launch_bounds__(kDtThreads) void distance_summary_kernel(const void* __restrict__ map, int4* __restrict__ sum,
                                                                     int H, int W, int chunk_rows) {
  using E = typename MapElem<DT>::type;
  const int x = blockIdx.x * kDtThreads + threadIdx.x;
  if (x >= W) return;
  const int y0 = blockIdx.y * chunk_rows;
  const int y1 = y0 + chunk_rows < H ? y0 + chunk_rows : H;
  const E* src = reinterpret_cast<const E*>(map) + (int64_t)blockIdx.z * H * W + x;
  int key_top = -1, run_top = 0, cur = kDtNoKey, run = 0;
  bool first = true;  // still inside the top run
  for (int r0 = y0; r0 < y1; r0 += kDtUnroll) {
    uint32_t v[kDtUnroll];
#pragma unroll
    for (int u = 0; u < kDtUnroll; ++u) v[u] = r0 + u < y1 ? (uint32_t)src[(int64_t)(r0 + u) * W] : 0u;
#pragma unroll
    for (int u = 0; u < kDtUnroll; ++u) {
      const int r = r0 + u;
      if (r >= y1) break;
      const int k = map_id<DT>(v[u]);
      if (k == cur) {
        ++run;
      } else {
        if (r == y0) {
          key_top = k;
        } else if (first) {
          run_top = run;
          first = false;
        }
        cur = k;
        run = 1;
      }
    }
  }
  if (first) run_top = run;
  sum[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * W + x] = make_int4(key_top, run_top, cur, run);
}

// the same grid.  g (B, H, W) uint16.
template <int DT>
__global__ __launch_bounds__(kDtThreads) void distance_cols_kernel(const void* __restrict__ map, const int4* __restrict__ sum,
                                                                  uint16_t* __restrict__ g, int H, int W, int chunk_rows,
                                                                  int border_outside) {
  using E = typename MapElem<DT>::type;
  const int x = blockIdx.x * kDtThreads + threadIdx.x;
  if (x >= W) return;
  const int c = blockIdx.y, chunks = gridDim.y;
  const int y0 = c * chunk_rows;
  const int y1 = y0 + chunk_rows < H ? y0 + chunk_rows : H;
  const int64_t img = (int64_t)blockIdx.z * H * W;
  const E* src = reinterpret_cast<const E*>(map) + img + x;
  uint16_t* dst = g + img + x;
  const int4* sb = sum + (int64_t)blockIdx.z * chunks * W + x;
  const bool inside = border_outside == 0;

  // the run that ends just above the chunk: its id, its length, and whether it reaches the image's top
  int prev = kDtNoKey, cnt = 0;
  bool open = true;
  for (int cc = c - 1; cc >= 0 && open; --cc) {
    const int4 s = sb[(int64_t)cc * W];
    if (cc == c - 1) prev = s.z;
    if (s.z != prev) {
      open = false;
      break;
    }
    cnt += s.w;
    open = s.y == chunk_rows;  // one id throughout: the run goes on above (a chunk above is never the short last one)
  }
  for (int r0 = y0; r0 < y1; r0 += kDtUnroll) {
    uint32_t v[kDtUnroll];
#pragma unroll
    for (int u = 0; u < kDtUnroll; ++u) v[u] = r0 + u < y1 ? (uint32_t)src[(int64_t)(r0 + u) * W] : 0u;
#pragma unroll
    for (int u = 0; u < kDtUnroll; ++u) {
      const int r = r0 + u;
      if (r >= y1) break;
      const int k = map_id<DT>(v[u]);
      const bool same = k == prev;
      cnt = same ? cnt + 1 : 1;
      open = same ? open : r == 0;
      prev = k;
      dst[(int64_t)r * W] = (uint16_t)(k < 0 ? 0 : ((open && inside) ? kDtNone : cnt));
    }
  }

  // the run that begins just below the chunk, and whether it reaches the image's bottom
  prev = kDtNoKey;
  cnt = 0;
  open = true;
  for (int cc = c + 1; cc < chunks && open; ++cc) {
    const int4 s = sb[(int64_t)cc * W];
    if (cc == c + 1) prev = s.x;
    if (s.x != prev) {
      open = false;
      break;
    }
    cnt += s.y;
    const int rows_cc = H - cc * chunk_rows < chunk_rows ? H - cc * chunk_rows : chunk_rows;
    open = s.y == rows_cc;
  }
  for (int r0 = y1 - 1; r0 >= y0; r0 -= kDtUnroll) {
    uint32_t v[kDtUnroll];
    uint16_t up[kDtUnroll];
#pragma unroll
    for (int u = 0; u < kDtUnroll; ++u) {
      const bool in = r0 - u >= y0;
      v[u] = in ? (uint32_t)src[(int64_t)(r0 - u) * W] : 0u;
      up[u] = in ? dst[(int64_t)(r0 - u) * W] : (uint16_t)0;  // this lane's own stores, in program order
    }
#pragma unroll
    for (int u = 0; u < kDtUnroll; ++u) {
      const int r = r0 - u;
      if (r < y0) break;
      const int k = map_id<DT>(v[u]);
      const bool same = k == prev;
      cnt = same ? cnt + 1 : 1;
      open = same ? open : r == H - 1;
      prev = k;
      const int down = k < 0 ? 0 : ((open && inside) ? kDtNone : cnt);
      if (down < (int)up[u]) dst[(int64_t)r * W] = (uint16_t)down;
    }
  }
}

// grid ceil(B * H / rpb): a workgroup owns rpb consecutive rows of the (B * H, W) stack, ids and g of all of them in LDS.
// kVec: W % 4 == 0 and map and g aligned, so a lane stages four pixels per load.
template <int DT, bool kVec>
__global__ __launch_bounds__(kDtRowThreadsWide) void distance_rows_kernel(const void* __restrict__ map,
                                                                         const uint16_t* __restrict__ g,
                                                                         int32_t* __restrict__ d2, int64_t rows, int W,
                                                                         int rpb, int border_outside) {
  using E = typename MapElem<DT>::type;
  extern __shared__ __align__(16) unsigned char dtmem[];
  int* skey = reinterpret_cast<int*>(dtmem);
  uint16_t* sg = reinterpret_cast<uint16_t*>(dtmem + (size_t)rpb * W * sizeof(int));
  uint16_t* sh = sg + (size_t)rpb * W;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t row0 = (int64_t)blockIdx.x * rpb;
  const int nrows = rows - row0 < rpb ? (int)(rows - row0) : rpb;
  const int n = nrows * W;
  const int64_t base = row0 * W;
  const E* src = reinterpret_cast<const E*>(map) + base;
  const uint16_t* gs = g + base;
  if (kVec) {
    for (int i = tid * 4; i < n; i += nt * 4) {  // n % 4 == 0
      uint32_t v[4];
      load_map4<DT>(src + i, v);
      const uint2 gq = *reinterpret_cast<const uint2*>(gs + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) skey[i + j] = map_id<DT>(v[j]);
      *reinterpret_cast<uint2*>(sg + i) = gq;  // rpb * W * 4 and i * 2 are multiples of 8
    }
  } else {
    for (int i = tid; i < n; i += nt) {
      skey[i] = map_id<DT>((uint32_t)src[i]);
      sg[i] = gs[i];
    }
  }
  __syncthreads();
  // h(x): the horizontal distance to the nearest position of the row that does not carry the pixel's id, kDtNone where
  // there is none (beyond the border lies such a position only in border-outside mode).  A run starts where the id
  // changes; the last change at or before a pixel is a bit scan of its 64-pixel segment's ballot, or, where the
  // segment has none before it, the last change of the segments to its left.  So: every (row, segment) notes its last
  // change (sl) and, for the run's end, its first change from the right (sr); a wave per row turns these into what
  // reaches each segment from either side, by the same ballot and bit scan over segments; every segment then has both
  // ends of its pixels' runs.
  const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int segs = (W + 63) >> 6;
  int* sl = reinterpret_cast<int*>(sh + (size_t)rpb * W);  // 8 * rpb * W bytes in: 4-byte aligned
  int* sr = sl + rpb * segs;
  auto changes = [&](int it, unsigned long long& ml, unsigned long long& mr) {  // the segment's ballots; its first x
    const int r = it / segs, x0 = (it - r * segs) << 6, x = x0 + lane;
    const int* kr = skey + r * W;
    ml = __ballot(x < W && (x == 0 || kr[x] != kr[x - 1]));
    mr = __ballot(x < W && (x == W - 1 || kr[x] != kr[x + 1]));
    return x0;
  };
  for (int it = wave; it < nrows * segs; it += nw) {  // wave-uniform
    unsigned long long ml, mr;
    const int x0 = changes(it, ml, mr);
    if (lane == 0) {
      sl[it] = ml ? x0 + 63 - __clzll(ml) : -1;
      sr[it] = mr ? x0 + __ffsll(mr) - 1 : -1;
    }
  }
  __syncthreads();
  for (int r = wave; r < nrows; r += nw) {
    int carry = 0;
    for (int s0 = 0; s0 < segs; s0 += 64) {
      const int sgi = s0 + lane;
      const int v = sgi < segs ? sl[r * segs + sgi] : -1;
      const unsigned long long m = __ballot(v >= 0);
      const unsigned long long below = m & ((1ull << lane) - 1ull);
      const int from = __shfl(v, below ? 63 - __clzll(below) : 0, 64);
      if (sgi < segs) sl[r * segs + sgi] = below ? from : carry;  // the last change before the segment
      carry = m ? __shfl(v, 63 - __clzll(m), 64) : carry;
    }
    carry = W - 1;
    for (int s0 = (segs - 1) / 64 * 64; s0 >= 0; s0 -= 64) {
      const int sgi = s0 + lane;
      const int v = sgi < segs ? sr[r * segs + sgi] : -1;
      const unsigned long long m = __ballot(v >= 0);
      const unsigned long long above = m & ~((2ull << lane) - 1ull);
      const int from = __shfl(v, above ? __ffsll(above) - 1 : 0, 64);
      if (sgi < segs) sr[r * segs + sgi] = above ? from : carry;  // the first change beyond the segment
      carry = m ? __shfl(v, __ffsll(m) - 1, 64) : carry;
    }
  }
  __syncthreads();
  for (int it = wave; it < nrows * segs; it += nw) {
    unsigned long long ml, mr;
    const int x0 = changes(it, ml, mr), x = x0 + lane;
    const unsigned long long below = ml & (~0ull >> (63 - lane)), above = mr & (~0ull << lane);
    const int start = below ? x0 + 63 - __clzll(below) : sl[it];  // the run's first and last pixel
    const int end = above ? x0 + __ffsll(above) - 1 : sr[it];
    int left = x - start + 1, right = end - x + 1;
    if (!border_outside) {
      left = start == 0 ? kDtNone : left;
      right = end == W - 1 ? kDtNone : right;
    }
    if (x < W) sh[(it / segs) * W + x] = (uint16_t)(left < right ? left : right);
  }
  __syncthreads();
  // d2(x) = min(g(x)^2, h(x)^2, min over s of s^2 + min(g(x - s), g(x + s))^2), the steps taken while s^2 is below the
  // best so far.  A step that reaches s >= h, leaves the run or is clamped at the row's end offers at least s^2 >= h^2 or
  // what a nearer step offered, so no step needs to know whose pixel it reads: ids are not looked at here, and a pixel
  // without an id is one with g = 0.  kDtWalk steps are read together, so a step waits for LDS once in kDtWalk.
  for (int i = tid; i < n; i += nt) {
    const int gv = sg[i];
    int best = 0;
    if (gv != 0) {
      const int r = i / W, x = i - r * W;
      const uint16_t* gr = sg + r * W;
      const int hv = sh[i];
      const int m0 = gv < hv ? gv : hv;
      best = m0 == kDtNone ? INT32_MAX : m0 * m0;
      const int far = x > W - 1 - x ? x : W - 1 - x;
      for (int s0 = 1; s0 <= far && s0 * s0 < best; s0 += kDtWalk) {  // s <= 16384
        int gm[kDtWalk];
#pragma unroll
        for (int j = 0; j < kDtWalk; ++j) {
          const int xl = x - s0 - j > 0 ? x - s0 - j : 0;
          const int xr = x + s0 + j < W ? x + s0 + j : W - 1;
          const int gl = gr[xl], gq = gr[xr];
          gm[j] = gl < gq ? gl : gq;
        }
#pragma unroll
        for (int j = 0; j < kDtWalk; ++j) {
          const int s = s0 + j;
          const int cand = gm[j] == kDtNone ? INT32_MAX : s * s + gm[j] * gm[j];  // <= 2^28 + 2^28
          best = cand < best ? cand : best;
        }
      }
    }
    d2[base + i] = best;
  }
}

// ---- aim points -------------------------------------------------------------------------------------------------
// workspace of B * N instances: best (uint64), then dmax, cx, cy (int32)
struct AimWs {
  unsigned long long* best;
  int32_t* dmax;
  int32_t* cx;
  int32_t* cy;
};

__device__ __host__ __forceinline__ AimWs aim_ws(void* workspace, int total) {
  AimWs w;
  w.best = reinterpret_cast<unsigned long long*>(workspace);
  w.dmax = reinterpret_cast<int32_t*>(w.best + total);
  w.cx = w.dmax + total;
  w.cy = w.cx + total;
  return w;
}

__global__ __launch_bounds__(kDtThreads) void aim_init_kernel(const long long* __restrict__ stats, AimWs w, int total) {
  const int i = blockIdx.x * kDtThreads + threadIdx.x;
  if (i >= total) return;
  w.best[i] = ~0ull;
  w.dmax[i] = -1;
  int cx = 0, cy = 0;
  if (stats != nullptr) {
    const long long* s = stats + (int64_t)i * 8;
    const long long area = s[0];
    if (area > 0) {
      cx = (int)((2 * s[5] + area) / (2 * area));
      cy = (int)((2 * s[6] + area) / (2 * area));
    }
  }
  w.cx[i] = cx;
  w.cy[i] = cy;
}

// f(p, raw, d) for every pixel p of [p0, p1) of one image; kVec: four pixels per lane and load
template <int DT, bool kVec, class F>
__device__ __forceinline__ void aim_pixels(const void* map, const int32_t* d2, int64_t img, int p0, int p1, F&& f) {
  using E = typename MapElem<DT>::type;
  const E* src = reinterpret_cast<const E*>(map) + img;
  const int32_t* dd = d2 + img;
  if (kVec) {
    for (int p = p0 + (int)threadIdx.x * 4; p < p1; p += kDtThreads * 4) {
      uint32_t v[4];
      load_map4<DT>(src + p, v);
      const int4 d = *reinterpret_cast<const int4*>(dd + p);
      f(p, v[0], d.x);
      f(p + 1, v[1], d.y);
      f(p + 2, v[2], d.z);
      f(p + 3, v[3], d.w);
    }
  } else {
    for (int p = p0 + (int)threadIdx.x; p < p1; p += kDtThreads) f(p, (uint32_t)src[p], dd[p]);
  }
}

// grid (ceil(H * W / span), B).  kArg false: dmax[r] = max d2 over the instance.  kArg true: best[r] = min over the
// pixels with d2 == dmax[r] of (centroid distance^2 << 32 | p).  kLds: a workgroup folds its pixels in LDS first.
template <int DT, bool kVec, bool kLds, bool kArg>
__global__ __launch_bounds__(kDtThreads) void aim_scan_kernel(const void* __restrict__ map, const int32_t* __restrict__ d2,
                                                             const int32_t* __restrict__ ids,
                                                             const int32_t* __restrict__ n_ids, AimWs w, int HW, int W,
                                                             int N, int span, int centred) {
  extern __shared__ __align__(16) unsigned char aimmem[];
  // LDS: [best (N x 8, kArg)] [dmax (N x 4)] [ids (N x 4, with a list)]
  unsigned long long* lbest = reinterpret_cast<unsigned long long*>(aimmem);
  int32_t* lmax = reinterpret_cast<int32_t*>(aimmem + ((kLds && kArg) ? (size_t)N * 8 : 0));
  int32_t* sids = lmax + (kLds ? N : 0);
  const int b = blockIdx.y, tid = threadIdx.x;
  const int p0 = blockIdx.x * span;
  const int p1 = HW - p0 < span ? HW : p0 + span;
  int n = 0;
  if (ids != nullptr) {
    n = n_ids[b];
    n = n < 0 ? 0 : (n > N ? N : n);
    for (int j = tid; j < n; j += kDtThreads) sids[j] = ids[(int64_t)b * N + j];
  }
  int32_t* gmax = w.dmax + (int64_t)b * N;
  unsigned long long* gbest = w.best + (int64_t)b * N;
  const int32_t* cx = w.cx + (int64_t)b * N;
  const int32_t* cy = w.cy + (int64_t)b * N;
  if (kLds)
    for (int j = tid; j < N; j += kDtThreads) {
      lmax[j] = kArg ? gmax[j] : -1;
      if (kArg) lbest[j] = ~0ull;
    }
  __syncthreads();
  const int32_t* idl = ids != nullptr ? sids : nullptr;
  int32_t* amax = kLds ? lmax : gmax;
  unsigned long long* abest = kLds ? lbest : gbest;
  // a maximum only grows and a minimum only shrinks, so a stale read can at worst ask for an atomic that changes nothing
  aim_pixels<DT, kVec>(map, d2, (int64_t)b * HW, p0, p1, [&](int p, uint32_t raw, int d) {
    const int r = row_of_key(map_id<DT>(raw), idl, n, N);
    if (r < 0) return;
    if (!kArg) {
      if (d > amax[r]) atomicMax(amax + r, d);
    } else if (d == amax[r]) {
      unsigned long long key = (unsigned long long)(unsigned)p;
      if (centred) {
        const int y = p / W, x = p - y * W;
        const long long dx = x - cx[r], dy = y - cy[r];
        key |= (unsigned long long)(dx * dx + dy * dy) << 32;
      }
      if (key < abest[r]) atomicMin(abest + r, key);
    }
  });
  if (kLds) {
    __syncthreads();
    for (int j = tid; j < N; j += kDtThreads) {
      if (!kArg) {
        if (lmax[j] >= 0) atomicMax(gmax + j, lmax[j]);
      } else if (lbest[j] != ~0ull) {
        atomicMin(gbest + j, lbest[j]);
      }
    }
  }
}

__global__ __launch_bounds__(kDtThreads) void aim_write_kernel(AimWs w, int32_t* __restrict__ points, int total, int W) {
  const int i = blockIdx.x * kDtThreads + threadIdx.x;
  if (i >= total) return;
  const int dmax = w.dmax[i];
  int4 row = make_int4(-1, -1, 0, 0);
  if (dmax >= 0) {
    const int p = (int)(w.best[i] & 0xffffffffull);
    row = make_int4(p % W, p / W, dmax, 0);
  }
  reinterpret_cast<int4*>(points)[i] = row;
}

static_assert(kDtThreads == kMapColumnThreads, "column_chunk_rows sizes the grid of the columns pass");

// the rows launch for one dtype and alignment
template <int DT, bool kVec>
int launch_rows(const char* who, const void* map, const uint16_t* g, int32_t* d2, int64_t rows, int W, int rpb,
                int threads, size_t lds, int border_outside, hipStream_t s) {
  auto kfn = distance_rows_kernel<DT, kVec>;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    set_error("%s: cannot reserve %zu bytes of LDS", who, lds);
    return WM2F_ELAUNCH;
  }
  hipLaunchKernelGGL(kfn, dim3((unsigned)ceil_div64(rows, rpb)), dim3(threads), lds, s, map, g, d2, rows, W, rpb,
                     border_outside);
  return WM2F_OK;
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_labelmap_distance_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch) return -1;
  const int chunks = ceil_div(H, column_chunk_rows(B, H, W, kDtMinChunkRows));
  return map_g_bytes(B, H, W) + (int64_t)B * chunks * W * (int64_t)sizeof(int4);
}

extern "C" int wm2f_labelmap_distance(const void* map, int dtype, int32_t* d2, void* workspace, int B, int H, int W,
                                      int border_outside, void* stream) {
  const char* who = "wm2f_labelmap_distance";
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad size", who);
  if (H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch) {
    set_error("%s: sides <= %d, B <= %d (got %d x %d, %d)", who, kMapMaxSide, kMapMaxBatch, H, W, B);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(map && d2 && workspace, "%s: null pointer", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  WM2F_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "%s: the workspace must be 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  uint16_t* g = reinterpret_cast<uint16_t*>(workspace);
  int4* sum = reinterpret_cast<int4*>(reinterpret_cast<unsigned char*>(workspace) + map_g_bytes(B, H, W));
  const int chunk_rows = column_chunk_rows(B, H, W, kDtMinChunkRows);
  const dim3 cgrid(ceil_div(W, kDtThreads), ceil_div(H, chunk_rows), B);
  for_map_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    hipLaunchKernelGGL(distance_summary_kernel<DT>, cgrid, dim3(kDtThreads), 0, s, map, sum, H, W, chunk_rows);
    hipLaunchKernelGGL(distance_cols_kernel<DT>, cgrid, dim3(kDtThreads), 0, s, map, sum, g, H, W, chunk_rows,
                       border_outside);
  });
  WM2F_CHECK_LAUNCH(who);

  const int64_t rows = (int64_t)B * H;
  int rpb = W >= kDtRowPixels ? 1 : kDtRowPixels / W;
  rpb = rpb > rows ? (int)rows : rpb;
  const int threads = W > kDtWideRow ? kDtRowThreadsWide : kDtThreads;
  const size_t lds = (size_t)rpb * W * (sizeof(int) + 2 * sizeof(uint16_t)) + (size_t)rpb * ceil_div(W, 64) * 2 * sizeof(int);
  const bool vec = map_vec4_ok(map, dtype, W);  // g is 16-byte aligned
  const int rc = for_map_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    return vec ? launch_rows<DT, true>(who, map, g, d2, rows, W, rpb, threads, lds, border_outside, s)
               : launch_rows<DT, false>(who, map, g, d2, rows, W, rpb, threads, lds, border_outside, s);
  });
  if (rc != WM2F_OK) return rc;
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int64_t wm2f_labelmap_aim_points_workspace(int B, int N) {
  if (B <= 0 || N <= 0 || B > kMapMaxBatch || N > kMapMaxIds) return -1;
  return (int64_t)B * N * 20;
}

extern "C" int wm2f_labelmap_aim_points(const void* map, int dtype, const int32_t* d2, const int32_t* ids,
                                        const int32_t* n_ids, const int64_t* stats, int32_t* points, void* workspace,
                                        int B, int H, int W, int N, void* stream) {
  const char* who = "wm2f_labelmap_aim_points";
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N > 0, "%s: bad size", who);
  if (H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch || N > kMapMaxIds) {
    set_error("%s: sides <= %d, B <= %d, N <= %d (got %d x %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch, kMapMaxIds, H, W,
              B, N);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(map && d2 && points && workspace, "%s: null pointer", who);
  WM2F_REQUIRE((ids == nullptr) == (n_ids == nullptr), "%s: ids and n_ids go together", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  WM2F_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0 && reinterpret_cast<uintptr_t>(points) % 16 == 0,
               "%s: the workspace must be 8-byte and points 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const int total = B * N;
  const AimWs w = aim_ws(workspace, total);
  const dim3 igrid(ceil_div(total, kDtThreads));
  hipLaunchKernelGGL(aim_init_kernel, igrid, dim3(kDtThreads), 0, s, reinterpret_cast<const long long*>(stats), w, total);
  // about 1024 workgroups in all, each a whole number of 1024-pixel steps and at least four of them
  const int HW = H * W;  // <= 2^28
  int span = ceil_div(HW, ceil_div(1024, B));
  span = span < 4096 ? 4096 : ceil_div(span, 1024) * 1024;
  const dim3 grid(ceil_div(HW, span), B);
  const bool lds = N <= kDtLdsMaxIds;
  const bool vec = map_vec4_ok(map, dtype, W) && reinterpret_cast<uintptr_t>(d2) % 16 == 0;
  const int centred = stats != nullptr;
  for_map_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    const auto pass = [&](auto arg) {  // kArg false: the maxima; true: the pixels that attain them
      constexpr bool kArg = decltype(arg)::value;
      const auto scan = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(kDtThreads), (lds ? (size_t)N * (kArg ? 12 : 4) : 0) + (ids ? (size_t)N * 4 : 0),
                           s, map, d2, ids, n_ids, w, HW, W, N, span, centred);
      };
      if (vec && lds) scan(aim_scan_kernel<DT, true, true, kArg>);
      else if (vec) scan(aim_scan_kernel<DT, true, false, kArg>);
      else if (lds) scan(aim_scan_kernel<DT, false, true, kArg>);
      else scan(aim_scan_kernel<DT, false, false, kArg>);
    };
    pass(std::false_type{});
    pass(std::true_type{});
  });
  hipLaunchKernelGGL(aim_write_kernel, igrid, dim3(kDtThreads), 0, s, w, points, total, W);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
