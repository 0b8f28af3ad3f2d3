// Nearest-instance maps and per-cell pixel counts of id maps on the device: for every pixel of a
// (B, H, W) map the nearest source instance within a cap and the squared Euclidean distance to it -- the exterior
// counterpart of distance.hip -- and the pixel counts of the cells of a sprayer's grid.  The semantics are written out in
// include/wm2f.h; tests/nearest_reference.py restates them with brute force and as the kernels walk them.
//
// Exact in integers and separable, with the key (d2, id):
//   nearest_cols : a lane per column over a chunk of rows.  It starts r = floor(sqrt(max_d2)) rows above its chunk, so it
//                  needs no summary of the chunks above, marches down counting the rows since the last source pixel
//                  (saturating at r + 1: none), then the same from r rows below back up, keeping the nearer of the two
//                  and the smaller id where they are equally far.  g uint16 and the id int32: 6 bytes per pixel.
//   nearest_rows : a workgroup stages whole rows of g and id in LDS, builds per row the prefix count of pixels with
//                  g <= r (ballots per 64-pixel segment, a scan over the segments, the ballots again), and a pixel whose
//                  window [x - r, x + r] counts none writes "none" after one subtraction: the typical pixel is soil with
//                  nothing in range.  Every other pixel walks s = 0, 1, ... while s <= r and s^2 <= its best, offering
//                  (s^2 + g(x -+ s)^2, id(x -+ s)); <= because a candidate at equal distance with a smaller id still has
//                  to be seen.  kNrWalk steps' reads are in flight together.
//   cell_counts  : a workgroup owns a tile of cells, counts its pixels into integer LDS accumulators and stores the tile:
//                  no atomics on memory, nothing to clear.
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kNrThreads = 256;
constexpr int kNrMinChunkRows = 32;   // columns pass: a chunk owns at least this many rows
constexpr int kNrUnroll = 8;          // rows of one column in flight
constexpr int kNrRowPixels = 1024;    // rows pass: short rows share a workgroup up to this many pixels
constexpr int kNrWideRow = 4096;      // rows pass: a longer row gets a workgroup of kNrRowThreadsWide threads
constexpr int kNrRowThreadsWide = 1024;
constexpr int kNrWalk = 4;            // rows pass: steps of a walk whose LDS reads are in flight together
constexpr int kCellPixelsX = 256;     // cell counts: a tile is about this many pixels wide,
constexpr int kCellPixelsY = 16;      //              about this many tall,
constexpr int kCellTileCells = 512;   //              and at most this many cells (32 KiB of accumulators at G = 8)

// grid (ceil(W / 256), chunks, B), 256 threads: a lane per column.  g (B, H, W) uint16, gid (B, H, W) int32.
template <int DT>
__global__ __launch_bounds__(kNrThreads) void nearest_cols_kernel(const void* __restrict__ map,
                                                                 const uint8_t* __restrict__ source,
                                                                 uint16_t* __restrict__ g, int32_t* __restrict__ gid,
                                                                 int H, int W, int N, int chunk_rows, int r) {
  using E = typename MapElem<DT>::type;
  __shared__ uint8_t ssrc[kMapMaxIds];
  if (source != nullptr)
    for (int j = threadIdx.x; j < N; j += kNrThreads) ssrc[j] = source[(int64_t)blockIdx.z * N + j];
  __syncthreads();
  const int x = blockIdx.x * kNrThreads + threadIdx.x;
  if (x >= W) return;
  const int y0 = blockIdx.y * chunk_rows;
  const int y1 = y0 + chunk_rows < H ? y0 + chunk_rows : H;
  const int64_t img = (int64_t)blockIdx.z * H * W;
  const E* src = reinterpret_cast<const E*>(map) + img + x;
  uint16_t* gd = g + img + x;
  int32_t* idd = gid + img + x;
  const int none = r + 1;
  auto source_id = [&](uint32_t raw) {  // the id of a source pixel, -1 for every other pixel
    const int k = map_id<DT>(raw);
    if (k < 0 || k >= N) return -1;
    return (source == nullptr || ssrc[k] != 0) ? k : -1;
  };

  int dist = none, last = -1;  // rows since the last source pixel, saturating; its id
  for (int r0 = y0 - r > 0 ? y0 - r : 0; r0 < y1; r0 += kNrUnroll) {
    uint32_t v[kNrUnroll];
#pragma unroll
    for (int u = 0; u < kNrUnroll; ++u) v[u] = r0 + u < y1 ? (uint32_t)src[(int64_t)(r0 + u) * W] : 0u;
#pragma unroll
    for (int u = 0; u < kNrUnroll; ++u) {
      const int y = r0 + u;
      if (y >= y1) break;
      const int k = source_id(v[u]);
      dist = k >= 0 ? 0 : (dist < none ? dist + 1 : none);
      last = k >= 0 ? k : last;
      if (y >= y0) {
        gd[(int64_t)y * W] = (uint16_t)dist;
        idd[(int64_t)y * W] = dist < none ? last : -1;
      }
    }
  }

  dist = none;
  last = -1;
  for (int r0 = y1 - 1 + r < H - 1 ? y1 - 1 + r : H - 1; r0 >= y0; r0 -= kNrUnroll) {
    uint32_t v[kNrUnroll];
    uint16_t up[kNrUnroll];
    int32_t uid[kNrUnroll];
#pragma unroll
    for (int u = 0; u < kNrUnroll; ++u) {
      const int y = r0 - u;
      v[u] = y >= y0 ? (uint32_t)src[(int64_t)y * W] : 0u;
      const bool own = y >= y0 && y < y1;  // this lane's own stores, in program order
      up[u] = own ? gd[(int64_t)y * W] : (uint16_t)0;
      uid[u] = own ? idd[(int64_t)y * W] : 0;
    }
#pragma unroll
    for (int u = 0; u < kNrUnroll; ++u) {
      const int y = r0 - u;
      if (y < y0) break;
      const int k = source_id(v[u]);
      dist = k >= 0 ? 0 : (dist < none ? dist + 1 : none);
      last = k >= 0 ? k : last;
      if (y < y1 && dist < none && (dist < (int)up[u] || (dist == (int)up[u] && last < uid[u]))) {
        gd[(int64_t)y * W] = (uint16_t)dist;
        idd[(int64_t)y * W] = last;
      }
    }
  }
}

// grid ceil(B * H / rpb): a workgroup owns rpb consecutive rows of the (B * H, W) stack, g, id and the prefix count of
// all of them in LDS.  kVec: W % 4 == 0, so a lane stages four pixels per load (the workspace is 16-byte aligned).
template <bool kVec>
__global__ __launch_bounds__(kNrRowThreadsWide) void nearest_rows_kernel(
    const void* __restrict__ map, int dtype, const uint8_t* __restrict__ source, const uint16_t* __restrict__ g,
    const int32_t* __restrict__ gid, int32_t* __restrict__ nearest, int32_t* __restrict__ d2, int64_t rows, int H, int W,
    int N, int rpb, int r, int max_d2, int blocked, int walk_all) {
  extern __shared__ __align__(16) unsigned char nrmem[];
  int* sid = reinterpret_cast<int*>(nrmem);
  uint16_t* sg = reinterpret_cast<uint16_t*>(nrmem + (size_t)rpb * W * sizeof(int));
  uint16_t* sp = sg + (size_t)rpb * W;
  int* segc = reinterpret_cast<int*>(sp + (size_t)rpb * W);  // 8 * rpb * W bytes in: 4-byte aligned
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t row0 = (int64_t)blockIdx.x * rpb;
  const int nrows = rows - row0 < rpb ? (int)(rows - row0) : rpb;
  const int n = nrows * W;
  const int64_t base = row0 * W;
  if (kVec) {
    for (int i = tid * 4; i < n; i += nt * 4) {  // n % 4 == 0
      *reinterpret_cast<int4*>(sid + i) = *reinterpret_cast<const int4*>(gid + base + i);
      *reinterpret_cast<uint2*>(sg + i) = *reinterpret_cast<const uint2*>(g + base + i);
    }
  } else {
    for (int i = tid; i < n; i += nt) {
      sid[i] = gid[base + i];
      sg[i] = g[base + i];
    }
  }
  __syncthreads();
  // sp(x): how many pixels of the row up to and including x have a source within r in their column
  const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int segs = (W + 63) >> 6;
  if (!walk_all) {
    for (int it = wave; it < nrows * segs; it += nw) {  // wave-uniform
      const int rr = it / segs, x = ((it - rr * segs) << 6) + lane;
      const unsigned long long m = __ballot(x < W && (int)sg[rr * W + x] <= r);
      if (lane == 0) segc[it] = __popcll(m);
    }
    __syncthreads();
    for (int rr = wave; rr < nrows; rr += nw) {
      int carry = 0;
      for (int s0 = 0; s0 < segs; s0 += 64) {
        const int sgi = s0 + lane;
        const int v = sgi < segs ? segc[rr * segs + sgi] : 0;
        int inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int t = __shfl_up(inc, d, 64);
          inc += lane >= d ? t : 0;
        }
        if (sgi < segs) segc[rr * segs + sgi] = carry + inc - v;  // the count before the segment
        carry += __shfl(inc, 63, 64);
      }
    }
    __syncthreads();
    for (int it = wave; it < nrows * segs; it += nw) {
      const int rr = it / segs, x = ((it - rr * segs) << 6) + lane;
      const unsigned long long m = __ballot(x < W && (int)sg[rr * W + x] <= r);
      if (x < W) sp[rr * W + x] = (uint16_t)(segc[it] + __popcll(m & (~0ull >> (63 - lane))));  // <= 16384
    }
    __syncthreads();
  }
  const unsigned long long none = (unsigned long long)(unsigned)(max_d2 + 1) << 32;
  for (int i = tid; i < n; i += nt) {
    const int rr = i / W, x = i - rr * W;
    int out_id = -1, out_d = INT32_MAX;
    bool query = true;
    if (blocked) {  // only with a source list: a pixel of an instance that is no source keeps its id
      uint32_t raw;
      int k;
      if (dtype == WM2F_U8) {
        raw = reinterpret_cast<const uint8_t*>(map)[base + i];
        k = map_id<WM2F_U8>(raw);
      } else {
        raw = reinterpret_cast<const uint32_t*>(map)[base + i];
        k = dtype == WM2F_F32 ? map_id<WM2F_F32>(raw) : map_id<WM2F_I32>(raw);
      }
      if (k >= 0 && k < N && source[((row0 + rr) / H) * N + k] == 0) {
        out_id = k;
        out_d = 0;
        query = false;
      }
    }
    if (query && !walk_all) {
      const uint16_t* pr = sp + rr * W;
      const int lo = x - r, hi = x + r < W ? x + r : W - 1;
      query = (int)pr[hi] != (lo > 0 ? (int)pr[lo - 1] : 0);
    }
    if (query) {
      const uint16_t* gr = sg + rr * W;
      const int* ir = sid + rr * W;
      unsigned long long best = none;
      const int g0 = gr[x];
      if (g0 * g0 <= max_d2) best = (unsigned long long)(unsigned)(g0 * g0) << 32 | (unsigned)ir[x];
      const int far = x > W - 1 - x ? x : W - 1 - x;
      for (int s0 = 1; s0 <= r && s0 <= far && s0 * s0 <= (int)(best >> 32); s0 += kNrWalk) {
        int xl[kNrWalk], xr[kNrWalk], gl[kNrWalk], gq[kNrWalk];
#pragma unroll
        for (int j = 0; j < kNrWalk; ++j) {  // clamped at the row's ends: the end pixel again, farther than it was
          xl[j] = x - s0 - j > 0 ? x - s0 - j : 0;
          xr[j] = x + s0 + j < W ? x + s0 + j : W - 1;
          gl[j] = gr[xl[j]];
          gq[j] = gr[xr[j]];
        }
#pragma unroll
        for (int j = 0; j < kNrWalk; ++j) {
          const int s2 = (s0 + j) * (s0 + j);  // s <= 1027, g <= 1025: far below 2^31
          const int cl = s2 + gl[j] * gl[j], cr = s2 + gq[j] * gq[j];
          if (cl <= (int)(best >> 32)) {
            const unsigned long long key = (unsigned long long)(unsigned)cl << 32 | (unsigned)ir[xl[j]];
            best = key < best ? key : best;
          }
          if (cr <= (int)(best >> 32)) {
            const unsigned long long key = (unsigned long long)(unsigned)cr << 32 | (unsigned)ir[xr[j]];
            best = key < best ? key : best;
          }
        }
      }
      if ((int)(best >> 32) <= max_d2) {
        out_d = (int)(best >> 32);
        out_id = (int)(unsigned)(best & 0xffffffffull);
      }
    }
    nearest[base + i] = out_id;
    d2[base + i] = out_d;
  }
}

// grid (ceil(GW / TC), ceil(GH / TR), B), 256 threads: the workgroup owns the cells [cy0, cy0 + TR) x [cx0, cx0 + TC).
// LDS: TR * TC * 2G int32 accumulators, then the image's group row (N bytes).
template <int DT>
__global__ __launch_bounds__(kNrThreads) void cell_counts_kernel(const void* __restrict__ map,
                                                                const uint8_t* __restrict__ group,
                                                                const int32_t* __restrict__ veto_d2, int veto_max,
                                                                int32_t* __restrict__ counts, int H, int W, int N, int G,
                                                                int cell_h, int cell_w, int off_y, int off_x, int GH,
                                                                int GW, int TR, int TC) {
  using E = typename MapElem<DT>::type;
  extern __shared__ __align__(16) unsigned char cellmem[];
  int* acc = reinterpret_cast<int*>(cellmem);
  const int cols = 2 * G, nacc = TR * TC * cols;
  uint8_t* sgrp = cellmem + (size_t)nacc * sizeof(int);
  const int tid = threadIdx.x, b = blockIdx.z;
  for (int j = tid; j < nacc; j += kNrThreads) acc[j] = 0;
  for (int j = tid; j < N; j += kNrThreads) sgrp[j] = group[(int64_t)b * N + j];
  __syncthreads();
  const int cx0 = blockIdx.x * TC, cy0 = blockIdx.y * TR;
  const int ncx = GW - cx0 < TC ? GW - cx0 : TC, ncy = GH - cy0 < TR ? GH - cy0 : TR;
  // the tile's pixels: cx0 < GW and cy0 < GH, so the window is never empty
  const int px0 = cx0 * cell_w - off_x > 0 ? cx0 * cell_w - off_x : 0;
  const int py0 = cy0 * cell_h - off_y > 0 ? cy0 * cell_h - off_y : 0;
  const int64_t ex = (int64_t)(cx0 + ncx) * cell_w - off_x, ey = (int64_t)(cy0 + ncy) * cell_h - off_y;
  const int px1 = ex < W ? (int)ex : W, py1 = ey < H ? (int)ey : H;
  const int rw = px1 - px0, total = rw * (py1 - py0);  // <= 2^28
  const int64_t img = (int64_t)b * H * W;
  const E* src = reinterpret_cast<const E*>(map) + img;
  for (int idx = tid; idx < total; idx += kNrThreads) {
    const int yy = idx / rw, y = py0 + yy, x = px0 + idx - yy * rw;
    const int64_t p = (int64_t)y * W + x;
    const int k = map_id<DT>((uint32_t)src[p]);
    if (k < 0 || k >= N) continue;
    const int gc = sgrp[k];
    if (gc >= G) continue;
    const int cyl = (y + off_y) / cell_h - cy0, cxl = (x + off_x) / cell_w - cx0;  // in [0, ncy) x [0, ncx)
    const bool veto = veto_d2 != nullptr && veto_d2[img + p] <= veto_max;
    atomicAdd(acc + (cyl * TC + cxl) * cols + (veto ? G : 0) + gc, 1);
  }
  __syncthreads();
  const int row_vals = ncx * cols;
  for (int j = tid; j < ncy * row_vals; j += kNrThreads) {
    const int cyl = j / row_vals, rem = j - cyl * row_vals;  // rem = cxl * cols + c, contiguous in acc and in counts
    counts[(((int64_t)b * GH + cy0 + cyl) * GW + cx0) * cols + rem] = acc[cyl * TC * cols + rem];
  }
}

static_assert(kNrThreads == kMapColumnThreads, "column_chunk_rows sizes the grid of the columns pass");

int isqrt_floor(int v) {
  int r = 0;
  while ((int64_t)(r + 1) * (r + 1) <= v) ++r;  // v <= 2^20: at most 1024 steps, on the host
  return r;
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_labelmap_nearest_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch) return -1;
  return map_g_bytes(B, H, W) + (int64_t)B * H * W * 4;
}

extern "C" int wm2f_labelmap_nearest(const void* map, int dtype, const uint8_t* source, int32_t* nearest, int32_t* d2,
                                     void* workspace, int B, int H, int W, int N, int max_d2, int flags, void* stream) {
  const char* who = "wm2f_labelmap_nearest";
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N > 0, "%s: bad size", who);
  WM2F_REQUIRE(max_d2 >= 0, "%s: max_d2 must not be negative (got %d)", who, max_d2);
  WM2F_REQUIRE((flags & ~(WM2F_NEAREST_BLOCKED | WM2F_NEAREST_WALK_ALL)) == 0, "%s: unknown flags %d", who, flags);
  if (H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch || N > kMapMaxIds || max_d2 > WM2F_NEAREST_MAX_D2) {
    set_error("%s: sides <= %d, B <= %d, N <= %d, max_d2 <= %d (got %d x %d, %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch,
              kMapMaxIds, WM2F_NEAREST_MAX_D2, H, W, B, N, max_d2);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(map && nearest && d2 && workspace, "%s: null pointer", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  WM2F_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "%s: the workspace must be 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  uint16_t* g = reinterpret_cast<uint16_t*>(workspace);
  int32_t* gid = reinterpret_cast<int32_t*>(reinterpret_cast<unsigned char*>(workspace) + map_g_bytes(B, H, W));
  const int r = isqrt_floor(max_d2);
  const int chunk_rows = column_chunk_rows(B, H, W, kNrMinChunkRows);
  const dim3 cgrid(ceil_div(W, kNrThreads), ceil_div(H, chunk_rows), B);
  for_map_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(nearest_cols_kernel<decltype(dt)::value>, cgrid, dim3(kNrThreads), 0, s, map, source, g, gid, H, W, N,
                       chunk_rows, r);
  });
  WM2F_CHECK_LAUNCH(who);

  const int64_t rows = (int64_t)B * H;
  int rpb = W >= kNrRowPixels ? 1 : kNrRowPixels / W;
  rpb = rpb > rows ? (int)rows : rpb;
  const int threads = W > kNrWideRow ? kNrRowThreadsWide : kNrThreads;
  const size_t lds = (size_t)rpb * W * (sizeof(int) + 2 * sizeof(uint16_t)) + (size_t)rpb * ceil_div(W, 64) * sizeof(int);
  const int blocked = (flags & WM2F_NEAREST_BLOCKED) != 0 && source != nullptr;  // without a list every instance is a source
  const int walk_all = (flags & WM2F_NEAREST_WALK_ALL) != 0;
  const dim3 rgrid((unsigned)ceil_div64(rows, rpb));
  const auto launch_rows = [&](auto kfn) {
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      set_error("%s: cannot reserve %zu bytes of LDS", who, lds);
      return WM2F_ELAUNCH;
    }
    hipLaunchKernelGGL(kfn, rgrid, dim3(threads), lds, s, map, dtype, source, g, gid, nearest, d2, rows, H, W, N, rpb, r,
                       max_d2, blocked, walk_all);
    return WM2F_OK;
  };
  const int rc = W % 4 == 0 ? launch_rows(nearest_rows_kernel<true>) : launch_rows(nearest_rows_kernel<false>);
  if (rc != WM2F_OK) return rc;
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_labelmap_cell_counts(const void* map, int dtype, const uint8_t* group, const int32_t* veto_d2,
                                         int veto_max, int32_t* counts, int B, int H, int W, int N, int G, int cell_h,
                                         int cell_w, int off_y, int off_x, void* stream) {
  const char* who = "wm2f_labelmap_cell_counts";
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N > 0 && cell_h > 0 && cell_w > 0, "%s: bad size", who);
  WM2F_REQUIRE(G >= 1 && G <= WM2F_CELL_MAX_GROUPS, "%s: 1 <= G <= %d (got %d)", who, WM2F_CELL_MAX_GROUPS, G);
  WM2F_REQUIRE(off_y >= 0 && off_y < cell_h && off_x >= 0 && off_x < cell_w, "%s: 0 <= offset < cell (got %d, %d in %d x %d)",
               who, off_y, off_x, cell_h, cell_w);
  WM2F_REQUIRE(veto_max >= 0, "%s: veto_max must not be negative (got %d)", who, veto_max);
  if (H > kMapMaxSide || W > kMapMaxSide || cell_h > kMapMaxSide || cell_w > kMapMaxSide || B > kMapMaxBatch || N > kMapMaxIds) {
    set_error("%s: sides and cells <= %d, B <= %d, N <= %d (got %d x %d, cells %d x %d, %d, %d)", who, kMapMaxSide,
              kMapMaxBatch, kMapMaxIds, H, W, cell_h, cell_w, B, N);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(map && group && counts, "%s: null pointer", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  hipStream_t s = (hipStream_t)stream;
  const int GH = ceil_div(H + off_y, cell_h), GW = ceil_div(W + off_x, cell_w);
  int TC = ceil_div(kCellPixelsX, cell_w);
  TC = TC > GW ? GW : TC;
  int TR = ceil_div(kCellPixelsY, cell_h);
  TR = TR > kCellTileCells / TC ? kCellTileCells / TC : TR;  // TC <= 256
  TR = TR > GH ? GH : TR;
  const dim3 grid(ceil_div(GW, TC), ceil_div(GH, TR), B);
  WM2F_REQUIRE(grid.y <= 65535u, "%s: too many tiles", who);  // at most 16384 rows of cells
  const size_t lds = (size_t)TR * TC * 2 * G * sizeof(int) + (size_t)N;
  for_map_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(cell_counts_kernel<decltype(dt)::value>, grid, dim3(kNrThreads), lds, s, map, group, veto_d2,
                       veto_max, counts, H, W, N, G, cell_h, cell_w, off_y, off_x, GH, GW, TR, TC);
  });
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
