// Boundary bands of id maps on the device: for every instance of a (B, H, W) map at once the pixels
// Boundary IoU (Cheng et al., CVPR 2021) keeps -- the mask minus its erosion by a (2d+1) x (2d+1) square, nothing
// beyond the image counting as mask.  A pixel is INTERIOR iff that square around it lies in the image and carries the
// pixel's id everywhere; every other pixel of an instance is in its band.  The semantics are written out in
// include/wm2f.h; tests/boundary_reference.py restates them with one loop over the (2d+1)^2 offsets.
//
// The square test is separable, and each direction is a run length, so the cost does not depend on d:
//   boundary_rows : a wave per row, 64 x PIX pixels per step.  c(x) = length of the run of equal ids ending at x is
//                   x - lastchange(x) + 1, and lastchange is a max-scan: inside a lane over its pixels, across the wave
//                   with six shuffles, across steps with a wave-uniform carry.  plane[x] = (c(x) >= 2d+1), one byte:
//                   the 2d+1 pixels ending at x are one id.  The row segment CENTRED at x is that test at x + d.
//   boundary_cols : a lane per column marching down a chunk of rows with its run counter in a register, rows coalesced
//                   across lanes; h(x, y) = plane[y][x + d] (0 past the row).  cnt(y) = rows ending at y with h set and
//                   one id; (x, y - d) is interior iff cnt(y) >= 2d+1.  A chunk owns the output rows [y0, y1), walks
//                   [y0 - d, y1 + d) (2d rows of warm-up: a count cut off at y0 - d still reaches 2d+1 where the true
//                   one does), writes every owned pixel's id when it passes it and -1 over it d rows later if it turns
//                   out interior -- the same lane, the same address, in program order.
// Everything is integer and no result depends on an order of accumulation.
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kBdThreads = 256;
constexpr int kBdWaves = kBdThreads / 64;
constexpr int kBdMinChunkRows = 64;   // vertical pass: a chunk owns at least this many rows (and at least 2d)
constexpr int kBdUnroll = 16;         // rows of one column per register set; two sets in flight

// grid ceil(B * H / 4), 256 threads: wave w of block k owns row 4k + w of the (B * H, W) stack.
template <int DT, int PIX>
__global__ __launch_bounds__(kBdThreads) void boundary_rows_kernel(const void* __restrict__ map,
                                                                  uint8_t* __restrict__ plane, int64_t rows, int W,
                                                                  int d) {
  using E = typename MapElem<DT>::type;
  constexpr int kStep = 64 * PIX;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kBdWaves + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const E* src = reinterpret_cast<const E*>(map) + row * W;
  uint8_t* dst = plane + row * W;
  const int need = 2 * d;  // c >= 2d+1  <=>  x - lastchange >= 2d

  auto load = [&](int xs, uint32_t (&v)[PIX]) {
    const int x = xs + lane * PIX;
#pragma unroll
    for (int j = 0; j < PIX; ++j) v[j] = 0u;
    if constexpr (PIX == 4) {  // W % 4 == 0 and an aligned map: the four pixels are inside the row together
      if (x < W) load_map4<DT>(src + x, v);
    } else {
      if (x < W) v[0] = (uint32_t)src[x];
    }
  };

  uint32_t cur[PIX], nxt[PIX];
  load(0, cur);
  int carry_lc = 0, carry_key = -1;  // wave-uniform: last change before this step, id of the pixel before it
  for (int xs = 0; xs < W; xs += kStep) {
    if (xs + kStep < W) load(xs + kStep, nxt);  // in flight during the scan
    const int x0 = xs + lane * PIX;
    int key[PIX];
#pragma unroll
    for (int j = 0; j < PIX; ++j) key[j] = map_id<DT>(cur[j]);
    int prev = __shfl_up(key[PIX - 1], 1, 64);
    if (lane == 0) prev = carry_key;
    int lc[PIX];  // last change at or before the pixel inside this lane, -1 for none
    int last = -1;
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
      const bool change = key[j] != prev || x0 + j == 0;
      last = change ? x0 + j : last;
      lc[j] = last;
      prev = key[j];
    }
    int scan = last;  // inclusive max-scan over the lanes; a lane below the offset gets its own value back
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(scan, o, 64);
      scan = up > scan ? up : scan;
    }
    scan = scan > carry_lc ? scan : carry_lc;
    int before = __shfl_up(scan, 1, 64);  // last change at or before the previous lane's last pixel
    if (lane == 0) before = carry_lc;
    uint32_t packed = 0u;
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
      const int l = lc[j] >= 0 ? lc[j] : before;
      packed |= (uint32_t)(x0 + j - l >= need) << (8 * j);
    }
    if (x0 < W) {
      if constexpr (PIX == 4) *reinterpret_cast<uint32_t*>(dst + x0) = packed;
      else dst[x0] = (uint8_t)packed;
    }
    carry_lc = __shfl(scan, 63, 64);
    carry_key = __shfl(key[PIX - 1], 63, 64);  // past the row's end in the last step only, where nothing follows
#pragma unroll
    for (int j = 0; j < PIX; ++j) cur[j] = nxt[j];
  }
}

// grid (ceil(W / 256), chunks, B), 256 threads: a lane per column, the chunk's rows top to bottom.
template <int DT>
__global__ __launch_bounds__(kBdThreads) void boundary_cols_kernel(const void* __restrict__ map,
                                                                  const uint8_t* __restrict__ plane,
                                                                  int32_t* __restrict__ out, int H, int W, int d,
                                                                  int chunk_rows) {
  using E = typename MapElem<DT>::type;
  const int x = blockIdx.x * kBdThreads + threadIdx.x;
  if (x >= W) return;
  const int y0 = blockIdx.y * chunk_rows;
  const int y1 = y0 + chunk_rows < H ? y0 + chunk_rows : H;
  const int rs = y0 - d > 0 ? y0 - d : 0;
  const int re = (int64_t)y1 + d < H ? y1 + d : H;
  const int64_t img = (int64_t)blockIdx.z * H * W;
  const E* src = reinterpret_cast<const E*>(map) + img + x;
  const bool has_h = (int64_t)x + d < W;  // the row segment centred at x ends inside the row
  const uint8_t* hp = plane + img + (has_h ? x + d : 0);
  int32_t* dst = out + img + x;
  const int need = 2 * d + 1;
  int prev = -1, cnt = 0;
  auto load = [&](int r0, uint32_t (&v)[kBdUnroll], uint8_t (&h)[kBdUnroll]) {
#pragma unroll
    for (int u = 0; u < kBdUnroll; ++u) {
      const int r = r0 + u;
      v[u] = r < re ? (uint32_t)src[(int64_t)r * W] : 0u;
      h[u] = (r < re && has_h) ? hp[(int64_t)r * W] : (uint8_t)0;
    }
  };
  auto walk = [&](int r0, const uint32_t (&v)[kBdUnroll], const uint8_t (&h)[kBdUnroll]) {
#pragma unroll
    for (int u = 0; u < kBdUnroll; ++u) {
      const int r = r0 + u;
      if (r >= re) break;
      const int k = map_id<DT>(v[u]);
      cnt = h[u] ? ((k == prev && r > rs) ? cnt + 1 : 1) : 0;
      prev = k;
      if (r >= y0 && r < y1) dst[(int64_t)r * W] = k;
      // the 2d+1 rows ending at r carry k: so does row r - d, which this lane wrote d rows ago
      if (cnt >= need && k >= 0 && r - d >= y0 && r - d < y1) dst[(int64_t)(r - d) * W] = -1;
    }
  };
  // two register sets: the next rows are requested before this set's stores are issued, so a set's loads never queue
  // behind stores (loads and stores share one in-order counter on this target)
  uint32_t va[kBdUnroll], vb[kBdUnroll];
  uint8_t ha[kBdUnroll], hb[kBdUnroll];
  load(rs, va, ha);
  for (int r0 = rs; r0 < re; r0 += 2 * kBdUnroll) {
    load(r0 + kBdUnroll, vb, hb);
    walk(r0, va, ha);
    load(r0 + 2 * kBdUnroll, va, ha);
    walk(r0 + kBdUnroll, vb, hb);
  }
}

static_assert(kBdThreads == kMapColumnThreads, "column_chunk_rows sizes the grid of the vertical pass");

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_labelmap_boundary_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch) return -1;
  return (int64_t)B * H * W;
}

extern "C" int wm2f_labelmap_boundary(const void* map, int dtype, int32_t* out, void* workspace, int B, int H, int W,
                                      int d, void* stream) {
  const char* who = "wm2f_labelmap_boundary";
  WM2F_REQUIRE(map && out && workspace, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && d >= 1, "%s: bad size", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  if (H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch || d > kMapMaxSide) {
    set_error("%s: sides <= %d, B <= %d, d <= %d (got %d x %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch, kMapMaxSide, H, W, B,
              d);
    return WM2F_EUNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  uint8_t* plane = reinterpret_cast<uint8_t*>(workspace);
  const bool vec = map_vec4_ok(map, dtype, W) && reinterpret_cast<uintptr_t>(plane) % 4 == 0;
  const int64_t rows = (int64_t)B * H;
  const dim3 rgrid((unsigned)ceil_div64(rows, kBdWaves));
  for_map_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (vec) hipLaunchKernelGGL((boundary_rows_kernel<DT, 4>), rgrid, dim3(kBdThreads), 0, s, map, plane, rows, W, d);
    else hipLaunchKernelGGL((boundary_rows_kernel<DT, 1>), rgrid, dim3(kBdThreads), 0, s, map, plane, rows, W, d);
  });
  WM2F_CHECK_LAUNCH(who);
  // row chunks: about kMapColumnWaves waves in all, each chunk at least kBdMinChunkRows and 2d rows (its 2d rows of
  // warm-up then cost at most what it owns; neighbouring chunks read them at about the same time)
  const int chunk_rows = column_chunk_rows(B, H, W, 2 * d > kBdMinChunkRows ? 2 * d : kBdMinChunkRows);
  const dim3 cgrid(ceil_div(W, kBdThreads), ceil_div(H, chunk_rows), B);
  for_map_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(boundary_cols_kernel<decltype(dt)::value>, cgrid, dim3(kBdThreads), 0, s, map, plane, out, H, W, d,
                       chunk_rows);
  });
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
