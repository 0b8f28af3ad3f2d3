// Blending the class scores of overlapping tiles into one semantic map (the contract is in
// include/wm2f.h, tests/tile_blend_reference.py restates it in numpy).
//
// One launch, no workspace, no atomics.  Per output pixel, over every view (flip f, tile row r, tile column c, in that
// order) whose tile covers it: the bilinear sample of every class from the view's small score grid (grid_logit, the
// function the semantic post-processing resizes with), weighted by a tent window capped at the ramp, summed with one
// rounding per product and per sum; then the first-max argmax and, when asked for, the normalised scores.
//
// A workgroup is 64 lanes along x by 4 rows; a lane owns two consecutive pixels, so that seg and every plane of
// out_scores go out as 8-byte stores when W is even (pixel by pixel otherwise, with the same values).  A wave is one
// image row: its covering tile rows are wave-uniform, the covering tile columns are found once per lane.
// Classes are held four at a time with a running best across the chunks; the taps and fractions of a (view, pixel)
// are loop-invariant over the classes of a chunk.  Two pixels and four classes were measured against one and four pixels
// and eight classes (profiles/tile_blend_variants.jsonl): the kernel is bound by the latency of its gathers, and the
// smaller register set (86 VGPRs against 145) keeps five waves per SIMD in flight where four pixels by eight keep three.
// blockIdx.x runs along the image row, so the workgroups in flight share a tile row and reread its score grids from
// L2 / Infinity Cache; nothing is staged through LDS.
// ys and xs are never trusted: coverage is tested in 64 bits and every view index stays inside (F, R, Cn).
#include "common.h"
#include "postprocess_grid.h"

namespace wm2f {
namespace {

constexpr int kTbLanes = 64;   // lanes along x
constexpr int kTbRows = 4;     // image rows (waves) per workgroup
constexpr int kTbPix = 2;      // consecutive pixels per lane
constexpr int kTbChunk = 4;    // classes held in registers per pass over the views
constexpr int kTbMaxSide = WM2F_TILE_MAX_SIDE;
constexpr int kTbMaxTiles = WM2F_TILE_MAX_TILES;

// local coordinate of image coordinate P in a tile of side t at origin o; -1 when the tile does not cover P
__device__ __forceinline__ int tile_local(int P, int o, int t) {
  const int64_t d = (int64_t)P - o;
  return (d >= 0 && d < t) ? (int)d : -1;
}

__device__ __forceinline__ int min3(int a, int b, int c) {
  const int m = a < b ? a : b;
  return m < c ? m : c;
}

// grid (ceil(W / 128), ceil(H / 4)), block (64, 4).  Grid g: h, w = the score grid, gh, gw = the tile (th, tw).
__global__ __launch_bounds__(kTbLanes* kTbRows) void tile_blend_kernel(
    const float* __restrict__ scores, const int32_t* __restrict__ ys, const int32_t* __restrict__ xs,
    const int32_t* __restrict__ flips, int32_t* __restrict__ seg, float* __restrict__ out_scores, int F, int R, int Cn,
    int C, Grid g, int ramp_y, int ramp_x, int H, int W) {
  const int Y = blockIdx.y * kTbRows + threadIdx.y;
  const int X0 = (blockIdx.x * kTbLanes + threadIdx.x) * kTbPix;
  if (Y >= H || X0 >= W) return;
  const int th = g.gh, tw = g.gw;

  // the covering tile rows (uniform in the wave) and columns (per lane: the union over its pixels, counted per pixel)
  int r_lo = R, r_hi = 0, nrows = 0;
  for (int r = 0; r < R; ++r) {
    if (tile_local(Y, ys[r], th) >= 0) {
      r_lo = r < r_lo ? r : r_lo;
      r_hi = r + 1;
      ++nrows;
    }
  }
  int c_lo = Cn, c_hi = 0;
  int ncols[kTbPix];
#pragma unroll
  for (int u = 0; u < kTbPix; ++u) ncols[u] = 0;
  for (int c = 0; c < Cn; ++c) {
    const int o = xs[c];
    bool any = false;
#pragma unroll
    for (int u = 0; u < kTbPix; ++u) {
      if (X0 + u < W && tile_local(X0 + u, o, tw) >= 0) {
        ++ncols[u];
        any = true;
      }
    }
    if (any) {
      c_lo = c < c_lo ? c : c_lo;
      c_hi = c + 1;
    }
  }
  bool none[kTbPix], sole[kTbPix];  // n == 0, n == 1
#pragma unroll
  for (int u = 0; u < kTbPix; ++u) {
    none[u] = nrows == 0 || ncols[u] == 0;
    sole[u] = F == 1 && nrows == 1 && ncols[u] == 1;
  }

  const int64_t plane = (int64_t)g.h * g.w;
  const int64_t out_plane = (int64_t)H * W;
  const int64_t T = (int64_t)R * Cn;
  const int64_t pix = (int64_t)Y * W + X0;
  const bool vec = (W & 1) == 0;  // then X0 + 1 < W, and the row starts of 8-byte aligned arrays are 8-byte aligned
  float best[kTbPix];
  int arg[kTbPix];
#pragma unroll
  for (int u = 0; u < kTbPix; ++u) {
    best[u] = 0.f;
    arg[u] = 0;
  }

  for (int c0 = 0; c0 < C; c0 += kTbChunk) {
    const int cn = C - c0 < kTbChunk ? C - c0 : kTbChunk;
    float acc[kTbPix][kTbChunk], wsum[kTbPix];
#pragma unroll
    for (int u = 0; u < kTbPix; ++u) {
      wsum[u] = 0.f;
#pragma unroll
      for (int j = 0; j < kTbChunk; ++j) acc[u][j] = 0.f;
    }
    for (int f = 0; f < F; ++f) {
      const int flip = flips[f];
      for (int r = r_lo; r < r_hi; ++r) {
        const int y = tile_local(Y, ys[r], th);
        if (y < 0) continue;  // uniform in the wave
        const int wy = min3(y + 1, th - y, ramp_y);
        const int sy = (flip & 2) ? th - 1 - y : y;
        for (int c = c_lo; c < c_hi; ++c) {
          const int o = xs[c];
          const float* p = scores + ((((int64_t)f * T + (int64_t)r * Cn + c) * C + c0) * plane);
#pragma unroll
          for (int u = 0; u < kTbPix; ++u) {
            const int x = X0 + u < W ? tile_local(X0 + u, o, tw) : -1;
            if (x < 0) continue;
            const int wx = min3(x + 1, tw - x, ramp_x);
            const float w = sole[u] ? 1.f : (float)(wy * wx);
            const int sx = (flip & 1) ? tw - 1 - x : x;
#pragma unroll
            for (int j = 0; j < kTbChunk; ++j) {
              if (j < cn) {
                const float v = grid_logit(p + j * plane, g, sy, sx);
                acc[u][j] = __fadd_rn(acc[u][j], __fmul_rn(w, v));
              }
            }
            wsum[u] = __fadd_rn(wsum[u], w);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kTbChunk; ++j) {
      if (j >= cn) break;
      const int k = c0 + j;
      float s[kTbPix];
#pragma unroll
      for (int u = 0; u < kTbPix; ++u) {
        const float a = acc[u][j];
        if (k == 0 || a > best[u]) {  // first max wins
          best[u] = a;
          arg[u] = k;
        }
        s[u] = none[u] ? 0.f : (sole[u] ? a : __fdiv_rn(a, wsum[u]));
      }
      if (out_scores) {
        float* po = out_scores + (int64_t)k * out_plane + pix;
        if (vec) {
          *(float2*)po = make_float2(s[0], s[1]);
        } else {
#pragma unroll
          for (int u = 0; u < kTbPix; ++u)
            if (X0 + u < W) po[u] = s[u];
        }
      }
    }
  }
  int32_t* ps = seg + pix;
  if (vec) {
    *(int2*)ps = make_int2(none[0] ? -1 : arg[0], none[1] ? -1 : arg[1]);
  } else {
#pragma unroll
    for (int u = 0; u < kTbPix; ++u)
      if (X0 + u < W) ps[u] = none[u] ? -1 : arg[u];
  }
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_tile_blend(const void* scores, const int32_t* ys, const int32_t* xs, const int32_t* flips,
                               int32_t* seg, void* out_scores, int F, int R, int Cn, int C, int gh, int gw, int th, int tw,
                               int ramp_y, int ramp_x, int H, int W, void* stream) {
  const char* who = "wm2f_tile_blend";
  WM2F_REQUIRE(F >= 1 && R >= 1 && Cn >= 1 && C >= 1, "%s: F, R, Cn and C must be at least 1", who);
  WM2F_REQUIRE(ramp_y >= 1 && ramp_x >= 1, "%s: the ramps must be at least 1", who);
  WM2F_REQUIRE(gh >= 1 && gw >= 1 && th >= 1 && tw >= 1 && H >= 1 && W >= 1, "%s: non-positive size", who);
  if (gh > kTbMaxSide || gw > kTbMaxSide || th > kTbMaxSide || tw > kTbMaxSide || H > kTbMaxSide || W > kTbMaxSide ||
      (int64_t)R * Cn > kTbMaxTiles) {
    set_error("%s: grid %d x %d, tile %d x %d, output %d x %d, %d x %d tiles: sides at most %d, at most %d tiles", who, gh,
              gw, th, tw, H, W, R, Cn, kTbMaxSide, kTbMaxTiles);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(scores && ys && xs && flips && seg, "%s: null pointer", who);
  WM2F_REQUIRE(((uintptr_t)seg & 7u) == 0 && ((uintptr_t)out_scores & 7u) == 0, "%s: seg and out_scores must be 8-byte aligned", who);
  Grid g;
  const int rc = make_grid(g, gh, gw, th, tw, who);
  if (rc != WM2F_OK) return rc;
  const dim3 grid(ceil_div(W, kTbLanes * kTbPix), ceil_div(H, kTbRows));
  hipLaunchKernelGGL(tile_blend_kernel, grid, dim3(kTbLanes, kTbRows), 0, (hipStream_t)stream, (const float*)scores, ys, xs,
                     flips, seg, (float*)out_scores, F, R, Cn, C, g, ramp_y, ramp_x, H, W);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
