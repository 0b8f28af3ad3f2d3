// The dependency's bilinear resize of mask logits to its fixed 384 x 384 grid, evaluated at one grid pixel on demand.
// Shared by the instance (postprocess.hip) and the semantic / panoptic (postprocess_sp.hip) post-processing kernels;
// the same function also resizes a 384 x 384 map to any target size (h, w = 384, gh, gw = target).
#pragma once
#include "common.h"

namespace wm2f {
namespace {

struct Grid {
  int h, w;      // logits
  int gh, gw;    // the dependency's fixed grid (384 x 384)
  float sh, sw;  // h / gh, w / gw: PyTorch's area_pixel_compute_scale (align_corners = False)
};

// upsample_bilinear2d(align_corners=False) at grid pixel (gy, gx): ATen UpSampleKernel.cpp HelperInterpLinear --
// source index scale * (i + 0.5) - 0.5 clamped at 0, second tap clamped to the last row / column, the x
// interpolation first, then y.  The products are kept unfused (as separate roundings).
__device__ __forceinline__ float grid_logit(const float* __restrict__ p, const Grid& g, int gy, int gx) {
  float sy = g.sh * ((float)gy + 0.5f) - 0.5f, sx = g.sw * ((float)gx + 0.5f) - 0.5f;
  sy = sy < 0.f ? 0.f : sy;
  sx = sx < 0.f ? 0.f : sx;
  int y0 = (int)sy, x0 = (int)sx;
  y0 = y0 > g.h - 1 ? g.h - 1 : y0;
  x0 = x0 > g.w - 1 ? g.w - 1 : x0;
  const int y1 = y0 + (y0 < g.h - 1 ? 1 : 0), x1 = x0 + (x0 < g.w - 1 ? 1 : 0);
  float ly = sy - (float)y0, lx = sx - (float)x0;
  ly = fminf(fmaxf(ly, 0.f), 1.f);
  lx = fminf(fmaxf(lx, 0.f), 1.f);
  const float hy = 1.f - ly, hx = 1.f - lx;
  const float v00 = p[y0 * g.w + x0], v01 = p[y0 * g.w + x1], v10 = p[y1 * g.w + x0], v11 = p[y1 * g.w + x1];
  const float t0 = __fadd_rn(__fmul_rn(hx, v00), __fmul_rn(lx, v01));
  const float t1 = __fadd_rn(__fmul_rn(hx, v10), __fmul_rn(lx, v11));
  return __fadd_rn(__fmul_rn(hy, t0), __fmul_rn(ly, t1));
}

int make_grid(Grid& g, int h, int w, int gh, int gw, const char* who) {
  WM2F_REQUIRE(h > 0 && w > 0 && gh > 0 && gw > 0, "%s: non-positive size", who);
  g.h = h;
  g.w = w;
  g.gh = gh;
  g.gw = gw;
  g.sh = (float)h / (float)gh;
  g.sw = (float)w / (float)gw;
  return WM2F_OK;
}

}  // namespace
}  // namespace wm2f
