// Mask2Former image preprocessing on the device: the resize / rescale / normalise / pad of
// Mask2FormerImageProcessorPil._preprocess (image_processing_pil_mask2former.py:485-585), bit-exact.
//
// wm2f_resize_normalize_u8: Pillow's two-pass 8-bit bilinear resample (fixed point, 22 fraction bits, uint8 clipped
//   between the passes) driven by host-built tap tables, then a float32 (channel, byte) lookup table, zero padding to
//   (Hp, Wp) and the int64 pixel mask.  Pass 1 (horizontal) writes the uint8 intermediate to a caller workspace; pass 2
//   (vertical + lookup + pad + mask) reads it.  Both are HBM-bound streams.
// wm2f_resize_nearest_labels: Pillow's nearest resize of id maps through host-built index tables, padding with
//   ignore_index and one presence flag per id value per image.
#include "common.h"

namespace wm2f {
namespace {

constexpr int kPrecisionBits = 22;  // Pillow Resample.c: PRECISION_BITS = 32 - 8 - 2
constexpr int kPreMaxImages = WM2F_PRE_MAX_IMAGES;

struct PreDesc {
  int64_t in_off;  // first byte of the image in the packed input
  int64_t ws_off;  // first byte of its (H, w, 3) intermediate in the workspace
  int H, W, h, w;  // input and output size
  int tx, cx, kx;  // column table: (xmin, count) pairs at tx, kx coefficients per column at cx
  int ty, cy, ky;  // row table, the same
};

struct PreArgs {
  int n;
  PreDesc d[kPreMaxImages];
};

__device__ __forceinline__ uint8_t clip8(int v) {
  v >>= kPrecisionBits;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// pass 1: out[y][x][c] = clip8(2^21 + sum_k coef[x][k] * in[y][xmin + k][c]) for every input row y, output column x.
__global__ __launch_bounds__(256) void resize_h_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ tab,
                                                       uint8_t* __restrict__ ws, const PreArgs args) {
  const PreDesc& d = args.d[blockIdx.z];
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= d.w || y >= d.H) return;
  int xmin = tab[d.tx + 2 * x];
  int cnt = tab[d.tx + 2 * x + 1];
  xmin = xmin < 0 ? 0 : (xmin >= d.W ? d.W - 1 : xmin);
  cnt = cnt > d.kx ? d.kx : cnt;
  cnt = cnt > d.W - xmin ? d.W - xmin : cnt;
  const int32_t* k = tab + d.cx + (int64_t)x * d.kx;
  const uint8_t* row = in + d.in_off + ((int64_t)y * d.W + xmin) * 3;
  int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
  for (int j = 0; j < cnt; ++j) {
    const int c = k[j];
    s0 += c * row[3 * j];
    s1 += c * row[3 * j + 1];
    s2 += c * row[3 * j + 2];
  }
  uint8_t* o = ws + d.ws_off + ((int64_t)y * d.w + x) * 3;
  o[0] = clip8(s0);
  o[1] = clip8(s1);
  o[2] = clip8(s2);
}

// pass 2: vertical taps over the intermediate, lookup, pad, mask.  One thread per padded output pixel.
__global__ __launch_bounds__(256) void resize_v_kernel(const uint8_t* __restrict__ ws, const int32_t* __restrict__ tab,
                                                       const float* __restrict__ lut, float* __restrict__ out,
                                                       int64_t* __restrict__ pmask, int Hp, int Wp, const PreArgs args) {
  const PreDesc& d = args.d[blockIdx.z];
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= Wp) return;
  const int64_t plane = (int64_t)Hp * Wp;
  const int64_t p = (int64_t)y * Wp + x;
  float* o = out + (int64_t)blockIdx.z * 3 * plane + p;
  if (y >= d.h || x >= d.w) {
    o[0] = 0.f;
    o[plane] = 0.f;
    o[2 * plane] = 0.f;
    pmask[(int64_t)blockIdx.z * plane + p] = 0;
    return;
  }
  int ymin = tab[d.ty + 2 * y];
  int cnt = tab[d.ty + 2 * y + 1];
  ymin = ymin < 0 ? 0 : (ymin >= d.H ? d.H - 1 : ymin);
  cnt = cnt > d.ky ? d.ky : cnt;
  cnt = cnt > d.H - ymin ? d.H - ymin : cnt;
  const int32_t* k = tab + d.cy + (int64_t)y * d.ky;
  const uint8_t* col = ws + d.ws_off + ((int64_t)ymin * d.w + x) * 3;
  const int64_t stride = (int64_t)d.w * 3;
  int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
  for (int j = 0; j < cnt; ++j) {
    const int c = k[j];
    const uint8_t* q = col + j * stride;
    s0 += c * q[0];
    s1 += c * q[1];
    s2 += c * q[2];
  }
  o[0] = lut[clip8(s0)];
  o[plane] = lut[256 + clip8(s1)];
  o[2 * plane] = lut[512 + clip8(s2)];
  pmask[(int64_t)blockIdx.z * plane + p] = 1;
}

struct LabDesc {
  int64_t in_off;  // first element of the map in the packed input
  int H, W, h, w;
  int xi, yi;      // offsets of the w column and h row source indices in the index table
};

struct LabArgs {
  int n;
  LabDesc d[kPreMaxImages];
};

template <typename T>
__global__ __launch_bounds__(256) void nearest_labels_kernel(const T* __restrict__ in, const int32_t* __restrict__ tab,
                                                             int32_t* __restrict__ out, uint8_t* __restrict__ present,
                                                             int Hp, int Wp, int ignore_index, const LabArgs args) {
  const LabDesc& d = args.d[blockIdx.z];
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= Wp) return;
  int32_t* o = out + (int64_t)blockIdx.z * Hp * Wp + (int64_t)y * Wp + x;
  if (y >= d.h || x >= d.w) {
    *o = ignore_index;
    return;
  }
  int xs = tab[d.xi + x], ys = tab[d.yi + y];
  xs = xs < 0 ? 0 : (xs >= d.W ? d.W - 1 : xs);
  ys = ys < 0 ? 0 : (ys >= d.H ? d.H - 1 : ys);
  const int v = (int)in[d.in_off + (int64_t)ys * d.W + xs];
  *o = v;
  if (v >= 0 && v < 256 && !present[blockIdx.z * 256 + v]) present[blockIdx.z * 256 + v] = 1;  // benign race: all write 1
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_resize_normalize_u8(const uint8_t* images, int64_t images_bytes, const int64_t* desc, const int32_t* tables,
                                        int64_t n_table, const float* lut, uint8_t* workspace, int64_t workspace_bytes,
                                        float* pixel_values, int64_t* pixel_mask, int B, int Hp, int Wp,
                                        void* stream) {
  const char* who = "wm2f_resize_normalize_u8";
  WM2F_REQUIRE(images && desc && tables && lut && workspace && pixel_values && pixel_mask, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && Hp > 0 && Wp > 0, "%s: need B, Hp, Wp > 0", who);
  if (B > kPreMaxImages || Hp > WM2F_PRE_MAX_SIDE || Wp > WM2F_PRE_MAX_SIDE) {
    set_error("%s: B = %d, (Hp, Wp) = (%d, %d) exceed the built bounds (B <= %d, sides <= %d)", who, B, Hp, Wp,
              kPreMaxImages, WM2F_PRE_MAX_SIDE);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(n_table > 0 && n_table < INT32_MAX && workspace_bytes > 0, "%s: bad table or workspace size", who);
  PreArgs a;
  a.n = B;
  int maxH = 0, maxw = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t* r = desc + (int64_t)b * WM2F_PRE_DESC_LEN;
    PreDesc& d = a.d[b];
    d.in_off = r[0];
    d.ws_off = r[1];
    d.H = (int)r[2], d.W = (int)r[3], d.h = (int)r[4], d.w = (int)r[5];
    d.tx = (int)r[6], d.cx = (int)r[7], d.kx = (int)r[8], d.ty = (int)r[9], d.cy = (int)r[10], d.ky = (int)r[11];
    WM2F_REQUIRE(r[2] > 0 && r[3] > 0 && r[4] > 0 && r[5] > 0 && r[2] <= WM2F_PRE_MAX_SIDE && r[3] <= WM2F_PRE_MAX_SIDE,
                 "%s: image %d: bad size (%lld, %lld) -> (%lld, %lld)", who, b, (long long)r[2], (long long)r[3],
                 (long long)r[4], (long long)r[5]);
    WM2F_REQUIRE(d.h <= Hp && d.w <= Wp, "%s: image %d: output (%d, %d) larger than the padded size", who, b, d.h, d.w);
    WM2F_REQUIRE(r[0] >= 0 && r[0] + (int64_t)d.H * d.W * 3 <= images_bytes, "%s: image %d: outside the input", who, b);
    WM2F_REQUIRE(r[1] >= 0 && r[1] + (int64_t)d.H * d.w * 3 <= workspace_bytes,
                 "%s: image %d: workspace too small or bad offsets", who, b);
    WM2F_REQUIRE(d.kx > 0 && d.ky > 0 && r[6] >= 0 && r[7] >= 0 && r[9] >= 0 && r[10] >= 0 &&
                     r[6] + 2 * (int64_t)d.w <= n_table && r[7] + (int64_t)d.w * d.kx <= n_table &&
                     r[9] + 2 * (int64_t)d.h <= n_table && r[10] + (int64_t)d.h * d.ky <= n_table,
                 "%s: image %d: table offsets outside the table", who, b);
    maxH = d.H > maxH ? d.H : maxH;
    maxw = d.w > maxw ? d.w : maxw;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)ceil_div(maxw, 256), (unsigned)maxH, (unsigned)B), dim3(256), 0, s,
                     images, tables, workspace, a);
  WM2F_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(resize_v_kernel, dim3((unsigned)ceil_div(Wp, 256), (unsigned)Hp, (unsigned)B), dim3(256), 0, s,
                     workspace, tables, lut, pixel_values, pixel_mask, Hp, Wp, a);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_resize_nearest_labels(const void* maps, int dtype, int64_t n_map_elems, const int64_t* desc, const int32_t* tables,
                                          int64_t n_table, int32_t* out, uint8_t* present, int B, int Hp, int Wp,
                                          int ignore_index, void* stream) {
  const char* who = "wm2f_resize_nearest_labels";
  WM2F_REQUIRE(maps && desc && tables && out && present, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && Hp > 0 && Wp > 0, "%s: need B, Hp, Wp > 0", who);
  if (dtype != WM2F_U8 && dtype != WM2F_I32) {
    set_error("%s: dtype %d not built (WM2F_U8 or WM2F_I32)", who, dtype);
    return WM2F_EUNSUPPORTED;
  }
  if (B > kPreMaxImages || Hp > WM2F_PRE_MAX_SIDE || Wp > WM2F_PRE_MAX_SIDE) {
    set_error("%s: B = %d, (Hp, Wp) = (%d, %d) exceed the built bounds (B <= %d, sides <= %d)", who, B, Hp, Wp,
              kPreMaxImages, WM2F_PRE_MAX_SIDE);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(n_table > 0 && n_table < INT32_MAX, "%s: bad table size", who);
  LabArgs a;
  a.n = B;
  for (int b = 0; b < B; ++b) {
    const int64_t* r = desc + (int64_t)b * WM2F_LAB_DESC_LEN;
    LabDesc& d = a.d[b];
    d.in_off = r[0];
    d.H = (int)r[1], d.W = (int)r[2], d.h = (int)r[3], d.w = (int)r[4], d.xi = (int)r[5], d.yi = (int)r[6];
    WM2F_REQUIRE(r[0] >= 0 && r[1] > 0 && r[2] > 0 && r[3] > 0 && r[4] > 0 && r[1] <= WM2F_PRE_MAX_SIDE &&
                     r[2] <= WM2F_PRE_MAX_SIDE && d.h <= Hp && d.w <= Wp,
                 "%s: image %d: bad size", who, b);
    WM2F_REQUIRE(r[0] + (int64_t)d.H * d.W <= n_map_elems, "%s: image %d: outside the input", who, b);
    WM2F_REQUIRE(r[5] >= 0 && r[6] >= 0 && r[5] + d.w <= n_table && r[6] + d.h <= n_table,
                 "%s: image %d: index table offsets outside the table", who, b);
  }
  hipStream_t s = (hipStream_t)stream;
  WM2F_REQUIRE(hipMemsetAsync(present, 0, (size_t)B * 256, s) == hipSuccess, "%s: clearing the flags failed", who);
  const dim3 grid((unsigned)ceil_div(Wp, 256), (unsigned)Hp, (unsigned)B);
  if (dtype == WM2F_U8)
    hipLaunchKernelGGL(nearest_labels_kernel<uint8_t>, grid, dim3(256), 0, s, (const uint8_t*)maps, tables, out, present,
                       Hp, Wp, ignore_index, a);
  else
    hipLaunchKernelGGL(nearest_labels_kernel<int32_t>, grid, dim3(256), 0, s, (const int32_t*)maps, tables, out,
                       present, Hp, Wp, ignore_index, a);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
