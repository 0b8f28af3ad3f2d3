// Training augmentation on the device: horizontal flip, resize and crop of Mask2Former inputs,
// bit-exact to Pillow's `transpose(FLIP_LEFT_RIGHT).resize((w, h)).crop(window)` followed by the processor's lookup and
// padding.  Only the crop window of the (h, w) resized frame is computed; the frame itself is never materialised.
//
// wm2f_augment_resize_normalize_u8: one launch.  A workgroup owns a kTileH x kTileW tile of the padded output.  It runs
//   Pillow's horizontal pass for the tile's columns over the source rows the tile's vertical taps reach, kChunk rows at
//   a time, into LDS as uint8 (clipped exactly as preprocess.hip's workspace bytes are), and adds each chunk's share of
//   the vertical taps into int32 registers.  The vertical sum is an exact integer sum (coefficients add up to 2^22, bytes
//   <= 255), so splitting it over chunks changes nothing; a downscale of any ratio stays one launch.  The store does the
//   clip, the (channel, byte) lookup, the zero padding and the pixel mask.  The source is read mirrored when flip is set:
//   column c of the flipped image is column W - 1 - c of the stored one, and the tap tables are those of the flipped image.
// wm2f_augment_nearest_labels: the id-map path, with the same mirrored source column, the window origin, ignore_index
//   padding and presence flags of the ids inside the window.
#include "common.h"

namespace wm2f {
namespace {

constexpr int kPrecisionBits = 22;  // Pillow Resample.c: PRECISION_BITS = 32 - 8 - 2
constexpr int kAugMaxImages = WM2F_PRE_MAX_IMAGES;
constexpr int kThreads = 256;
constexpr int kTileW = 128;  // a 32-lane half wave reads one 128-byte LDS row: conflict-free ds_read_b32
constexpr int kTileH = 16;   // two output rows per thread, four columns each
constexpr int kChunk = 64;   // source rows of the horizontal pass held in LDS at once: 3 * 64 * 128 = 24 KiB
constexpr int kRegTaps = 6;  // column coefficients kept in registers (covers every upscale and downscales to 1 / 2.5)

struct AugDesc {
  int64_t in_off;  // first byte of the image in the packed input
  int H, W, h, w;  // stored size and virtual resized size
  int tx, cx, kx;  // column table of W -> w: (xmin, count) pairs at tx, kx coefficients per column at cx
  int ty, cy, ky;  // row table of H -> h
  int flip, y0, x0, ch, cw;
};

struct AugArgs {
  AugDesc d[kAugMaxImages];
};

__device__ __forceinline__ uint8_t clip8(int v) {
  v >>= kPrecisionBits;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

template <bool kVec>
__device__ __forceinline__ void store_row(float* __restrict__ o, int64_t* __restrict__ m, int64_t plane, const float (&v)[3][4],
                                          const int (&inside)[4], int x, int Wp) {
  if (kVec) {
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    *reinterpret_cast<longlong2*>(m) = make_longlong2(inside[0], inside[1]);
    *reinterpret_cast<longlong2*>(m + 2) = make_longlong2(inside[2], inside[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (x + i >= Wp) break;
      o[i] = v[0][i];
      o[plane + i] = v[1][i];
      o[2 * plane + i] = v[2][i];
      m[i] = inside[i];
    }
  }
}

// kVec: Wp % 4 == 0, so every thread's four pixels are 16-byte aligned in every plane and lie inside the row.
template <bool kVec>
__global__ __launch_bounds__(kThreads) void augment_image_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ tab,
                                                                 const float* __restrict__ lut, float* __restrict__ out,
                                                                 int64_t* __restrict__ pmask, int Hp, int Wp,
                                                                 const AugArgs args) {
  __shared__ __attribute__((aligned(16))) uint8_t s_px[3][kChunk][kTileW];
  __shared__ float s_lut[768];
  __shared__ int s_ymin[kTileH], s_ycnt[kTileH];

  const AugDesc& d = args.d[blockIdx.z];
  const int t = threadIdx.x;
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;  // tile origin in the padded output
  const int64_t plane = (int64_t)Hp * Wp;
  float* obase = out + (int64_t)blockIdx.z * 3 * plane;
  int64_t* mbase = pmask + (int64_t)blockIdx.z * plane;

  // the vertical pass's view of this thread: rows vy and vy + 8 of the tile, columns vx .. vx + 3
  const int vy = t >> 5, vx = (t & 31) * 4;
  int acc[2][3][4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[r][c][i] = 1 << (kPrecisionBits - 1);

  const bool has_pixels = ty0 < d.ch && tx0 < d.cw;  // block-uniform
  if (has_pixels) {
    for (int i = t; i < 768; i += kThreads) s_lut[i] = lut[i];
    if (t < kTileH) {
      int ymin = 0, cnt = 0;
      if (ty0 + t < d.ch) {
        const int gy = d.y0 + ty0 + t;
        ymin = tab[d.ty + 2 * gy];
        cnt = tab[d.ty + 2 * gy + 1];
        ymin = ymin < 0 ? 0 : (ymin >= d.H ? d.H - 1 : ymin);
        cnt = cnt > d.ky ? d.ky : cnt;
        cnt = cnt > d.H - ymin ? d.H - ymin : cnt;
        cnt = cnt < 0 ? 0 : cnt;
      }
      s_ymin[t] = ymin;
      s_ycnt[t] = cnt;
    }
    __syncthreads();
    int lo = d.H, hi = 0;  // source rows [lo, hi) the tile's vertical taps reach
#pragma unroll
    for (int i = 0; i < kTileH; ++i) {
      if (s_ycnt[i] > 0) {
        lo = s_ymin[i] < lo ? s_ymin[i] : lo;
        hi = s_ymin[i] + s_ycnt[i] > hi ? s_ymin[i] + s_ycnt[i] : hi;
      }
    }

    // the horizontal pass's view of this thread: column hx of the tile, rows hr, hr + 2, ... of the chunk
    const int hx = t & (kTileW - 1), hr = t >> 7;
    const bool hvalid = tx0 + hx < d.cw;
    int xmin = 0, xcnt = 0;
    const int32_t* kcol = tab;
    int kreg[kRegTaps];
    if (hvalid) {
      const int gx = d.x0 + tx0 + hx;
      xmin = tab[d.tx + 2 * gx];
      xcnt = tab[d.tx + 2 * gx + 1];
      xmin = xmin < 0 ? 0 : (xmin >= d.W ? d.W - 1 : xmin);
      xcnt = xcnt > d.kx ? d.kx : xcnt;
      xcnt = xcnt > d.W - xmin ? d.W - xmin : xcnt;
      xcnt = xcnt < 0 ? 0 : xcnt;
      kcol = tab + d.cx + (int64_t)gx * d.kx;
    }
#pragma unroll
    for (int j = 0; j < kRegTaps; ++j) kreg[j] = j < xcnt ? kcol[j] : 0;
    // byte offset of tap j's pixel in a stored row: mirrored when flipped
    const int first = d.flip ? (d.W - 1 - xmin) * 3 : xmin * 3;
    const int step = d.flip ? -3 : 3;
    const uint8_t* img = in + d.in_off;

    for (int r0 = lo; r0 < hi; r0 += kChunk) {
      const int R = hi - r0 < kChunk ? hi - r0 : kChunk;
      if (hvalid) {
        for (int rr = hr; rr < R; rr += kThreads / kTileW) {
          const uint8_t* p = img + (int64_t)(r0 + rr) * d.W * 3 + first;
          int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
          if (xcnt <= kRegTaps) {
#pragma unroll
            for (int j = 0; j < kRegTaps; ++j) {
              if (j < xcnt) {
                const uint8_t* q = p + j * step;
                s0 += kreg[j] * q[0];
                s1 += kreg[j] * q[1];
                s2 += kreg[j] * q[2];
              }
            }
          } else {
            for (int j = 0; j < xcnt; ++j) {
              const int c = kcol[j];
              const uint8_t* q = p + j * step;
              s0 += c * q[0];
              s1 += c * q[1];
              s2 += c * q[2];
            }
          }
          s_px[0][rr][hx] = clip8(s0);
          s_px[1][rr][hx] = clip8(s1);
          s_px[2][rr][hx] = clip8(s2);
        }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int oy = vy + 8 * r;
        const int ymin = s_ymin[oy], cnt = s_ycnt[oy];
        if (cnt > 0 && tx0 + vx < d.cw) {
          const int32_t* krow = tab + d.cy + (int64_t)(d.y0 + ty0 + oy) * d.ky;
          int j0 = r0 - ymin, j1 = r0 + R - ymin;  // taps of this row that fall into the chunk
          j0 = j0 < 0 ? 0 : j0;
          j1 = j1 > cnt ? cnt : j1;
          for (int j = j0; j < j1; ++j) {
            const int c = krow[j];
            const int rr = ymin + j - r0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              const uint32_t wd = *reinterpret_cast<const uint32_t*>(&s_px[ch][rr][vx]);
              acc[r][ch][0] += c * (int)(wd & 255u);
              acc[r][ch][1] += c * (int)((wd >> 8) & 255u);
              acc[r][ch][2] += c * (int)((wd >> 16) & 255u);
              acc[r][ch][3] += c * (int)(wd >> 24);
            }
          }
        }
      }
      __syncthreads();  // the next chunk overwrites s_px
    }
  }

  // store: lookup inside the window, zeros and mask 0 outside
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int y = ty0 + vy + 8 * r, x = tx0 + vx;
    if (y >= Hp || x >= Wp) continue;
    float v[3][4];
    int inside[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      inside[i] = (has_pixels && y < d.ch && x + i < d.cw) ? 1 : 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c][i] = inside[i] ? s_lut[c * 256 + clip8(acc[r][c][i])] : 0.f;
    }
    const int64_t p = (int64_t)y * Wp + x;
    store_row<kVec>(obase + p, mbase + p, plane, v, inside, x, Wp);
  }
}

struct AugLabDesc {
  int64_t in_off;  // first element of the map in the packed input
  int H, W, h, w;
  int xi, yi;      // offsets of the w column and h row source indices in the index table
  int flip, y0, x0, ch, cw;
};

struct AugLabArgs {
  AugLabDesc d[kAugMaxImages];
};

// four consecutive pixels of one padded output row per thread
template <typename T, bool kVec>
__global__ __launch_bounds__(kThreads) void augment_labels_kernel(const T* __restrict__ in, const int32_t* __restrict__ tab,
                                                                  int32_t* __restrict__ out, uint8_t* __restrict__ present,
                                                                  int Hp, int Wp, int ignore_index, const AugLabArgs args) {
  const AugLabDesc& d = args.d[blockIdx.z];
  const int x = (blockIdx.x * kThreads + threadIdx.x) * 4;
  const int y = blockIdx.y;
  if (x >= Wp) return;
  int v[4] = {ignore_index, ignore_index, ignore_index, ignore_index};
  if (y < d.ch) {
    int ys = tab[d.yi + d.y0 + y];
    ys = ys < 0 ? 0 : (ys >= d.H ? d.H - 1 : ys);
    const T* row = in + d.in_off + (int64_t)ys * d.W;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (x + i < d.cw) {
        int xs = tab[d.xi + d.x0 + x + i];
        xs = xs < 0 ? 0 : (xs >= d.W ? d.W - 1 : xs);
        xs = d.flip ? d.W - 1 - xs : xs;
        v[i] = (int)row[xs];
        if (v[i] >= 0 && v[i] < 256 && !present[blockIdx.z * 256 + v[i]])
          present[blockIdx.z * 256 + v[i]] = 1;  // benign race: all write 1
      }
    }
  }
  int32_t* o = out + (int64_t)blockIdx.z * Hp * Wp + (int64_t)y * Wp + x;
  if (kVec) {
    *reinterpret_cast<int4*>(o) = make_int4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x + i < Wp) o[i] = v[i];
  }
}

// the window and virtual-frame checks both entry points share; r points at (flip, y0, x0, ch, cw)
int check_window(const char* who, int b, const int64_t* r, int64_t h, int64_t w, int Hp, int Wp) {
  if (h > WM2F_AUG_MAX_VIRTUAL || w > WM2F_AUG_MAX_VIRTUAL) {
    set_error("%s: image %d: resized frame (%lld, %lld) exceeds the built bound (sides <= %d)", who, b, (long long)h,
              (long long)w, WM2F_AUG_MAX_VIRTUAL);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(r[0] == 0 || r[0] == 1, "%s: image %d: flip must be 0 or 1, got %lld", who, b, (long long)r[0]);
  WM2F_REQUIRE(r[1] >= 0 && r[2] >= 0 && r[3] > 0 && r[4] > 0 && r[1] + r[3] <= h && r[2] + r[4] <= w,
               "%s: image %d: window origin (%lld, %lld) size (%lld, %lld) outside the (%lld, %lld) frame", who, b,
               (long long)r[1], (long long)r[2], (long long)r[3], (long long)r[4], (long long)h, (long long)w);
  WM2F_REQUIRE(r[3] <= Hp && r[4] <= Wp, "%s: image %d: window (%lld, %lld) larger than the padded size", who, b,
               (long long)r[3], (long long)r[4]);
  return WM2F_OK;
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_augment_resize_normalize_u8(const uint8_t* images, int64_t images_bytes, const int64_t* desc,
                                                const int32_t* tables, int64_t n_table, const float* lut,
                                                float* pixel_values, int64_t* pixel_mask, int B, int Hp, int Wp,
                                                void* stream) {
  const char* who = "wm2f_augment_resize_normalize_u8";
  WM2F_REQUIRE(images && desc && tables && lut && pixel_values && pixel_mask, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && Hp > 0 && Wp > 0, "%s: need B, Hp, Wp > 0", who);
  if (B > kAugMaxImages || Hp > WM2F_PRE_MAX_SIDE || Wp > WM2F_PRE_MAX_SIDE) {
    set_error("%s: B = %d, (Hp, Wp) = (%d, %d) exceed the built bounds (B <= %d, sides <= %d)", who, B, Hp, Wp,
              kAugMaxImages, WM2F_PRE_MAX_SIDE);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(n_table > 0 && n_table < INT32_MAX, "%s: bad table size", who);
  AugArgs a;
  for (int b = 0; b < B; ++b) {
    const int64_t* r = desc + (int64_t)b * WM2F_AUG_PRE_DESC_LEN;
    AugDesc& d = a.d[b];
    WM2F_REQUIRE(r[1] > 0 && r[2] > 0 && r[3] > 0 && r[4] > 0, "%s: image %d: bad size (%lld, %lld) -> (%lld, %lld)", who,
                 b, (long long)r[1], (long long)r[2], (long long)r[3], (long long)r[4]);
    if (r[1] > WM2F_PRE_MAX_SIDE || r[2] > WM2F_PRE_MAX_SIDE) {
      set_error("%s: image %d: source (%lld, %lld) exceeds the built bound (sides <= %d)", who, b, (long long)r[1],
                (long long)r[2], WM2F_PRE_MAX_SIDE);
      return WM2F_EUNSUPPORTED;
    }
    const int rc = check_window(who, b, r + 11, r[3], r[4], Hp, Wp);
    if (rc != WM2F_OK) return rc;
    d.in_off = r[0];
    d.H = (int)r[1], d.W = (int)r[2], d.h = (int)r[3], d.w = (int)r[4];
    WM2F_REQUIRE(r[0] >= 0 && r[0] + (int64_t)d.H * d.W * 3 <= images_bytes, "%s: image %d: outside the input", who, b);
    WM2F_REQUIRE(r[7] > 0 && r[10] > 0 && r[7] <= WM2F_PRE_MAX_SIDE && r[10] <= WM2F_PRE_MAX_SIDE && r[5] >= 0 &&
                     r[6] >= 0 && r[8] >= 0 && r[9] >= 0 && r[5] + 2 * r[4] <= n_table && r[6] + r[4] * r[7] <= n_table &&
                     r[8] + 2 * r[3] <= n_table && r[9] + r[3] * r[10] <= n_table,
                 "%s: image %d: table offsets outside the table", who, b);
    d.tx = (int)r[5], d.cx = (int)r[6], d.kx = (int)r[7], d.ty = (int)r[8], d.cy = (int)r[9], d.ky = (int)r[10];
    d.flip = (int)r[11], d.y0 = (int)r[12], d.x0 = (int)r[13], d.ch = (int)r[14], d.cw = (int)r[15];
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div(Wp, kTileW), (unsigned)ceil_div(Hp, kTileH), (unsigned)B);
  if (Wp % 4 == 0)
    hipLaunchKernelGGL(augment_image_kernel<true>, grid, dim3(kThreads), 0, s, images, tables, lut, pixel_values,
                       pixel_mask, Hp, Wp, a);
  else
    hipLaunchKernelGGL(augment_image_kernel<false>, grid, dim3(kThreads), 0, s, images, tables, lut, pixel_values,
                       pixel_mask, Hp, Wp, a);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_augment_nearest_labels(const void* maps, int dtype, int64_t n_map_elems, const int64_t* desc,
                                           const int32_t* tables, int64_t n_table, int32_t* out, uint8_t* present, int B,
                                           int Hp, int Wp, int ignore_index, void* stream) {
  const char* who = "wm2f_augment_nearest_labels";
  WM2F_REQUIRE(maps && desc && tables && out && present, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && Hp > 0 && Wp > 0, "%s: need B, Hp, Wp > 0", who);
  if (dtype != WM2F_U8 && dtype != WM2F_I32) {
    set_error("%s: dtype %d not built (WM2F_U8 or WM2F_I32)", who, dtype);
    return WM2F_EUNSUPPORTED;
  }
  if (B > kAugMaxImages || Hp > WM2F_PRE_MAX_SIDE || Wp > WM2F_PRE_MAX_SIDE) {
    set_error("%s: B = %d, (Hp, Wp) = (%d, %d) exceed the built bounds (B <= %d, sides <= %d)", who, B, Hp, Wp,
              kAugMaxImages, WM2F_PRE_MAX_SIDE);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(n_table > 0 && n_table < INT32_MAX, "%s: bad table size", who);
  AugLabArgs a;
  for (int b = 0; b < B; ++b) {
    const int64_t* r = desc + (int64_t)b * WM2F_AUG_LAB_DESC_LEN;
    AugLabDesc& d = a.d[b];
    WM2F_REQUIRE(r[0] >= 0 && r[1] > 0 && r[2] > 0 && r[3] > 0 && r[4] > 0, "%s: image %d: bad size", who, b);
    if (r[1] > WM2F_PRE_MAX_SIDE || r[2] > WM2F_PRE_MAX_SIDE) {
      set_error("%s: image %d: source (%lld, %lld) exceeds the built bound (sides <= %d)", who, b, (long long)r[1],
                (long long)r[2], WM2F_PRE_MAX_SIDE);
      return WM2F_EUNSUPPORTED;
    }
    const int rc = check_window(who, b, r + 7, r[3], r[4], Hp, Wp);
    if (rc != WM2F_OK) return rc;
    d.in_off = r[0];
    d.H = (int)r[1], d.W = (int)r[2], d.h = (int)r[3], d.w = (int)r[4], d.xi = (int)r[5], d.yi = (int)r[6];
    d.flip = (int)r[7], d.y0 = (int)r[8], d.x0 = (int)r[9], d.ch = (int)r[10], d.cw = (int)r[11];
    WM2F_REQUIRE(r[0] + (int64_t)d.H * d.W <= n_map_elems, "%s: image %d: outside the input", who, b);
    WM2F_REQUIRE(r[5] >= 0 && r[6] >= 0 && r[5] + r[4] <= n_table && r[6] + r[3] <= n_table,
                 "%s: image %d: index table offsets outside the table", who, b);
  }
  hipStream_t s = (hipStream_t)stream;
  WM2F_REQUIRE(hipMemsetAsync(present, 0, (size_t)B * 256, s) == hipSuccess, "%s: clearing the flags failed", who);
  const dim3 grid((unsigned)ceil_div(ceil_div(Wp, 4), kThreads), (unsigned)Hp, (unsigned)B);
  const bool vec = Wp % 4 == 0;
#define WM2F_AUG_LAB_LAUNCH(T, V)                                                                                   \
  hipLaunchKernelGGL((augment_labels_kernel<T, V>), grid, dim3(kThreads), 0, s, (const T*)maps, tables, out, present, \
                     Hp, Wp, ignore_index, a)
  if (dtype == WM2F_U8) {
    if (vec) WM2F_AUG_LAB_LAUNCH(uint8_t, true); else WM2F_AUG_LAB_LAUNCH(uint8_t, false);
  } else {
    if (vec) WM2F_AUG_LAB_LAUNCH(int32_t, true); else WM2F_AUG_LAB_LAUNCH(int32_t, false);
  }
#undef WM2F_AUG_LAB_LAUNCH
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
