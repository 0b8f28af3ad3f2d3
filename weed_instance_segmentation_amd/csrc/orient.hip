// Orientation augmentation on the device: vertical flip, quarter turns and rotation by any angle of
// packed uint8 HWC RGB images and of uint8 / int32 id maps, out of place, byte for byte what Pillow 12.2 makes of
// transpose(FLIP_TOP_BOTTOM), transpose(ROTATE_90 / 180 / 270) and rotate(angle, BILINEAR or NEAREST, expand=False,
// fillcolor).  The arithmetic is the contract comment of include/wm2f.h.
//
// orient_kernel<BPP>: one launch for the whole batch, BPP = bytes per pixel (3: image, bilinear; 1 and 4: id maps,
// nearest).  A workgroup owns a 64 x 64 tile of the output frame and builds it in LDS in the output's layout:
//   flips and turns (affine = 0): the tile's source footprint is a 64 x 64 rectangle of the stored image.  Its rows are
//     read as contiguous runs and every byte is put at its turned place in LDS (the transpose happens there; the LDS row
//     stride is an odd number of dwords, so a column of the tile spreads over the banks);
//   rotation (affine = 1): one thread per output pixel, sixteen pixels per thread.  The source coordinate is computed
//     once, in float64 (image) or 16.16 fixed point (map), and the three channels come from the same four taps.  A
//     rotated 64 x 64 tile reads a compact patch of at most 92 x 92 source pixels, which L1 and L2 serve.  The flip and
//     the turn are folded into the tap's address, so a rotation after a turn is still one pass.
//   Then the tile's rows are written as contiguous runs.
// Access: a 3-byte pixel row starts at any byte.  Runs are read and written as aligned dwords where a dword lies wholly
// inside the run, and byte by byte at its two ends (the head / tail rule of photometric.hip, per run instead of per
// image); nothing outside an image is read or written.
//
// The rotation must not be fused: Pillow rounds every product before the sum.  Contraction is switched off for the whole
// file, by the pragma below and by -ffp-contract=off in _build.py.
#include "common.h"

#pragma clang fp contract(off)

namespace wm2f {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;
constexpr int kOrientMaxImages = WM2F_PRE_MAX_IMAGES;
constexpr int kRunDwords = kTile + 1;  // dwords a source run can touch: 64 * 4 bytes aligned, or 64 * 3 + 3 + 3 bytes
constexpr int kRowItems = kTile + 2;   // work items of an output row: the head, up to 64 body dwords, the tail

struct OrientDesc {
  int64_t in_off, out_off;  // first byte of the stored image and of its output
  int H, W;                 // stored size
  int vflip, turns, affine;
  uint32_t fill;            // r | g << 8 | b << 16, or the id
  int64_t c[6];             // float64 bit patterns of the matrix (image) or the 16.16 terms (map)
};

struct OrientArgs {
  OrientDesc d[kOrientMaxImages];
};

// the turned frame and where its pixel (xt, yt) is stored: xs = cx0 + cxx xt + cxy yt, ys = cy0 + cyx xt + cyy yt
struct TurnMap {
  int Ho, Wo;
  int cx0, cxx, cxy, cy0, cyx, cyy;
};

__device__ __forceinline__ TurnMap turn_map(const OrientDesc& d) {
  TurnMap m;
  const int H = d.H, W = d.W;
  m.Ho = (d.turns & 1) ? W : H;
  m.Wo = (d.turns & 1) ? H : W;
  switch (d.turns) {
    case 0: m.cx0 = 0, m.cxx = 1, m.cxy = 0, m.cy0 = 0, m.cyx = 0, m.cyy = 1; break;
    case 1: m.cx0 = W - 1, m.cxx = 0, m.cxy = -1, m.cy0 = 0, m.cyx = 1, m.cyy = 0; break;
    case 2: m.cx0 = W - 1, m.cxx = -1, m.cxy = 0, m.cy0 = H - 1, m.cyx = 0, m.cyy = -1; break;
    default: m.cx0 = 0, m.cxx = 0, m.cxy = 1, m.cy0 = H - 1, m.cyx = -1, m.cyy = 0; break;
  }
  if (d.vflip) m.cy0 = H - 1 - m.cy0, m.cyx = -m.cyx, m.cyy = -m.cyy;  // the flip comes first: it acts on the stored rows
  return m;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int BPP>
__global__ __launch_bounds__(kThreads) void orient_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          const OrientArgs args) {
  constexpr int kStride = kTile * BPP + 4;  // bytes; 49, 17 or 65 dwords
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[kTile * kStride];

  const OrientDesc& d = args.d[blockIdx.z];
  const TurnMap tm = turn_map(d);
  const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
  if (tx0 >= tm.Wo || ty0 >= tm.Ho) return;  // block-uniform
  const int tw = tm.Wo - tx0 < kTile ? tm.Wo - tx0 : kTile, th = tm.Ho - ty0 < kTile ? tm.Ho - ty0 : kTile;
  const int t = threadIdx.x;
  const int W = d.W;
  const uint8_t* img = src + d.in_off;

  if (d.affine) {
    // element index of turned pixel (xt, yt) in the stored image: e0 + sx xt + sy yt
    const int e0 = tm.cy0 * W + tm.cx0, sx = tm.cyx * W + tm.cxx, sy = tm.cyy * W + tm.cxy;
    const int lx = t & (kTile - 1), x = tx0 + lx;
    if (x < tm.Wo) {
      for (int ly = t >> 6; ly < th; ly += kThreads / kTile) {
        const int y = ty0 + ly;
        uint8_t* o = s_tile + ly * kStride + lx * BPP;
        if constexpr (BPP == 3) {
          const double xi = (double)x + 0.5, yi = (double)y + 0.5;
          double xin = __longlong_as_double(d.c[0]) * xi + __longlong_as_double(d.c[1]) * yi + __longlong_as_double(d.c[2]);
          double yin = __longlong_as_double(d.c[3]) * xi + __longlong_as_double(d.c[4]) * yi + __longlong_as_double(d.c[5]);
          if (xin < 0.0 || xin >= (double)tm.Wo || yin < 0.0 || yin >= (double)tm.Ho) {
            o[0] = (uint8_t)(d.fill & 255u), o[1] = (uint8_t)((d.fill >> 8) & 255u), o[2] = (uint8_t)((d.fill >> 16) & 255u);
            continue;
          }
          xin -= 0.5, yin -= 0.5;
          const double fx = floor(xin), fy = floor(yin);
          const double dx = xin - fx, dy = yin - fy;
          const int X = (int)fx, Y = (int)fy;  // -1 .. Wo - 1, -1 .. Ho - 1
          const int x0 = clampi(X, 0, tm.Wo - 1), x1 = clampi(X + 1, 0, tm.Wo - 1), yc = clampi(Y, 0, tm.Ho - 1);
          const bool two = Y + 1 >= 0 && Y + 1 < tm.Ho;
          const uint8_t* p00 = img + (int64_t)(e0 + sx * x0 + sy * yc) * 3;
          const uint8_t* p01 = img + (int64_t)(e0 + sx * x1 + sy * yc) * 3;
          const uint8_t* p10 = two ? img + (int64_t)(e0 + sx * x0 + sy * (Y + 1)) * 3 : p00;
          const uint8_t* p11 = two ? img + (int64_t)(e0 + sx * x1 + sy * (Y + 1)) * 3 : p01;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double a = (double)p00[c], b = (double)p01[c];
            const double v1 = a + (b - a) * dx;
            double v2 = v1;
            if (two) {
              const double a2 = (double)p10[c], b2 = (double)p11[c];
              v2 = a2 + (b2 - a2) * dx;
            }
            o[c] = (uint8_t)(int)(v1 + (v2 - v1) * dy);
          }
        } else {
          const int64_t xs = (d.c[2] + d.c[1] * y + d.c[0] * x) >> 16, ys = (d.c[5] + d.c[4] * y + d.c[3] * x) >> 16;
          const bool in = xs >= 0 && xs < tm.Wo && ys >= 0 && ys < tm.Ho;
          const int e = in ? e0 + sx * (int)xs + sy * (int)ys : 0;
          if constexpr (BPP == 4)
            *reinterpret_cast<uint32_t*>(o) = in ? reinterpret_cast<const uint32_t*>(img)[e] : d.fill;
          else
            o[0] = in ? img[e] : (uint8_t)d.fill;
        }
      }
    }
  } else {
    // the tile's footprint in the stored image: rows ry0 .. ry0 + rrows - 1, columns rx0 .. rx0 + rcols - 1
    const int xa = tm.cx0 + tm.cxx * tx0 + tm.cxy * ty0, xb = tm.cx0 + tm.cxx * (tx0 + tw - 1) + tm.cxy * (ty0 + th - 1);
    const int ya = tm.cy0 + tm.cyx * tx0 + tm.cyy * ty0, yb = tm.cy0 + tm.cyx * (tx0 + tw - 1) + tm.cyy * (ty0 + th - 1);
    const int rx0 = xa < xb ? xa : xb, rcols = (xa < xb ? xb - xa : xa - xb) + 1;
    const int ry0 = ya < yb ? ya : yb, rrows = (ya < yb ? yb - ya : ya - yb) + 1;
    const int n = rcols * BPP;
    for (int idx = t; idx < rrows * kRunDwords; idx += kThreads) {
      const int k = idx / kRunDwords, j = idx - k * kRunDwords;
      const uint8_t* run = img + ((int64_t)(ry0 + k) * W + rx0) * BPP;
      const int lo = 4 * j - (int)(reinterpret_cast<uintptr_t>(run) & 3u);  // the dword's first byte, counted in the run
      if (lo >= n) continue;
      uint32_t w = 0;
      if (lo >= 0 && lo + 4 <= n) {
        w = *reinterpret_cast<const uint32_t*>(run + lo);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (lo + b >= 0 && lo + b < n) w |= (uint32_t)run[lo + b] << (8 * b);
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = lo + b;
        if (i < 0 || i >= n) continue;
        const int p = i / BPP, c = i - p * BPP;
        const int ux = rx0 + p - tm.cx0, uy = ry0 + k - tm.cy0;
        // the map is a signed permutation: its inverse is its transpose
        const int xt = tm.cxx * ux + tm.cyx * uy, yt = tm.cxy * ux + tm.cyy * uy;
        s_tile[(yt - ty0) * kStride + (xt - tx0) * BPP + c] = (uint8_t)((w >> (8 * b)) & 255u);
      }
    }
  }
  __syncthreads();

  // the tile's rows go out as contiguous runs: bytes up to the first 4-byte boundary, aligned dwords, bytes behind them
  uint8_t* out = dst + d.out_off;
  const int n = tw * BPP;
  for (int idx = t; idx < th * kRowItems; idx += kThreads) {
    const int r = idx / kRowItems, j = idx - r * kRowItems;
    uint8_t* row = out + ((int64_t)(ty0 + r) * tm.Wo + tx0) * BPP;
    const uint8_t* s = s_tile + r * kStride;
    int head = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 3u)) & 3u);
    head = head < n ? head : n;
    const int nb = (n - head) >> 2, tail = (n - head) & 3;
    if (j == 0) {
      for (int b = 0; b < head; ++b) row[b] = s[b];
    } else if (j <= nb) {
      const int o = head + 4 * (j - 1);
      *reinterpret_cast<uint32_t*>(row + o) =
          (uint32_t)s[o] | ((uint32_t)s[o + 1] << 8) | ((uint32_t)s[o + 2] << 16) | ((uint32_t)s[o + 3] << 24);
    } else if (j == kRowItems - 1) {
      const int o = head + 4 * nb;
      for (int b = 0; b < tail; ++b) row[o + b] = s[o + b];
    }
  }
}

bool finite_bits(int64_t bits) { return (((uint64_t)bits >> 52) & 0x7ffu) != 0x7ffu; }

// the checks and the launch of all three entry points.  Images count in_off, out_off and the two sizes in bytes (a pixel
// is three of them), maps count them in elements.
template <int BPP>
int orient_launch(const char* who, const void* src, int64_t src_count, void* dst, int64_t dst_count, const int64_t* desc,
                  int B, void* stream) {
  constexpr int64_t kPix = BPP == 3 ? 3 : 1;     // counted units per pixel
  constexpr int64_t kUnit = BPP == 3 ? 1 : BPP;  // bytes per counted unit
  WM2F_REQUIRE(src && dst && desc, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && src_count > 0 && dst_count > 0, "%s: need B > 0 and non-empty buffers", who);
  if (B > kOrientMaxImages) {
    set_error("%s: B = %d exceeds the built bound (B <= %d)", who, B, kOrientMaxImages);
    return WM2F_EUNSUPPORTED;
  }
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
  WM2F_REQUIRE(s0 % kUnit == 0 && d0 % kUnit == 0, "%s: pointers must be aligned to the element", who);
  WM2F_REQUIRE(s0 + (uint64_t)(src_count * kUnit) <= d0 || d0 + (uint64_t)(dst_count * kUnit) <= s0,
               "%s: src and dst overlap (the call is out of place)", who);
  OrientArgs a = {};
  int64_t lo[kOrientMaxImages], hi[kOrientMaxImages];
  int max_h = 0, max_w = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t* r = desc + (int64_t)b * WM2F_ORIENT_DESC_LEN;
    WM2F_REQUIRE(r[1] > 0 && r[2] > 0, "%s: image %d: bad size (%lld, %lld)", who, b, (long long)r[1], (long long)r[2]);
    if (r[1] > WM2F_PRE_MAX_SIDE || r[2] > WM2F_PRE_MAX_SIDE) {
      set_error("%s: image %d: (%lld, %lld) exceeds the built bound (sides <= %d)", who, b, (long long)r[1],
                (long long)r[2], WM2F_PRE_MAX_SIDE);
      return WM2F_EUNSUPPORTED;
    }
    const int64_t count = r[1] * r[2] * kPix;
    WM2F_REQUIRE(r[0] >= 0 && r[0] <= src_count && count <= src_count - r[0], "%s: image %d: outside the input", who, b);
    WM2F_REQUIRE(r[3] >= 0 && r[3] <= dst_count && count <= dst_count - r[3], "%s: image %d: outside the output", who, b);
    lo[b] = r[3], hi[b] = r[3] + count;
    for (int o = 0; o < b; ++o)
      WM2F_REQUIRE(hi[o] <= lo[b] || hi[b] <= lo[o], "%s: the outputs of images %d and %d overlap", who, o, b);
    WM2F_REQUIRE(r[4] == 0 || r[4] == 1, "%s: image %d: vflip must be 0 or 1, got %lld", who, b, (long long)r[4]);
    WM2F_REQUIRE(r[5] >= 0 && r[5] <= 3, "%s: image %d: turns = %lld, expected 0 .. 3", who, b, (long long)r[5]);
    WM2F_REQUIRE(r[6] == 0 || r[6] == 1, "%s: image %d: affine must be 0 or 1, got %lld", who, b, (long long)r[6]);
    OrientDesc& d = a.d[b];
    d.in_off = r[0] * kUnit, d.out_off = r[3] * kUnit;
    d.H = (int)r[1], d.W = (int)r[2], d.vflip = (int)r[4], d.turns = (int)r[5], d.affine = (int)r[6];
    if (BPP == 3) {
      for (int k = 0; k < 3; ++k)
        WM2F_REQUIRE(r[19 + k] >= 0 && r[19 + k] <= 255, "%s: image %d: fill byte %d = %lld, expected 0 .. 255", who, b, k,
                     (long long)r[19 + k]);
      d.fill = (uint32_t)r[19] | ((uint32_t)r[20] << 8) | ((uint32_t)r[21] << 16);
    } else {
      WM2F_REQUIRE(BPP == 1 ? (r[19] >= 0 && r[19] <= 255) : (r[19] >= INT32_MIN && r[19] <= INT32_MAX),
                   "%s: image %d: the fill id %lld does not fit the map's type", who, b, (long long)r[19]);
      d.fill = (uint32_t)r[19];
    }
    for (int k = 0; k < 6 && d.affine; ++k) {
      if (BPP == 3) {
        WM2F_REQUIRE(finite_bits(r[7 + k]), "%s: image %d: matrix entry %d is not finite", who, b, k);
        d.c[k] = r[7 + k];
      } else {
        WM2F_REQUIRE(r[13 + k] >= INT32_MIN && r[13 + k] <= INT32_MAX, "%s: image %d: fixed-point term %d leaves int32", who,
                     b, k);
        d.c[k] = r[13 + k];
      }
    }
    const int Ho = (d.turns & 1) ? d.W : d.H, Wo = (d.turns & 1) ? d.H : d.W;
    max_h = Ho > max_h ? Ho : max_h;
    max_w = Wo > max_w ? Wo : max_w;
  }
  const dim3 grid((unsigned)ceil_div(max_w, kTile), (unsigned)ceil_div(max_h, kTile), (unsigned)B);
  hipLaunchKernelGGL(orient_kernel<BPP>, grid, dim3(kThreads), 0, (hipStream_t)stream, static_cast<const uint8_t*>(src),
                     static_cast<uint8_t*>(dst), a);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_orient_u8(const uint8_t* src, int64_t src_bytes, uint8_t* dst, int64_t dst_bytes, const int64_t* desc,
                              int B, void* stream) {
  return orient_launch<3>("wm2f_orient_u8", src, src_bytes, dst, dst_bytes, desc, B, stream);
}

extern "C" int wm2f_orient_labels_u8(const uint8_t* src, int64_t src_elems, uint8_t* dst, int64_t dst_elems,
                                     const int64_t* desc, int B, void* stream) {
  return orient_launch<1>("wm2f_orient_labels_u8", src, src_elems, dst, dst_elems, desc, B, stream);
}

extern "C" int wm2f_orient_labels_i32(const int32_t* src, int64_t src_elems, int32_t* dst, int64_t dst_elems,
                                      const int64_t* desc, int B, void* stream) {
  return orient_launch<4>("wm2f_orient_labels_i32", src, src_elems, dst, dst_elems, desc, B, stream);
}
