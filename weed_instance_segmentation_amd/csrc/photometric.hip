// Colour jitter on the device: brightness, contrast, saturation and hue of packed uint8 HWC RGB
// images, in place, byte for byte what Pillow 12.2 makes of ImageEnhance.Brightness / Contrast / Color and of a hue shift
// through convert("HSV") / convert("RGB").  The arithmetic is the contract comment of include/wm2f.h.
//
// photometric_kernel<true>, the sum launch: only for images whose chain holds a contrast step.  Applies the steps in
//   front of it per pixel in registers, adds up L as integers (wave shuffle, LDS across the four waves, one 64-bit vector
//   atomic add per workgroup) into the image's workspace word.  Integer sums do not depend on the schedule.
// photometric_kernel<false>, the apply launch: the whole chain per pixel in registers, the contrast mean formed in
//   float64 from the workspace word, bytes written back where they were read.
//
// Access: an image starts at any byte (in_off is a multiple of 3, not of 4).  The first (address mod 4) pixels are the
// head: after them a pixel starts on a 4-byte boundary, because 3 k = -address (mod 4) has the solution k = address mod 4.
// From there a thread takes four pixels = 12 bytes = three aligned dwords; a wave reads 768 contiguous bytes.  The last
// (npix - head) mod 4 pixels are the tail.  Head and tail go byte by byte, through workgroup 0 of the image.
//
// The blend must not be fused: t = fl32(fl32(d) + fl32(a * fl32(v - d))) rounds the product before the sum.  It is written
// with __fmul_rn / __fadd_rn; those are plain operators in the HIP headers, so contraction is also switched off for the
// whole file, by the pragma below and by -ffp-contract=off in _build.py (the float64 steps of the hue path need it too).
#include "common.h"

#pragma clang fp contract(off)

namespace wm2f {
namespace {

constexpr int kThreads = 256;
constexpr int kPhotoMaxImages = WM2F_PRE_MAX_IMAGES;
constexpr int kMaxOps = 4;
constexpr int kMaxBlocks = 4096;     // per apply launch, over all images: the rest is a grid-stride loop
constexpr int kMaxBlocksSum = 1024;  // per sum launch: every workgroup ends in an atomic add on one of B adjacent words

struct PhotoDesc {
  int64_t in_off;  // first byte of the image in the packed buffer
  int64_t npix;
  int slot;        // the image's workspace word
  int n_ops;       // steps to run: the whole chain (apply) or the steps in front of contrast (sum)
  int has_hue;     // some step to run is a hue step: the workgroup builds the hue tables
  int kind[kMaxOps];
  uint32_t param[kMaxOps];  // float32 bits of the factor, or dh
};

struct PhotoArgs {
  PhotoDesc d[kPhotoMaxImages];
};

// hsv -> rgb reads its byte inputs through tables: (i, f) of H and fs of S take 256 values each, and building them per
// workgroup keeps two float64 divisions out of the per-pixel path.  The arithmetic is the contract's, entry by entry.
struct HueTables {
  float f[256];   // float32(hf - floor(hf)), hf = float64(float32(H)) * 6 / 255
  float fs[256];  // float32(float64(S) / 255)
  uint8_t i[256]; // floor(hf) mod 6
};

__device__ __forceinline__ void build_hue_tables(HueTables& tb, int t) {
  for (int k = t; k < 256; k += kThreads) {
    const double hf = (double)(float)k * 6.0 / 255.0;
    const double fl = floor(hf);
    tb.f[k] = (float)(hf - fl);
    tb.i[k] = (uint8_t)((int)fl % 6);
    tb.fs[k] = (float)((double)k / 255.0);
  }
}

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ __forceinline__ int blend(int d, int v, float a) {
  const float t = __fadd_rn((float)d, __fmul_rn(a, (float)(v - d)));
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ void hue_shift(int& r, int& g, int& b, int dh, const HueTables& tb) {
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
  int H = 0, S = 0;
  const int V = mx;
  if (mx != mn) {
    const float cr = (float)(mx - mn);
    const float s = cr / (float)mx;
    float h;
    if (r == mx) {
      h = (float)(mx - b) / cr - (float)(mx - g) / cr;
    } else if (g == mx) {
      h = (float)(2.0 + (double)((float)(mx - r) / cr) - (double)((float)(mx - b) / cr));
    } else {
      h = (float)(4.0 + (double)((float)(mx - g) / cr) - (double)((float)(mx - r) / cr));
    }
    double x = (double)h / 6.0 + 1.0;  // in [5/6, 11/6): fmod(x, 1) exactly
    x = x >= 1.0 ? x - 1.0 : x;
    H = clip8((int)((double)(float)x * 255.0));
    S = clip8((int)((double)s * 255.0));
  }
  H = (H + dh) & 255;
  if (S == 0) {
    r = g = b = V;
    return;
  }
  const int i = tb.i[H];
  const float f = tb.f[H], fs = tb.fs[S];
  const double v = (double)V;
  const int p = clip8((int)round(v * (1.0 - (double)fs)));
  // odd sextants use q = V (1 - fs f) with fs f a float32 product, even ones t = V (1 - fs (1 - f)) in float64
  const double x = (i & 1) ? (double)__fmul_rn(fs, f) : __dmul_rn((double)fs, 1.0 - (double)f);
  const int w = clip8((int)round(v * (1.0 - x)));
  switch (i) {
    case 0: r = V, g = w, b = p; break;
    case 1: r = w, g = V, b = p; break;
    case 2: r = p, g = V, b = w; break;
    case 3: r = p, g = w, b = V; break;
    case 4: r = w, g = p, b = V; break;
    default: r = V, g = p, b = w; break;
  }
}

// the steps to run, copied once into scalar registers: a step then costs no load inside the pixel loop
struct Chain {
  int n;
  int kind[kMaxOps];
  uint32_t param[kMaxOps];
};

__device__ __forceinline__ Chain chain_of(const PhotoDesc& d) {
  Chain ch;
  ch.n = d.n_ops;
#pragma unroll
  for (int k = 0; k < kMaxOps; ++k) ch.kind[k] = d.kind[k], ch.param[k] = d.param[k];
  return ch;
}

// the chain on N pixels held as bytes r, g, b, r, g, b, ... in registers; `m` is the contrast mean (unused when no step
// is contrast).  Steps outside, pixels inside: the step's kind is wave-uniform (the chain is the image's), and the N
// pixels of a step are independent work for the divisions of the hue path.
template <int N>
__device__ __forceinline__ void run_chain(int (&c)[3 * N], const Chain& ch, int m, const HueTables& tb) {
#pragma unroll 1
  for (int k = 0; k < ch.n; ++k) {
    const int kind = k == 0 ? ch.kind[0] : (k == 1 ? ch.kind[1] : (k == 2 ? ch.kind[2] : ch.kind[3]));
    const uint32_t param = k == 0 ? ch.param[0] : (k == 1 ? ch.param[1] : (k == 2 ? ch.param[2] : ch.param[3]));
    if (kind == WM2F_PHOTO_HUE) {
#pragma unroll
      for (int j = 0; j < N; ++j) hue_shift(c[3 * j], c[3 * j + 1], c[3 * j + 2], (int)param, tb);
    } else {
      const float a = __uint_as_float(param);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int L = luma(c[3 * j], c[3 * j + 1], c[3 * j + 2]);
        const int d = kind == WM2F_PHOTO_SATURATION ? L : (kind == WM2F_PHOTO_CONTRAST ? m : 0);  // brightness: 0
        c[3 * j] = blend(d, c[3 * j], a), c[3 * j + 1] = blend(d, c[3 * j + 1], a), c[3 * j + 2] = blend(d, c[3 * j + 2], a);
      }
    }
  }
}

// the geometry every workgroup of an image shares
struct Span {
  uint8_t* base;   // the image's first byte
  int head;        // pixels in front of the first 4-byte boundary that is also a pixel boundary
  int64_t groups;  // four-pixel groups of the body
  int tail;        // pixels behind the body
};

__device__ __forceinline__ Span span_of(uint8_t* images, const PhotoDesc& d) {
  Span s;
  s.base = images + d.in_off;
  const int mis = (int)(reinterpret_cast<uintptr_t>(s.base) & 3u);
  s.head = (int64_t)mis < d.npix ? mis : (int)d.npix;
  s.groups = (d.npix - s.head) >> 2;
  s.tail = (int)((d.npix - s.head) & 3);
  return s;
}

// kSum: add up L of the chain's prefix; otherwise run the chain and write back
template <bool kSum>
__global__ __launch_bounds__(kThreads) void photometric_kernel(uint8_t* __restrict__ images,
                                                               unsigned long long* __restrict__ sums,
                                                               const PhotoArgs args) {
  __shared__ HueTables s_tb;
  __shared__ unsigned long long s_part[kThreads / kWave];
  const PhotoDesc& d = args.d[blockIdx.y];
  const int t = threadIdx.x;
  const Span sp = span_of(images, d);
  // workgroups the image has no body for leave at once (workgroup 0 stays for the head and the tail)
  if (blockIdx.x > 0 && (int64_t)blockIdx.x * kThreads >= sp.groups) return;
  if (d.has_hue) {
    build_hue_tables(s_tb, t);
    __syncthreads();
  }
  int m = 0;
  if (!kSum) {
    // int(S / (H W) + 0.5) in float64; S < 2^53 and the division is correctly rounded, as Python's
    m = (int)((double)sums[d.slot] / (double)d.npix + 0.5);
  }
  const Chain ch = chain_of(d);
  unsigned long long acc = 0;

  uint8_t* body = sp.base + 3 * sp.head;
  for (int64_t q = (int64_t)blockIdx.x * kThreads + t; q < sp.groups; q += (int64_t)gridDim.x * kThreads) {
    uint32_t* p = reinterpret_cast<uint32_t*>(body + 12 * q);
    uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
    int c[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[j] = (w0 >> (8 * j)) & 255u;
      c[4 + j] = (w1 >> (8 * j)) & 255u;
      c[8 + j] = (w2 >> (8 * j)) & 255u;
    }
    run_chain<4>(c, ch, m, s_tb);
    if (kSum) {
#pragma unroll
      for (int j = 0; j < 4; ++j) acc += (unsigned)luma(c[3 * j], c[3 * j + 1], c[3 * j + 2]);
    }
    if (!kSum) {
      w0 = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
      w1 = (uint32_t)c[4] | ((uint32_t)c[5] << 8) | ((uint32_t)c[6] << 16) | ((uint32_t)c[7] << 24);
      w2 = (uint32_t)c[8] | ((uint32_t)c[9] << 8) | ((uint32_t)c[10] << 16) | ((uint32_t)c[11] << 24);
      p[0] = w0, p[1] = w1, p[2] = w2;
    }
  }

  // head and tail, byte by byte: lanes 0 .. head - 1 of wave 0 and lanes 0 .. tail - 1 of wave 1 of workgroup 0
  if (blockIdx.x == 0) {
    uint8_t* px = nullptr;
    if (t < sp.head) px = sp.base + 3 * t;
    if (t >= kWave && t - kWave < sp.tail) px = body + 12 * sp.groups + 3 * (t - kWave);
    if (px) {
      int c[3] = {px[0], px[1], px[2]};
      run_chain<1>(c, ch, m, s_tb);
      if (kSum) {
        acc += (unsigned)luma(c[0], c[1], c[2]);
      } else {
        px[0] = (uint8_t)c[0], px[1] = (uint8_t)c[1], px[2] = (uint8_t)c[2];
      }
    }
  }

  if (kSum) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) acc += __shfl_down(acc, o, kWave);
    if ((t & (kWave - 1)) == 0) s_part[t / kWave] = acc;
    __syncthreads();
    if (t == 0) {
      unsigned long long s = 0;
#pragma unroll
      for (int w = 0; w < kThreads / kWave; ++w) s += s_part[w];
      atomicAdd(&sums[d.slot], s);
    }
  }
}

unsigned grid_x(int64_t max_npix, int n_images, int max_blocks) {
  const int64_t want = ceil_div64(ceil_div64(max_npix, 4), kThreads);
  const int64_t cap = max_blocks / n_images > 32 ? max_blocks / n_images : 32;
  return (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_photometric_workspace(int B) {
  if (B <= 0 || B > kPhotoMaxImages) return -1;
  return (int64_t)B * (int64_t)sizeof(int64_t);
}

extern "C" int wm2f_photometric_u8(uint8_t* images, int64_t images_bytes, const int64_t* desc, void* workspace, int B,
                                   void* stream) {
  const char* who = "wm2f_photometric_u8";
  WM2F_REQUIRE(images && desc && workspace, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && images_bytes > 0, "%s: need B > 0 and images_bytes > 0", who);
  WM2F_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "%s: workspace must be 8-byte aligned", who);
  if (B > kPhotoMaxImages) {
    set_error("%s: B = %d exceeds the built bound (B <= %d)", who, B, kPhotoMaxImages);
    return WM2F_EUNSUPPORTED;
  }
  PhotoArgs apply = {}, sum = {};
  int n_apply = 0, n_sum = 0;
  int64_t max_apply = 0, max_sum = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t* r = desc + (int64_t)b * WM2F_PHOTO_DESC_LEN;
    WM2F_REQUIRE(r[1] > 0 && r[2] > 0, "%s: image %d: bad size (%lld, %lld)", who, b, (long long)r[1], (long long)r[2]);
    if (r[1] > WM2F_PRE_MAX_SIDE || r[2] > WM2F_PRE_MAX_SIDE) {
      set_error("%s: image %d: (%lld, %lld) exceeds the built bound (sides <= %d)", who, b, (long long)r[1],
                (long long)r[2], WM2F_PRE_MAX_SIDE);
      return WM2F_EUNSUPPORTED;
    }
    const int64_t npix = r[1] * r[2];
    WM2F_REQUIRE(r[0] >= 0 && r[0] <= images_bytes && npix * 3 <= images_bytes - r[0], "%s: image %d: outside the input",
                 who, b);
    WM2F_REQUIRE(r[3] >= 0 && r[3] <= kMaxOps, "%s: image %d: n_ops = %lld, expected 0 .. %d", who, b, (long long)r[3],
                 kMaxOps);
    const int n = (int)r[3];
    if (n == 0) continue;  // untouched, and no workgroup spent on it
    PhotoDesc d = {};
    d.in_off = r[0], d.npix = npix, d.slot = b, d.n_ops = n;
    int seen = 0, contrast_at = -1, hue_at = -1;
    for (int k = 0; k < n; ++k) {
      const int64_t kind = r[4 + 2 * k], param = r[5 + 2 * k];
      WM2F_REQUIRE(kind >= WM2F_PHOTO_BRIGHTNESS && kind <= WM2F_PHOTO_HUE, "%s: image %d: step %d: unknown kind %lld", who,
                   b, k, (long long)kind);
      WM2F_REQUIRE(!(seen & (1 << kind)), "%s: image %d: kind %lld is repeated", who, b, (long long)kind);
      seen |= 1 << kind;
      if (kind == WM2F_PHOTO_HUE) {
        WM2F_REQUIRE(param >= 0 && param <= 255, "%s: image %d: hue dh = %lld, expected 0 .. 255", who, b, (long long)param);
        hue_at = k;
      } else {
        WM2F_REQUIRE(param >= 0 && param <= (int64_t)UINT32_MAX, "%s: image %d: step %d: the factor is not float32 bits",
                     who, b, k);
        const uint32_t bits = (uint32_t)param;
        // finite and not negative: sign clear (or a zero), exponent below all ones
        WM2F_REQUIRE(((bits >> 31) == 0 || (bits << 1) == 0) && ((bits >> 23) & 255u) != 255u,
                     "%s: image %d: step %d: the factor must be finite and >= 0", who, b, k);
        if (kind == WM2F_PHOTO_CONTRAST) contrast_at = k;
      }
      d.kind[k] = (int)kind;
      d.param[k] = (uint32_t)param;
    }
    d.has_hue = hue_at >= 0;
    apply.d[n_apply++] = d;
    max_apply = npix > max_apply ? npix : max_apply;
    if (contrast_at >= 0) {
      d.n_ops = contrast_at;
      d.has_hue = hue_at >= 0 && hue_at < contrast_at;
      sum.d[n_sum++] = d;
      max_sum = npix > max_sum ? npix : max_sum;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  WM2F_REQUIRE(hipMemsetAsync(workspace, 0, (size_t)B * sizeof(int64_t), s) == hipSuccess, "%s: clearing the sums failed",
               who);
  unsigned long long* sums = static_cast<unsigned long long*>(workspace);
  if (n_sum > 0) {
    hipLaunchKernelGGL(photometric_kernel<true>, dim3(grid_x(max_sum, n_sum, kMaxBlocksSum), (unsigned)n_sum),
                       dim3(kThreads), 0, s, images, sums, sum);
    WM2F_CHECK_LAUNCH(who);
  }
  if (n_apply > 0) {
    hipLaunchKernelGGL(photometric_kernel<false>, dim3(grid_x(max_apply, n_apply, kMaxBlocks), (unsigned)n_apply),
                       dim3(kThreads), 0, s, images, sums, apply);
    WM2F_CHECK_LAUNCH(who);
  }
  return WM2F_OK;
}
