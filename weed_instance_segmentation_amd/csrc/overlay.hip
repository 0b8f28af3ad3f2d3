// Segmentation overlays and contours on the device: B pictures and their id maps -> the pictures with
// every listed segment filled at its alpha and outlined at full colour, in ONE read of picture and map whatever the
// number of segments.  The semantics are written out in include/wm2f.h; tests/overlay_reference.py restates them twice.
//
//   overlay : grid (W / 128, H / 32, B), 256 threads, a tile of 32 rows x 128 pixels per workgroup.
//             1. the image's tables (ids, order, rgba) go to LDS while N <= kOvLdsMaxIds; above it they stay in global
//                memory (L2) and the same code reads them there.
//             2. every pixel of the tile and of its halo (R = max(inner, outer) rows, one quad of 4 columns) is turned
//                into its ENTRY -- the position of its value in the id list, by binary search, with the previous pixel's
//                answer reused along a run -- and stored in LDS as int16: -1 no entry, -2 outside the picture.  Four
//                pixels per lane and load when W % 4 == 0 and the pointers are aligned.
//             3. a lane owns 4 consecutive pixels.  It ORs together the differences between its first entry and the
//                8-byte LDS words that cover its diamond neighbourhood: zero (nearly always) means no contour anywhere
//                on its pixels.  Otherwise it walks the diamond of each pixel and keeps the candidate of greatest
//                order.  Then fill or contour colour, 12 bytes out.
// Everything is integer, nothing is accumulated: bit-identical from run to run.
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kOvThreads = 256;
constexpr int kOvTileW = 128;
constexpr int kOvTileH = 32;
constexpr int kOvMaxR = 4;                              // inner, outer <= 4
constexpr int kOvHaloX = 4;                             // a whole quad each side, so that quads stay aligned
constexpr int kOvStride = kOvTileW + 2 * kOvHaloX;      // 136 entries = 272 B per LDS row (8-byte words stay aligned)
constexpr int kOvRows = kOvTileH + 2 * kOvMaxR;         // 40 rows: 10880 B of entries
constexpr int kOvRowQuads = kOvStride / 4;              // 34
constexpr int kOvQuads = kOvTileW / 4 * kOvTileH / kOvThreads;  // 4 quads per lane
constexpr int kOvLdsMaxIds = 1024;                      // 12 B per entry: 12 KiB, with the tile six workgroups per CU
constexpr int kOvNone = -1;                             // what list_row gives for a value that is not listed
constexpr int kOvOutside = -2;
static_assert(kMapMaxIds <= 32767, "entries are stored as int16");
static_assert(kOvQuads * kOvThreads * 4 == kOvTileW * kOvTileH, "tile / thread mapping");

// entry of a raw map value in the image's ascending id list (n of them), kOvNone when it is not listed
template <int DT>
__device__ __forceinline__ int entry_of(uint32_t raw, const int32_t* ids, int n) {
  int v;
  return map_int<DT>(raw, v) ? list_row(v, ids, n) : kOvNone;
}

__device__ __forceinline__ uint32_t blend8(uint32_t img, uint32_t col, uint32_t a) {
  return (img * (255u - a) + col * a + 127u) / 255u;
}

template <int DT, bool kLds>
__global__ __launch_bounds__(kOvThreads) void overlay_kernel(const uint8_t* __restrict__ image,
                                                             const void* __restrict__ map,
                                                             const int32_t* __restrict__ ids,
                                                             const int32_t* __restrict__ n_ids,
                                                             const uint32_t* __restrict__ rgba,
                                                             const int32_t* __restrict__ order, uint32_t def_rgba,
                                                             int inner, int outer, uint8_t* __restrict__ out, int H,
                                                             int W, int N, int vec) {
  using E = typename MapElem<DT>::type;
  __shared__ __align__(16) int16_t tile[kOvRows * kOvStride];
  __shared__ int32_t tab[kLds ? 3 * kOvLdsMaxIds : 1];
  const int tid = threadIdx.x, b = blockIdx.z;
  const int x0 = blockIdx.x * kOvTileW, y0 = blockIdx.y * kOvTileH;
  const int R = inner > outer ? inner : outer;

  int n = 0;
  if (N > 0) {
    n = n_ids[b];
    n = n < 0 ? 0 : (n > N ? N : n);
  }
  const int32_t* gid = ids + (int64_t)b * N;
  const int32_t* gord = order + (int64_t)b * N;
  const uint32_t* gcol = rgba + (int64_t)b * N;
  if (kLds)
    for (int j = tid; j < n; j += kOvThreads) {
      tab[j] = gid[j];
      tab[kOvLdsMaxIds + j] = gord[j];
      tab[2 * kOvLdsMaxIds + j] = (int32_t)gcol[j];
    }
  const int32_t* sid = kLds ? tab : gid;
  const int32_t* sord = kLds ? tab + kOvLdsMaxIds : gord;
  const uint32_t* scol = kLds ? reinterpret_cast<const uint32_t*>(tab + 2 * kOvLdsMaxIds) : gcol;

  // this lane's pixels of the picture, in flight while the entries are made
  const uint8_t* img = image + (int64_t)b * H * W * 3;
  uint32_t px[kOvQuads][3];
#pragma unroll
  for (int k = 0; k < kOvQuads; ++k) {
    const int q = tid + k * kOvThreads;
    const int y = y0 + (q >> 5), x = x0 + (q & 31) * 4;
    px[k][0] = px[k][1] = px[k][2] = 0u;
    if (y < H && x < W) {
      const uint8_t* p = img + ((int64_t)y * W + x) * 3;
      if (vec) {
        const uint32_t* p4 = reinterpret_cast<const uint32_t*>(p);
        px[k][0] = p4[0];
        px[k][1] = p4[1];
        px[k][2] = p4[2];
      } else {
#pragma unroll
        for (int i = 0; i < 12; ++i)
          if (x + i / 3 < W) px[k][i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
      }
    }
  }
  __syncthreads();  // the tables

  // entries of the tile and its halo
  const E* mp = reinterpret_cast<const E*>(map) + (int64_t)b * H * W;
  const int items = (kOvTileH + 2 * R) * kOvRowQuads;
  for (int it = tid; it < items; it += kOvThreads) {
    const int r = it / kOvRowQuads, c4 = it - r * kOvRowQuads;
    const int gy = y0 - R + r, gx = x0 - kOvHaloX + c4 * 4;
    int e[4] = {kOvOutside, kOvOutside, kOvOutside, kOvOutside};
    if (gy >= 0 && gy < H && gx + 3 >= 0 && gx < W) {
      const E* p = mp + (int64_t)gy * W + gx;
      uint32_t raw[4] = {0u, 0u, 0u, 0u};
      bool in[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) in[j] = gx + j >= 0 && gx + j < W;
      if (vec) {  // gx and W are multiples of 4: the quad is inside as a whole
        load_map4<DT>(p, raw);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (in[j]) raw[j] = (uint32_t)p[j];
      }
      uint32_t last_raw = 0u;
      int last_e = kOvNone;
      bool have = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!in[j]) continue;
        if (!have || raw[j] != last_raw) {
          last_raw = raw[j];
          last_e = entry_of<DT>(raw[j], sid, n);
          have = true;
        }
        e[j] = last_e;
      }
    }
    uint2 w;
    w.x = ((uint32_t)e[0] & 0xffffu) | ((uint32_t)e[1] << 16);
    w.y = ((uint32_t)e[2] & 0xffffu) | ((uint32_t)e[3] << 16);
    *reinterpret_cast<uint2*>(tile + r * kOvStride + c4 * 4) = w;
  }
  __syncthreads();

  uint8_t* dst = out + (int64_t)b * H * W * 3;
#pragma unroll
  for (int k = 0; k < kOvQuads; ++k) {
    const int q = tid + k * kOvThreads;
    const int ly = q >> 5, lx = (q & 31) * 4;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    const int16_t* row = tile + (ly + R) * kOvStride + kOvHaloX + lx;  // the entry of pixel (y, x)
    const uint2 mid = *reinterpret_cast<const uint2*>(row);
    int e[4], cont[4];
    e[0] = (int16_t)(mid.x & 0xffffu);
    e[1] = (int16_t)(mid.x >> 16);
    e[2] = (int16_t)(mid.y & 0xffffu);
    e[3] = (int16_t)(mid.y >> 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) cont[j] = kOvNone;
    if (R > 0) {
      // anything in the words over this lane's neighbourhood that is not its first entry?  (Cells of those words beyond
      // the diamond count too: the answer may only err towards the exact walk.)
      const uint32_t splat = ((uint32_t)e[0] & 0xffffu) * 0x10001u;
      uint32_t diff = (mid.x ^ splat) | (mid.y ^ splat);
      for (int dy = -R; dy <= R; ++dy) {
        const int16_t* r2 = row + dy * kOvStride;
        const uint2 c = *reinterpret_cast<const uint2*>(r2);
        diff |= (c.x ^ splat) | (c.y ^ splat);
        if (R - (dy < 0 ? -dy : dy) > 0) {
          const uint2 l = *reinterpret_cast<const uint2*>(r2 - 4);
          const uint2 rr = *reinterpret_cast<const uint2*>(r2 + 4);
          diff |= (l.x ^ splat) | (l.y ^ splat) | (rr.x ^ splat) | (rr.y ^ splat);
        }
      }
      if (diff != 0u) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (x + j >= W) continue;
          const int ep = e[j];
          int best_o = -1, best_e = kOvNone;
          bool differs_inside = false;
          for (int dy = -R; dy <= R; ++dy) {
            const int ady = dy < 0 ? -dy : dy;
            const int16_t* r2 = row + dy * kOvStride + j;
            for (int dx = ady - R; dx <= R - ady; ++dx) {
              const int eq = r2[dx];
              if (eq == ep || eq == kOvOutside) continue;
              const int d = ady + (dx < 0 ? -dx : dx);
              differs_inside = differs_inside || d <= inner;
              if (d <= outer && eq >= 0) {
                const int o = sord[eq];
                if (o >= 0 && (o > best_o || (o == best_o && eq > best_e))) {
                  best_o = o;
                  best_e = eq;
                }
              }
            }
          }
          if (differs_inside && ep >= 0) {
            const int o = sord[ep];
            if (o >= 0 && (o > best_o || (o == best_o && ep > best_e))) {
              best_o = o;
              best_e = ep;
            }
          }
          cont[j] = best_e;
        }
      }
    }
    uint32_t ow[3] = {0u, 0u, 0u};
    int last_e = kOvOutside;
    uint32_t fill = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e[j] != last_e) {  // a picture pixel is never kOvOutside: the first one always looks its colour up
        last_e = e[j];
        fill = e[j] >= 0 ? scol[e[j]] : def_rgba;
      }
      const bool on = cont[j] >= 0;
      uint32_t c = fill;
      if (on) c = scol[cont[j]];
      const uint32_t a = on ? 255u : c >> 24;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int i = 3 * j + ch;
        const uint32_t v = (px[k][i >> 2] >> (8 * (i & 3))) & 0xffu;
        ow[i >> 2] |= blend8(v, (c >> (8 * ch)) & 0xffu, a) << (8 * (i & 3));
      }
    }
    uint8_t* p = dst + ((int64_t)y * W + x) * 3;
    if (vec) {
      uint32_t* p4 = reinterpret_cast<uint32_t*>(p);
      p4[0] = ow[0];
      p4[1] = ow[1];
      p4[2] = ow[2];
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (x + i / 3 < W) p[i] = (uint8_t)(ow[i >> 2] >> (8 * (i & 3)));
    }
  }
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_labelmap_overlay(const uint8_t* image, const void* map, int dtype, const int32_t* ids,
                                     const int32_t* n_ids, const uint8_t* rgba, const int32_t* order,
                                     uint32_t default_rgba, int inner, int outer, uint8_t* out, int B, int H, int W,
                                     int N, void* stream) {
  const char* who = "wm2f_labelmap_overlay";
  WM2F_REQUIRE(image && map && out, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N >= 0, "%s: bad size", who);
  WM2F_REQUIRE(N == 0 || (ids && n_ids && rgba && order), "%s: N > 0 needs ids, n_ids, rgba and order", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  WM2F_REQUIRE(inner >= 0 && inner <= kOvMaxR && outer >= 0 && outer <= kOvMaxR, "%s: 0 <= inner, outer <= %d", who,
               kOvMaxR);
  WM2F_REQUIRE(reinterpret_cast<uintptr_t>(rgba) % 4 == 0, "%s: rgba must be 4-byte aligned", who);
  if (H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch || N > kMapMaxIds) {
    set_error("%s: sides <= %d, B <= %d, N <= %d (got %d x %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch, kMapMaxIds, H, W,
              B, N);
    return WM2F_EUNSUPPORTED;
  }
  const int64_t bytes = (int64_t)B * H * W * 3;
  const uintptr_t ia = reinterpret_cast<uintptr_t>(image), oa = reinterpret_cast<uintptr_t>(out);
  WM2F_REQUIRE(oa + (uintptr_t)bytes <= ia || ia + (uintptr_t)bytes <= oa,
               "%s: out must not overlap image (neighbours are read)", who);
  hipStream_t s = (hipStream_t)stream;
  const int vec = map_vec4_ok(map, dtype, W) && ia % 4 == 0 && oa % 4 == 0;
  const dim3 grid(ceil_div(W, kOvTileW), ceil_div(H, kOvTileH), B);
  const uint32_t* col = reinterpret_cast<const uint32_t*>(rgba);
  for_map_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kOvThreads), 0, s, image, map, ids, n_ids, col, order, default_rgba, inner, outer,
                         out, H, W, N, vec);
    };
    if (N <= kOvLdsMaxIds) launch(overlay_kernel<DT, true>);
    else launch(overlay_kernel<DT, false>);
  });
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
