// What the kernels that read typed id maps share: the element type of a map, how a raw map value
// becomes an id, the lookup in an ascending id list, the four-pixel load, the common limits, and on the host the checks
// and the dtype dispatch of their entry points.  A (B, H, W) map is fp32, int32 or uint8; a kernel is instantiated per
// dtype DT and reads every value as a uint32_t `raw`: the bits of a float, an int32 as it is, a uint8 zero-extended.
// Device functions, constants and small host helpers only: loops, launches and workspaces stay with the callers.
#pragma once
#include <type_traits>

#include "common.h"

namespace wm2f {

// ---- limits of the id-map entry points ------------------------------------------------------------------------------
constexpr int kMapMaxSide = 16384;
constexpr int kMapMaxBatch = 32;
constexpr int kMapMaxIds = 4096;

// ---- element type ---------------------------------------------------------------------------------------------------
template <int DT>
struct MapElem {
  using type = uint32_t;  // fp32 (its bits) and int32
};
template <>
struct MapElem<WM2F_U8> {
  using type = uint8_t;
};

// ---- decode -----------------------------------------------------------------------------------------------------------
// the integer a float stands for, from its bits: +-0 and exact integers in [1, 2^24); anything else (negative, a
// fraction, 2^24 and above, infinity, NaN) stands for none
__device__ __forceinline__ bool f32_bits_to_int(uint32_t u, int& out) {
  if ((u << 1) == 0u) {
    out = 0;
    return true;
  }
  if (u >> 31) return false;
  const int e = (int)(u >> 23) - 127;
  if (e < 0 || e > 23) return false;
  const uint32_t m = (u & 0x7fffffu) | 0x800000u;
  const int sh = 23 - e;
  if (m & ((1u << sh) - 1u)) return false;
  out = (int)(m >> sh);
  return true;
}

// the integer a raw map value stands for; false for a float that stands for none (so never for an integer map, whose
// negative values come through as they are).  Every rule below, and every caller with a rule of its own, starts here.
template <int DT>
__device__ __forceinline__ bool map_int(uint32_t raw, int& v) {
  if (DT == WM2F_F32) return f32_bits_to_int(raw, v);
  v = (int)raw;
  return true;
}

// id or -1, no upper bound.  negative int: -1; >= N: the value; -1 / -1.0f: -1; non-integer float: -1
template <int DT>
__device__ __forceinline__ int map_id(uint32_t raw) {
  int v;
  if (!map_int<DT>(raw, v)) return -1;
  return v < 0 ? -1 : v;
}

// id in [0, N) or -1.  negative int: -1; >= N: -1; -1 / -1.0f: -1; non-integer float: -1
template <int DT>
__device__ __forceinline__ int map_id_below(uint32_t raw, int N) {
  int v;
  if (!map_int<DT>(raw, v)) return -1;
  return (v >= 0 && v < N) ? v : -1;
}

// is the value -1 / -1.0f, the background of the maps that tell it from other values that are no id
template <int DT>
__device__ __forceinline__ bool map_is_background(uint32_t raw) {
  return raw == (DT == WM2F_F32 ? 0xbf800000u : 0xffffffffu);  // never a zero-extended uint8
}

// background, id in [0, N), or out of range.  negative int other than -1: kMapOutOfRange; >= N: kMapOutOfRange;
// -1 / -1.0f: kMapBackground; non-integer float: kMapOutOfRange
constexpr int kMapBackground = -1;
constexpr int kMapOutOfRange = -2;
template <int DT>
__device__ __forceinline__ int map_id_or_code(uint32_t raw, int N) {
  if (map_is_background<DT>(raw)) return kMapBackground;
  int v;
  if (!map_int<DT>(raw, v)) return kMapOutOfRange;
  return (v >= 0 && v < N) ? v : kMapOutOfRange;
}

// ---- list lookup ------------------------------------------------------------------------------------------------------
// the first position of the ascending list ids[0, n) whose id is not below v, n for none
__device__ __forceinline__ int list_lower_bound(int v, const int32_t* ids, int n) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// position of v in the ascending list ids[0, n), -1 when it is not listed
__device__ __forceinline__ int list_row(int v, const int32_t* ids, int n) {
  const int lo = list_lower_bound(v, ids, n);
  return (lo < n && ids[lo] == v) ? lo : -1;
}

// ---- four-pixel load ----------------------------------------------------------------------------------------------------
// four consecutive pixels in one load: a dword of a uint8 map, 16 bytes of a 4-byte map.  p is aligned to the load
// (map_vec4_ok below and a pixel index that is a multiple of 4)
template <int DT>
__device__ __forceinline__ void load_map4(const typename MapElem<DT>::type* p, uint32_t (&v)[4]) {
  if (DT == WM2F_U8) {
    const uint32_t w4 = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (w4 >> (8 * j)) & 0xffu;
  } else {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    v[0] = q.x;
    v[1] = q.y;
    v[2] = q.z;
    v[3] = q.w;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
#define WM2F_REQUIRE_MAP_DTYPE(dtype, who) \
  WM2F_REQUIRE((dtype) == WM2F_F32 || (dtype) == WM2F_I32 || (dtype) == WM2F_U8, "%s: map must be fp32, int32 or uint8", who)

// f(std::integral_constant<int, DT>{}) for the map's dtype (checked before), and what f returns: a generic lambda that
// launches kernel<decltype(dt)::value> instantiates the kernel for all three
template <class F>
__host__ __forceinline__ auto for_map_dtype(int dtype, F&& f) {
  if (dtype == WM2F_F32) return f(std::integral_constant<int, WM2F_F32>{});
  if (dtype == WM2F_I32) return f(std::integral_constant<int, WM2F_I32>{});
  return f(std::integral_constant<int, WM2F_U8>{});
}

// the same for the entry points that take fp32 and int32 only
template <class F>
__host__ __forceinline__ auto for_map_dtype_f32_i32(int dtype, F&& f) {
  if (dtype == WM2F_F32) return f(std::integral_constant<int, WM2F_F32>{});
  return f(std::integral_constant<int, WM2F_I32>{});
}

__host__ __forceinline__ size_t map_elem_bytes(int dtype) { return dtype == WM2F_U8 ? 1 : 4; }

// may a lane take four pixels of a row in one load: rows are whole quads and the map is aligned to the load
__host__ __forceinline__ bool map_vec4_ok(const void* map, int dtype, int W) {
  return W % 4 == 0 && reinterpret_cast<uintptr_t>(map) % (map_elem_bytes(dtype) * 4) == 0;
}

// rows per chunk of a columns pass (a lane per column, 256-thread workgroups, grid (ceil(W / 256), chunks, B)): about
// kMapColumnWaves waves in all, a chunk of at least min_rows rows and at most the image
constexpr int kMapColumnThreads = 256;
constexpr int kMapColumnWaves = 2048;
__host__ __forceinline__ int column_chunk_rows(int B, int H, int W, int min_rows) {
  const int col_blocks = ceil_div(W, kMapColumnThreads);
  const int want = ceil_div(kMapColumnWaves, B * col_blocks * (kMapColumnThreads / kWave));
  int chunk_rows = ceil_div(H, want);
  chunk_rows = chunk_rows < min_rows ? min_rows : chunk_rows;
  return chunk_rows > H ? H : chunk_rows;
}

// bytes of a (B, H, W) uint16 plane at the head of a workspace, what follows it at a 16-byte boundary
__host__ __forceinline__ int64_t map_g_bytes(int B, int H, int W) { return ((int64_t)B * H * W * 2 + 15) / 16 * 16; }

}  // namespace wm2f
