// Connected-component labelling of class maps with OpenCV's component numbering: the cv2 steps of
// the reference's dataset loaders (datasets/pheno_bench/dataset.py:48-135, crop_weed dataset_from_png_annotations.py).
//
// Two pixels join when they are 8-neighbours and carry the same nonzero class.  The union-find, the tile geometry and
// the unions across tile borders are labelling.h's, which carries their arguments: the root of a set is the
// smallest linear pixel index in it, whatever the schedule.  Phases are separate kernels (no inter-workgroup hand-off in
// a launch):
//   ccl_local_kernel     nearest resize + class mapping on load, union-find of one 32 x 32 tile in LDS;
//   ccl_merge_kernel     labelling.h's merge step across tile borders (corner diagonals included);
//   ccl_flatten_kernel   every tile root points at its final root (so the per-pixel pass below takes two hops, not a
//                        walk along a chain of tiles);
//   ccl_finalize_kernel  every pixel points at its root; the first 2 x 2 block of each component (atomicMin at its
//                        root) and the compact list of roots;
//   ccl_keys_kernel      the sort key (class, first block) of each root (the sort itself is the caller's);
//   ccl_assign_kernel    ids 1, 2, ... in sorted order (255 skipped on request) written at each root;
//   ccl_paint_kernel     out[p] = id[root(p)], or the background value.
// wm2f_resize_nearest is the plain nearest resize (cv2.resize INTER_NEAREST) through the same index tables.
#include "common.h"
#include "labelling.h"

namespace wm2f {
namespace {

constexpr int kThreads = 256;

struct Colors {
  int n;
  uint8_t rgb[WM2F_CCL_MAX_COLORS * 3];
};

// Workspace carve (include/wm2f.h): parent, class, first block / id, root list, each H * W int32, then the count of
// tile roots (the root list holds the tile roots until the finalize kernel rewrites it with the final roots).
struct Ws {
  int32_t* parent;
  int32_t* cls;
  uint32_t* slot;
  int32_t* roots;
  int32_t* n_tile_roots;
};

__host__ __device__ inline Ws carve(void* ws, int64_t n) {
  int32_t* b = (int32_t*)ws;
  return Ws{b, b + n, (uint32_t*)(b + 2 * n), b + 3 * n, b + 4 * n};
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The class of output pixel (y, x): source pixel (ty[y], tx[x]) (identity without tables) through the mode's mapping.
template <typename T, int kMode>
__device__ __forceinline__ int load_class(const T* __restrict__ src, int src_H, int src_W, const int32_t* __restrict__ ty,
                                          const int32_t* __restrict__ tx, int y, int x, const Colors& colors) {
  const int sy = ty ? clampi(ty[y], src_H - 1) : y;
  const int sx = tx ? clampi(tx[x], src_W - 1) : x;
  if constexpr (kMode == WM2F_CCL_RGB) {
    const uint8_t* px = (const uint8_t*)src + ((int64_t)sy * src_W + sx) * 3;
    const uint8_t r = px[0], g = px[1], b = px[2];
    for (int k = 0; k < colors.n; ++k)
      if (colors.rgb[3 * k] == r && colors.rgb[3 * k + 1] == g && colors.rgb[3 * k + 2] == b) return k + 1;
    return 0;
  } else {
    const int v = (int)src[(int64_t)sy * src_W + sx];
    return kMode == WM2F_CCL_BINARY ? (v != 0) : v;
  }
}

// Local phase: one workgroup per 32 x 32 tile.  Loads (and resizes / classifies) the tile, writes the class map, joins
// 8-neighbours inside the tile in LDS and writes every pixel's tile-local root as a global linear index.  Background
// pixels, and those outside the map (class 0 there too), point at themselves.
template <typename T, int kMode>
__global__ __launch_bounds__(kLabelThreads) void ccl_local_kernel(const T* __restrict__ src, int src_H, int src_W,
                                                                  const int32_t* __restrict__ ty,
                                                                  const int32_t* __restrict__ tx, int H, int W, Ws ws,
                                                                  const Colors colors) {
  __shared__ int32_t s_parent[kLabelTilePx];
  __shared__ int32_t s_cls[kLabelTilePx];
  const int x0 = blockIdx.x * kLabelTile, y0 = blockIdx.y * kLabelTile;
#pragma unroll
  for (int k = 0; k < kLabelRows; ++k) {
    const auto [lx, ly, li] = tile_pixel(k);
    const int y = y0 + ly, x = x0 + lx;
    int c = 0;
    if (y < H && x < W) {
      c = load_class<T, kMode>(src, src_H, src_W, ty, tx, y, x, colors);
      ws.cls[(int64_t)y * W + x] = c;
    }
    s_cls[li] = c;
    s_parent[li] = li;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kLabelRows; ++k) {
    const auto [lx, ly, li] = tile_pixel(k);
    const int c = s_cls[li];
    if (c == 0) continue;  // background, or outside the map (class 0 there too)
    constexpr int kS = __HIP_MEMORY_SCOPE_WORKGROUP;
    if (lx > 0 && s_cls[li - 1] == c) unite<kS>(s_parent, li, li - 1);
    if (ly > 0) {
      if (lx > 0 && s_cls[li - kLabelTile - 1] == c) unite<kS>(s_parent, li, li - kLabelTile - 1);
      if (s_cls[li - kLabelTile] == c) unite<kS>(s_parent, li, li - kLabelTile);
      if (lx < kLabelTile - 1 && s_cls[li - kLabelTile + 1] == c) unite<kS>(s_parent, li, li - kLabelTile + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kLabelRows; ++k) {
    const auto [lx, ly, li] = tile_pixel(k);
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    const int r = find_root<__HIP_MEMORY_SCOPE_WORKGROUP>(s_parent, li);
    const int g = tile_to_image(r, y0, x0, W);
    ws.parent[(int64_t)y * W + x] = g;
    if (r == li && s_cls[li] != 0) ws.roots[atomicAdd(ws.n_tile_roots, 1)] = g;
  }
}

// Merge phase: one thread per pixel on the top row or the left column of a tile (other than the map's own edge), joined
// with its 8-neighbours of the same class in the tile above or to the left by labelling.h's rule.
__global__ __launch_bounds__(kThreads) void ccl_merge_kernel(int H, int W, Ws ws) {
  BorderPixel b;
  if (!border_pixel((int64_t)blockIdx.x * kThreads + threadIdx.x, H, W, b)) return;
  border_unite<8>(ws.cls, ws.parent, H, W, b, [](int c) { return c != 0; });
}

// Every tile root (listed by the local phase) points at its final root; roots are final once the merge kernel has
// ended, so a concurrent write of parent[q] only ever replaces an ancestor with the root.
__global__ __launch_bounds__(kThreads) void ccl_flatten_kernel(int64_t n_max, Ws ws) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_max || i >= *ws.n_tile_roots) return;
  const int q = ws.roots[i];
  ws.parent[q] = find_root<__HIP_MEMORY_SCOPE_AGENT>(ws.parent, q);
}

// Every foreground pixel points at its final root; its 2 x 2 block index goes into the root's slot by atomicMin (the
// slots were filled with 0xFF); each root appends itself to the root list.  Roots are final here (the merge kernel has
// ended), so a concurrent write of parent[p] only ever replaces an ancestor with the root.
__global__ __launch_bounds__(kThreads) void ccl_finalize_kernel(int H, int W, Ws ws, int32_t* __restrict__ count) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  if (ws.cls[p] == 0) return;
  const int r = find_root<__HIP_MEMORY_SCOPE_AGENT>(ws.parent, (int)p);
  ws.parent[p] = r;
  const int y = (int)(p / W), x = (int)(p % W);
  // The root is the component's first pixel in raster order, so no pixel lies on an earlier block row than the root's:
  // only the root's block row competes for the first block (one slot would otherwise take an atomic per pixel).
  if ((y >> 1) == ((r / W) >> 1)) atomicMin(ws.slot + r, (uint32_t)(y >> 1) * (uint32_t)((W + 1) >> 1) + (uint32_t)(x >> 1));
  if (r == p) ws.roots[atomicAdd(count, 1)] = r;
}

// key[i] = class * 2^32 + first block of root i (keys are distinct: same-class pixels of one 2 x 2 block are joined).
__global__ __launch_bounds__(kThreads) void ccl_keys_kernel(int n, Ws ws, int64_t* __restrict__ keys) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int r = ws.roots[i];
  keys[i] = (int64_t)ws.cls[r] * 4294967296LL + (int64_t)ws.slot[r];
}

// The i-th root in key order gets id i + 1 (one more from 255 on when skip_255); its class goes to comp_class[i].
__global__ __launch_bounds__(kThreads) void ccl_assign_kernel(int n, const int64_t* __restrict__ order, int skip_255, Ws ws,
                                                              int32_t* __restrict__ comp_class) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t o = order[i];
  const int r = ws.roots[o < 0 ? 0 : (o >= n ? n - 1 : o)];
  const int id = i + 1 + ((skip_255 && i + 1 >= 255) ? 1 : 0);
  ws.slot[r] = (uint32_t)id;
  if (comp_class) comp_class[i] = ws.cls[r];
}

__global__ __launch_bounds__(kThreads) void ccl_paint_kernel(int64_t n_px, Ws ws, int background, int32_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= n_px) return;
  out[p] = ws.cls[p] == 0 ? background : (int32_t)ws.slot[ws.parent[p]];
}

template <int kBytes>
struct Px {
  uint8_t b[kBytes];
};

template <int kBytes>
__global__ __launch_bounds__(kThreads) void resize_nearest_kernel(const Px<kBytes>* __restrict__ src, int src_H, int src_W,
                                                                  const int32_t* __restrict__ ty,
                                                                  const int32_t* __restrict__ tx, Px<kBytes>* __restrict__ dst,
                                                                  int H, int W) {
  const int x = blockIdx.x * kThreads + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= W) return;
  const int sy = clampi(ty[y], src_H - 1), sx = clampi(tx[x], src_W - 1);
  dst[(int64_t)y * W + x] = src[(int64_t)sy * src_W + sx];
}

template <typename T, int kMode>
void launch_local(const void* src, int src_H, int src_W, const int32_t* ty, const int32_t* tx, int H, int W, const Ws& ws,
                  const Colors& colors, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(W, kLabelTile), (unsigned)ceil_div(H, kLabelTile));
  hipLaunchKernelGGL((ccl_local_kernel<T, kMode>), grid, dim3(kLabelThreads), 0, s, (const T*)src, src_H, src_W, ty, tx,
                     H, W, ws, colors);
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_ccl_workspace(int H, int W) {
  if (H <= 0 || W <= 0 || H > WM2F_PRE_MAX_SIDE || W > WM2F_PRE_MAX_SIDE) return -1;
  return (4 * (int64_t)H * W + 4) * (int64_t)sizeof(int32_t);
}

extern "C" int wm2f_ccl_label(const void* src, int mode, int src_dtype, int src_H, int src_W, const int32_t* ty,
                              const int32_t* tx, const uint8_t* colors, int n_colors, int H, int W, void* workspace,
                              int32_t* count, void* stream) {
  const char* who = "wm2f_ccl_label";
  WM2F_REQUIRE(src && workspace && count, "%s: null pointer", who);
  WM2F_REQUIRE(H > 0 && W > 0 && src_H > 0 && src_W > 0, "%s: need positive sizes", who);
  if (H > WM2F_PRE_MAX_SIDE || W > WM2F_PRE_MAX_SIDE || src_H > WM2F_PRE_MAX_SIDE || src_W > WM2F_PRE_MAX_SIDE) {
    set_error("%s: sides must be <= %d", who, WM2F_PRE_MAX_SIDE);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE((ty == nullptr) == (tx == nullptr), "%s: give both index tables or neither", who);
  WM2F_REQUIRE(ty || (src_H == H && src_W == W), "%s: without index tables the source size must equal (H, W)", who);
  Colors cl;
  cl.n = 0;
  if (mode == WM2F_CCL_RGB) {
    WM2F_REQUIRE(src_dtype == WM2F_U8, "%s: RGB maps are uint8", who);
    WM2F_REQUIRE(colors && n_colors > 0, "%s: RGB mode needs colours", who);
    if (n_colors > WM2F_CCL_MAX_COLORS) {
      set_error("%s: %d colours, at most %d are built", who, n_colors, WM2F_CCL_MAX_COLORS);
      return WM2F_EUNSUPPORTED;
    }
    cl.n = n_colors;
    for (int i = 0; i < 3 * n_colors; ++i) cl.rgb[i] = colors[i];
  } else {
    WM2F_REQUIRE(mode == WM2F_CCL_VALUE || mode == WM2F_CCL_BINARY, "%s: unknown mode %d", who, mode);
    if (src_dtype != WM2F_U8 && src_dtype != WM2F_U16 && src_dtype != WM2F_I32) {
      set_error("%s: dtype %d not built (WM2F_U8, WM2F_U16 or WM2F_I32)", who, src_dtype);
      return WM2F_EUNSUPPORTED;
    }
  }
  const int64_t n_px = (int64_t)H * W;
  const Ws ws = carve(workspace, n_px);
  hipStream_t s = (hipStream_t)stream;
  WM2F_REQUIRE(hipMemsetAsync(ws.slot, 0xFF, (size_t)n_px * sizeof(uint32_t), s) == hipSuccess &&
                   hipMemsetAsync(count, 0, sizeof(int32_t), s) == hipSuccess &&
                   hipMemsetAsync(ws.n_tile_roots, 0, sizeof(int32_t), s) == hipSuccess,
               "%s: clearing the workspace failed", who);
  if (mode == WM2F_CCL_RGB)
    launch_local<uint8_t, WM2F_CCL_RGB>(src, src_H, src_W, ty, tx, H, W, ws, cl, s);
  else if (mode == WM2F_CCL_VALUE && src_dtype == WM2F_U8)
    launch_local<uint8_t, WM2F_CCL_VALUE>(src, src_H, src_W, ty, tx, H, W, ws, cl, s);
  else if (mode == WM2F_CCL_VALUE && src_dtype == WM2F_U16)
    launch_local<uint16_t, WM2F_CCL_VALUE>(src, src_H, src_W, ty, tx, H, W, ws, cl, s);
  else if (mode == WM2F_CCL_VALUE)
    launch_local<int32_t, WM2F_CCL_VALUE>(src, src_H, src_W, ty, tx, H, W, ws, cl, s);
  else if (src_dtype == WM2F_U8)
    launch_local<uint8_t, WM2F_CCL_BINARY>(src, src_H, src_W, ty, tx, H, W, ws, cl, s);
  else if (src_dtype == WM2F_U16)
    launch_local<uint16_t, WM2F_CCL_BINARY>(src, src_H, src_W, ty, tx, H, W, ws, cl, s);
  else
    launch_local<int32_t, WM2F_CCL_BINARY>(src, src_H, src_W, ty, tx, H, W, ws, cl, s);
  WM2F_CHECK_LAUNCH(who);
  const int64_t n_border = border_count(H, W).n_border;
  if (n_border > 0) {
    hipLaunchKernelGGL(ccl_merge_kernel, dim3((unsigned)ceil_div64(n_border, kThreads)), dim3(kThreads), 0, s, H, W,
                       ws);
    WM2F_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(ccl_flatten_kernel, dim3((unsigned)ceil_div64(n_px, kThreads)), dim3(kThreads), 0, s, n_px, ws);
    WM2F_CHECK_LAUNCH(who);
  }
  hipLaunchKernelGGL(ccl_finalize_kernel, dim3((unsigned)ceil_div64(n_px, kThreads)), dim3(kThreads), 0, s, H, W, ws,
                     count);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_ccl_keys(const void* workspace, int n, int H, int W, int64_t* keys, void* stream) {
  const char* who = "wm2f_ccl_keys";
  WM2F_REQUIRE(workspace && (keys || n == 0), "%s: null pointer", who);
  WM2F_REQUIRE(H > 0 && W > 0 && H <= WM2F_PRE_MAX_SIDE && W <= WM2F_PRE_MAX_SIDE, "%s: bad size", who);
  WM2F_REQUIRE(n >= 0 && (int64_t)n <= (int64_t)H * W, "%s: n = %d outside [0, H * W]", who, n);
  if (n == 0) return WM2F_OK;
  hipLaunchKernelGGL(ccl_keys_kernel, dim3((unsigned)ceil_div(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, n,
                     carve((void*)workspace, (int64_t)H * W), keys);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_ccl_paint(void* workspace, const int64_t* order, int n, int H, int W, int skip_255, int background,
                              int32_t* out, int32_t* comp_class, void* stream) {
  const char* who = "wm2f_ccl_paint";
  WM2F_REQUIRE(workspace && out && (order || n == 0), "%s: null pointer", who);
  WM2F_REQUIRE(H > 0 && W > 0 && H <= WM2F_PRE_MAX_SIDE && W <= WM2F_PRE_MAX_SIDE, "%s: bad size", who);
  const int64_t n_px = (int64_t)H * W;
  WM2F_REQUIRE(n >= 0 && (int64_t)n <= n_px, "%s: n = %d outside [0, H * W]", who, n);
  const Ws ws = carve(workspace, n_px);
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    hipLaunchKernelGGL(ccl_assign_kernel, dim3((unsigned)ceil_div(n, kThreads)), dim3(kThreads), 0, s, n, order,
                       skip_255, ws, comp_class);
    WM2F_CHECK_LAUNCH(who);
  }
  hipLaunchKernelGGL(ccl_paint_kernel, dim3((unsigned)ceil_div64(n_px, kThreads)), dim3(kThreads), 0, s, n_px, ws,
                     background, out);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_resize_nearest(const void* src, int elem_bytes, int src_H, int src_W, const int32_t* ty,
                                   const int32_t* tx, void* dst, int H, int W, void* stream) {
  const char* who = "wm2f_resize_nearest";
  WM2F_REQUIRE(src && ty && tx && dst, "%s: null pointer", who);
  WM2F_REQUIRE(H > 0 && W > 0 && src_H > 0 && src_W > 0, "%s: need positive sizes", who);
  if (H > WM2F_PRE_MAX_SIDE || W > WM2F_PRE_MAX_SIDE || src_H > WM2F_PRE_MAX_SIDE || src_W > WM2F_PRE_MAX_SIDE) {
    set_error("%s: sides must be <= %d", who, WM2F_PRE_MAX_SIDE);
    return WM2F_EUNSUPPORTED;
  }
  const dim3 grid((unsigned)ceil_div(W, kThreads), (unsigned)H);
  hipStream_t s = (hipStream_t)stream;
  switch (elem_bytes) {
    case 1:
      hipLaunchKernelGGL(resize_nearest_kernel<1>, grid, dim3(kThreads), 0, s, (const Px<1>*)src, src_H, src_W, ty, tx,
                         (Px<1>*)dst, H, W);
      break;
    case 2:
      hipLaunchKernelGGL(resize_nearest_kernel<2>, grid, dim3(kThreads), 0, s, (const Px<2>*)src, src_H, src_W, ty, tx,
                         (Px<2>*)dst, H, W);
      break;
    case 3:
      hipLaunchKernelGGL(resize_nearest_kernel<3>, grid, dim3(kThreads), 0, s, (const Px<3>*)src, src_H, src_W, ty, tx,
                         (Px<3>*)dst, H, W);
      break;
    case 4:
      hipLaunchKernelGGL(resize_nearest_kernel<4>, grid, dim3(kThreads), 0, s, (const Px<4>*)src, src_H, src_W, ty, tx,
                         (Px<4>*)dst, H, W);
      break;
    default:
      set_error("%s: element size %d not built (1, 2, 3 or 4 bytes)", who, elem_bytes);
      return WM2F_EUNSUPPORTED;
  }
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
