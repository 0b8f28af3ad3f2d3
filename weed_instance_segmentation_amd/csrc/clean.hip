// Repair of id maps on the device: per instance drop small pieces, keep the largest piece, fill the
// holes it encloses, renumber what is left -- for a whole (B, H, W) stack in a fixed chain of launches, whatever the
// number of instances.  The contract is written out in include/wm2f.h; tests/clean_reference.py restates it with
// scipy.ndimage.label.
//
// One labelling, written once as a template over two modes, runs twice:
//   kPieces  pixels with an id, joined when 8-neighbours of equal id   (on the decoded map)
//   kFree    pixels without an id, joined when 4-neighbours            (on the map after the pieces were chosen)
// Its union-find, tile geometry and unions across tile borders are labelling.h's, which carries their arguments and
// loop bounds: the root of a set is its smallest linear pixel index -- the piece's "first pixel" -- whatever the
// schedule.  Phases that need every workgroup of the one before are separate launches; nothing polls or waits across
// workgroups:
//   clean_init     stats and best <- 0
//   clean_local    a 32 x 32 tile per workgroup: union-find in LDS, then per TILE root in LDS its pixel count (and in
//                  kFree a border flag and the min / max of the 4-adjacent ids); written at the tile root's pixel
//   clean_merge    labelling.h's merge step across tile borders on the global parents
//   clean_flatten  every tile root points at its final root and adds its tile's count (flag, min, max) there: one
//                  integer atomic per (tile, tile root), never one per pixel
//   clean_best     per final piece of id k: area_in, pieces_in, and one 64-bit atomicMax of
//                  area << 32 | (0xFFFFFFFF - first pixel) on best[b][k], gathered per workgroup in LDS first
//   clean_keep     every pixel of a piece that is not kept becomes free; per kept piece pieces_kept, area_kept
//   (local, merge, flatten in kFree when holes are filled)
//   clean_holes    per free component that is a hole of k: holes_filled, pixels_filled (one add per hole)
//   clean_relabel  a workgroup per image: area_out, new_id, the id table and n_out
//   clean_paint    out[p] = table[id of p, or of the hole p lies in], -1 when free
// Everything is integer and every accumulation is an integer atomic: the result does not depend on the schedule.
//
// No loop depends on a map value: a value is decoded to an id in [0, N) or to "free" before anything indexes with it.
#include <type_traits>

#include "labelling.h"
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kClThreads = 256;
constexpr int kClBestPx = 16;                                 // pixels per thread of clean_best
constexpr int kClBestLdsIds = 1024;                           // 20 B of LDS per id: 20 KiB at the cap
constexpr uint32_t kClBorder = 0x80000000u;                   // a free component touches the image border (areas < 2^29)
constexpr int kClNoId = 0x7fffffff;                           // min of no 4-adjacent id (the max of none is -1)
constexpr int kClOutside = -2;                                // LDS key of a tile pixel beyond the image

enum { kPieces = 0, kFree = 1 };
template <int kMode>
constexpr int kModeConn = kMode == kPieces ? 8 : 4;  // pieces are 8-connected, free components 4-connected

// Workspace carve (include/wm2f.h).  Per image: best (N) and the id table (N); per pixel: the id (-1 free), the
// union-find parent as a linear index inside the image, and at root pixels the count (kFree: | kClBorder) and the
// min / max of the 4-adjacent ids.
struct ClWs {
  unsigned long long* best;
  int32_t* lut;
  int32_t* key;
  int32_t* parent;
  uint32_t* area;
  int32_t* lo;
  int32_t* hi;
};

__host__ inline int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }

__host__ inline ClWs carve(void* ws, int64_t n_ids, int64_t n_px) {
  char* b = (char*)ws;
  const int64_t ids8 = round16(n_ids * 8), ids4 = round16(n_ids * 4), px = round16(n_px * 4);
  ClWs w;
  w.best = (unsigned long long*)b;
  w.lut = (int32_t*)(b + ids8);
  w.key = (int32_t*)(b + ids8 + ids4);
  w.parent = (int32_t*)(b + ids8 + ids4 + px);
  w.area = (uint32_t*)(b + ids8 + ids4 + 2 * px);
  w.lo = (int32_t*)(b + ids8 + ids4 + 3 * px);
  w.hi = (int32_t*)(b + ids8 + ids4 + 4 * px);
  return w;
}

template <int kMode>
__device__ __forceinline__ bool is_active(int key) {
  return kMode == kPieces ? key >= 0 : key == -1;
}

// the id a free component is a hole of, -1 for none: no border flag, one id around it, and not above the limit
__device__ __forceinline__ int hole_of(uint32_t area, int lo, int hi, long long max_hole) {
  if (area & kClBorder) return -1;
  if (lo != hi) return -1;  // kClNoId / -1 when nothing with an id touches it
  if (max_hole >= 0 && (long long)area > max_hole) return -1;
  return lo;
}

__global__ __launch_bounds__(kClThreads) void clean_init_kernel(long long* __restrict__ stats,
                                                                unsigned long long* __restrict__ best, int n_ids) {
  const int i = blockIdx.x * kClThreads + threadIdx.x;
  if (i >= n_ids) return;
  long long* s = stats + (int64_t)i * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = 0;
  best[i] = 0ull;
}

// Local phase: grid (tiles_x, tiles_y, B), a workgroup per 32 x 32 tile.  kPieces decodes the map (dtype DT) and writes
// the id of every pixel; kFree reads those ids back.  Writes for every pixel of the image its tile-local root as a
// linear index of the image (a pixel that is not active points at itself), and at every pixel its tile's count if it is
// a tile root, 0 otherwise.
template <int kMode, int DT>
__global__ __launch_bounds__(kLabelThreads) void clean_local_kernel(const void* __restrict__ map, ClWs ws, int H, int W,
                                                                 int N) {
  using E = typename MapElem<DT>::type;
  constexpr int kAux = kMode == kFree ? kLabelTilePx : 1;
  __shared__ int32_t s_parent[kLabelTilePx];
  __shared__ int32_t s_key[kLabelTilePx];
  __shared__ uint32_t s_cnt[kLabelTilePx];
  __shared__ int32_t s_lo[kAux];
  __shared__ int32_t s_hi[kAux];
  const int x0 = blockIdx.x * kLabelTile, y0 = blockIdx.y * kLabelTile;
  const int64_t img = (int64_t)blockIdx.z * H * W;
  int32_t* key = ws.key + img;
#pragma unroll
  for (int k = 0; k < kLabelRows; ++k) {
    const auto [lx, ly, li] = tile_pixel(k);
    const int y = y0 + ly, x = x0 + lx;
    int c = kClOutside;
    if (y < H && x < W) {
      const int64_t p = (int64_t)y * W + x;
      if (kMode == kPieces) {
        c = map_id_below<DT>((uint32_t)reinterpret_cast<const E*>(map)[img + p], N);
        key[p] = c;
      } else {
        c = key[p];
      }
    }
    s_key[li] = c;
    s_parent[li] = li;
    s_cnt[li] = 0u;
    if constexpr (kMode == kFree) {
      s_lo[li] = kClNoId;
      s_hi[li] = -1;
    }
  }
  __syncthreads();
  // the neighbour loop stays in the kernel: through a function shared with ccl.hip the kFree instance measured about
  // 1 % slower at B = 8
#pragma unroll
  for (int k = 0; k < kLabelRows; ++k) {
    const auto [lx, ly, li] = tile_pixel(k);
    const int c = s_key[li];
    if (!is_active<kMode>(c)) continue;
    constexpr int kS = __HIP_MEMORY_SCOPE_WORKGROUP;
    if (lx > 0 && s_key[li - 1] == c) unite<kS>(s_parent, li, li - 1);
    if (ly > 0) {
      if (s_key[li - kLabelTile] == c) unite<kS>(s_parent, li, li - kLabelTile);
      if constexpr (kMode == kPieces) {
        if (lx > 0 && s_key[li - kLabelTile - 1] == c) unite<kS>(s_parent, li, li - kLabelTile - 1);
        if (lx < kLabelTile - 1 && s_key[li - kLabelTile + 1] == c) unite<kS>(s_parent, li, li - kLabelTile + 1);
      }
    }
  }
  __syncthreads();
  int root[kLabelRows];
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < kLabelRows; ++k) {
    const auto [lx, ly, li] = tile_pixel(k);
    [[maybe_unused]] const int y = y0 + ly, x = x0 + lx;
    const bool act = is_active<kMode>(s_key[li]);
    const int r = act ? find_root<__HIP_MEMORY_SCOPE_WORKGROUP>(s_parent, li) : -1;
    root[k] = r;
    // count: a wave whose active pixels share one root (the inside of a piece: nearly every wave) adds once
    const unsigned long long mask = __ballot(act);
    if (mask != 0ull) {  // wave-uniform
      const int leader = __ffsll((long long)mask) - 1;
      const int r0 = __shfl(r, leader, 64);
      if (__ballot(act && r == r0) == mask) {
        if (lane == leader) atomicAdd(&s_cnt[r0], (uint32_t)__popcll(mask));
      } else if (act) {
        atomicAdd(&s_cnt[r], 1u);
      }
    }
    if constexpr (kMode == kFree) {
      if (!act) continue;
      if (y == 0 || x == 0 || y == H - 1 || x == W - 1) atomicOr(&s_cnt[r], kClBorder);
      // the four 4-neighbours inside the image; those beyond the tile are read from the id map
      const int64_t p = (int64_t)y * W + x;
      int nk[4];
      nk[0] = x > 0 ? (lx > 0 ? s_key[li - 1] : key[p - 1]) : -1;
      nk[1] = x + 1 < W ? (lx < kLabelTile - 1 ? s_key[li + 1] : key[p + 1]) : -1;
      nk[2] = y > 0 ? (ly > 0 ? s_key[li - kLabelTile] : key[p - W]) : -1;
      nk[3] = y + 1 < H ? (ly < kLabelTile - 1 ? s_key[li + kLabelTile] : key[p + W]) : -1;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (nk[j] >= 0) {
          atomicMin(&s_lo[r], nk[j]);
          atomicMax(&s_hi[r], nk[j]);
        }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kLabelRows; ++k) {
    const auto [lx, ly, li] = tile_pixel(k);
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    const int64_t p = (int64_t)y * W + x;
    const int r = root[k];
    const bool is_root = r == li;
    ws.parent[img + p] = r < 0 ? (int)p : tile_to_image(r, y0, x0, W);
    ws.area[img + p] = is_root ? s_cnt[li] : 0u;
    if constexpr (kMode == kFree) {
      ws.lo[img + p] = is_root ? s_lo[li] : kClNoId;
      ws.hi[img + p] = is_root ? s_hi[li] : -1;
    }
  }
}

// Merge phase: grid (ceil(n_border / 256), B), a thread per pixel on the top row or the left column of a tile (other than
// the image's own edge), joined with its neighbours across that border by labelling.h's rule, which makes one union per
// run of pixels.  (Measured on a 1024 x 1024 map whose background is one free component: one union per border pixel
// kept this launch at 0.10 ms, 62k unions walking to one root; one per run is what is left.)
template <int kMode>
__global__ __launch_bounds__(kClThreads) void clean_merge_kernel(ClWs ws, int H, int W) {
  BorderPixel b;
  if (!border_pixel((int64_t)blockIdx.x * kClThreads + threadIdx.x, H, W, b)) return;
  const int64_t img = (int64_t)blockIdx.y * H * W;
  border_unite<kModeConn<kMode>>(ws.key + img, ws.parent + img, H, W, b,
                                 [](int k) { return is_active<kMode>(k); });
}

// Flatten phase: grid (ceil(H * W / 256), B), a thread per pixel; only tile roots (count != 0) do anything.  Roots are
// final here (the merge launch has ended), so a concurrent write of parent[q] only ever replaces an ancestor with the
// root.  A tile root that is not the final root adds what its tile counted at the final root, whose own slot holds its
// own tile's share: one atomic per (tile, tile root).  Nothing is added to a slot that is read here as a tile's share.
template <int kMode>
__global__ __launch_bounds__(kClThreads) void clean_flatten_kernel(ClWs ws, int n_px) {
  const int p = blockIdx.x * kClThreads + threadIdx.x;
  if (p >= n_px) return;
  const int64_t img = (int64_t)blockIdx.y * n_px;
  uint32_t* area = ws.area + img;
  const uint32_t a = area[p];
  if (a == 0u) return;
  int32_t* parent = ws.parent + img;
  const int r = find_root<__HIP_MEMORY_SCOPE_AGENT>(parent, p);
  if (r == p) return;
  __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicAdd(area + r, a & ~kClBorder);
  if (kMode == kFree) {
    if (a & kClBorder) atomicOr(area + r, kClBorder);
    const int lo = ws.lo[img + p], hi = ws.hi[img + p];
    if (hi >= 0) {  // some pixel of this tile's share touches an id
      atomicMin(ws.lo + img + r, lo);
      atomicMax(ws.hi + img + r, hi);
    }
  }
}

// grid (ceil(H * W / 4096), B): a workgroup reads 4096 pixels, 16 per thread; the final roots of pieces report area_in,
// pieces_in and the candidate for the largest piece.  While N <= kClBestLdsIds the workgroup gathers them per id in LDS
// and flushes the ids it saw, three integer atomics each -- a map of 65k pieces on six ids otherwise sends 196k atomics
// to six rows (0.47 ms measured at 1024 x 1024); above the cap the roots go to the result directly.
template <bool kLds>
__global__ __launch_bounds__(kClThreads) void clean_best_kernel(ClWs ws, long long* __restrict__ stats, int n_px, int N) {
  constexpr int kIds = kLds ? kClBestLdsIds : 1;
  __shared__ unsigned long long s_area[kIds];
  __shared__ unsigned long long s_best[kIds];
  __shared__ uint32_t s_cnt[kIds];
  const int64_t img = (int64_t)blockIdx.y * n_px;
  unsigned long long* rows = reinterpret_cast<unsigned long long*>(stats + (int64_t)blockIdx.y * N * 8);
  unsigned long long* best = ws.best + (int64_t)blockIdx.y * N;
  if constexpr (kLds) {
    for (int k = threadIdx.x; k < N; k += kClThreads) {
      s_area[k] = 0ull;
      s_best[k] = 0ull;
      s_cnt[k] = 0u;
    }
    __syncthreads();
  }
  const int base = blockIdx.x * (kClThreads * kClBestPx) + threadIdx.x;
#pragma unroll
  for (int i = 0; i < kClBestPx; ++i) {
    const int p = base + i * kClThreads;
    if (p >= n_px) break;
    const int k = ws.key[img + p];
    if (k < 0 || ws.parent[img + p] != p) continue;
    const unsigned long long a = ws.area[img + p];
    const unsigned long long cand = (a << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)p);
    if constexpr (kLds) {
      atomicAdd(&s_area[k], a);
      atomicAdd(&s_cnt[k], 1u);
      atomicMax(&s_best[k], cand);
    } else {
      atomicAdd(rows + (int64_t)k * 8, a);
      atomicAdd(rows + (int64_t)k * 8 + 1, 1ull);
      atomicMax(best + k, cand);
    }
  }
  if constexpr (kLds) {
    __syncthreads();
    for (int k = threadIdx.x; k < N; k += kClThreads) {
      const uint32_t c = s_cnt[k];
      if (c == 0u) continue;  // flush only what this workgroup saw
      atomicAdd(rows + (int64_t)k * 8, s_area[k]);
      atomicAdd(rows + (int64_t)k * 8 + 1, (unsigned long long)c);
      atomicMax(best + k, s_best[k]);
    }
  }
}

// a thread per pixel: two hops to the final root (pixel -> tile root -> final root); a piece that is not kept is freed
__global__ __launch_bounds__(kClThreads) void clean_keep_kernel(ClWs ws, long long* __restrict__ stats, int n_px, int N,
                                                                int keep, long long min_area) {
  const int p = blockIdx.x * kClThreads + threadIdx.x;
  if (p >= n_px) return;
  const int64_t img = (int64_t)blockIdx.y * n_px;
  const int k = ws.key[img + p];
  if (k < 0) return;
  const int r = ws.parent[img + ws.parent[img + p]];
  const unsigned long long a = ws.area[img + r];
  const int64_t row = (int64_t)blockIdx.y * N + k;
  bool kept = (long long)a >= min_area;
  if (keep == WM2F_CLEAN_KEEP_LARGEST)
    kept = kept && ws.best[row] == ((a << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)r));
  if (!kept) {
    ws.key[img + p] = -1;
  } else if (r == p) {
    unsigned long long* s = reinterpret_cast<unsigned long long*>(stats + row * 8);
    atomicAdd(s + 2, 1ull);
    atomicAdd(s + 3, a);
  }
}

// a thread per pixel; the final roots of free components that are holes report: one add per hole
__global__ __launch_bounds__(kClThreads) void clean_holes_kernel(ClWs ws, long long* __restrict__ stats, int n_px, int N,
                                                                 long long max_hole) {
  const int p = blockIdx.x * kClThreads + threadIdx.x;
  if (p >= n_px) return;
  const int64_t img = (int64_t)blockIdx.y * n_px;
  if (ws.key[img + p] != -1 || ws.parent[img + p] != p) return;
  const uint32_t a = ws.area[img + p];
  const int k = hole_of(a, ws.lo[img + p], ws.hi[img + p], max_hole);
  if (k < 0 || k >= N) return;  // an adjacent id is a decoded id, so always below N
  unsigned long long* s = reinterpret_cast<unsigned long long*>(stats + ((int64_t)blockIdx.y * N + k) * 8);
  atomicAdd(s + 4, 1ull);
  atomicAdd(s + 5, (unsigned long long)a);
}

// grid B, a workgroup per image: thread t owns the ids [t * chunk, (t + 1) * chunk), chunk = ceil(N / 256) <= 16
__global__ __launch_bounds__(kClThreads) void clean_relabel_kernel(ClWs ws, long long* __restrict__ stats,
                                                                   int32_t* __restrict__ n_out, int N, int relabel) {
  __shared__ int s_scan[kClThreads];
  const int b = blockIdx.x, t = threadIdx.x;
  const int chunk = ceil_div(N, kClThreads);
  const int k0 = t * chunk, k1 = k0 + chunk < N ? k0 + chunk : N;
  long long* st = stats + (int64_t)b * N * 8;
  int mine = 0;
  for (int k = k0; k < k1; ++k) {
    const long long area_out = st[(int64_t)k * 8 + 3] + st[(int64_t)k * 8 + 5];
    st[(int64_t)k * 8 + 6] = area_out;
    mine += area_out > 0;
  }
  s_scan[t] = mine;
  __syncthreads();
  for (int o = 1; o < kClThreads; o <<= 1) {  // inclusive scan, 8 rounds
    const int v = t >= o ? s_scan[t - o] : 0;
    __syncthreads();
    s_scan[t] += v;
    __syncthreads();
  }
  int next = s_scan[t] - mine;
  for (int k = k0; k < k1; ++k) {
    const bool some = st[(int64_t)k * 8 + 6] > 0;
    const int id = some ? (relabel ? next : k) : -1;
    next += some;
    st[(int64_t)k * 8 + 7] = id;
    ws.lut[(int64_t)b * N + k] = id;
  }
  if (t == kClThreads - 1) n_out[b] = s_scan[t];
}

// grid (ceil(H * W / (256 * PIX)), B): PIX = 4 pixels per thread with 16-byte loads and stores, or 1
template <typename O, int PIX>
__global__ __launch_bounds__(kClThreads) void clean_paint_kernel(ClWs ws, O* __restrict__ out, int n_px, int N, int fill,
                                                                 long long max_hole) {
  const int p0 = (blockIdx.x * kClThreads + threadIdx.x) * PIX;
  if (p0 >= n_px) return;  // PIX == 4: n_px % 4 == 0, the four pixels are inside together
  const int64_t img = (int64_t)blockIdx.y * n_px;
  const int32_t* lut = ws.lut + (int64_t)blockIdx.y * N;
  int k[PIX];
  if constexpr (PIX == 4) {
    const int4 q = *reinterpret_cast<const int4*>(ws.key + img + p0);
    k[0] = q.x;
    k[1] = q.y;
    k[2] = q.z;
    k[3] = q.w;
  } else {
    k[0] = ws.key[img + p0];
  }
  O v[PIX];
#pragma unroll
  for (int j = 0; j < PIX; ++j) {
    int id = k[j];
    if (id < 0 && fill) {
      const int r = ws.parent[img + ws.parent[img + p0 + j]];
      id = hole_of(ws.area[img + r], ws.lo[img + r], ws.hi[img + r], max_hole);
    }
    v[j] = (O)((id >= 0 && id < N) ? lut[id] : -1);
  }
  if constexpr (PIX == 4) {
    struct alignas(16) V4 {
      O a, b, c, d;
    };
    *reinterpret_cast<V4*>(out + img + p0) = V4{v[0], v[1], v[2], v[3]};
  } else {
    out[img + p0] = v[0];
  }
}

template <int kMode, int DT>
void launch_labelling(const void* map, const ClWs& ws, int B, int H, int W, int N, hipStream_t s) {
  const dim3 tiles((unsigned)ceil_div(W, kLabelTile), (unsigned)ceil_div(H, kLabelTile), (unsigned)B);
  hipLaunchKernelGGL((clean_local_kernel<kMode, DT>), tiles, dim3(kLabelThreads), 0, s, map, ws, H, W, N);
  // the merge and flatten launches are part of the chain at every size: a map of one tile runs them over nothing
  const int64_t n_border = border_count(H, W).n_border;
  const int n_px = H * W;
  hipLaunchKernelGGL((clean_merge_kernel<kMode>), dim3((unsigned)(n_border > 0 ? ceil_div64(n_border, kClThreads) : 1), (unsigned)B),
                     dim3(kClThreads), 0, s, ws, H, W);
  hipLaunchKernelGGL((clean_flatten_kernel<kMode>), dim3((unsigned)ceil_div(n_px, kClThreads), (unsigned)B),
                     dim3(kClThreads), 0, s, ws, n_px);
}

int64_t workspace_bytes(int B, int H, int W, int N) {
  const int64_t n_ids = (int64_t)B * N, n_px = (int64_t)B * H * W;
  return round16(n_ids * 8) + round16(n_ids * 4) + 5 * round16(n_px * 4);
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_labelmap_clean_workspace(int B, int H, int W, int N) {
  if (B <= 0 || H <= 0 || W <= 0 || N < 0 || H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch || N > kMapMaxIds) return -1;
  return workspace_bytes(B, H, W, N);
}

extern "C" int wm2f_labelmap_clean(const void* map, int dtype, void* out, int out_dtype, int64_t* stats, int32_t* n_out,
                                   void* workspace, int B, int H, int W, int N, int keep, int64_t min_area,
                                   int fill_holes, int64_t max_hole_area, int relabel, int phase, void* stream) {
  const char* who = "wm2f_labelmap_clean";
  WM2F_REQUIRE(phase >= WM2F_CLEAN_ALL && phase <= WM2F_CLEAN_PAINT, "%s: unknown phase %d", who, phase);
  WM2F_REQUIRE(map && out && n_out && workspace && (stats || N == 0), "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N >= 0, "%s: bad size", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  WM2F_REQUIRE(out_dtype == WM2F_F32 || out_dtype == WM2F_I32, "%s: out must be fp32 or int32", who);
  WM2F_REQUIRE(keep == WM2F_CLEAN_KEEP_ALL || keep == WM2F_CLEAN_KEEP_LARGEST, "%s: unknown keep mode %d", who, keep);
  WM2F_REQUIRE((fill_holes == 0 || fill_holes == 1) && (relabel == 0 || relabel == 1), "%s: fill_holes and relabel are 0 or 1",
               who);
  WM2F_REQUIRE(min_area >= 0, "%s: min_area must not be negative", who);
  WM2F_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "%s: the workspace must be 8-byte aligned", who);
  if (H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch || N > kMapMaxIds) {
    set_error("%s: sides <= %d, B <= %d, N <= %d (got %d x %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch, kMapMaxIds, H, W, B,
              N);
    return WM2F_EUNSUPPORTED;
  }
  const int64_t all_px = (int64_t)B * H * W;
  const uintptr_t m0 = reinterpret_cast<uintptr_t>(map), m1 = m0 + (uintptr_t)all_px * map_elem_bytes(dtype);
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + (uintptr_t)all_px * 4;
  WM2F_REQUIRE(o1 <= m0 || m1 <= o0, "%s: out overlaps map", who);
  const uintptr_t w0 = reinterpret_cast<uintptr_t>(workspace), w1 = w0 + (uintptr_t)workspace_bytes(B, H, W, N);
  WM2F_REQUIRE((o1 <= w0 || w1 <= o0) && (m1 <= w0 || w1 <= m0), "%s: the workspace overlaps map or out", who);

  hipStream_t s = (hipStream_t)stream;
  const ClWs ws = carve(workspace, (int64_t)B * N, all_px);
  long long* st = reinterpret_cast<long long*>(stats);
  const int n_px = H * W;  // <= 2^28
  const dim3 px_grid((unsigned)ceil_div(n_px, kClThreads), (unsigned)B);
  const auto runs = [phase](int ph) { return phase == WM2F_CLEAN_ALL || phase == ph; };
  if (runs(WM2F_CLEAN_PIECES)) {
    if (B * N > 0)
      hipLaunchKernelGGL(clean_init_kernel, dim3(ceil_div(B * N, kClThreads)), dim3(kClThreads), 0, s, st, ws.best, B * N);
    for_map_dtype(dtype, [&](auto dt) { launch_labelling<kPieces, decltype(dt)::value>(map, ws, B, H, W, N, s); });
    WM2F_CHECK_LAUNCH(who);
  }
  if (runs(WM2F_CLEAN_CHOOSE)) {
    const dim3 best_grid((unsigned)ceil_div(n_px, kClThreads * kClBestPx), (unsigned)B);
    if (N <= kClBestLdsIds) hipLaunchKernelGGL(clean_best_kernel<true>, best_grid, dim3(kClThreads), 0, s, ws, st, n_px, N);
    else hipLaunchKernelGGL(clean_best_kernel<false>, best_grid, dim3(kClThreads), 0, s, ws, st, n_px, N);
    hipLaunchKernelGGL(clean_keep_kernel, px_grid, dim3(kClThreads), 0, s, ws, st, n_px, N, keep, (long long)min_area);
    WM2F_CHECK_LAUNCH(who);
  }
  if (runs(WM2F_CLEAN_HOLES) && fill_holes) {
    launch_labelling<kFree, WM2F_I32>(nullptr, ws, B, H, W, N, s);
    hipLaunchKernelGGL(clean_holes_kernel, px_grid, dim3(kClThreads), 0, s, ws, st, n_px, N, (long long)max_hole_area);
    WM2F_CHECK_LAUNCH(who);
  }
  if (!runs(WM2F_CLEAN_PAINT)) return WM2F_OK;
  hipLaunchKernelGGL(clean_relabel_kernel, dim3((unsigned)B), dim3(kClThreads), 0, s, ws, st, n_out, N, relabel);
  const bool vec = W % 4 == 0 && o0 % 16 == 0 && reinterpret_cast<uintptr_t>(ws.key) % 16 == 0;
  const dim3 vgrid((unsigned)ceil_div(n_px, kClThreads * 4), (unsigned)B);
  const auto paint = [&](auto* o) {  // o: out as the type it is painted in
    using O = std::remove_pointer_t<decltype(o)>;
    if (vec) hipLaunchKernelGGL((clean_paint_kernel<O, 4>), vgrid, dim3(kClThreads), 0, s, ws, o, n_px, N, fill_holes,
                                (long long)max_hole_area);
    else hipLaunchKernelGGL((clean_paint_kernel<O, 1>), px_grid, dim3(kClThreads), 0, s, ws, o, n_px, N, fill_holes,
                            (long long)max_hole_area);
  };
  if (out_dtype == WM2F_F32) paint((float*)out);
  else paint((int32_t*)out);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
