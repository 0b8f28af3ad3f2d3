// The structure of skeletons on the device: the decomposition of every skeleton of an id map into
// branches and node clusters, the pruning of spurs by rounds, and per-id sums over the graph.  The contract is written
// out in include/wm2f.h; tests/skeleton_graph_reference.py restates it in numpy with scipy.ndimage.label.
//
// One decomposition (4 launches), shared by both entry points, on labelling.h's union-find, tile geometry and border
// unions with key = 2 id + [node pixel] and 8-connectivity -- the root of a set is its smallest linear pixel index:
//   graph_local    a 32 x 32 tile per workgroup: the ids of the tile and a one-pixel ring into LDS, b per pixel, the key,
//                  union-find in LDS; writes key, the tile-local root as an image index, and clears the record planes
//   graph_merge    labelling.h's merge step across tile borders on the global parents
//   graph_flatten  every live pixel points at its final root
//   graph_record   a thread per pixel: pixels and free ends per component, and per branch the smallest and largest
//                  label among the clusters it touches and the largest d2 among the node pixels it touches; integer
//                  atomicAdd / Min / Max on planes indexed by root pixel, the counts added once per wave where the
//                  wave's live pixels share a root
// wm2f_labelmap_skeleton_graph (1 + 4 + 1 launches): clear the sums; the decomposition; graph_labels writes the label
//   map and, at root pixels only, adds the component's terms to its id's row.
// wm2f_labelmap_skeleton_prune (1 + rounds * (5 + the thinning's launches) + 1 launches): a clear; per round the
//   decomposition, prune_delete (a thread per pixel: a path pixel reads its branch's record and goes when the branch is
//   a spur) into a workspace plane, and wm2f_labelmap_skeleton on that plane into out; prune_status.  A round of an
//   image starts only if the round before it removed something there (the live counts the thinning reports, device
//   memory only): otherwise its kernels return at once and the thinning copies the plane to out unchanged.
// Everything is integer; add, min and max commute: the result is bit-identical from run to run.  No kernel waits on
// another workgroup; phases that need every workgroup of the one before are separate launches.
#include "labelling.h"
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kGrThreads = 256;
constexpr int kGrCols = 8;
constexpr int kGrMaxRounds = 64;
constexpr int kGrMaxRethin = 16;
constexpr int kGrMaxMinPixels = 1 << 20;
constexpr int kGrMaxRatioQ = 1024;
constexpr int kGrPCap = 1 << 20;
constexpr int kGrNoCluster = 0x7fffffff;  // cmin of a branch without a contact (its cmax is -1)
constexpr int kGrHalo = kLabelTile + 2;

// per pixel: the key (2 id + node, -1 dead), the union-find parent as a linear index inside the image, and at root
// pixels the component's pixels, free ends, smallest / largest touched cluster and largest touched d2
struct GrWs {
  int32_t* key;
  int32_t* parent;
  int32_t* px;
  int32_t* ends;
  int32_t* cmin;
  int32_t* cmax;
  int32_t* dmax;
};
constexpr int kGrPlanes = 7;

__host__ inline int64_t gr_round16(int64_t v) { return (v + 15) / 16 * 16; }
__host__ inline int64_t gr_plane_bytes(int B, int H, int W) { return gr_round16((int64_t)B * H * W * 4); }

__host__ inline GrWs gr_carve(char* b, int64_t plane) {
  GrWs w;
  w.key = (int32_t*)b;
  w.parent = (int32_t*)(b + plane);
  w.px = (int32_t*)(b + 2 * plane);
  w.ends = (int32_t*)(b + 3 * plane);
  w.cmin = (int32_t*)(b + 4 * plane);
  w.cmax = (int32_t*)(b + 5 * plane);
  w.dmax = (int32_t*)(b + 6 * plane);
  return w;
}

__device__ __forceinline__ int gr_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Has the image's chain ended: `live` holds per image the live pixels at the start (row 0) and after every round so far
// (row j, 4 ints per image, the first is the count); round `round` (from 0) of image b runs when it is one of the first
// two or the round before it removed something.  A round that removes nothing leaves a fixed point of both steps, and
// its plane and out then both hold that state.
__device__ __forceinline__ bool gr_round_over(const int32_t* live, int B, int b, int round) {
  if (live == nullptr || round < 1) return false;
  return live[((int64_t)round * B + b) * 4] == live[((int64_t)(round - 1) * B + b) * 4];
}

// the row of a raw value: its id in [0, N), or its position in the image's ascending list; -1: dead
__device__ __forceinline__ int gr_row(int v, const int32_t* ids, int n, int N) {
  if (v < 0) return -1;
  if (ids == nullptr) return v < N ? v : -1;
  return list_row(v, ids, n);
}

// grid (tiles_x, tiles_y, B).  first_live: where round 0 counts the image's live pixels (cleared before), or null.
__global__ __launch_bounds__(kLabelThreads) void graph_local_kernel(const int32_t* __restrict__ skel,
                                                                    const int32_t* __restrict__ ids,
                                                                    const int32_t* __restrict__ n_ids, GrWs ws, int H, int W,
                                                                    int N, const int32_t* live, int round,
                                                                    int32_t* first_live) {
  __shared__ int32_t s_id[kGrHalo * kGrHalo];
  __shared__ int32_t s_key[kLabelTilePx];
  __shared__ int32_t s_parent[kLabelTilePx];
  const int b = blockIdx.z;
  if (gr_round_over(live, gridDim.z, b, round)) return;
  const int x0 = blockIdx.x * kLabelTile, y0 = blockIdx.y * kLabelTile;
  const int64_t img = (int64_t)b * H * W;
  const int32_t* list = ids == nullptr ? nullptr : ids + (int64_t)b * N;
  int n = 0;
  if (ids != nullptr) {
    n = n_ids[b];
    n = n < 0 ? 0 : (n > N ? N : n);
  }
  for (int i = threadIdx.x; i < kGrHalo * kGrHalo; i += kLabelThreads) {
    const int y = y0 - 1 + i / kGrHalo, x = x0 - 1 + i % kGrHalo;
    s_id[i] = (y >= 0 && y < H && x >= 0 && x < W) ? gr_row(skel[img + (int64_t)y * W + x], list, n, N) : -1;
  }
  __syncthreads();
  int n_live = 0;
#pragma unroll
  for (int k = 0; k < kLabelRows; ++k) {
    const auto [lx, ly, li] = tile_pixel(k);
    const int h = (ly + 1) * kGrHalo + lx + 1;
    const int c = s_id[h];
    int key = -1;
    if (c >= 0) {  // a cell outside the image is dead
      const int nb = (s_id[h - kGrHalo - 1] == c) + (s_id[h - kGrHalo] == c) + (s_id[h - kGrHalo + 1] == c) + (s_id[h - 1] == c) +
                     (s_id[h + 1] == c) + (s_id[h + kGrHalo - 1] == c) + (s_id[h + kGrHalo] == c) + (s_id[h + kGrHalo + 1] == c);
      key = 2 * c + (nb >= 3 ? 1 : 0);
      ++n_live;
    }
    s_key[li] = key;
    s_parent[li] = li;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kLabelRows; ++k) {
    const auto [lx, ly, li] = tile_pixel(k);
    const int c = s_key[li];
    if (c < 0) continue;
    constexpr int kS = __HIP_MEMORY_SCOPE_WORKGROUP;
    if (lx > 0 && s_key[li - 1] == c) unite<kS>(s_parent, li, li - 1);
    if (ly > 0) {
      if (s_key[li - kLabelTile] == c) unite<kS>(s_parent, li, li - kLabelTile);
      if (lx > 0 && s_key[li - kLabelTile - 1] == c) unite<kS>(s_parent, li, li - kLabelTile - 1);
      if (lx < kLabelTile - 1 && s_key[li - kLabelTile + 1] == c) unite<kS>(s_parent, li, li - kLabelTile + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kLabelRows; ++k) {
    const auto [lx, ly, li] = tile_pixel(k);
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    const int p = y * W + x;
    const int c = s_key[li];
    ws.key[img + p] = c;
    ws.parent[img + p] = c < 0 ? p : tile_to_image(find_root<__HIP_MEMORY_SCOPE_WORKGROUP>(s_parent, li), y0, x0, W);
    ws.px[img + p] = 0;
    ws.ends[img + p] = 0;
    ws.cmin[img + p] = kGrNoCluster;
    ws.cmax[img + p] = -1;
    ws.dmax[img + p] = 0;
  }
  if (first_live != nullptr) {
    const int sum = gr_wave_sum(n_live);
    if ((threadIdx.x & 63) == 0 && sum != 0) atomicAdd(first_live + b * 4, sum);
  }
}

// grid (ceil(n_border / 256), B), a thread per pixel on the top row or the left column of a tile
__global__ __launch_bounds__(kGrThreads) void graph_merge_kernel(GrWs ws, int H, int W, const int32_t* live, int round) {
  if (gr_round_over(live, gridDim.y, blockIdx.y, round)) return;
  BorderPixel bp;
  if (!border_pixel((int64_t)blockIdx.x * kGrThreads + threadIdx.x, H, W, bp)) return;
  const int64_t img = (int64_t)blockIdx.y * H * W;
  border_unite<8>(ws.key + img, ws.parent + img, H, W, bp, [](int k) { return k >= 0; });
}

// grid (ceil(H * W / 256), B), a thread per pixel.  The roots are final (the merge launch has ended), so a concurrent
// store to parent[q] only ever replaces an ancestor of q with q's root: a walk through q still ends at that root.
__global__ __launch_bounds__(kGrThreads) void graph_flatten_kernel(GrWs ws, int n_px, const int32_t* live, int round) {
  if (gr_round_over(live, gridDim.y, blockIdx.y, round)) return;
  const int p = blockIdx.x * kGrThreads + threadIdx.x;
  if (p >= n_px) return;
  const int64_t img = (int64_t)blockIdx.y * n_px;
  if (ws.key[img + p] < 0) return;
  int32_t* parent = ws.parent + img;
  const int r = find_root<__HIP_MEMORY_SCOPE_AGENT>(parent, p);
  if (r != p) __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (ceil(W / 64), ceil(H / 4), B), a thread per pixel, a wave per 64 pixels of a row.  d2 may be null (no dmax).
__global__ __launch_bounds__(kGrThreads) void graph_record_kernel(GrWs ws, const int32_t* __restrict__ d2, int H, int W,
                                                                  const int32_t* live, int round) {
  const int b = blockIdx.z;
  if (gr_round_over(live, gridDim.z, b, round)) return;
  const int x = (int)blockIdx.x * 64 + (threadIdx.x & 63), y = (int)blockIdx.y * 4 + (threadIdx.x >> 6);
  const int64_t img = (int64_t)b * H * W;
  const int32_t* key = ws.key + img;
  const bool inside = x < W && y < H;
  const int p = inside ? y * W + x : 0;
  const int c = inside ? key[p] : -1;
  const bool act = c >= 0;
  const unsigned long long mask = __ballot(act);
  if (mask == 0ull) return;  // wave-uniform: no live pixel among the wave's 64
  const int r = act ? ws.parent[img + p] : -1;
  int end = 0;
  if (act && (c & 1) == 0) {  // a path pixel: its ring, whether it is a free end, its contacts
    constexpr int dy[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, dx[8] = {0, 1, 1, 1, 0, -1, -1, -1};
    unsigned ring = 0u, nodes = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int yy = y + dy[i], xx = x + dx[i];
      const int q = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? key[yy * W + xx] : -1;
      if (q >= 0 && (q >> 1) == (c >> 1)) {
        ring |= 1u << i;
        nodes |= (unsigned)(q & 1) << i;
      }
    }
    const int nb = __popc(ring);
    const int X = __popc(~ring & 0xffu & ((ring >> 1) | ((ring & 1u) << 7)));  // bit i: !p(i) & p(i + 1) around the ring
    end = (nb <= 1 || (nb == 2 && X == 1)) ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (!((nodes >> i) & 1u)) continue;
      const int q = (y + dy[i]) * W + x + dx[i];
      const int cl = ws.parent[img + q];
      atomicMin(ws.cmin + img + r, cl);
      atomicMax(ws.cmax + img + r, cl);
      if (d2 != nullptr) {
        const int d = d2[img + q];
        if (d > 0) atomicMax(ws.dmax + img + r, d);
      }
    }
  }
  // the counts: a wave whose live pixels share one root adds once
  const int leader = __ffsll((long long)mask) - 1;
  const int r0 = __shfl(r, leader);
  if (__ballot(act && r != r0) == 0ull) {
    const int ends = gr_wave_sum(end);
    if ((int)(threadIdx.x & 63) == leader) {
      atomicAdd(ws.px + img + r0, __popcll(mask));
      if (ends != 0) atomicAdd(ws.ends + img + r0, ends);
    }
  } else if (act) {
    atomicAdd(ws.px + img + r, 1);
    if (end) atomicAdd(ws.ends + img + r, 1);
  }
}

// grid (ceil(H * W / 256), B), a thread per pixel: the label map, and one add per root to the row of its id
__global__ __launch_bounds__(kGrThreads) void graph_labels_kernel(GrWs ws, int32_t* __restrict__ labels,
                                                                  unsigned long long* __restrict__ sums, int n_px, int N) {
  const int p = blockIdx.x * kGrThreads + threadIdx.x;
  if (p >= n_px) return;
  const int64_t img = (int64_t)blockIdx.y * n_px;
  const int c = ws.key[img + p];
  if (c < 0) {
    labels[img + p] = -1;
    return;
  }
  const int r = ws.parent[img + p];
  labels[img + p] = (c & 1) ? -2 - r : r;
  if (r != p) return;
  unsigned long long* o = sums + ((int64_t)blockIdx.y * N + (c >> 1)) * kGrCols;  // a key's id is a row below N
  const unsigned long long P = (unsigned long long)ws.px[img + p];
  if (c & 1) {
    atomicAdd(o + 2, 1ull);
    atomicAdd(o + 3, P);
    return;
  }
  const int T = ws.ends[img + p];
  const int lo = ws.cmin[img + p], hi = ws.cmax[img + p];
  atomicAdd(o + 0, 1ull);
  if (T != 0) atomicAdd(o + 4, (unsigned long long)T);
  if (T >= 1 && hi >= 0) {
    atomicAdd(o + 1, 1ull);
    atomicMax(o + 5, P);
  }
  atomicMax(o + 6, P);
  if (T == 0 && (hi < 0 || lo == hi)) atomicAdd(o + 7, 1ull);
}

// grid (ceil(H * W / 256), B), a thread per pixel: the state after the round's deletions
__global__ __launch_bounds__(kGrThreads) void prune_delete_kernel(GrWs ws, int32_t* __restrict__ dst, int n_px, int min_pixels,
                                                                  int ratio_q, const int32_t* live, int round) {
  if (gr_round_over(live, gridDim.y, blockIdx.y, round)) return;
  const int p = blockIdx.x * kGrThreads + threadIdx.x;
  if (p >= n_px) return;
  const int64_t img = (int64_t)blockIdx.y * n_px;
  const int c = ws.key[img + p];
  int v = c < 0 ? -1 : (c >> 1);
  if (c >= 0 && (c & 1) == 0) {
    const int r = ws.parent[img + p];
    const int P = ws.px[img + r], T = ws.ends[img + r], lo = ws.cmin[img + r], hi = ws.cmax[img + r];
    if (T >= 1 && hi >= 0 && lo == hi) {
      const long long Pc = P < kGrPCap ? P : kGrPCap;
      const long long D = ws.dmax[img + r];
      if (P <= min_pixels || 256ll * Pc * Pc <= (long long)ratio_q * ratio_q * D) v = -1;
    }
  }
  dst[img + p] = v;
}

// grid ceil(B / 256): status[b] = [pixels left, rounds that removed something, removed in the last round, removed in all]
__global__ __launch_bounds__(kGrThreads) void prune_status_kernel(const int32_t* __restrict__ live, int32_t* __restrict__ status,
                                                                  int B, int rounds) {
  const int b = blockIdx.x * kGrThreads + threadIdx.x;
  if (b >= B) return;
  int busy = 0;
  for (int j = 1; j <= rounds; ++j) busy += live[((int64_t)j * B + b) * 4] != live[((int64_t)(j - 1) * B + b) * 4] ? 1 : 0;
  const int first = live[b * 4], left = live[((int64_t)rounds * B + b) * 4];
  status[b * 4 + 0] = left;
  status[b * 4 + 1] = busy;
  status[b * 4 + 2] = live[((int64_t)(rounds - 1) * B + b) * 4] - left;
  status[b * 4 + 3] = first - left;
}

// the four launches of one decomposition
void launch_graph(const int32_t* skel, const int32_t* ids, const int32_t* n_ids, const int32_t* d2, const GrWs& ws, int B,
                  int H, int W, int N, const int32_t* live, int round, int32_t* first_live, hipStream_t s) {
  const dim3 tiles((unsigned)ceil_div(W, kLabelTile), (unsigned)ceil_div(H, kLabelTile), (unsigned)B);
  hipLaunchKernelGGL(graph_local_kernel, tiles, dim3(kLabelThreads), 0, s, skel, ids, n_ids, ws, H, W, N, live, round,
                     first_live);
  // the merge launch is part of the chain at every size: a map of one tile runs it over nothing
  const int64_t n_border = border_count(H, W).n_border;
  const int n_px = H * W;  // <= 2^28
  hipLaunchKernelGGL(graph_merge_kernel, dim3((unsigned)(n_border > 0 ? ceil_div64(n_border, kGrThreads) : 1), (unsigned)B),
                     dim3(kGrThreads), 0, s, ws, H, W, live, round);
  hipLaunchKernelGGL(graph_flatten_kernel, dim3((unsigned)ceil_div(n_px, kGrThreads), (unsigned)B), dim3(kGrThreads), 0, s, ws,
                     n_px, live, round);
  hipLaunchKernelGGL(graph_record_kernel, dim3((unsigned)ceil_div(W, 64), (unsigned)ceil_div(H, 4), (unsigned)B),
                     dim3(kGrThreads), 0, s, ws, d2, H, W, live, round);
}

bool gr_size_ok(int B, int H, int W, int N) {
  return H <= kMapMaxSide && W <= kMapMaxSide && B <= kMapMaxBatch && N <= kMapMaxIds;
}

// bytes of the rows of live counts: the start and every round, (B, 4) int32 each (the thinning's status rows)
__host__ inline int64_t gr_live_bytes(int B) { return gr_round16((int64_t)(kGrMaxRounds + 1) * B * 16); }

bool gr_apart(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), a1 = a0 + (uintptr_t)a_bytes;
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(b), b1 = b0 + (uintptr_t)b_bytes;
  return a1 <= b0 || b1 <= a0;
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_labelmap_skeleton_graph_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || !gr_size_ok(B, H, W, 0)) return -1;
  return kGrPlanes * gr_plane_bytes(B, H, W);
}

extern "C" int wm2f_labelmap_skeleton_graph(const int32_t* skel, const int32_t* ids, const int32_t* n_ids, int32_t* labels,
                                            int64_t* sums, void* workspace, int B, int H, int W, int N, void* stream) {
  const char* who = "wm2f_labelmap_skeleton_graph";
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N >= 0, "%s: bad size", who);
  if (!gr_size_ok(B, H, W, N)) {
    set_error("%s: sides <= %d, B <= %d, N <= %d (got %d x %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch, kMapMaxIds, H, W, B,
              N);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(skel && labels && workspace && (sums || N == 0), "%s: null pointer", who);
  WM2F_REQUIRE((ids == nullptr) == (n_ids == nullptr), "%s: ids and n_ids go together", who);
  WM2F_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "%s: the workspace must be 16-byte aligned", who);
  const int64_t map_bytes = (int64_t)B * H * W * 4;
  WM2F_REQUIRE(gr_apart(labels, map_bytes, skel, map_bytes), "%s: labels overlaps skel", who);
  hipStream_t s = (hipStream_t)stream;
  if (N > 0 && hipMemsetAsync(sums, 0, (size_t)B * N * kGrCols * sizeof(int64_t), s) != hipSuccess) {
    set_error("%s: clearing the result failed", who);
    return WM2F_ELAUNCH;
  }
  const GrWs ws = gr_carve(reinterpret_cast<char*>(workspace), gr_plane_bytes(B, H, W));
  launch_graph(skel, ids, n_ids, nullptr, ws, B, H, W, N, nullptr, 0, nullptr, s);
  const int n_px = H * W;
  hipLaunchKernelGGL(graph_labels_kernel, dim3((unsigned)ceil_div(n_px, kGrThreads), (unsigned)B), dim3(kGrThreads), 0, s, ws,
                     labels, reinterpret_cast<unsigned long long*>(sums), n_px, N);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int64_t wm2f_labelmap_skeleton_prune_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || !gr_size_ok(B, H, W, 0)) return -1;
  const int64_t thin = wm2f_labelmap_skeleton_workspace(B, H, W);
  if (thin < 0) return -1;
  return (kGrPlanes + 1) * gr_plane_bytes(B, H, W) + gr_live_bytes(B) + gr_round16(thin);
}

extern "C" int wm2f_labelmap_skeleton_prune(const int32_t* skel, const int32_t* d2, int32_t* out, int32_t* status,
                                            void* workspace, int B, int H, int W, int N, int min_pixels, int ratio_q,
                                            int rounds, int rethin, void* stream) {
  const char* who = "wm2f_labelmap_skeleton_prune";
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N >= 0, "%s: bad size", who);
  if (!gr_size_ok(B, H, W, N)) {
    set_error("%s: sides <= %d, B <= %d, N <= %d (got %d x %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch, kMapMaxIds, H, W, B,
              N);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(min_pixels >= 0 && min_pixels <= kGrMaxMinPixels, "%s: 0 <= min_pixels <= %d, got %d", who, kGrMaxMinPixels,
               min_pixels);
  WM2F_REQUIRE(ratio_q >= 0 && ratio_q <= kGrMaxRatioQ, "%s: 0 <= ratio_q <= %d, got %d", who, kGrMaxRatioQ, ratio_q);
  WM2F_REQUIRE(rounds >= 1 && rounds <= kGrMaxRounds, "%s: 1 <= rounds <= %d, got %d", who, kGrMaxRounds, rounds);
  WM2F_REQUIRE(rethin >= 1 && rethin <= kGrMaxRethin, "%s: 1 <= rethin <= %d, got %d", who, kGrMaxRethin, rethin);
  WM2F_REQUIRE(skel && d2 && out && status && workspace, "%s: null pointer", who);
  WM2F_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0,
               "%s: workspace must be 16-byte aligned, out 4-byte aligned", who);
  const int64_t map_bytes = (int64_t)B * H * W * 4;
  WM2F_REQUIRE(gr_apart(out, map_bytes, skel, map_bytes) && gr_apart(out, map_bytes, d2, map_bytes),
               "%s: out overlaps skel or d2", who);

  hipStream_t s = (hipStream_t)stream;
  const int64_t plane = gr_plane_bytes(B, H, W);
  char* base = reinterpret_cast<char*>(workspace);
  const GrWs ws = gr_carve(base, plane);
  int32_t* state = reinterpret_cast<int32_t*>(base + kGrPlanes * plane);  // the round's deletions, before its thinning
  int32_t* live = reinterpret_cast<int32_t*>(base + (kGrPlanes + 1) * plane);
  void* thin_ws = base + (kGrPlanes + 1) * plane + gr_live_bytes(B);
  if (hipMemsetAsync(live, 0, (size_t)B * 16, s) != hipSuccess) {
    set_error("%s: clearing the counters failed", who);
    return WM2F_ELAUNCH;
  }
  const int n_px = H * W;
  for (int r = 0; r < rounds; ++r) {
    const int32_t* src = r == 0 ? skel : out;
    launch_graph(src, nullptr, nullptr, d2, ws, B, H, W, N, live, r, r == 0 ? live : nullptr, s);
    hipLaunchKernelGGL(prune_delete_kernel, dim3((unsigned)ceil_div(n_px, kGrThreads), (unsigned)B), dim3(kGrThreads), 0, s, ws,
                       state, n_px, min_pixels, ratio_q, live, r);
    WM2F_CHECK_LAUNCH(who);
    // the thinning's status row is [pixels left, ...]: the round's row of live counts
    const int rc = wm2f_labelmap_skeleton(state, WM2F_I32, out, live + (int64_t)(r + 1) * B * 4, thin_ws, B, H, W, N, rethin, 0,
                                          stream);
    if (rc != WM2F_OK) return rc;
  }
  hipLaunchKernelGGL(prune_status_kernel, dim3((unsigned)ceil_div(B, kGrThreads)), dim3(kGrThreads), 0, s, live, status, B, rounds);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
