// Splitting touching instances of id maps on the device: a watershed of the interior distance.  Every
// pixel ascends the squared distance map of wm2f_labelmap_distance to a peak; the pixels of one peak are a basin; basins
// of one id are merged, in synchronous rounds, across their highest pass when the neck there is wide against the lower
// part's own clearance.  The rule is written out in include/wm2f.h; tests/split_reference.py restates it in numpy.
//
// One int32 per pixel, lab, carries the whole forest: first up(p), then the pixel's peak, then the peak pixel of the
// pixel's group.  A pointer only ever moves to a pixel of larger key, so following it ends, whatever other threads write
// meanwhile, and the fixed point does not depend on the schedule.
//   split_init     counters, keep slots, info rows
//   split_ascent   decodes the map (key: id in [0, N) or -1), writes up(p) into lab, clears the pass slot of every peak,
//                  counts the peaks
//   split_flatten  every pixel follows lab to its fixed point and stores it (here: the basins)
//   per round, each launch returning at once when the round before linked nothing:
//     split_pass     a pixel and its four forward neighbours: where ids agree and groups differ, a 64-bit atomicMax of
//                    (min d2 << 32 | ~peak of the other group) into both groups' slots, after a look at the slot
//     split_decide   a thread per group peak: reads and clears its slot, links itself under the other peak by the rule,
//                    counts the links
//     split_flatten  as above (now: the groups)
//   split_keep     per id a 64-bit atomicMax of the keys of its groups' peaks: the group that keeps the id
//   split_count    per 1024 pixels the number of peaks of groups that do not keep their id; the kept ids' info rows
//   split_scan     a workgroup per image: exclusive scan of those counts, and the status row
//   split_assign   the extra groups' ids in raster order of their peaks, and their info rows
//   split_paint    out[p]
// Everything is integer; the atomics are max and add on integers, so no result depends on an order.
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kSpThreads = 256;
constexpr int kSpMaxRounds = 32;
constexpr int kSpMaxDen = 1024;
constexpr int kSpChunk = 4 * kSpThreads;  // pixels per workgroup of the numbering passes
constexpr int kSpCounters = kSpMaxRounds + 2;  // per image: the links of every round, the basins, and one to pad
constexpr int kSpBasins = kSpMaxRounds;
constexpr int kSpExtraFlag = -2;  // nid of an extra group's peak between split_count and split_assign
constexpr int kS = __HIP_MEMORY_SCOPE_AGENT;

// Workspace carve (include/wm2f.h).  Per pixel: key, lab, and 8 bytes that hold a group's best pass during the rounds
// and the new ids (nid, int32) afterwards.  Per image: keep (M), the chunk counts and the counters.
struct SpWs {
  int32_t* key;
  int32_t* lab;
  unsigned long long* best;
  unsigned long long* keep;
  int32_t* chunk;
  int32_t* cnt;
};

__host__ inline int64_t sp_round16(int64_t v) { return (v + 15) / 16 * 16; }
__host__ inline int sp_chunks(int H, int W) { return ceil_div(H * W, kSpChunk); }

__host__ inline int64_t sp_workspace_bytes(int B, int H, int W, int M) {
  const int64_t n_px = (int64_t)B * H * W;
  return sp_round16(n_px * 8) + 2 * sp_round16(n_px * 4) + sp_round16((int64_t)B * M * 8) +
         sp_round16((int64_t)B * sp_chunks(H, W) * 4) + sp_round16((int64_t)B * kSpCounters * 4);
}

__host__ inline SpWs sp_carve(void* ws, int B, int H, int W, int M) {
  char* b = (char*)ws;
  const int64_t n_px = (int64_t)B * H * W;
  SpWs w;
  w.best = (unsigned long long*)b;
  b += sp_round16(n_px * 8);
  w.key = (int32_t*)b;
  b += sp_round16(n_px * 4);
  w.lab = (int32_t*)b;
  b += sp_round16(n_px * 4);
  w.keep = (unsigned long long*)b;
  b += sp_round16((int64_t)B * M * 8);
  w.chunk = (int32_t*)b;
  b += sp_round16((int64_t)B * sp_chunks(H, W) * 4);
  w.cnt = (int32_t*)b;
  return w;
}

__device__ __forceinline__ unsigned long long sp_key(int d2, int lin) {
  return ((unsigned long long)(uint32_t)d2 << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)lin);
}

// adds the number of set lanes to *counter, once per wave; call it wave-uniformly
__device__ __forceinline__ void sp_count(bool flag, int32_t* counter) {
  const unsigned long long m = __ballot(flag);
  if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(counter, (int)__popcll(m));
}

__device__ __forceinline__ int sp_follow(int32_t* lab, int x) {
  int n = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, kS);
  while (n != x) {  // keys strictly increase along the way: at most as many steps as the image has pixels
    x = n;
    n = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, kS);
  }
  return x;
}

// grid ceil(max(B * kSpCounters, B * M) / 256)
__global__ __launch_bounds__(kSpThreads) void split_init_kernel(SpWs ws, int32_t* __restrict__ info, int B, int M) {
  const int i = blockIdx.x * kSpThreads + threadIdx.x;
  if (i < B * kSpCounters) ws.cnt[i] = 0;
  if (i < B * M) {
    ws.keep[i] = 0ull;
    reinterpret_cast<int4*>(info)[i] = make_int4(-1, -1, -1, 0);
  }
}

// grid (ceil(H * W / 256), B), a thread per pixel
template <int DT>
__global__ __launch_bounds__(kSpThreads) void split_ascent_kernel(const void* __restrict__ map,
                                                                  const int32_t* __restrict__ d2, SpWs ws, int H, int W,
                                                                  int N) {
  using E = typename MapElem<DT>::type;
  const int n_px = H * W;
  const int p = blockIdx.x * kSpThreads + threadIdx.x;
  const int64_t img = (int64_t)blockIdx.y * n_px;
  bool peak = false;
  if (p < n_px) {
    const E* src = reinterpret_cast<const E*>(map) + img;
    const int32_t* dd = d2 + img;
    const int k = map_id_below<DT>((uint32_t)src[p], N);
    int up = p;
    if (k >= 0) {
      const int y = p / W, x = p - y * W;
      unsigned long long top = sp_key(dd[p], p);
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if (dy == 0 && dx == 0) continue;
          const int yy = y + dy, xx = x + dx;
          if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
          const int q = yy * W + xx;
          if (map_id_below<DT>((uint32_t)src[q], N) != k) continue;
          const unsigned long long kq = sp_key(dd[q], q);
          if (kq > top) {
            top = kq;
            up = q;
          }
        }
      }
      peak = up == p;
      if (peak) ws.best[img + p] = 0ull;
    }
    ws.key[img + p] = k;
    ws.lab[img + p] = up;
  }
  sp_count(peak, ws.cnt + blockIdx.y * kSpCounters + kSpBasins);
}

// the early exit: a round after one that linked nothing would link nothing either (the image is blockIdx.y everywhere)
__device__ __forceinline__ bool split_skips(const SpWs& ws, int round) {
  return round > 0 && ws.cnt[blockIdx.y * kSpCounters + round - 1] == 0;
}

// grid (ceil(H * W / 256), B), a thread per pixel; `round` 0 for the basins
__global__ __launch_bounds__(kSpThreads) void split_flatten_kernel(SpWs ws, int n_px, int round) {
  if (split_skips(ws, round)) return;
  const int p = blockIdx.x * kSpThreads + threadIdx.x;
  if (p >= n_px) return;
  const int64_t img = (int64_t)blockIdx.y * n_px;
  if (ws.key[img + p] < 0) return;
  int32_t* lab = ws.lab + img;
  const int first = __hip_atomic_load(lab + p, __ATOMIC_RELAXED, kS);
  const int r = sp_follow(lab, first);
  if (r != first) __hip_atomic_store(lab + p, r, __ATOMIC_RELAXED, kS);
}

// grid (ceil(H * W / 256), B).  lab is flat here: every pixel holds its group's peak.
__global__ __launch_bounds__(kSpThreads) void split_pass_kernel(const int32_t* __restrict__ d2, SpWs ws, int H, int W,
                                                                int round) {
  if (split_skips(ws, round)) return;
  const int n_px = H * W;
  const int p = blockIdx.x * kSpThreads + threadIdx.x;
  if (p >= n_px) return;
  const int64_t img = (int64_t)blockIdx.y * n_px;
  const int32_t* key = ws.key + img;
  const int k = key[p];
  if (k < 0) return;
  const int32_t* lab = ws.lab + img;
  const int32_t* dd = d2 + img;
  unsigned long long* best = ws.best + img;
  const int y = p / W, x = p - y * W;
  const int g = lab[p];
  const int ox[4] = {1, -1, 0, 1}, oy[4] = {0, 1, 1, 1};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int yy = y + oy[j], xx = x + ox[j];
    if (yy >= H || xx < 0 || xx >= W) continue;
    const int q = yy * W + xx;
    if (key[q] != k) continue;
    const int gq = lab[q];
    if (gq == g) continue;
    const int dp = dd[p], dq = dd[q];
    const unsigned long long s = (unsigned long long)(uint32_t)(dp < dq ? dp : dq) << 32;
    const unsigned long long to_g = s | (unsigned long long)(0xFFFFFFFFu - (uint32_t)gq);
    const unsigned long long to_q = s | (unsigned long long)(0xFFFFFFFFu - (uint32_t)g);
    // a maximum only grows, so a stale look can at worst ask for an atomic that changes nothing
    if (to_g > __hip_atomic_load(best + g, __ATOMIC_RELAXED, kS)) atomicMax(best + g, to_g);
    if (to_q > __hip_atomic_load(best + gq, __ATOMIC_RELAXED, kS)) atomicMax(best + gq, to_q);
  }
}

// grid (ceil(H * W / 256), B): the threads of group peaks decide.  A decision reads its own slot and two distances, and
// writes its own slot and its own lab: no decision sees another one's.
__global__ __launch_bounds__(kSpThreads) void split_decide_kernel(const int32_t* __restrict__ d2, SpWs ws, int n_px,
                                                                  int round, long long num2, long long den2,
                                                                  int min_peak_d2) {
  if (split_skips(ws, round)) return;
  const int p = blockIdx.x * kSpThreads + threadIdx.x;
  const int64_t img = (int64_t)blockIdx.y * n_px;
  bool linked = false;
  if (p < n_px && ws.key[img + p] >= 0 && ws.lab[img + p] == p) {
    const unsigned long long b = ws.best[img + p];
    if (b != 0ull) {
      ws.best[img + p] = 0ull;
      const int o = (int)(0xFFFFFFFFu - (uint32_t)(b & 0xFFFFFFFFull));
      const long long s = (long long)(b >> 32);
      const int mine = d2[img + p];
      linked = sp_key(d2[img + o], o) > sp_key(mine, p) &&
               (mine < min_peak_d2 || s * den2 >= num2 * (long long)mine);
      if (linked) __hip_atomic_store(ws.lab + img + p, o, __ATOMIC_RELAXED, kS);
    }
  }
  sp_count(linked, ws.cnt + blockIdx.y * kSpCounters + round);
}

// grid (ceil(H * W / 256), B)
__global__ __launch_bounds__(kSpThreads) void split_keep_kernel(const int32_t* __restrict__ d2, SpWs ws, int n_px, int M) {
  const int p = blockIdx.x * kSpThreads + threadIdx.x;
  if (p >= n_px) return;
  const int64_t img = (int64_t)blockIdx.y * n_px;
  const int k = ws.key[img + p];
  if (k < 0 || ws.lab[img + p] != p) return;
  unsigned long long* keep = ws.keep + (int64_t)blockIdx.y * M + k;
  const unsigned long long mine = sp_key(d2[img + p], p);
  if (mine > __hip_atomic_load(keep, __ATOMIC_RELAXED, kS)) atomicMax(keep, mine);
}

// grid (chunks, B): thread t owns the pixels chunk * 1024 + j * 256 + t.  nid[p] = the id of the group whose peak p is
// (the kept id, or kSpExtraFlag until split_assign), -1 where p is no group's peak.
__global__ __launch_bounds__(kSpThreads) void split_count_kernel(const int32_t* __restrict__ d2, SpWs ws,
                                                                 int32_t* __restrict__ info, int n_px, int W, int M) {
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const int64_t img = (int64_t)blockIdx.y * n_px;
  int32_t* nid = reinterpret_cast<int32_t*>(ws.best + img);  // 4 * p < 8 * n_px: inside this image's slots
  int mine = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = blockIdx.x * kSpChunk + j * kSpThreads + threadIdx.x;
    bool extra = false;
    if (p < n_px) {
      const int k = ws.key[img + p];
      int id = -1;
      if (k >= 0 && ws.lab[img + p] == p) {
        const int d = d2[img + p];
        extra = sp_key(d, p) != ws.keep[(int64_t)blockIdx.y * M + k];
        id = extra ? kSpExtraFlag : k;
        if (!extra) reinterpret_cast<int4*>(info)[(int64_t)blockIdx.y * M + k] = make_int4(k, p % W, p / W, d);
      }
      nid[p] = id;
    }
    mine += (int)__popcll(__ballot(extra));
  }
  if ((threadIdx.x & 63) == 0 && mine != 0) atomicAdd(&s_n, mine);
  __syncthreads();
  if (threadIdx.x == 0) ws.chunk[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s_n;
}

// grid B, 1024 threads: the chunk counts become exclusive prefix sums; status
constexpr int kSpScanThreads = 1024;
__global__ __launch_bounds__(kSpScanThreads) void split_scan_kernel(SpWs ws, int32_t* __restrict__ status, int chunks,
                                                                    int N, int rounds) {
  __shared__ int s_scan[kSpScanThreads];
  const int b = blockIdx.x, t = threadIdx.x;
  int32_t* c = ws.chunk + (int64_t)b * chunks;
  const int per = ceil_div(chunks, kSpScanThreads);
  const int i0 = t * per < chunks ? t * per : chunks, i1 = i0 + per < chunks ? i0 + per : chunks;
  int mine = 0;
  for (int i = i0; i < i1; ++i) mine += c[i];
  s_scan[t] = mine;
  __syncthreads();
  for (int o = 1; o < kSpScanThreads; o <<= 1) {  // inclusive scan, 10 rounds
    const int v = t >= o ? s_scan[t - o] : 0;
    __syncthreads();
    s_scan[t] += v;
    __syncthreads();
  }
  int run = s_scan[t] - mine;
  for (int i = i0; i < i1; ++i) {
    const int v = c[i];
    c[i] = run;
    run += v;
  }
  if (t == kSpScanThreads - 1) {
    const int32_t* cnt = ws.cnt + b * kSpCounters;
    reinterpret_cast<int4*>(status)[b] = make_int4(N + s_scan[t], cnt[kSpBasins], cnt[rounds - 1], rounds);
  }
}

// grid (chunks, B), split_count's layout: the flagged peaks of the chunk in raster order, after the chunks before it
__global__ __launch_bounds__(kSpThreads) void split_assign_kernel(const int32_t* __restrict__ d2, SpWs ws,
                                                                  int32_t* __restrict__ info, int n_px, int W, int N,
                                                                  int M) {
  __shared__ int s_cnt[4 * (kSpThreads / 64)];
  const int64_t img = (int64_t)blockIdx.y * n_px;
  int32_t* nid = reinterpret_cast<int32_t*>(ws.best + img);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int kWaves = kSpThreads / 64;
  bool flag[4];
  int before[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = blockIdx.x * kSpChunk + j * kSpThreads + threadIdx.x;
    flag[j] = p < n_px && nid[p] == kSpExtraFlag;
    const unsigned long long m = __ballot(flag[j]);
    before[j] = (int)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[j * kWaves + wave] = (int)__popcll(m);
  }
  __syncthreads();
  const int base = N + ws.chunk[(int64_t)blockIdx.y * gridDim.x + blockIdx.x];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!flag[j]) continue;
    const int p = blockIdx.x * kSpChunk + j * kSpThreads + threadIdx.x;
    int id = base + before[j];
    for (int i = 0; i < j * kWaves + wave; ++i) id += s_cnt[i];
    nid[p] = id;
    if (id < M) reinterpret_cast<int4*>(info)[(int64_t)blockIdx.y * M + id] = make_int4(ws.key[img + p], p % W, p / W, d2[img + p]);
  }
}

// grid (ceil(H * W / 256), B)
__global__ __launch_bounds__(kSpThreads) void split_paint_kernel(SpWs ws, int32_t* __restrict__ out, int n_px, int M) {
  const int p = blockIdx.x * kSpThreads + threadIdx.x;
  if (p >= n_px) return;
  const int64_t img = (int64_t)blockIdx.y * n_px;
  const int k = ws.key[img + p];
  int v = -1;
  if (k >= 0) {
    const int id = reinterpret_cast<const int32_t*>(ws.best + img)[ws.lab[img + p]];
    v = id < M ? id : k;  // past the id space: not split off
  }
  out[img + p] = v;
}

bool sp_size_ok(int B, int H, int W, int N, int M) {
  return H <= kMapMaxSide && W <= kMapMaxSide && B <= kMapMaxBatch && N <= M && M <= kMapMaxIds;
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_labelmap_split_workspace(int B, int H, int W, int M) {
  if (B <= 0 || H <= 0 || W <= 0 || M < 0 || !sp_size_ok(B, H, W, 0, M)) return -1;
  return sp_workspace_bytes(B, H, W, M);
}

extern "C" int wm2f_labelmap_split(const void* map, int dtype, const int32_t* d2, int32_t* out, int32_t* info,
                                   int32_t* status, void* workspace, int B, int H, int W, int N, int M, int num, int den,
                                   int min_peak_d2, int rounds, void* stream) {
  const char* who = "wm2f_labelmap_split";
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N >= 0 && M >= 0, "%s: bad size", who);
  if (!sp_size_ok(B, H, W, N, M)) {
    set_error("%s: sides <= %d, B <= %d, N <= M <= %d (got %d x %d, %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch, kMapMaxIds,
              H, W, B, N, M);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(rounds >= 1 && rounds <= kSpMaxRounds, "%s: 1 <= rounds <= %d, got %d", who, kSpMaxRounds, rounds);
  WM2F_REQUIRE(den >= 1 && den <= kSpMaxDen && num >= 0 && num <= den, "%s: 0 <= num <= den, 1 <= den <= %d, got %d / %d",
               who, kSpMaxDen, num, den);
  WM2F_REQUIRE(min_peak_d2 >= 0, "%s: min_peak_d2 must not be negative", who);
  WM2F_REQUIRE(map && d2 && out && status && workspace && (info || M == 0), "%s: null pointer", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  WM2F_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0 && reinterpret_cast<uintptr_t>(info) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(status) % 16 == 0,
               "%s: workspace, info and status must be 16-byte aligned", who);
  const int64_t all_px = (int64_t)B * H * W;
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + (uintptr_t)all_px * 4;
  const uintptr_t m0 = reinterpret_cast<uintptr_t>(map), m1 = m0 + (uintptr_t)all_px * map_elem_bytes(dtype);
  const uintptr_t d0 = reinterpret_cast<uintptr_t>(d2), d1 = d0 + (uintptr_t)all_px * 4;
  WM2F_REQUIRE((o1 <= m0 || m1 <= o0) && (o1 <= d0 || d1 <= o0), "%s: out overlaps map or d2", who);

  hipStream_t s = (hipStream_t)stream;
  const SpWs ws = sp_carve(workspace, B, H, W, M);
  const int n_px = H * W;  // <= 2^28
  const dim3 px_grid((unsigned)ceil_div(n_px, kSpThreads), (unsigned)B);
  const int chunks = sp_chunks(H, W);
  const dim3 chunk_grid((unsigned)chunks, (unsigned)B);
  const int n_init = B * (M > kSpCounters ? M : kSpCounters);
  hipLaunchKernelGGL(split_init_kernel, dim3(ceil_div(n_init, kSpThreads)), dim3(kSpThreads), 0, s, ws, info, B, M);
  for_map_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(split_ascent_kernel<decltype(dt)::value>, px_grid, dim3(kSpThreads), 0, s, map, d2, ws, H, W, N);
  });
  hipLaunchKernelGGL(split_flatten_kernel, px_grid, dim3(kSpThreads), 0, s, ws, n_px, 0);
  WM2F_CHECK_LAUNCH(who);
  const long long num2 = (long long)num * num, den2 = (long long)den * den;
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(split_pass_kernel, px_grid, dim3(kSpThreads), 0, s, d2, ws, H, W, r);
    hipLaunchKernelGGL(split_decide_kernel, px_grid, dim3(kSpThreads), 0, s, d2, ws, n_px, r, num2, den2, min_peak_d2);
    hipLaunchKernelGGL(split_flatten_kernel, px_grid, dim3(kSpThreads), 0, s, ws, n_px, r);
  }
  WM2F_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(split_keep_kernel, px_grid, dim3(kSpThreads), 0, s, d2, ws, n_px, M);
  hipLaunchKernelGGL(split_count_kernel, chunk_grid, dim3(kSpThreads), 0, s, d2, ws, info, n_px, W, M);
  hipLaunchKernelGGL(split_scan_kernel, dim3((unsigned)B), dim3(kSpScanThreads), 0, s, ws, status, chunks, N, rounds);
  hipLaunchKernelGGL(split_assign_kernel, chunk_grid, dim3(kSpThreads), 0, s, d2, ws, info, n_px, W, N, M);
  hipLaunchKernelGGL(split_paint_kernel, px_grid, dim3(kSpThreads), 0, s, ws, out, n_px, M);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
