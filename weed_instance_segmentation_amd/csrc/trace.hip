// Tracing id maps into polygons on the device, the inverse of polygon.hip and a sibling of rle.hip.
// The contract -- boundary sides as directed edges, the left-first successor, leaders, ranks, the two emission rules, the
// CSR layout -- is written out in include/wm2f.h; tests/trace_reference.py restates it with plain loops.  Everything is
// integer and every place in the result is computed, never drawn from an atomic, so the result is bit-identical from run
// to run.  The chain is the same for any number of ids, segments and loops:
//   count    trace_count_kernel: one thread per pixel, the side mask from the four neighbours, an exclusive scan of the
//            edge counts inside the block of kTracePixels pixels; the workspace word of a pixel is (prefix in the block
//            << 4) | mask, the block's total goes to a table that trace_block_scan_kernel (one block) turns into
//            exclusive offsets, the grand total E into counts[0].  The index of edge (pixel, side) is
//            offset[block] + prefix + popcount(mask & ((1 << side) - 1)): edges are numbered in key order.
//   link     trace_link_kernel: one thread per pixel with a boundary side.  For each side it reads the two pixels ahead
//            (left-first rule), looks the successor's index up in the workspace words and stores key[e], next[e] and
//            prev[next[e]] (every edge has one predecessor, so each word has one writer).
//   rank     trace_jump_kernel, ceil(log2 E) launches: pointer jumping BACKWARDS.  After round r an edge knows the
//            lowest index among itself and its 2^r - 1 predecessors, how many hops back its first occurrence lies, and
//            its 2^r-th predecessor.  A window that wraps the loop meets the minimum again further back and keeps the
//            nearer one, so at the end the minimum is the loop's leader and the hop count is the rank.
//   flags    trace_flags_kernel: one thread per edge, the emission rule of the chosen coordinates, and the leader mark.
//   loops    trace_loops_kernel: a leader stores its loop's sort key (image * N + id) << 32 | leader and its length.
//   scatter  trace_scatter_kernel: an edge goes to base[loop] + rank in loop order with its flag and its area term.
//   emit     trace_emit_kernel: a flagged place stores its point at (inclusive flag prefix) - 1.
// Between them the host layer runs prefix sums over edge-sized arrays and one sort over the loops (ops/trace.py).
// Every store is guarded by the range of the array it goes to, so a bad table cannot write elsewhere.
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kTracePixels = 256;     // pixels (and threads) of a count block
constexpr int kTraceThreads = 256;    // per-edge kernels
constexpr int kTraceScanThreads = 1024;
constexpr int kTraceMaxBatch = 4096;
constexpr int kTraceEdgeArrays = 9;   // key, next, prev, leader, rank, and four more for the jumping
constexpr int kIdBackground = kMapBackground;
constexpr int kIdOut = kMapOutOfRange;  // a value outside [-1, N)
constexpr int kIdOffMap = -3;           // beyond the map

template <int DT>
struct MapReader {
  using E = typename MapElem<DT>::type;
  const E* base;  // of the image
  int H, W, N;
  __device__ __forceinline__ int at(int y, int x) const {
    if (y < 0 || y >= H || x < 0 || x >= W) return kIdOffMap;
    return map_id_or_code<DT>((uint32_t)base[y * W + x], N);
  }
};

// heading d: 0 east, 1 south, 2 west, 3 north (x right, y down)
__device__ __forceinline__ int head_dx(int d) { return d == 0 ? 1 : d == 2 ? -1 : 0; }
__device__ __forceinline__ int head_dy(int d) { return d == 1 ? 1 : d == 3 ? -1 : 0; }

// exclusive scan of v over a block of kThreads threads (a multiple of 64); total in every thread
template <int kThreads>
__device__ __forceinline__ int block_exclusive_scan(int v, int* __restrict__ wave_sums, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  __syncthreads();  // the sums of an earlier call have been read
  if (lane == kWave - 1) wave_sums[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kThreads / kWave; ++w) {
    const int s = wave_sums[w];
    if (w < wave) before += s;
    all += s;
  }
  total = all;
  return before + inc - v;
}

// ---- count ----------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(kTracePixels) void trace_count_kernel(const void* __restrict__ map,
                                                                   uint32_t* __restrict__ words,
                                                                   int32_t* __restrict__ block_totals,
                                                                   int32_t* __restrict__ counts, int B, int H, int W,
                                                                   int N) {
  __shared__ int wave_sums[kTracePixels / kWave];
  const int HW = H * W, total_pixels = B * HW;  // < 2^29
  const int g = blockIdx.x * kTracePixels + threadIdx.x;
  int mask = 0;
  if (g < total_pixels) {
    const int b = g / HW, rem = g - b * HW, y = rem / W, x = rem - y * W;
    MapReader<DT> m{reinterpret_cast<const typename MapReader<DT>::E*>(map) + (int64_t)b * HW, H, W, N};
    const int k = m.at(y, x);
    if (k == kIdOut) atomicAdd(counts + 1 + b, 1);
    if (k >= 0) {
      mask = (m.at(y - 1, x) != k ? 1 : 0) | (m.at(y, x + 1) != k ? 2 : 0) | (m.at(y + 1, x) != k ? 4 : 0) |
             (m.at(y, x - 1) != k ? 8 : 0);
    }
  }
  int total;
  const int before = block_exclusive_scan<kTracePixels>(__popc(mask), wave_sums, total);  // <= 4 * 255
  if (g < total_pixels) words[g] = ((uint32_t)before << 4) | (uint32_t)mask;
  if (threadIdx.x == 0) block_totals[blockIdx.x] = total;
}

// block_totals (n) -> exclusive offsets in place; counts[0] <- the grand total
__global__ __launch_bounds__(kTraceScanThreads) void trace_block_scan_kernel(int32_t* __restrict__ block_totals, int n,
                                                                             int32_t* __restrict__ counts) {
  __shared__ int wave_sums[kTraceScanThreads / kWave];
  int carry = 0;
  for (int i0 = 0; i0 < n; i0 += kTraceScanThreads) {  // block-uniform
    const int i = i0 + threadIdx.x;
    const int v = i < n ? block_totals[i] : 0;
    int total;
    const int before = block_exclusive_scan<kTraceScanThreads>(v, wave_sums, total);
    if (i < n) block_totals[i] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) counts[0] = carry;
}

__device__ __forceinline__ int edge_index(const uint32_t* __restrict__ words, const int32_t* __restrict__ block_offsets,
                                          int g, int side) {
  const uint32_t w = words[g];
  return block_offsets[g / kTracePixels] + (int)(w >> 4) + __popc(w & 15u & ((1u << side) - 1u));
}

// ---- link -----------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(kTracePixels) void trace_link_kernel(const void* __restrict__ map,
                                                                  const uint32_t* __restrict__ words,
                                                                  const int32_t* __restrict__ block_offsets,
                                                                  int32_t* __restrict__ key, int32_t* __restrict__ next,
                                                                  int32_t* __restrict__ prev, int E, int B, int H, int W,
                                                                  int N) {
  const int HW = H * W, total_pixels = B * HW;
  const int g = blockIdx.x * kTracePixels + threadIdx.x;
  if (g >= total_pixels) return;
  const uint32_t word = words[g];
  const int mask = (int)(word & 15u);
  if (mask == 0) return;
  const int b = g / HW, rem = g - b * HW, y = rem / W, x = rem - y * W;
  MapReader<DT> m{reinterpret_cast<const typename MapReader<DT>::E*>(map) + (int64_t)b * HW, H, W, N};
  const int k = m.at(y, x);
  const int first = block_offsets[g / kTracePixels] + (int)(word >> 4);
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    if (!(mask & (1 << d))) continue;
    const int e = first + __popc(mask & ((1 << d) - 1));
    const int rx = x + head_dx(d), ry = y + head_dy(d);      // the pixel ahead-right
    const int left = (d + 3) & 3;
    const int lx = rx + head_dx(left), ly = ry + head_dy(left);  // the pixel ahead-left
    int sg, sd;  // the successor's pixel and side
    if (m.at(ly, lx) == k) {
      sg = b * HW + ly * W + lx;
      sd = left;
    } else if (m.at(ry, rx) == k) {
      sg = b * HW + ry * W + rx;
      sd = d;
    } else {
      sg = g;
      sd = (d + 1) & 3;
    }
    const int e2 = edge_index(words, block_offsets, sg, sd);
    if (e >= 0 && e < E) {
      key[e] = 4 * g + d;
      next[e] = e2;
      if (e2 >= 0 && e2 < E) prev[e2] = e;
    }
  }
}

// ---- rank: pointer jumping backwards --------------------------------------------------------------------------------
// In: (m, off, pv) of windows of `len` edges (kFirst: the window is the edge itself and pv is prev).  Out: of 2 * len.
template <bool kFirst>
__global__ __launch_bounds__(kTraceThreads) void trace_jump_kernel(const int32_t* __restrict__ m_in,
                                                                   const int32_t* __restrict__ off_in,
                                                                   const int32_t* __restrict__ pv_in,
                                                                   int32_t* __restrict__ m_out,
                                                                   int32_t* __restrict__ off_out,
                                                                   int32_t* __restrict__ pv_out, int E, uint32_t len) {
  const int e = blockIdx.x * kTraceThreads + threadIdx.x;
  if (e >= E) return;
  int p = pv_in[e];
  if (p < 0 || p >= E) p = e;  // never for a table the link launch wrote
  const int ma = kFirst ? e : m_in[e], mb = kFirst ? p : m_in[p];
  int m = ma;
  uint32_t off = kFirst ? 0u : (uint32_t)off_in[e];
  if (mb < ma) {  // a tie is the same edge met again after a whole turn: the nearer one stays
    m = mb;
    off = len + (kFirst ? 0u : (uint32_t)off_in[p]);
  }
  m_out[e] = m;
  off_out[e] = (int32_t)off;
  pv_out[e] = pv_in[p];
}

__device__ __forceinline__ int in_range(int v, int n) { return v >= 0 && v < n; }

// ---- flags ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTraceThreads) void trace_flags_kernel(const int32_t* __restrict__ key,
                                                                    const int32_t* __restrict__ next,
                                                                    const int32_t* __restrict__ prev,
                                                                    const int32_t* __restrict__ leader,
                                                                    int32_t* __restrict__ flag, int32_t* __restrict__ lead,
                                                                    int E, int H, int W, int coords, int simplify) {
  const int e = blockIdx.x * kTraceThreads + threadIdx.x;
  if (e >= E) return;
  const int ke = key[e], g = ke >> 2, d = ke & 3;
  int pe = prev[e];
  if (!in_range(pe, E)) pe = e;
  const int kp = key[pe];
  const bool is_lead = leader[e] == e;
  int f;
  if (coords == 0) {
    f = simplify ? (kp & 3) != d : 1;
  } else {
    const int a = kp >> 2;
    if (a == g) {
      f = 0;
      if (is_lead) {  // a loop round one pixel: no edge changes pixel, its leader emits the pixel
        int h = e;
        bool same = true;
        for (int i = 0; i < 3; ++i) {
          h = next[h];
          if (!in_range(h, E)) { same = false; break; }
          same = same && (key[h] >> 2) == g;
        }
        f = same ? 1 : 0;
      }
    } else if (!simplify) {
      f = 1;
    } else {
      int h = e;
      int c = g;
      for (int i = 0; i < 4 && c == g; ++i) {  // at most three edges of this pixel follow
        h = next[h];
        if (!in_range(h, E)) break;
        c = key[h] >> 2;
      }
      // a, g and c lie in one image: the image's offset cancels in the differences
      const int ay = a / W, ax = a - ay * W, by = g / W, bx = g - by * W, cy = c / W, cx = c - cy * W;
      f = !(bx - ax == cx - bx && by - ay == cy - by);
    }
  }
  flag[e] = f;
  lead[e] = is_lead ? 1 : 0;
}

// ---- loops ----------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(kTraceThreads) void trace_loops_kernel(const void* __restrict__ map,
                                                                    const int32_t* __restrict__ key,
                                                                    const int32_t* __restrict__ prev,
                                                                    const int32_t* __restrict__ leader,
                                                                    const int32_t* __restrict__ rank,
                                                                    const int32_t* __restrict__ lead_prefix,
                                                                    int64_t* __restrict__ loop_key,
                                                                    int32_t* __restrict__ loop_len, int E, int n_loops,
                                                                    int B, int H, int W, int N) {
  using T = typename MapReader<DT>::E;
  const int e = blockIdx.x * kTraceThreads + threadIdx.x;
  if (e >= E || leader[e] != e) return;
  const int j = lead_prefix[e] - 1;
  if (!in_range(j, n_loops)) return;
  const int g = key[e] >> 2, HW = H * W;
  int id = in_range(g, B * HW) ? map_id_or_code<DT>((uint32_t)reinterpret_cast<const T*>(map)[g], N) : 0;
  if (id < 0) id = 0;  // never: an edge belongs to a pixel with an id
  const int b = g / HW;
  const int pe = prev[e];
  loop_key[j] = ((int64_t)(b * N + id) << 32) | (int64_t)e;
  loop_len[j] = in_range(pe, E) ? rank[pe] + 1 : 0;
}

// ---- scatter to loop order ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTraceThreads) void trace_scatter_kernel(const int32_t* __restrict__ key,
                                                                      const int32_t* __restrict__ leader,
                                                                      const int32_t* __restrict__ rank,
                                                                      const int32_t* __restrict__ flag,
                                                                      const int32_t* __restrict__ lead_prefix,
                                                                      const int32_t* __restrict__ loop_place,
                                                                      const int32_t* __restrict__ loop_base,
                                                                      int32_t* __restrict__ flag_sorted,
                                                                      int32_t* __restrict__ edge_sorted,
                                                                      int32_t* __restrict__ term_sorted, int E,
                                                                      int n_loops, int H, int W) {
  const int e = blockIdx.x * kTraceThreads + threadIdx.x;
  if (e >= E) return;
  const int l = leader[e];
  if (!in_range(l, E)) return;
  const int j = lead_prefix[l] - 1;
  if (!in_range(j, n_loops)) return;
  const int i = loop_place[j];
  if (!in_range(i, n_loops)) return;
  const int r = rank[e];
  const int64_t pos = (int64_t)loop_base[i] + r;
  if (r < 0 || pos >= (int64_t)loop_base[i + 1] || pos >= (int64_t)E) return;
  const int ke = key[e], g = ke >> 2, d = ke & 3;
  const int rem = g % (H * W), y = rem / W, x = rem - y * W;
  // x_tail * y_head - x_head * y_tail of the unit edge
  const int term = d == 0 ? -y : d == 1 ? x + 1 : d == 2 ? y + 1 : -x;
  flag_sorted[pos] = flag[e];
  edge_sorted[pos] = e;
  term_sorted[pos] = term;
}

// ---- emit -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTraceThreads) void trace_emit_kernel(const int32_t* __restrict__ key,
                                                                   const int32_t* __restrict__ flag_sorted,
                                                                   const int32_t* __restrict__ edge_sorted,
                                                                   const int32_t* __restrict__ flag_prefix,
                                                                   int2* __restrict__ points, int E, int P, int H, int W,
                                                                   int coords) {
  const int pos = blockIdx.x * kTraceThreads + threadIdx.x;
  if (pos >= E || !flag_sorted[pos]) return;
  const int idx = flag_prefix[pos] - 1, e = edge_sorted[pos];
  if (!in_range(idx, P) || !in_range(e, E)) return;
  const int ke = key[e], g = ke >> 2, d = ke & 3;
  const int rem = g % (H * W), y = rem / W, x = rem - y * W;
  int2 p = make_int2(x, y);
  if (coords == 0) {  // the tail vertex: top (x, y), right (x + 1, y), bottom (x + 1, y + 1), left (x, y + 1)
    p.x += (d == 1 || d == 2) ? 1 : 0;
    p.y += (d == 2 || d == 3) ? 1 : 0;
  }
  points[idx] = p;
}

bool trace_sizes_ok(int B, int H, int W, int N) {
  if (B <= 0 || H <= 0 || W <= 0 || N < 0 || N > WM2F_RLE_MAX_IDS || B > kTraceMaxBatch) return false;
  return 4 * (int64_t)B * H * W < ((int64_t)1 << 31);
}

int trace_blocks(int B, int H, int W) { return ceil_div(B * H * W, kTracePixels); }

int check_trace(const char* who, int dtype, int B, int H, int W, int N) {
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N >= 0, "%s: bad size", who);
  if (!trace_sizes_ok(B, H, W, N)) {
    set_error("%s: 4 * B * H * W < 2^31, B <= %d, N <= %d (got %d x %d x %d, N = %d)", who, kTraceMaxBatch,
              WM2F_RLE_MAX_IDS, B, H, W, N);
    return WM2F_EUNSUPPORTED;
  }
  return WM2F_OK;
}

struct EdgeArrays {
  int32_t *key, *next, *prev, *leader, *rank, *pv, *m2, *off2, *pv2;
};

EdgeArrays edge_arrays(void* edge_workspace, int E) {
  int32_t* p = (int32_t*)edge_workspace;
  const int64_t n = E;
  return {p, p + n, p + 2 * n, p + 3 * n, p + 4 * n, p + 5 * n, p + 6 * n, p + 7 * n, p + 8 * n};
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_trace_workspace(int B, int H, int W, int N) {
  if (!trace_sizes_ok(B, H, W, N)) return -1;
  return ((int64_t)B * H * W + trace_blocks(B, H, W)) * (int64_t)sizeof(int32_t);
}

extern "C" int64_t wm2f_trace_edge_workspace(int64_t E) {
  if (E <= 0 || E >= ((int64_t)1 << 31)) return -1;
  return kTraceEdgeArrays * E * (int64_t)sizeof(int32_t);
}

extern "C" int wm2f_trace_rounds(int64_t E) {
  if (E <= 0 || E >= ((int64_t)1 << 31)) return -1;
  int r = 1;  // at least one: the first round also sets the tables up
  while (((int64_t)1 << r) < E) ++r;
  return r;
}

extern "C" int wm2f_trace_count(const void* map, int dtype, int32_t* counts, void* workspace, int B, int H, int W, int N,
                                void* stream) {
  const char* who = "wm2f_trace_count";
  WM2F_REQUIRE(map && counts && workspace, "%s: null pointer", who);
  if (const int rc = check_trace(who, dtype, B, H, W, N)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = trace_blocks(B, H, W);
  uint32_t* words = (uint32_t*)workspace;
  int32_t* block_totals = (int32_t*)workspace + (int64_t)B * H * W;
  WM2F_REQUIRE(hipMemsetAsync(counts, 0, (size_t)(B + 1) * sizeof(int32_t), s) == hipSuccess, "%s: clearing failed", who);
  for_map_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(trace_count_kernel<decltype(dt)::value>, dim3(blocks), dim3(kTracePixels), 0, s, map, words,
                       block_totals, counts, B, H, W, N);
  });
  WM2F_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(trace_block_scan_kernel, dim3(1), dim3(kTraceScanThreads), 0, s, block_totals, blocks, counts);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_trace_link(const void* map, int dtype, const void* workspace, void* edge_workspace, int E, int B,
                               int H, int W, int N, void* stream) {
  const char* who = "wm2f_trace_link";
  WM2F_REQUIRE(map && workspace && edge_workspace, "%s: null pointer", who);
  WM2F_REQUIRE(E > 0, "%s: no edges", who);
  if (const int rc = check_trace(who, dtype, B, H, W, N)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t* words = (const uint32_t*)workspace;
  const int32_t* block_offsets = (const int32_t*)workspace + (int64_t)B * H * W;
  const EdgeArrays a = edge_arrays(edge_workspace, E);
  // a map that changed since the count launch leaves words unwritten: they must still be in range
  WM2F_REQUIRE(hipMemsetAsync(a.key, 0, (size_t)3 * E * sizeof(int32_t), s) == hipSuccess, "%s: clearing failed", who);
  for_map_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(trace_link_kernel<decltype(dt)::value>, dim3(trace_blocks(B, H, W)), dim3(kTracePixels), 0, s, map,
                       words, block_offsets, a.key, a.next, a.prev, E, B, H, W, N);
  });
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_trace_rank(void* edge_workspace, int E, void* stream) {
  const char* who = "wm2f_trace_rank";
  WM2F_REQUIRE(edge_workspace, "%s: null pointer", who);
  WM2F_REQUIRE(E > 0, "%s: no edges", who);
  hipStream_t s = (hipStream_t)stream;
  const EdgeArrays a = edge_arrays(edge_workspace, E);
  const int rounds = wm2f_trace_rounds(E), grid = ceil_div(E, kTraceThreads);
  for (int r = 1; r <= rounds; ++r) {  // the last round writes (leader, rank, pv)
    const bool to_final = ((rounds - r) & 1) == 0;
    int32_t *mo = to_final ? a.leader : a.m2, *oo = to_final ? a.rank : a.off2, *po = to_final ? a.pv : a.pv2;
    const int32_t *mi = to_final ? a.m2 : a.leader, *oi = to_final ? a.off2 : a.rank, *pi = to_final ? a.pv2 : a.pv;
    const uint32_t len = 1u << (r - 1);
    if (r == 1)
      hipLaunchKernelGGL(trace_jump_kernel<true>, dim3(grid), dim3(kTraceThreads), 0, s, nullptr, nullptr, a.prev, mo, oo,
                         po, E, len);
    else
      hipLaunchKernelGGL(trace_jump_kernel<false>, dim3(grid), dim3(kTraceThreads), 0, s, mi, oi, pi, mo, oo, po, E, len);
    WM2F_CHECK_LAUNCH(who);
  }
  return WM2F_OK;
}

extern "C" int wm2f_trace_flags(const void* edge_workspace, int32_t* flag, int32_t* lead, int E, int H, int W, int coords,
                                int simplify, void* stream) {
  const char* who = "wm2f_trace_flags";
  WM2F_REQUIRE(edge_workspace && flag && lead, "%s: null pointer", who);
  WM2F_REQUIRE(E > 0 && H > 0 && W > 0, "%s: bad size", who);
  WM2F_REQUIRE(coords == 0 || coords == 1, "%s: coords must be 0 (crack) or 1 (pixel), got %d", who, coords);
  const EdgeArrays a = edge_arrays(const_cast<void*>(edge_workspace), E);
  hipLaunchKernelGGL(trace_flags_kernel, dim3(ceil_div(E, kTraceThreads)), dim3(kTraceThreads), 0, (hipStream_t)stream,
                     a.key, a.next, a.prev, a.leader, flag, lead, E, H, W, coords, simplify ? 1 : 0);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_trace_loops(const void* map, int dtype, const void* edge_workspace, const int32_t* lead_prefix,
                                int64_t* loop_key, int32_t* loop_len, int E, int n_loops, int B, int H, int W, int N,
                                void* stream) {
  const char* who = "wm2f_trace_loops";
  WM2F_REQUIRE(map && edge_workspace && lead_prefix && loop_key && loop_len, "%s: null pointer", who);
  WM2F_REQUIRE(E > 0 && n_loops > 0, "%s: nothing to do", who);
  if (const int rc = check_trace(who, dtype, B, H, W, N)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const EdgeArrays a = edge_arrays(const_cast<void*>(edge_workspace), E);
  WM2F_REQUIRE(hipMemsetAsync(loop_key, 0, (size_t)n_loops * sizeof(int64_t), s) == hipSuccess &&
                   hipMemsetAsync(loop_len, 0, (size_t)n_loops * sizeof(int32_t), s) == hipSuccess,
               "%s: clearing failed", who);
  for_map_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(trace_loops_kernel<decltype(dt)::value>, dim3(ceil_div(E, kTraceThreads)), dim3(kTraceThreads), 0, s,
                       map, a.key, a.prev, a.leader, a.rank, lead_prefix, loop_key, loop_len, E, n_loops, B, H, W, N);
  });
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_trace_scatter(const void* edge_workspace, const int32_t* flag, const int32_t* lead_prefix,
                                  const int32_t* loop_place, const int32_t* loop_base, int32_t* flag_sorted,
                                  int32_t* edge_sorted, int32_t* term_sorted, int E, int n_loops, int H, int W,
                                  void* stream) {
  const char* who = "wm2f_trace_scatter";
  WM2F_REQUIRE(edge_workspace && flag && lead_prefix && loop_place && loop_base && flag_sorted && edge_sorted && term_sorted,
               "%s: null pointer", who);
  WM2F_REQUIRE(E > 0 && n_loops > 0 && H > 0 && W > 0, "%s: bad size", who);
  hipStream_t s = (hipStream_t)stream;
  const EdgeArrays a = edge_arrays(const_cast<void*>(edge_workspace), E);
  WM2F_REQUIRE(hipMemsetAsync(flag_sorted, 0, (size_t)E * sizeof(int32_t), s) == hipSuccess &&
                   hipMemsetAsync(term_sorted, 0, (size_t)E * sizeof(int32_t), s) == hipSuccess,
               "%s: clearing failed", who);
  hipLaunchKernelGGL(trace_scatter_kernel, dim3(ceil_div(E, kTraceThreads)), dim3(kTraceThreads), 0, s, a.key, a.leader,
                     a.rank, flag, lead_prefix, loop_place, loop_base, flag_sorted, edge_sorted, term_sorted, E, n_loops, H,
                     W);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_trace_emit(const void* edge_workspace, const int32_t* flag_sorted, const int32_t* edge_sorted,
                               const int32_t* flag_prefix, int32_t* points, int E, int P, int H, int W, int coords,
                               void* stream) {
  const char* who = "wm2f_trace_emit";
  WM2F_REQUIRE(edge_workspace && flag_sorted && edge_sorted && flag_prefix && points, "%s: null pointer", who);
  WM2F_REQUIRE(E > 0 && P > 0 && H > 0 && W > 0, "%s: bad size", who);
  WM2F_REQUIRE(coords == 0 || coords == 1, "%s: coords must be 0 (crack) or 1 (pixel), got %d", who, coords);
  hipStream_t s = (hipStream_t)stream;
  const EdgeArrays a = edge_arrays(const_cast<void*>(edge_workspace), E);
  WM2F_REQUIRE(hipMemsetAsync(points, 0, (size_t)P * 2 * sizeof(int32_t), s) == hipSuccess, "%s: clearing failed", who);
  hipLaunchKernelGGL(trace_emit_kernel, dim3(ceil_div(E, kTraceThreads)), dim3(kTraceThreads), 0, s, a.key, flag_sorted,
                     edge_sorted, flag_prefix, (int2*)points, E, P, H, W, coords);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
