// Run-length encoding and decoding of id maps on the device.  The contract -- toggle positions,
// slots, scan orders, the CSR layout -- is written out in include/wm2f.h; tests/rle_reference.py restates it with plain
// loops.  Everything is integer and every toggle's place in the result is computed, never drawn from an atomic, so the
// result is bit-identical from run to run.
//
// The flattened map is cut into GROUPS of consecutive scan positions; group g of image b owns row (b, g) of a
// (B, G, N + 1) int32 table in the workspace.
//   order 0 (row-major)    a group is a run of whole rows, kRleMinGroup positions or more, at most kRleMaxGroups per
//                          image.  One wave owns a group and walks it 64 positions at a time (one coalesced load per
//                          step, kRleUnroll steps in flight).  A lane compares its slot with its left neighbour's (a
//                          wave shuffle; lane 0 takes the last slot of the step before, so runs cross row ends).  Steps
//                          without a transition -- nearly all of them -- end there.  Otherwise the wave loops over the
//                          distinct slots that toggle in the step: a ballot of the lanes that toggle slot k, a popcount
//                          of the lanes below for the rank, and one lane advances slot k's cursor in LDS.
//   order 1 (column-major) a group is one column.  A lane owns a column and walks down it, so a wave reads 64 adjacent
//                          pixels of a row per load and never strides by W.  The lane's cursors are its own row of the
//                          table, in global memory, touched only at a transition.
//   count launch           rle_count_kernel fills the table with each group's toggles per slot (order 0: counted in
//                          LDS, every entry stored; order 1: the table is cleared first and a lane increments its own
//                          row), rle_scan_kernel turns every slot's column of the table into exclusive prefixes along g
//                          and stores the totals.
//   write launch           the same walk; a toggle of slot k goes to offsets[b][k] + prefix[b][g][k] + its rank inside
//                          the group.  A position is stored only inside its slot's range of the CSR array.
//   paint                  rle_check_kernel refuses the whole call if one run is bad (the first bad run's index, by
//                          atomicMin, in a status word), rle_rank_kernel takes one wave per run and raises a rank map in
//                          scan order to the run's index + 1 (atomicMax: the later run wins whatever the schedule),
//                          rle_resolve_kernel writes values[rank - 1] where a rank was set.  Both return at once when the
//                          status word is set, so a refused call stores nothing into the map.
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kRleMinGroup = 2048;   // positions of an order-0 group, at least
constexpr int kRleMaxGroups = 1024;  // order-0 groups per image, at most
constexpr int kRleUnroll = 8;
constexpr int kRleNone = -1;  // beyond either end of the map
constexpr int kRleOut = -2;   // a value outside [-1, N)
constexpr int kScanThreads = 256;
constexpr int kPaintThreads = 256;

// slot of a map value: 0 for the background, id + 1 for an id in [0, N), kRleOut for everything else
template <int DT>
__device__ __forceinline__ int slot_of(uint32_t raw, int N) {
  if (map_is_background<DT>(raw)) return 0;
  int v;
  if (!map_int<DT>(raw, v)) return kRleOut;
  return (v >= 0 && v < N) ? v + 1 : kRleOut;  // map_id_or_code's ids, one up
}

// rows of an order-0 group
__host__ __device__ __forceinline__ int rle_group_rows(int H, int W) {
  const int a = ceil_div(kRleMinGroup, W), b = ceil_div(H, kRleMaxGroups);
  const int r = a > b ? a : b;
  return r > H ? H : r;
}

__host__ __device__ __forceinline__ int rle_groups(int H, int W, int order) {
  return order == 0 ? ceil_div(H, rle_group_rows(H, W)) : W;
}

// ---- order 0: one wave per group ------------------------------------------------------------------------------------
// kWrite == false: table row (b, g) <- the group's toggles per slot, out_of_range[b] += its values outside [-1, N).
// kWrite == true : table row (b, g) holds the exclusive prefixes; the positions go to out.
template <int DT, bool kWrite>
__global__ __launch_bounds__(kWave) void rle_rows_kernel(const void* __restrict__ map, int32_t* __restrict__ table,
                                                         int32_t* __restrict__ out_of_range,
                                                         const int32_t* __restrict__ offsets, int32_t* __restrict__ out,
                                                         int H, int W, int N, int rows) {
  using E = typename MapElem<DT>::type;
  extern __shared__ int32_t cursor[];  // N + 1: the group's count (count launch) or next rank (write launch) per slot
  const int lane = threadIdx.x, g = blockIdx.x, b = blockIdx.y, N1 = N + 1;
  const int HW = H * W;  // <= 2^28
  int32_t* row = table + ((int64_t)b * gridDim.x + g) * N1;
  for (int k = lane; k < N1; k += kWave) cursor[k] = kWrite ? row[k] : 0;
  __syncthreads();
  const E* base = reinterpret_cast<const E*>(map) + (int64_t)b * HW;
  const int32_t* offs = kWrite ? offsets + (int64_t)b * N1 : nullptr;
  const int t0 = g * rows * W;  // g * rows < H
  const bool last = g == (int)gridDim.x - 1;
  const int t1 = last ? HW + 1 : t0 + rows * W;  // the last group also owns the closing position HW
  int carry = t0 > 0 ? slot_of<DT>((uint32_t)base[t0 - 1], N) : kRleNone;
  int n_out = 0;
  for (int s0 = t0; s0 < t1; s0 += kWave * kRleUnroll) {  // wave-uniform
    uint32_t raw[kRleUnroll];
#pragma unroll
    for (int u = 0; u < kRleUnroll; ++u) {
      const int t = s0 + u * kWave + lane;
      raw[u] = t < HW ? (uint32_t)base[t] : 0u;
    }
#pragma unroll
    for (int u = 0; u < kRleUnroll; ++u) {
      const int ts = s0 + u * kWave;
      if (ts >= t1) break;  // wave-uniform
      const int t = ts + lane;
      const int cur = t < HW ? slot_of<DT>(raw[u], N) : kRleNone;
      int prev = __shfl_up(cur, 1);
      if (lane == 0) prev = carry;
      carry = __shfl(cur, kWave - 1);  // kRleNone past the map's end, where nothing follows
      if (!kWrite) n_out += __popcll(__ballot(t < t1 && cur == kRleOut));
      const bool differ = t < t1 && prev != cur;
      bool pend_prev = differ && prev >= 0, pend_cur = differ && cur >= 0;
      unsigned long long todo = __ballot(pend_prev || pend_cur);
      while (todo != 0ull) {  // one round per distinct slot that toggles in this step
        const int src = __ffsll(todo) - 1;
        const int k = __shfl(pend_prev ? prev : cur, src);
        const bool hit = (pend_prev && prev == k) || (pend_cur && cur == k);  // a lane toggles a slot at most once
        const unsigned long long hits = __ballot(hit);
        const int at = cursor[k];
        if (kWrite && hit) {
          const int64_t idx = (int64_t)offs[k] + at + __popcll(hits & ((1ull << lane) - 1ull));
          if (idx < (int64_t)offs[k + 1]) out[idx] = t;  // never outside the slot's range, whatever the table holds
        }
        __syncthreads();  // every lane has read the cursor
        if (lane == src) cursor[k] = at + __popcll(hits);
        __syncthreads();
        if (pend_prev && prev == k) pend_prev = false;
        if (pend_cur && cur == k) pend_cur = false;
        todo = __ballot(pend_prev || pend_cur);
      }
    }
  }
  if (!kWrite) {
    __syncthreads();
    for (int k = lane; k < N1; k += kWave) row[k] = cursor[k];
    if (lane == 0 && n_out) atomicAdd(out_of_range + b, n_out);
  }
}

// ---- order 1: one lane per column -----------------------------------------------------------------------------------
// Column x is group x; its closing position (x + 1) * H belongs to group x + 1, or to group W - 1 for the last column.
template <int DT, bool kWrite>
__global__ __launch_bounds__(kWave) void rle_cols_kernel(const void* __restrict__ map, int32_t* __restrict__ table,
                                                         int32_t* __restrict__ out_of_range,
                                                         const int32_t* __restrict__ offsets, int32_t* __restrict__ out,
                                                         int H, int W, int N) {
  using E = typename MapElem<DT>::type;
  const int x = blockIdx.x * kWave + threadIdx.x, b = blockIdx.y, N1 = N + 1;
  if (x >= W) return;
  const int HW = H * W;
  int32_t* row = table + ((int64_t)b * W + x) * N1;  // this lane's own
  const E* base = reinterpret_cast<const E*>(map) + (int64_t)b * HW;
  const int32_t* offs = kWrite ? offsets + (int64_t)b * N1 : nullptr;
  int n_out = 0;
  auto toggle = [&](int k, int t) {
    const int at = row[k];
    row[k] = at + 1;
    if (kWrite) {
      const int64_t idx = (int64_t)offs[k] + at;
      if (at >= 0 && idx < (int64_t)offs[k + 1]) out[idx] = t;
    }
  };
  int prev = x > 0 ? slot_of<DT>((uint32_t)base[(int64_t)(H - 1) * W + x - 1], N) : kRleNone;
  for (int y0 = 0; y0 < H; y0 += kRleUnroll) {
    uint32_t raw[kRleUnroll];
#pragma unroll
    for (int u = 0; u < kRleUnroll; ++u) raw[u] = y0 + u < H ? (uint32_t)base[(int64_t)(y0 + u) * W + x] : 0u;
#pragma unroll
    for (int u = 0; u < kRleUnroll; ++u) {
      if (y0 + u >= H) break;
      const int cur = slot_of<DT>(raw[u], N);
      n_out += cur == kRleOut;
      if (cur != prev) {
        const int t = x * H + y0 + u;
        if (prev >= 0) toggle(prev, t);
        if (cur >= 0) toggle(cur, t);
      }
      prev = cur;
    }
  }
  if (x == W - 1 && prev >= 0) toggle(prev, HW);
  if (!kWrite && n_out) atomicAdd(out_of_range + b, n_out);
}

// table (B, G, N + 1): every slot's counts along g -> exclusive prefixes; counts (B, N + 1) <- the totals
__global__ __launch_bounds__(kScanThreads) void rle_scan_kernel(int32_t* __restrict__ table, int32_t* __restrict__ counts,
                                                                int B, int G, int N1) {
  const int i = blockIdx.x * kScanThreads + threadIdx.x;
  if (i >= B * N1) return;
  const int b = i / N1, k = i - b * N1;
  int32_t* p = table + (int64_t)b * G * N1 + k;
  int run = 0;
  for (int g = 0; g < G; ++g) {
    const int c = p[(int64_t)g * N1];
    p[(int64_t)g * N1] = run;
    run += c;
  }
  counts[i] = run;
}

// ---- paint ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPaintThreads) void rle_check_kernel(const int32_t* __restrict__ runs, int R, int B, int HW,
                                                                  int32_t* __restrict__ status) {
  const int r = blockIdx.x * kPaintThreads + threadIdx.x;
  if (r >= R) return;
  const int b = runs[4 * r], s = runs[4 * r + 1], len = runs[4 * r + 2];
  if (b < 0 || b >= B || s < 0 || len < 0 || (int64_t)s + len > (int64_t)HW) atomicMin(status, r);
}

// one wave per run
__global__ __launch_bounds__(kPaintThreads) void rle_rank_kernel(const int32_t* __restrict__ runs, int R, int HW,
                                                                 const int32_t* __restrict__ status,
                                                                 int32_t* __restrict__ rank) {
  if (*status != INT32_MAX) return;  // refused: nothing is stored
  const int r = blockIdx.x * (kPaintThreads / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const int b = runs[4 * r], s = runs[4 * r + 1], len = runs[4 * r + 2];  // checked: 0 <= s, s + len <= HW
  int32_t* p = rank + (int64_t)b * HW + s;
  for (int i = lane; i < len; i += kWave) atomicMax(p + i, r + 1);
}

__global__ __launch_bounds__(kPaintThreads) void rle_resolve_kernel(const int32_t* __restrict__ runs, int R, int H, int W,
                                                                    int order, const int32_t* __restrict__ status,
                                                                    const int32_t* __restrict__ rank,
                                                                    int32_t* __restrict__ out) {
  if (*status != INT32_MAX) return;
  const int p = blockIdx.x * kPaintThreads + threadIdx.x, b = blockIdx.y;  // pixel y * W + x
  const int HW = H * W;
  if (p >= HW) return;
  int t = p;
  if (order == 1) {
    const int y = p / W, x = p - y * W;
    t = x * H + y;
  }
  const int r = rank[(int64_t)b * HW + t];
  if (r > 0 && r <= R) out[(int64_t)b * HW + p] = runs[4 * (r - 1) + 3];
}

int check_sizes(const char* who, int B, int H, int W, int N, int order) {
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N >= 0, "%s: bad size", who);
  WM2F_REQUIRE(order == 0 || order == 1, "%s: order must be 0 (row-major) or 1 (column-major), got %d", who, order);
  if (H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch || N > WM2F_RLE_MAX_IDS) {
    set_error("%s: sides <= %d, B <= %d, N <= %d (got %d x %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch, WM2F_RLE_MAX_IDS,
              H, W, B, N);
    return WM2F_EUNSUPPORTED;
  }
  return WM2F_OK;
}

template <bool kWrite>
void launch_walk(const void* map, int dtype, int32_t* table, int32_t* out_of_range, const int32_t* offsets, int32_t* out,
                 int B, int H, int W, int N, int order, hipStream_t s) {
  const size_t shm = (size_t)(N + 1) * sizeof(int32_t);
  for_map_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (order == 0)
      hipLaunchKernelGGL((rle_rows_kernel<DT, kWrite>), dim3(rle_groups(H, W, 0), B), dim3(kWave), shm, s, map, table,
                         out_of_range, offsets, out, H, W, N, rle_group_rows(H, W));
    else
      hipLaunchKernelGGL((rle_cols_kernel<DT, kWrite>), dim3(ceil_div(W, kWave), B), dim3(kWave), 0, s, map, table,
                         out_of_range, offsets, out, H, W, N);
  });
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_rle_workspace(int B, int H, int W, int N, int order) {
  if (B <= 0 || H <= 0 || W <= 0 || N < 0 || H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch ||
      N > WM2F_RLE_MAX_IDS || (order != 0 && order != 1))
    return -1;
  return (int64_t)B * rle_groups(H, W, order) * (N + 1) * (int64_t)sizeof(int32_t);
}

extern "C" int wm2f_labelmap_toggle_counts(const void* map, int dtype, int32_t* counts, int32_t* out_of_range,
                                           void* workspace, int B, int H, int W, int N, int order, void* stream) {
  const char* who = "wm2f_labelmap_toggle_counts";
  WM2F_REQUIRE(map && counts && out_of_range && workspace, "%s: null pointer", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  if (const int rc = check_sizes(who, B, H, W, N, order)) return rc;
  hipStream_t s = (hipStream_t)stream;
  int32_t* table = (int32_t*)workspace;
  WM2F_REQUIRE(hipMemsetAsync(out_of_range, 0, (size_t)B * sizeof(int32_t), s) == hipSuccess, "%s: clearing failed", who);
  if (order == 1)  // the column walk increments; the row walk stores every entry
    WM2F_REQUIRE(hipMemsetAsync(table, 0, (size_t)wm2f_rle_workspace(B, H, W, N, order), s) == hipSuccess,
                 "%s: clearing the table failed", who);
  launch_walk<false>(map, dtype, table, out_of_range, nullptr, nullptr, B, H, W, N, order, s);
  WM2F_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(rle_scan_kernel, dim3(ceil_div(B * (N + 1), kScanThreads)), dim3(kScanThreads), 0, s, table, counts,
                     B, rle_groups(H, W, order), N + 1);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_labelmap_toggles(const void* map, int dtype, const int32_t* offsets, int32_t* positions,
                                     void* workspace, int B, int H, int W, int N, int order, void* stream) {
  const char* who = "wm2f_labelmap_toggles";
  WM2F_REQUIRE(map && offsets && positions && workspace, "%s: null pointer", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  if (const int rc = check_sizes(who, B, H, W, N, order)) return rc;
  launch_walk<true>(map, dtype, (int32_t*)workspace, nullptr, offsets, positions, B, H, W, N, order, (hipStream_t)stream);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int64_t wm2f_rle_paint_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch) return -1;
  return (int64_t)B * H * W * (int64_t)sizeof(int32_t);
}

extern "C" int wm2f_rle_paint(int32_t* out, const int32_t* runs, int R, int32_t* status, void* workspace, int B, int H,
                              int W, int order, void* stream) {
  const char* who = "wm2f_rle_paint";
  WM2F_REQUIRE(out && status && workspace, "%s: null pointer", who);
  WM2F_REQUIRE(R >= 0 && (R == 0 || runs), "%s: bad run list", who);
  if (const int rc = check_sizes(who, B, H, W, 0, order)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W;
  const int32_t ok = INT32_MAX;  // "no bad run": the status word is the smallest bad index
  WM2F_REQUIRE(hipMemsetD32Async((hipDeviceptr_t)status, ok, 1, s) == hipSuccess, "%s: setting the status failed", who);
  if (R == 0) return WM2F_OK;
  int32_t* rank = (int32_t*)workspace;
  WM2F_REQUIRE(hipMemsetAsync(rank, 0, (size_t)wm2f_rle_paint_workspace(B, H, W), s) == hipSuccess,
               "%s: clearing the rank map failed", who);
  hipLaunchKernelGGL(rle_check_kernel, dim3(ceil_div(R, kPaintThreads)), dim3(kPaintThreads), 0, s, runs, R, B, HW,
                     status);
  WM2F_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(rle_rank_kernel, dim3(ceil_div(R, kPaintThreads / kWave)), dim3(kPaintThreads), 0, s, runs, R, HW,
                     (const int32_t*)status, rank);
  WM2F_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(rle_resolve_kernel, dim3(ceil_div(HW, kPaintThreads), B), dim3(kPaintThreads), 0, s, runs, R, H, W,
                     order, (const int32_t*)status, (const int32_t*)rank, out);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
