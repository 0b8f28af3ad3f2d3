// Crop rows of id maps on the device: the Hough accumulator of the voting pixels with its energies,
// and every instance's relation to a set of parallel lines.  The semantics are written out in include/wm2f.h;
// tests/rows_reference.py restates them with numpy, one angle and one pixel at a time.
//
//   wm2f_labelmap_row_votes (3 launches)
//     clear       : acc (B, T, R) <- 0.
//     row_votes   : a workgroup owns a 64 x 64 tile of pixels and walks a share of the angle bands (16 angles each; the
//                   host deals the bands out so that a small map still fills the chip).  It loads the tile once, four
//                   pixels a lane, and compacts the voting pixels into an LDS list of packed tile coordinates by ballot
//                   and prefix, one LDS atomic a wave for the slot; a tile without a voter returns there.  Per band a
//                   lane keeps the 16 angles' (c, s, origin) in registers, ROTATED by its lane number, so that the lanes
//                   of one instruction vote into 16 different histograms: neighbouring voters of one plant fall into the
//                   same bin of one angle, and without the rotation their LDS atomics would serialise on one address.
//                   The histogram is 16 angles x 128 bins (a 64 x 64 tile spans at most 91 one-pixel bins); its non-zero
//                   bins go to acc by integer atomicAdd, consecutive lanes on consecutive bins.
//     row_energy  : a workgroup per (image, angle) squares and sums the row of acc in 64 bits.
//   wm2f_labelmap_row_bands (2 launches)
//     clear       : counts (B, N, 3) <- 0.
//     row_bands   : a workgroup owns a strip of whole rows, a lane four consecutive pixels.  The image's row positions are
//                   staged in LDS and the nearest one is found by binary search; the zone byte is written for every
//                   pixel; a lane folds its pixels of one id before it adds.  Accumulators in LDS while
//                   N <= kRbLdsMaxIds (24 B each), flushed for the ids the strip saw by 64-bit integer atomics; above the
//                   cap the same code adds straight into the result.
// Everything is integer, atomics are integer adds: results are bit-identical from run to run.
#include "labelmap.h"

namespace wm2f {
namespace {

// ---- votes ---------------------------------------------------------------------------------------------------------------
constexpr int kRvThreads = 256;
constexpr int kRvTile = 64;                      // pixels a side
constexpr int kRvBand = 16;                      // angles per band
constexpr int kRvBins = 128;                     // histogram bins per angle: > 63 (|c| + s) / 2^14 + 2 = 91.1
constexpr int kRvMaxAngles = 1024;
constexpr int kRvMinShift = 14, kRvMaxShift = 20;
constexpr int kRvTargetGroups = 2048;            // workgroups the host aims at when it deals out the bands
constexpr int kRvPasses = kRvTile / (kRvThreads / (kRvTile / 4));  // 4: a pass is 16 rows of 16 quads

template <int DT, bool kVec>
__global__ __launch_bounds__(kRvThreads) void row_votes_kernel(const void* __restrict__ map,
                                                               const uint8_t* __restrict__ vote,
                                                               const int32_t* __restrict__ cs, int32_t* __restrict__ acc,
                                                               int H, int W, int N, int T, int R, int shift, int tiles_x) {
  using E = typename MapElem<DT>::type;
  __shared__ uint32_t hist[kRvBand * kRvBins];
  __shared__ uint16_t voters[kRvTile * kRvTile];
  __shared__ uint8_t svote[kMapMaxIds];
  __shared__ int sc[kRvBand], ss[kRvBand], sorg[kRvBand], sbase[kRvBand];
  __shared__ int count;
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = blockIdx.z;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kRvTile, y0 = ty * kRvTile;
  const E* base = reinterpret_cast<const E*>(map) + (int64_t)b * H * W;

  // the tile, four pixels a lane and four passes of 16 rows, all loads before the first use
  const int q = tid & 15, r = tid >> 4;
  uint32_t v[kRvPasses][4];
#pragma unroll
  for (int p = 0; p < kRvPasses; ++p) {
    const int y = y0 + p * 16 + r, x = x0 + q * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[p][j] = 0xffffffffu;  // no id in any dtype: -1, a NaN, and N <= 4096 for a uint8 map
    if (y < H) {
      const E* src = base + (int64_t)y * W + x;
      if (kVec) {
        if (x < W) load_map4<DT>(src, v[p]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x + j < W) v[p][j] = (uint32_t)src[j];
      }
    }
  }
  for (int j = tid; j < N; j += kRvThreads) svote[j] = vote[(int64_t)b * N + j];
  if (tid == 0) count = 0;
  __syncthreads();

  // compact the voters: ballot and prefix within a wave, one LDS atomic a wave for its slots
#pragma unroll
  for (int p = 0; p < kRvPasses; ++p) {
    const int y = y0 + p * 16 + r, x = x0 + q * 4;
    bool on[4];
    unsigned long long m[4];
    int total = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int id = map_id_below<DT>(v[p][j], N);
      on[j] = y < H && x + j < W && id >= 0 && svote[id] != 0;
      m[j] = __ballot(on[j]);
      total += __popcll(m[j]);
    }
    if (total == 0) continue;  // wave-uniform
    int slot = 0;
    if (lane == 0) slot = atomicAdd(&count, total);
    slot = __builtin_amdgcn_readfirstlane(slot);
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (on[j]) voters[slot + __popcll(m[j] & below)] = (uint16_t)((q * 4 + j) | ((p * 16 + r) << 6));
      slot += __popcll(m[j]);
    }
  }
  __syncthreads();
  const int n = count;
  if (n == 0) return;

  const int bands = ceil_div(T, kRvBand);
  int32_t* out = acc + (int64_t)b * T * R;
  const int rot = lane & (kRvBand - 1);
  for (int band = blockIdx.y; band < bands; band += gridDim.y) {  // workgroup-uniform
    const int t0 = band * kRvBand;
    const int na = T - t0 < kRvBand ? T - t0 : kRvBand;
    for (int j = tid; j < kRvBand * kRvBins; j += kRvThreads) hist[j] = 0u;
    if (tid < kRvBand) {
      int c = 0, s = 0, org = 0, bb = 0;
      if (tid < na) {
        c = cs[2 * (t0 + tid)];
        s = cs[2 * (t0 + tid) + 1];
        const int off = c < 0 ? -c * (W - 1) : 0;
        // the smallest value over the tile's 64 x 64 positions (whether they are pixels or not): its bin is the origin
        const int low = (c < 0 ? x0 + kRvTile - 1 : x0) * c + y0 * s + off;
        bb = low >> shift;
        org = x0 * c + y0 * s + off - bb * (1 << shift);
      }
      sc[tid] = c;
      ss[tid] = s;
      sorg[tid] = org;
      sbase[tid] = bb;
    }
    __syncthreads();
    int rc[kRvBand], rs[kRvBand], ro[kRvBand];
#pragma unroll
    for (int a = 0; a < kRvBand; ++a) {
      const int g = (a + rot) & (kRvBand - 1);
      rc[a] = sc[g];
      rs[a] = ss[g];
      ro[a] = sorg[g];
    }
    for (int i = tid; i < n; i += kRvThreads) {
      const int packed = voters[i];
      const int lx = packed & 63, ly = packed >> 6;
#pragma unroll
      for (int a = 0; a < kRvBand; ++a) {
        const int g = (a + rot) & (kRvBand - 1);
        const int bin = (lx * rc[a] + ly * rs[a] + ro[a]) >> shift;  // in [0, 91): the tile's span from its origin
        if (g < na) atomicAdd(&hist[g * kRvBins + (bin & (kRvBins - 1))], 1u);
      }
    }
    __syncthreads();
    for (int j = tid; j < kRvBand * kRvBins; j += kRvThreads) {
      const uint32_t cnt = hist[j];
      if (cnt == 0u) continue;
      const int a = j / kRvBins;
      const int bin = sbase[a] + (j - a * kRvBins);
      if (a < na && bin >= 0 && bin < R) atomicAdd(out + (int64_t)(t0 + a) * R + bin, (int)cnt);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kRvThreads) void row_energy_kernel(const int32_t* __restrict__ acc,
                                                                long long* __restrict__ energy, int R) {
  __shared__ unsigned long long part[kRvThreads];
  const int tid = threadIdx.x;
  const int32_t* row = acc + (int64_t)blockIdx.x * R;
  unsigned long long sum = 0ull;
  for (int j = tid; j < R; j += kRvThreads) {
    const unsigned long long a = (unsigned long long)(uint32_t)row[j];
    sum += a * a;
  }
  part[tid] = sum;
  __syncthreads();
  for (int d = kRvThreads / 2; d > 0; d >>= 1) {
    if (tid < d) part[tid] += part[tid + d];
    __syncthreads();
  }
  if (tid == 0) energy[blockIdx.x] = (long long)part[0];
}

// ---- bands ---------------------------------------------------------------------------------------------------------------
constexpr int kRbThreads = 256;
constexpr int kRbLdsMaxIds = 1024;  // 24 B + 4 B of id list each, and 4 KiB of row positions: 32 KiB
constexpr int kRbMaxRows = 1024;    // row positions per image
constexpr int kRbCols = 3;
constexpr int kRbTargetGroups = 2048;

template <int DT>
__device__ __forceinline__ int rb_row_of(uint32_t raw, const int32_t* ids, int n, int N) {
  int v;
  if (!map_int<DT>(raw, v)) return -1;
  if (ids == nullptr) return (v >= 0 && v < N) ? v : -1;
  return list_row(v, ids, n);
}

template <int DT, bool kVec, bool kLds>
__global__ __launch_bounds__(kRbThreads) void row_bands_kernel(const void* __restrict__ map,
                                                               const int32_t* __restrict__ ids,
                                                               const int32_t* __restrict__ n_ids,
                                                               const int32_t* __restrict__ line,
                                                               const int32_t* __restrict__ rho,
                                                               long long* __restrict__ counts,
                                                               uint8_t* __restrict__ zone, int H, int W, int N, int Kmax,
                                                               int band, int strip_rows) {
  using E = typename MapElem<DT>::type;
  extern __shared__ __align__(8) unsigned char shmem[];
  unsigned long long* lacc = reinterpret_cast<unsigned long long*>(shmem);
  int32_t* srho = reinterpret_cast<int32_t*>(shmem + (kLds ? (size_t)N * kRbCols * sizeof(unsigned long long) : 0));
  int32_t* sids = srho + Kmax;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int y0 = blockIdx.x * strip_rows;
  const int y1 = y0 + strip_rows < H ? y0 + strip_rows : H;
  const int c = line[b * 4], s = line[b * 4 + 1], off = line[b * 4 + 2];
  int K = line[b * 4 + 3];
  K = K < 0 ? 0 : (K > Kmax ? Kmax : K);
  int n = 0;
  if (ids != nullptr) {
    n = n_ids[b];
    n = n < 0 ? 0 : (n > N ? N : n);
    for (int j = tid; j < n; j += kRbThreads) sids[j] = ids[(int64_t)b * N + j];
  }
  for (int j = tid; j < K; j += kRbThreads) srho[j] = rho[(int64_t)b * Kmax + j];
  if (kLds)
    for (int j = tid; j < N * kRbCols; j += kRbThreads) lacc[j] = 0ull;
  __syncthreads();
  const int32_t* idl = ids != nullptr ? sids : nullptr;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts) + (int64_t)b * N * kRbCols;
  const E* base = reinterpret_cast<const E*>(map) + (int64_t)b * H * W;
  uint8_t* zbase = zone != nullptr ? zone + (int64_t)b * H * W : nullptr;
  const int quads = (W + 3) >> 2;
  const int items = (y1 - y0) * quads;
  for (int i = tid; i < items; i += kRbThreads) {
    const int ry = i / quads;
    const int y = y0 + ry, x = (i - ry * quads) * 4;
    const int nv = W - x < 4 ? W - x : 4;
    const E* src = base + (int64_t)y * W + x;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (kVec) {
      load_map4<DT>(src, v);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nv) v[j] = (uint32_t)src[j];
    }
    // the pixel's position along the normal, wrapped like the host's int32; the differences are taken in 64 bits
    const int p0 = (int)((uint32_t)x * (uint32_t)c + (uint32_t)y * (uint32_t)s + (uint32_t)off);
    uint32_t zbits = 0u;
    int cur = -1;
    unsigned long long n_all = 0ull, n_in = 0ull;
    long long sum = 0;
    const auto flush = [&]() {
      if (cur < 0) return;
      unsigned long long* a = kLds ? lacc + cur * kRbCols : out + (int64_t)cur * kRbCols;
      atomicAdd(a, n_all);
      if (n_in) atomicAdd(a + 1, n_in);
      atomicAdd(a + 2, (unsigned long long)sum);
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= nv) break;
      const int p = (int)((uint32_t)p0 + (uint32_t)j * (uint32_t)c);
      bool in = false;
      if (K > 0) {
        const int lo = list_lower_bound(p, srho, K);  // the first row not below p
        long long d = lo < K ? (long long)srho[lo] - p : (long long)1 << 40;
        if (lo > 0) {
          const long long d2 = (long long)p - srho[lo - 1];
          d = d2 < d ? d2 : d;
        }
        in = d <= (long long)band;
      }
      zbits |= (in ? 1u : 0u) << (8 * j);
      const int row = rb_row_of<DT>(v[j], idl, n, N);
      if (row != cur) {
        flush();
        cur = row;
        n_all = 0ull;
        n_in = 0ull;
        sum = 0;
      }
      n_all += 1ull;
      n_in += in ? 1ull : 0ull;
      sum += p;
    }
    flush();
    if (zbase != nullptr) {
      uint8_t* z = zbase + (int64_t)y * W + x;
      if (kVec) {
        *reinterpret_cast<uint32_t*>(z) = zbits;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < nv) z[j] = (uint8_t)((zbits >> (8 * j)) & 1u);
      }
    }
  }
  if (kLds) {
    __syncthreads();
    for (int j = tid; j < N; j += kRbThreads) {
      if (lacc[j * kRbCols] == 0ull) continue;  // flush only what this strip saw
#pragma unroll
      for (int k = 0; k < kRbCols; ++k) atomicAdd(out + (int64_t)j * kRbCols + k, lacc[j * kRbCols + k]);
    }
  }
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_labelmap_row_votes(const void* map, int dtype, const uint8_t* vote, const int32_t* cs, int32_t* acc,
                                       int64_t* energy, int B, int H, int W, int N, int T, int shift, void* stream) {
  const char* who = "wm2f_labelmap_row_votes";
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N > 0 && T > 0, "%s: bad size", who);
  WM2F_REQUIRE(shift >= kRvMinShift && shift <= kRvMaxShift, "%s: shift must be in [%d, %d], got %d", who, kRvMinShift,
               kRvMaxShift, shift);
  if (H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch || N > kMapMaxIds || T > kRvMaxAngles) {
    set_error("%s: sides <= %d, B <= %d, N <= %d, T <= %d (got %d x %d, %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch,
              kMapMaxIds, kRvMaxAngles, H, W, B, N, T);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(map && vote && cs && acc && energy, "%s: null pointer", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  hipStream_t s = (hipStream_t)stream;
  const int R = (int)((((int64_t)(W + H - 2)) << 14) >> shift) + 1;
  if (hipMemsetAsync(acc, 0, (size_t)B * T * R * sizeof(int32_t), s) != hipSuccess) {
    set_error("%s: clearing the accumulator failed", who);
    return WM2F_ELAUNCH;
  }
  const int tiles_x = ceil_div(W, kRvTile), tiles_y = ceil_div(H, kRvTile);
  const int tiles = tiles_x * tiles_y;  // <= 2^16
  const int bands = ceil_div(T, kRvBand);
  int groups = ceil_div(kRvTargetGroups, tiles * B);
  groups = groups < 1 ? 1 : (groups > bands ? bands : groups);
  const dim3 grid(tiles, groups, B);
  const bool vec = map_vec4_ok(map, dtype, W);
  for_map_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (vec) hipLaunchKernelGGL((row_votes_kernel<DT, true>), grid, dim3(kRvThreads), 0, s, map, vote, cs, acc, H, W, N, T, R, shift, tiles_x);
    else hipLaunchKernelGGL((row_votes_kernel<DT, false>), grid, dim3(kRvThreads), 0, s, map, vote, cs, acc, H, W, N, T, R, shift, tiles_x);
  });
  hipLaunchKernelGGL(row_energy_kernel, dim3(B * T), dim3(kRvThreads), 0, s, acc, reinterpret_cast<long long*>(energy), R);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_labelmap_row_bands(const void* map, int dtype, const int32_t* ids, const int32_t* n_ids,
                                       const int32_t* line, const int32_t* rho, int64_t* counts, uint8_t* zone, int B, int H,
                                       int W, int N, int Kmax, int band, void* stream) {
  const char* who = "wm2f_labelmap_row_bands";
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N > 0 && Kmax >= 0 && band >= 0, "%s: bad size", who);
  if (H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch || N > kMapMaxIds || Kmax > kRbMaxRows) {
    set_error("%s: sides <= %d, B <= %d, N <= %d, Kmax <= %d (got %d x %d, %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch,
              kMapMaxIds, kRbMaxRows, H, W, B, N, Kmax);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(map && line && counts && (rho || Kmax == 0), "%s: null pointer", who);
  WM2F_REQUIRE((ids == nullptr) == (n_ids == nullptr), "%s: ids and n_ids go together", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  hipStream_t s = (hipStream_t)stream;
  long long* out = reinterpret_cast<long long*>(counts);
  if (hipMemsetAsync(out, 0, (size_t)B * N * kRbCols * sizeof(long long), s) != hipSuccess) {
    set_error("%s: clearing the result failed", who);
    return WM2F_ELAUNCH;
  }
  // a strip of whole rows per workgroup: about kRbTargetGroups of them, at least 4096 pixels each
  int rows = ceil_div(H, ceil_div(kRbTargetGroups, B));
  const int min_rows = ceil_div(4096, W);
  rows = rows < min_rows ? min_rows : rows;
  rows = rows > H ? H : rows;
  const dim3 grid(ceil_div(H, rows), B);
  const bool lds = N <= kRbLdsMaxIds;
  const bool vec = map_vec4_ok(map, dtype, W) && (zone == nullptr || reinterpret_cast<uintptr_t>(zone) % 4 == 0);
  const size_t shm = (lds ? (size_t)N * kRbCols * sizeof(unsigned long long) : 0) + (size_t)Kmax * sizeof(int32_t) +
                     (ids ? (size_t)N * sizeof(int32_t) : 0);
  for_map_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kRbThreads), shm, s, map, ids, n_ids, line, rho, out, zone, H, W, N, Kmax, band, rows);
    };
    if (vec && lds) launch(row_bands_kernel<DT, true, true>);
    else if (vec) launch(row_bands_kernel<DT, true, false>);
    else if (lds) launch(row_bands_kernel<DT, false, true>);
    else launch(row_bands_kernel<DT, false, false>);
  });
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
