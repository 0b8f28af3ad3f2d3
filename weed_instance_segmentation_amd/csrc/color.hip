// Per-instance colour sums of id maps and vegetation-index histograms and masks of pictures on the device (DESIGN
// section 47).  The semantics are written out in include/wm2f.h; tests/color_reference.py restates them in numpy, one id
// at a time.  Pictures are (B, H, W, 3) uint8, packed; everything is integer and there is no division instruction: the
// two floor divisions (the Q12 normalised index by R + G + B <= 765, the hue by the chroma <= 255) multiply by
// ceil(2^37 / d) from a 766-entry table (exact for numerators below 2^27: d (ceil(2^37 / d)) - 2^37 < d <= 2^10).
//
//   wm2f_labelmap_color_stats (a memset and 1 launch)
//     color_stats  : instance_stats.hip's walk -- grid (strips, B), 256 threads, a workgroup owns a strip of whole rows, a
//                    wave takes 256 consecutive pixels of one row per load, four pixels per lane.  A batch of kCoUnroll
//                    items first loads the map, then turns values into result rows, then loads 12 picture bytes per lane
//                    for the lanes that hold a listed id -- a wave without one neither loads nor decodes the picture --
//                    and only then does the arithmetic.
//                    - A wave whose pixels all carry one listed id adds its pixels into 14 per-lane 32-bit partial sums
//                      (and the hue bins, counted per wave by ballots, into lane k's counter for bin k).  The partials
//                      stay in registers while the wave's following items carry the same id, at most kCoFlushItems of
//                      them (16 x 256 x 65025 < 2^32); then one butterfly reduction per column, and lane c adds column
//                      c, lane k bin k: two atomic instructions per flush.
//                    - In a mixed wave a lane folds its own runs and adds once per run and column.
//                    Accumulators live in LDS while N <= kCoLdsMaxIds = 240: 88 B per id (seven 64-bit sums -- the six
//                    products and the signed sum of q -- and seven 32-bit ones, which a strip of at most 2^22 pixels
//                    cannot overflow), 4 K B of hue bins, 4 B of id list, next to the 6128 B of the reciprocal table:
//                    at most 240 x (88 + 144 + 4) + 6128 = 62768 B, inside the 64 KiB a launch gets without asking.  A
//                    workgroup flushes the non-zero sums with 64-bit integer atomics.  Above the cap the same code adds
//                    into the result.
//   wm2f_image_index_hist (a memset and 1 launch): a picture is a flat run of H W pixels; a workgroup takes a chunk of
//                    them, four per lane and load, into an LDS histogram of bins 32-bit counters (at most 8161: 32 KiB),
//                    a lane's equal neighbours folded into one add, and flushes the non-zero bins.
//   wm2f_image_index_mask (a memset of 8 B bytes and 1 launch): the same walk; a lane writes its four mask bytes as one
//                    dword and counts; one 64-bit atomic per workgroup.
// Vector paths (dword loads and stores) where the bases and the row or picture lengths are multiples of 4, byte paths
// elsewhere.  Integer atomics only: results are bit-identical from run to run.
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kCoThreads = 256;
constexpr int kCoWaves = kCoThreads / 64;
constexpr int kCoPix = 4;
constexpr int kCoSeg = 64 * kCoPix;
constexpr int kCoUnroll = 4;
constexpr int kCoLdsMaxIds = 240;
constexpr int kCoMaxStripRows = 256;  // a strip has at most 2^22 pixels: its 32-bit sums stay below 2^30
constexpr int kCoCols = 14;
constexpr int kCoFlushItems = 16;
constexpr int kCoAccBytes = 88;
constexpr int kCoMaxWeight = 32;
constexpr int kCoRecN = 766;
constexpr int kCoRecShift = 37;
constexpr int kCoHueShift = 18;  // h < 360, bin width <= 360: h ceil(2^18 / w) >> 18 is h / w (359 x 359 < 2^18)

struct RecipTable {
  unsigned long long m[kCoRecN];
};
constexpr RecipTable make_recip() {
  RecipTable t{};
  for (int d = 1; d < kCoRecN; ++d) t.m[d] = ((1ull << kCoRecShift) + (unsigned)d - 1ull) / (unsigned)d;
  return t;
}
__device__ const RecipTable kCoRecip = make_recip();

struct CoParams {
  int a, b, c;
  int dark, bright;
  int K, min_chroma, hue_mul;
};

// floor(n / d) for |n| + d < 2^27 and m = ceil(2^37 / d); d = 0 (m = 0) gives 0
__device__ __forceinline__ int floor_div(int n, int d, unsigned long long m) {
  const uint32_t u = n >= 0 ? (uint32_t)n : (uint32_t)(-n + d - 1);
  const int q = (int)(((unsigned long long)u * m) >> kCoRecShift);
  return n >= 0 ? q : -q;
}

// byte i of the 12 a lane holds in three dwords
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[3], int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

__device__ __forceinline__ int index_of(const CoParams& prm, uint32_t R, uint32_t G, uint32_t B) {
  return prm.a * (int)R + prm.b * (int)G + prm.c * (int)B;
}

// one pixel into the 14 columns of include/wm2f.h; p[11] is a two's-complement sum
__device__ __forceinline__ void add_pixel(uint32_t (&p)[kCoCols], uint32_t R, uint32_t G, uint32_t B, int thr,
                                          const CoParams& prm, const unsigned long long* rec) {
  p[0] += 1u;
  p[1] += R;
  p[2] += G;
  p[3] += B;
  p[4] += R * R;
  p[5] += G * G;
  p[6] += B * B;
  p[7] += R * G;
  p[8] += R * B;
  p[9] += G * B;
  const int I = index_of(prm, R, G, B);
  p[10] += I > thr ? 1u : 0u;
  const int s = (int)(R + G + B);
  p[11] += (uint32_t)floor_div(I * 4096, s, rec[s]);
  const uint32_t mx = max(R, max(G, B));
  p[12] += (int)mx < prm.dark ? 1u : 0u;
  p[13] += (int)mx >= prm.bright ? 1u : 0u;
}

// the pixel's hue bin, -1 below the chroma threshold
__device__ __forceinline__ int hue_bin(uint32_t R, uint32_t G, uint32_t B, const CoParams& prm,
                                       const unsigned long long* rec) {
  const int r = (int)R, g = (int)G, b = (int)B;
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b)), cr = mx - mn;
  if (cr < prm.min_chroma) return -1;  // min_chroma >= 1: cr > 0 below
  int num, base;
  if (mx == r) {
    num = g - b;
    base = 0;
  } else if (mx == g) {
    num = b - r;
    base = 120;
  } else {
    num = r - g;
    base = 240;
  }
  int h = base + floor_div(60 * num, cr, rec[cr]);
  if (h < 0) h += 360;
  return (int)(((uint32_t)h * (uint32_t)prm.hue_mul) >> kCoHueShift);
}

template <int DT>
__device__ __forceinline__ int co_row_of(uint32_t raw, const int32_t* ids, int n, int N) {
  int v;
  if (!map_int<DT>(raw, v)) return -1;
  if (ids == nullptr) return (v >= 0 && v < N) ? v : -1;
  return list_row(v, ids, n);
}

// v, the 32-bit partial of column col (col 11 signed), into result row r: the LDS record or the result
template <bool kLds>
__device__ __forceinline__ void add_col(unsigned char* acc, long long* st, int r, int col, uint32_t v) {
  const long long sv = col == 11 ? (long long)(int32_t)v : (long long)v;
  if (kLds) {
    unsigned char* rcd = acc + (size_t)r * kCoAccBytes;
    if ((col >= 4 && col <= 9) || col == 11) {
      atomicAdd(reinterpret_cast<unsigned long long*>(rcd) + (col == 11 ? 6 : col - 4), (unsigned long long)sv);
    } else {
      const int slot = col < 4 ? col : (col == 10 ? 4 : (col == 12 ? 5 : 6));
      atomicAdd(reinterpret_cast<uint32_t*>(rcd + 56) + slot, v);
    }
  } else {
    atomicAdd(reinterpret_cast<unsigned long long*>(st + (int64_t)r * kCoCols + col), (unsigned long long)sv);
  }
}

template <bool kLds>
__device__ __forceinline__ void add_hue(uint32_t* hacc, long long* hue, int r, int K, int bin, uint32_t v) {
  if (kLds) atomicAdd(hacc + r * K + bin, v);
  else atomicAdd(reinterpret_cast<unsigned long long*>(hue + ((int64_t)r * K + bin)), (unsigned long long)v);
}

// kVec: W % 4 == 0 and map and picture aligned, so a lane's four pixels are one map load and three picture dwords
template <int DT, bool kVec, bool kLds>
__global__ __launch_bounds__(kCoThreads) void color_stats_kernel(
    const uint8_t* __restrict__ img, const void* __restrict__ map, const int32_t* __restrict__ ids,
    const int32_t* __restrict__ n_ids, const int32_t* __restrict__ thresholds, long long* __restrict__ sums,
    long long* __restrict__ hue, int H, int W, int N, int strip_rows, CoParams prm) {
  using E = typename MapElem<DT>::type;
  extern __shared__ __align__(8) unsigned char comem[];
  const int Kh = hue != nullptr ? prm.K : 0;
  unsigned long long* rec = reinterpret_cast<unsigned long long*>(comem);
  unsigned char* acc = comem + kCoRecN * 8;
  uint32_t* hacc = reinterpret_cast<uint32_t*>(acc + (kLds ? (size_t)N * kCoAccBytes : 0));
  int32_t* sids = reinterpret_cast<int32_t*>(hacc + (kLds ? N * Kh : 0));
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int y0 = blockIdx.x * strip_rows;
  const int y1 = y0 + strip_rows < H ? y0 + strip_rows : H;
  int n = 0;
  if (ids != nullptr) {
    n = n_ids[b];
    n = n < 0 ? 0 : (n > N ? N : n);
    for (int j = tid; j < n; j += kCoThreads) sids[j] = ids[(int64_t)b * N + j];
  }
  for (int j = tid; j < kCoRecN; j += kCoThreads) rec[j] = kCoRecip.m[j];
  if (kLds) {
    uint32_t* z = reinterpret_cast<uint32_t*>(acc);
    const int words = N * (kCoAccBytes / 4 + Kh);  // the records and the hue bins behind them
    for (int j = tid; j < words; j += kCoThreads) z[j] = 0u;
  }
  __syncthreads();
  const int32_t* idl = ids != nullptr ? sids : nullptr;
  const int thr = thresholds[b];
  long long* st = sums + (int64_t)b * N * kCoCols;
  long long* hu = hue != nullptr ? hue + (int64_t)b * N * Kh : nullptr;
  const E* base = reinterpret_cast<const E*>(map) + (int64_t)b * H * W;
  const uint8_t* ibase = img + (int64_t)b * H * W * 3;
  const int segs = (W + kCoSeg - 1) / kCoSeg;

  // the wave's pending partials: result row cur, pend items in them; hl is lane k's count of hue bin k
  int cur = -1, pend = 0;
  uint32_t p[kCoCols];
  uint32_t hl = 0u;
#pragma unroll
  for (int c = 0; c < kCoCols; ++c) p[c] = 0u;
  const auto flush = [&]() {  // wave-uniform
    if (cur >= 0 && pend > 0) {
#pragma unroll
      for (int c = 0; c < kCoCols; ++c)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) p[c] += (uint32_t)__shfl_xor((int)p[c], off);
      // every lane holds the totals now: through scalar registers, so that "lane c takes column c" stays a chain of
      // selects and p[] stays in registers
      uint32_t mine = 0u;
#pragma unroll
      for (int c = 0; c < kCoCols; ++c) {
        const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)p[c]);
        mine = lane == c ? total : mine;
      }
      if (lane < kCoCols && mine != 0u) add_col<kLds>(acc, st, cur, lane, mine);
      if (lane < Kh && hl != 0u) add_hue<kLds>(hacc, hu, cur, Kh, lane, hl);
    }
#pragma unroll
    for (int c = 0; c < kCoCols; ++c) p[c] = 0u;
    hl = 0u;
    pend = 0;
  };

  int y = y0, seg = wave;
  while (seg >= segs) {
    seg -= segs;
    ++y;
  }
  while (y < y1) {  // wave-uniform
    int iy[kCoUnroll], ix[kCoUnroll];
    uint32_t v[kCoUnroll][kCoPix];  // raw map values, then result rows
    uint32_t w[kCoUnroll][3];       // a lane's 12 picture bytes
    bool uni[kCoUnroll], need[kCoUnroll];
#pragma unroll
    for (int u = 0; u < kCoUnroll; ++u) {
      iy[u] = y;
      ix[u] = seg * kCoSeg;
      seg += kCoWaves;
      while (seg >= segs) {
        seg -= segs;
        ++y;
      }
    }
#pragma unroll
    for (int u = 0; u < kCoUnroll; ++u) {
      const int x = ix[u] + lane * kCoPix;
#pragma unroll
      for (int j = 0; j < kCoPix; ++j) v[u][j] = 0u;
      if (iy[u] < y1) {
        const E* q = base + (int64_t)iy[u] * W + x;
        if (kVec) {
          if (x < W) load_map4<DT>(q, v[u]);
        } else {
#pragma unroll
          for (int j = 0; j < kCoPix; ++j)
            if (x + j < W) v[u][j] = (uint32_t)q[j];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kCoUnroll; ++u) {
      uni[u] = false;
      need[u] = false;
      w[u][0] = w[u][1] = w[u][2] = 0u;
      if (iy[u] >= y1) continue;  // wave-uniform
      const int x = ix[u] + lane * kCoPix;
      const int nv = W - x < 0 ? 0 : (W - x < kCoPix ? W - x : kCoPix);
      const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)v[u][0]);  // lane 0's first pixel is inside
      bool same = true;
#pragma unroll
      for (int j = 0; j < kCoPix; ++j) same = same && (j >= nv || v[u][j] == first);
      uni[u] = __ballot(same) == ~0ull;
      bool any = false;
      if (uni[u]) {
        const int r = co_row_of<DT>(first, idl, n, N);
#pragma unroll
        for (int j = 0; j < kCoPix; ++j) v[u][j] = (uint32_t)(j < nv ? r : -1);
        any = r >= 0 && nv > 0;
      } else {
#pragma unroll
        for (int j = 0; j < kCoPix; ++j) {
          const int r = j < nv ? co_row_of<DT>(v[u][j], idl, n, N) : -1;
          v[u][j] = (uint32_t)r;
          any = any || r >= 0;
        }
      }
      need[u] = __ballot(any) != 0ull;
      if (any) {  // then x < W
        const uint8_t* q = ibase + ((int64_t)iy[u] * W + x) * 3;
        if (kVec) {
          const uint32_t* q4 = reinterpret_cast<const uint32_t*>(q);
          w[u][0] = q4[0];
          w[u][1] = q4[1];
          w[u][2] = q4[2];
        } else {
#pragma unroll
          for (int i = 0; i < 3 * kCoPix; ++i)
            if (i / 3 < nv) w[u][i >> 2] |= (uint32_t)q[i] << (8 * (i & 3));
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kCoUnroll; ++u) {
      if (iy[u] >= y1) break;   // wave-uniform; later items of the batch are past the strip too
      if (!need[u]) continue;   // no listed id in the wave: nothing to decode
      if (uni[u]) {
        const int r = __builtin_amdgcn_readfirstlane((int)v[u][0]);
        if (r != cur || pend == kCoFlushItems) {
          flush();
          cur = r;
        }
        ++pend;
#pragma unroll
        for (int j = 0; j < kCoPix; ++j) {
          const bool in = (int)v[u][j] >= 0;
          const uint32_t R = byte_of(w[u], 3 * j), G = byte_of(w[u], 3 * j + 1), B = byte_of(w[u], 3 * j + 2);
          if (in) add_pixel(p, R, G, B, thr, prm, rec);
          if (Kh > 0) {  // wave-uniform
            const int bin = in ? hue_bin(R, G, B, prm, rec) : -1;
            unsigned long long m = __ballot(bin >= 0);
            while (m != 0ull) {
              const int k = __builtin_amdgcn_readlane(bin, __ffsll((long long)m) - 1);
              const unsigned long long e = __ballot(bin == k);
              if (lane == k) hl += (uint32_t)__popcll(e);
              m &= ~e;
            }
          }
        }
        continue;
      }
      uint32_t t[kCoCols];
#pragma unroll
      for (int c = 0; c < kCoCols; ++c) t[c] = 0u;
#pragma unroll
      for (int j = 0; j < kCoPix; ++j) {
        const int r = (int)v[u][j];
        if (r < 0) continue;
        const uint32_t R = byte_of(w[u], 3 * j), G = byte_of(w[u], 3 * j + 1), B = byte_of(w[u], 3 * j + 2);
        add_pixel(t, R, G, B, thr, prm, rec);
        if (Kh > 0) {
          const int bin = hue_bin(R, G, B, prm, rec);
          if (bin >= 0) add_hue<kLds>(hacc, hu, r, Kh, bin, 1u);
        }
        const bool last = j == kCoPix - 1 || (int)v[u][j + 1 < kCoPix ? j + 1 : j] != r;
        if (last) {  // the lane's run of r ends here
#pragma unroll
          for (int c = 0; c < kCoCols; ++c) {
            if (t[c] != 0u) add_col<kLds>(acc, st, r, c, t[c]);
            t[c] = 0u;
          }
        }
      }
    }
  }
  flush();
  if (kLds) {
    __syncthreads();
    for (int e = tid; e < N * kCoCols; e += kCoThreads) {
      const int j = e / kCoCols, col = e - j * kCoCols;
      const unsigned char* rcd = acc + (size_t)j * kCoAccBytes;
      unsigned long long val;
      if ((col >= 4 && col <= 9) || col == 11) {
        val = reinterpret_cast<const unsigned long long*>(rcd)[col == 11 ? 6 : col - 4];
      } else {
        const int slot = col < 4 ? col : (col == 10 ? 4 : (col == 12 ? 5 : 6));
        val = reinterpret_cast<const uint32_t*>(rcd + 56)[slot];
      }
      if (val != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(st + e), val);  // only what this strip saw
    }
    for (int e = tid; e < N * Kh; e += kCoThreads) {
      const uint32_t val = hacc[e];
      if (val != 0u) atomicAdd(reinterpret_cast<unsigned long long*>(hu + e), (unsigned long long)val);
    }
  }
}

// ---- whole-picture index: histogram and mask ------------------------------------------------------------------------------
// the 12 bytes of pixels [p, p + 4) of a flat picture into three dwords; bytes of pixels at and past p1 stay 0
template <bool kVec>
__device__ __forceinline__ void load_pixels4(const uint8_t* base, int64_t p, int64_t p1, uint32_t (&w)[3]) {
  const uint8_t* q = base + p * 3;
  if (kVec) {  // whole quads only
    const uint32_t* q4 = reinterpret_cast<const uint32_t*>(q);
    w[0] = q4[0];
    w[1] = q4[1];
    w[2] = q4[2];
  } else {
    w[0] = w[1] = w[2] = 0u;
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (p + i / 3 < p1) w[i >> 2] |= (uint32_t)q[i] << (8 * (i & 3));
  }
}

template <bool kVec>
__global__ __launch_bounds__(kCoThreads) void index_hist_kernel(const uint8_t* __restrict__ img,
                                                                long long* __restrict__ hist, int64_t npix,
                                                                int64_t chunk, int bins, int imin, CoParams prm) {
  extern __shared__ __align__(8) unsigned char comem[];
  uint32_t* hh = reinterpret_cast<uint32_t*>(comem);
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int j = tid; j < bins; j += kCoThreads) hh[j] = 0u;
  __syncthreads();
  const uint8_t* base = img + (int64_t)b * npix * 3;
  const int64_t p0 = (int64_t)blockIdx.x * chunk;
  const int64_t p1 = p0 + chunk < npix ? p0 + chunk : npix;
  for (int64_t p = p0 + tid * 4; p < p1; p += kCoThreads * 4) {
    uint32_t w[3];
    load_pixels4<kVec>(base, p, p1, w);
    const int nv = p1 - p < 4 ? (int)(p1 - p) : 4;
    int run = -1, len = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= nv) break;
      const int bin = index_of(prm, byte_of(w, 3 * j), byte_of(w, 3 * j + 1), byte_of(w, 3 * j + 2)) - imin;
      if (bin != run) {
        if (len > 0) atomicAdd(hh + run, (uint32_t)len);
        run = bin;
        len = 0;
      }
      ++len;
    }
    if (len > 0) atomicAdd(hh + run, (uint32_t)len);
  }
  __syncthreads();
  long long* out = hist + (int64_t)b * bins;
  for (int j = tid; j < bins; j += kCoThreads)
    if (hh[j] != 0u) atomicAdd(reinterpret_cast<unsigned long long*>(out + j), (unsigned long long)hh[j]);
}

template <bool kVec>
__global__ __launch_bounds__(kCoThreads) void index_mask_kernel(const uint8_t* __restrict__ img,
                                                                const int32_t* __restrict__ thresholds,
                                                                uint8_t* __restrict__ mask, long long* __restrict__ counts,
                                                                int64_t npix, int64_t chunk, CoParams prm) {
  __shared__ uint32_t part[kCoWaves];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int thr = thresholds[b];
  const uint8_t* base = img + (int64_t)b * npix * 3;
  uint8_t* mb = mask + (int64_t)b * npix;
  const int64_t p0 = (int64_t)blockIdx.x * chunk;
  const int64_t p1 = p0 + chunk < npix ? p0 + chunk : npix;
  uint32_t on = 0u;
#pragma unroll 2  // unbounded, the compiler unrolls the vector path eightfold: 137 VGPRs and three waves per SIMD
  for (int64_t p = p0 + tid * 4; p < p1; p += kCoThreads * 4) {
    uint32_t w[3];
    load_pixels4<kVec>(base, p, p1, w);
    const int nv = p1 - p < 4 ? (int)(p1 - p) : 4;
    uint32_t m4 = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int I = index_of(prm, byte_of(w, 3 * j), byte_of(w, 3 * j + 1), byte_of(w, 3 * j + 2));
      const uint32_t m = (j < nv && I > thr) ? 1u : 0u;
      m4 |= m << (8 * j);
      on += m;
    }
    if (kVec) {
      *reinterpret_cast<uint32_t*>(mb + p) = m4;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nv) mb[p + j] = (uint8_t)((m4 >> (8 * j)) & 0xffu);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) on += (uint32_t)__shfl_xor((int)on, off);
  if (lane == 0) part[wave] = on;
  __syncthreads();
  if (tid == 0) {
    uint32_t s = 0u;
    for (int i = 0; i < kCoWaves; ++i) s += part[i];  // a chunk has fewer than 2^32 pixels
    if (s != 0u) atomicAdd(reinterpret_cast<unsigned long long*>(counts + b), (unsigned long long)s);
  }
}

// the checks the three entry points share; 0 or the code to return
int check_picture(const char* who, int ca, int cb, int cc, int B, int H, int W) {
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad size", who);
  const int weight = abs(ca) + abs(cb) + abs(cc);
  WM2F_REQUIRE(ca >= -kCoMaxWeight && ca <= kCoMaxWeight && cb >= -kCoMaxWeight && cb <= kCoMaxWeight &&
                   cc >= -kCoMaxWeight && cc <= kCoMaxWeight && weight >= 1 && weight <= kCoMaxWeight,
               "%s: the coefficients must not all be zero and |a| + |b| + |c| <= %d, got (%d, %d, %d)", who, kCoMaxWeight,
               ca, cb, cc);
  if (H > kMapMaxSide || W > kMapMaxSide || B > kMapMaxBatch) {
    set_error("%s: sides <= %d, B <= %d (got %d x %d, %d)", who, kMapMaxSide, kMapMaxBatch, H, W, B);
    return WM2F_EUNSUPPORTED;
  }
  return WM2F_OK;
}

// pixels of a workgroup of the flat walks: about 1024 workgroups in all, at least 4096 pixels, whole 1024-pixel turns
int64_t flat_chunk(int B, int64_t npix) {
  int64_t chunk = ceil_div64(npix, ceil_div(1024, B));
  chunk = chunk < 4096 ? 4096 : chunk;
  return ceil_div64(chunk, kCoThreads * 4) * (kCoThreads * 4);
}

bool aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_labelmap_color_stats(const uint8_t* image, const void* map, int dtype, const int32_t* ids,
                                         const int32_t* n_ids, int ca, int cb, int cc, const int32_t* thresholds, int dark,
                                         int bright, int K, int min_chroma, int64_t* sums, int64_t* hue, int B, int H,
                                         int W, int N, void* stream) {
  const char* who = "wm2f_labelmap_color_stats";
  WM2F_REQUIRE(N > 0, "%s: bad size", who);
  if (const int rc = check_picture(who, ca, cb, cc, B, H, W)) return rc;
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  WM2F_REQUIRE(dark >= 0 && dark <= 255 && bright >= 0 && bright <= 255, "%s: dark and bright are bytes, got %d and %d",
               who, dark, bright);
  WM2F_REQUIRE(hue == nullptr || (K >= 1 && K <= 36 && 360 % K == 0), "%s: K must divide 360 and be in [1, 36], got %d",
               who, K);
  WM2F_REQUIRE(hue == nullptr || (min_chroma >= 1 && min_chroma <= 255), "%s: min_chroma must be in [1, 255], got %d", who,
               min_chroma);
  if (N > kMapMaxIds) {
    set_error("%s: N <= %d (got %d)", who, kMapMaxIds, N);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(image && map && thresholds && sums, "%s: null pointer", who);
  WM2F_REQUIRE((ids == nullptr) == (n_ids == nullptr), "%s: ids and n_ids go together", who);
  hipStream_t s = (hipStream_t)stream;
  const int Kh = hue ? K : 0;
  if (hipMemsetAsync(sums, 0, (size_t)B * N * kCoCols * sizeof(int64_t), s) != hipSuccess ||
      (hue && hipMemsetAsync(hue, 0, (size_t)B * N * Kh * sizeof(int64_t), s) != hipSuccess)) {
    set_error("%s: clearing the results failed", who);
    return WM2F_ELAUNCH;
  }
  // about 1024 strips in all, at least 4096 pixels and at most kCoMaxStripRows rows each
  int rows = ceil_div(H, ceil_div(1024, B));
  const int min_rows = ceil_div(4096, W);
  rows = rows < min_rows ? min_rows : rows;
  rows = rows > kCoMaxStripRows ? kCoMaxStripRows : rows;
  rows = rows > H ? H : rows;
  const dim3 grid(ceil_div(H, rows), B);
  const bool lds = N <= kCoLdsMaxIds;
  const bool vec = map_vec4_ok(map, dtype, W) && aligned4(image);
  const size_t shm = (size_t)kCoRecN * 8 + (lds ? (size_t)N * (kCoAccBytes + 4 * Kh) : 0) + (ids ? (size_t)N * 4 : 0);
  CoParams prm{ca, cb, cc, dark, bright, Kh, min_chroma, 0};
  if (Kh) prm.hue_mul = ((1 << kCoHueShift) + 360 / Kh - 1) / (360 / Kh);
  long long* out = reinterpret_cast<long long*>(sums);
  long long* hout = reinterpret_cast<long long*>(hue);
  for_map_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kCoThreads), shm, s, image, map, ids, n_ids, thresholds, out, hout, H, W, N,
                         rows, prm);
    };
    if (vec && lds) launch(color_stats_kernel<DT, true, true>);
    else if (vec) launch(color_stats_kernel<DT, true, false>);
    else if (lds) launch(color_stats_kernel<DT, false, true>);
    else launch(color_stats_kernel<DT, false, false>);
  });
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_image_index_hist(const uint8_t* image, int ca, int cb, int cc, int64_t* hist, int B, int H, int W,
                                     void* stream) {
  const char* who = "wm2f_image_index_hist";
  if (const int rc = check_picture(who, ca, cb, cc, B, H, W)) return rc;
  WM2F_REQUIRE(image && hist, "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  const int bins = 255 * (abs(ca) + abs(cb) + abs(cc)) + 1;
  const int imin = 255 * ((ca < 0 ? ca : 0) + (cb < 0 ? cb : 0) + (cc < 0 ? cc : 0));
  if (hipMemsetAsync(hist, 0, (size_t)B * bins * sizeof(int64_t), s) != hipSuccess) {
    set_error("%s: clearing the histogram failed", who);
    return WM2F_ELAUNCH;
  }
  const int64_t npix = (int64_t)H * W, chunk = flat_chunk(B, npix);
  const dim3 grid((unsigned)ceil_div64(npix, chunk), B);
  const CoParams prm{ca, cb, cc, 0, 0, 0, 0, 0};
  long long* out = reinterpret_cast<long long*>(hist);
  const size_t shm = (size_t)bins * 4;
  if (npix % 4 == 0 && aligned4(image))
    hipLaunchKernelGGL(index_hist_kernel<true>, grid, dim3(kCoThreads), shm, s, image, out, npix, chunk, bins, imin, prm);
  else
    hipLaunchKernelGGL(index_hist_kernel<false>, grid, dim3(kCoThreads), shm, s, image, out, npix, chunk, bins, imin, prm);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_image_index_mask(const uint8_t* image, int ca, int cb, int cc, const int32_t* thresholds,
                                     uint8_t* mask, int64_t* counts, int B, int H, int W, void* stream) {
  const char* who = "wm2f_image_index_mask";
  if (const int rc = check_picture(who, ca, cb, cc, B, H, W)) return rc;
  WM2F_REQUIRE(image && thresholds && mask && counts, "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)B * sizeof(int64_t), s) != hipSuccess) {
    set_error("%s: clearing the counts failed", who);
    return WM2F_ELAUNCH;
  }
  const int64_t npix = (int64_t)H * W, chunk = flat_chunk(B, npix);
  const dim3 grid((unsigned)ceil_div64(npix, chunk), B);
  const CoParams prm{ca, cb, cc, 0, 0, 0, 0, 0};
  long long* out = reinterpret_cast<long long*>(counts);
  if (npix % 4 == 0 && aligned4(image) && aligned4(mask))
    hipLaunchKernelGGL(index_mask_kernel<true>, grid, dim3(kCoThreads), 0, s, image, thresholds, mask, out, npix, chunk, prm);
  else
    hipLaunchKernelGGL(index_mask_kernel<false>, grid, dim3(kCoThreads), 0, s, image, thresholds, mask, out, npix, chunk,
                       prm);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
