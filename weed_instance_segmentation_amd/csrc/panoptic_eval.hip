// Panoptic quality and semantic mIoU on the device: the pixel-free half of panopticapi's pq_compute
// -- which torchmetrics' PanopticQuality follows -- on the joint histogram wm2f_labelmap_pair_counts leaves, and the
// confusion matrix of class maps.  The semantics are written out in include/wm2f.h;
// tests/panoptic_quality_reference.py restates them in plain loops over pixels.
//
//   panoptic_match     : one 256-thread workgroup per image.  Pass 1 walks the histogram row by row with the lanes across
//                        the GT columns (coalesced): a lane owns its columns' sums in LDS (no atomics), a row's sum is a
//                        wave reduction and one LDS add per wave, its void count is the row's column 0.  Pass 2 walks the
//                        existing prediction rows again and reads only the bins whose two labels agree; a pair with
//                        2 * inter > union (int64) is a match, and since segments are disjoint at most one bin of a row
//                        and one of a column can be, so the owner of the column writes the match with no arbitration.
//                        Pass 3 writes the prediction states.
//   semantic_confusion : grid (chunks, B), 256 threads, four pixels per lane and load.  Bins live in LDS (int32) while
//                        C <= kScLdsMaxC and are flushed, the non-zero ones only, with 64-bit adds; above that the adds go
//                        to the result directly.  A wave whose lanes all hit one bin -- the inside of a region, most of a
//                        map -- issues one add of the lane count.
// Everything is integer but the one division per matched pair, so both results are bit-identical from run to run.
#include <type_traits>

#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kPmThreads = 256;
constexpr int kPmMaxP = 1024;   // prediction rows per image: 16 B of LDS each
constexpr int kPmMaxG = 4096;   // GT columns per image (the histogram's own cap): 8 B of LDS each; 48 KiB at both caps
constexpr int32_t kPmAbsent = INT32_MIN;

__global__ __launch_bounds__(kPmThreads) void panoptic_match_kernel(const int32_t* __restrict__ hist,
                                                                    const int32_t* __restrict__ pred_label,
                                                                    const int32_t* __restrict__ gt_label,
                                                                    const int32_t* __restrict__ n_pred,
                                                                    const int32_t* __restrict__ n_gt,
                                                                    int32_t* __restrict__ gt_match,
                                                                    double* __restrict__ gt_iou,
                                                                    uint8_t* __restrict__ pred_state, int P, int G,
                                                                    int void_as_background) {
  extern __shared__ int32_t pmem[];
  int32_t* g_area = pmem;        // (G) column sums
  int32_t* g_lab = g_area + G;   // (G) kPmAbsent beyond n_gt
  int32_t* p_area = g_lab + G;   // (P) row sums
  int32_t* p_void = p_area + P;  // (P) column 0 of the row
  int32_t* p_lab = p_void + P;   // (P) kPmAbsent beyond n_pred
  int32_t* p_hit = p_lab + P;    // (P) the row matched a GT column
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int np = n_pred[b] < 0 ? 0 : (n_pred[b] < P ? n_pred[b] : P);
  const int ng = n_gt[b] < 0 ? 0 : (n_gt[b] < G ? n_gt[b] : G);
  const int64_t stride = (int64_t)G + 1;
  const int32_t* hb = hist + (int64_t)b * (P + 1) * stride;
  for (int c = tid; c < G; c += kPmThreads) {
    g_area[c] = 0;
    g_lab[c] = c < ng ? gt_label[(int64_t)b * G + c] : kPmAbsent;
  }
  for (int p = tid; p < P; p += kPmThreads) {
    p_area[p] = 0;
    p_void[p] = 0;
    p_lab[p] = p < np ? pred_label[(int64_t)b * P + p] : kPmAbsent;
    p_hit[p] = 0;
  }
  __syncthreads();
  // pass 1: areas.  Column j of the histogram belongs to thread j % 256 in every row.
  for (int r = 0; r <= P; ++r) {
    const int32_t* row = hb + r * stride;
    int sum = 0;
    for (int j = tid; j <= G; j += kPmThreads) {
      const int v = row[j];
      sum += v;
      if (v != 0) {
        if (j > 0) g_area[j - 1] += v;
        else if (r > 0) p_void[r - 1] = v;
      }
    }
    if (r > 0) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
      if (lane == 0 && sum != 0) atomicAdd(p_area + r - 1, sum);
    }
  }
  __syncthreads();
  // pass 2: matching.  GT column c (histogram column c + 1) belongs to thread c % 256, which also initialises it.
  int32_t* gm = gt_match + (int64_t)b * G;
  double* gi = gt_iou + (int64_t)b * G;
  for (int c = tid; c < G; c += kPmThreads) {
    gm[c] = (g_lab[c] != kPmAbsent && g_area[c] > 0) ? -1 : -2;
    gi[c] = 0.0;
  }
  for (int p = 0; p < np; ++p) {  // workgroup-uniform
    const int lab = p_lab[p], area = p_area[p];
    if (lab == kPmAbsent || area == 0) continue;
    const int64_t own = (int64_t)area - (void_as_background ? 0 : p_void[p]);
    const int32_t* row = hb + (p + 1) * stride + 1;
    for (int c = tid; c < ng; c += kPmThreads) {
      if (g_lab[c] != lab) continue;
      const int64_t inter = row[c];
      if (inter <= 0) continue;
      const int64_t uni = own + (int64_t)g_area[c] - inter;
      if (2 * inter > uni) {
        gm[c] = p;
        gi[c] = (double)inter / (double)uni;
        p_hit[p] = 1;
      }
    }
  }
  __syncthreads();
  // pass 3: what became of every prediction row
  for (int p = tid; p < P; p += kPmThreads) {
    uint8_t st;
    if (p_lab[p] == kPmAbsent || p_area[p] == 0) st = 3;
    else if (p_hit[p]) st = 0;
    else st = (!void_as_background && 2 * (int64_t)p_void[p] > (int64_t)p_area[p]) ? 2 : 1;
    pred_state[(int64_t)b * P + p] = st;
  }
}

constexpr int kScThreads = 256;
constexpr int kScPix = 4;                       // pixels per lane per load
constexpr int kScStep = kScThreads * kScPix;
constexpr int kScLdsMaxC = 64;                  // 16 KiB of int32 bins: eight workgroups per CU fit 160 KiB of LDS
constexpr int kScMaxC = 1024;
constexpr int kScMaxIds = 4096;                 // listed raw ids per image: 8 B of LDS each

// four consecutive elements as one load (int64: two)
template <typename T>
__device__ __forceinline__ void load4(const T* p, T (&v)[kScPix]) {
  if constexpr (sizeof(T) == 1) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < kScPix; ++j) v[j] = (T)((w >> (8 * j)) & 0xffu);
  } else if constexpr (sizeof(T) == 4) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    v[0] = (T)q.x;
    v[1] = (T)q.y;
    v[2] = (T)q.z;
    v[3] = (T)q.w;
  } else {
    const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(p);
    const ulonglong2 c = *reinterpret_cast<const ulonglong2*>(p + 2);
    v[0] = (T)a.x;
    v[1] = (T)a.y;
    v[2] = (T)c.x;
    v[3] = (T)c.y;
  }
}

// kVec: n_pixels % 4 == 0 and both maps aligned for load4, so a lane's four pixels are inside the chunk or outside
// it together.  ids == nullptr: gt holds classes; otherwise raw ids, looked up in the image's ascending list.
template <typename PT, typename GT, bool kVec, bool kLds>
__global__ __launch_bounds__(kScThreads) void semantic_confusion_kernel(const PT* __restrict__ pred, const GT* __restrict__ gt,
                                                                        const int32_t* __restrict__ ids,
                                                                        const int32_t* __restrict__ cls,
                                                                        const int32_t* __restrict__ n_ids,
                                                                        unsigned long long* __restrict__ conf,
                                                                        unsigned long long* __restrict__ n_out, int64_t n,
                                                                        int G, int C, int ignore_index, int background_label,
                                                                        int64_t chunk) {
  extern __shared__ int32_t smem[];
  int32_t* s_ids = smem;
  int32_t* s_cls = smem + G;
  int32_t* bins = smem + 2 * G;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  int ng = 0;
  if (ids != nullptr) {
    ng = n_ids[b] < 0 ? 0 : (n_ids[b] < G ? n_ids[b] : G);
    for (int j = tid; j < ng; j += kScThreads) {
      s_ids[j] = ids[(int64_t)b * G + j];
      s_cls[j] = cls[(int64_t)b * G + j];
    }
  }
  if (kLds)
    for (int j = tid; j < C * C; j += kScThreads) bins[j] = 0;
  __syncthreads();
  const PT* pb = pred + (int64_t)b * n;
  const GT* gb = gt + (int64_t)b * n;
  const int64_t start = (int64_t)blockIdx.x * chunk;
  const int64_t end = start + chunk < n ? start + chunk : n;
  int out = 0;
  for (int64_t base = start; base < end; base += kScStep) {  // uniform trip count: ballots below
    const int64_t i = base + (int64_t)tid * kScPix;
    PT pv[kScPix];
    GT gv[kScPix];
    bool ok[kScPix];
    if (kVec) {
      const bool in = i < end;
#pragma unroll
      for (int j = 0; j < kScPix; ++j) {
        ok[j] = in;
        pv[j] = PT(0);
        gv[j] = GT(0);
      }
      if (in) {
        load4(pb + i, pv);
        load4(gb + i, gv);
      }
    } else {
#pragma unroll
      for (int j = 0; j < kScPix; ++j) {
        ok[j] = i + j < end;
        pv[j] = ok[j] ? pb[i + j] : PT(0);
        gv[j] = ok[j] ? gb[i + j] : GT(0);
      }
    }
#pragma unroll
    for (int j = 0; j < kScPix; ++j) {
      int bin = -1;
      if (ok[j]) {
        int g = (int)gv[j];
        if (ids != nullptr) {
          const int lo = list_lower_bound(g, s_ids, ng);
          g = (lo < ng && s_ids[lo] == g) ? s_cls[lo] : background_label;
        }
        if (g >= 0 && g < C && g != ignore_index) {
          const long long p = (long long)pv[j];
          if (p >= 0 && p < C) bin = g * C + (int)p;
          else ++out;
        }
      }
      const int first = __shfl(bin, 0, 64);
      const bool same = bin == first;
      const unsigned long long m = __ballot(same);
      if (kLds) {
        if (same) {
          if (lane == 0 && first >= 0) atomicAdd(bins + first, (int)__popcll(m));
        } else if (bin >= 0) {
          atomicAdd(bins + bin, 1);
        }
      } else {
        if (same) {
          if (lane == 0 && first >= 0) atomicAdd(conf + first, (unsigned long long)__popcll(m));
        } else if (bin >= 0) {
          atomicAdd(conf + bin, 1ull);
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) out += __shfl_xor(out, o, 64);
  if (lane == 0 && out) atomicAdd(n_out, (unsigned long long)out);
  if (kLds) {
    __syncthreads();
    for (int j = tid; j < C * C; j += kScThreads)
      if (bins[j]) atomicAdd(conf + j, (unsigned long long)bins[j]);
  }
}

template <typename PT, typename GT>
void launch_confusion(bool vec, bool lds, dim3 grid, size_t shm, hipStream_t s, const PT* pred, const GT* gt,
                      const int32_t* ids, const int32_t* cls, const int32_t* n_ids, unsigned long long* conf,
                      unsigned long long* n_out, int64_t n, int G, int C, int ignore_index, int background_label,
                      int64_t chunk) {
  const auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kScThreads), shm, s, pred, gt, ids, cls, n_ids, conf, n_out, n, G, C, ignore_index,
                       background_label, chunk);
  };
  if (vec && lds) launch(semantic_confusion_kernel<PT, GT, true, true>);
  else if (vec) launch(semantic_confusion_kernel<PT, GT, true, false>);
  else if (lds) launch(semantic_confusion_kernel<PT, GT, false, true>);
  else launch(semantic_confusion_kernel<PT, GT, false, false>);
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_panoptic_match(const int32_t* hist, const int32_t* pred_label, const int32_t* gt_label,
                                   const int32_t* n_pred, const int32_t* n_gt, int32_t* gt_match, double* gt_iou,
                                   uint8_t* pred_state, int B, int P, int G, int void_as_background, void* stream) {
  const char* who = "wm2f_panoptic_match";
  WM2F_REQUIRE(hist && n_pred && n_gt, "%s: null pointer", who);
  WM2F_REQUIRE(P == 0 || (pred_label && pred_state), "%s: null prediction pointer", who);
  WM2F_REQUIRE(G == 0 || (gt_label && gt_match && gt_iou), "%s: null GT pointer", who);
  WM2F_REQUIRE(B > 0 && B < 65536 && P >= 0 && G >= 0, "%s: bad size", who);
  if (P > kPmMaxP || G > kPmMaxG) {
    set_error("%s: at most %d prediction rows and %d GT columns per image (got %d, %d)", who, kPmMaxP, kPmMaxG, P, G);
    return WM2F_EUNSUPPORTED;
  }
  const size_t shm = ((size_t)2 * G + (size_t)4 * P) * sizeof(int32_t);
  hipLaunchKernelGGL(panoptic_match_kernel, dim3(B), dim3(kPmThreads), shm, (hipStream_t)stream, hist, pred_label,
                     gt_label, n_pred, n_gt, gt_match, gt_iou, pred_state, P, G, void_as_background);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_semantic_confusion(const void* pred, int pred_dtype, const void* gt, int gt_dtype,
                                       const int32_t* gt_ids, const int32_t* gt_cls, const int32_t* n_ids, int64_t* conf,
                                       int64_t* n_out_of_range, int B, int64_t n_pixels, int G, int C, int ignore_index,
                                       int background_label, void* stream) {
  const char* who = "wm2f_semantic_confusion";
  WM2F_REQUIRE(pred && gt && conf && n_out_of_range, "%s: null pointer", who);
  WM2F_REQUIRE((gt_ids == nullptr) == (gt_cls == nullptr) && (gt_ids == nullptr) == (n_ids == nullptr),
               "%s: gt_ids, gt_cls and n_ids go together", who);
  WM2F_REQUIRE(gt_ids != nullptr || G == 0, "%s: G without an id list", who);
  WM2F_REQUIRE(B > 0 && B < 65536 && n_pixels > 0 && n_pixels < ((int64_t)1 << 31) && G >= 0 && C > 0, "%s: bad size", who);
  WM2F_REQUIRE(pred_dtype == WM2F_I64 || pred_dtype == WM2F_I32 || pred_dtype == WM2F_U8,
               "%s: prediction map must be int64, int32 or uint8", who);
  WM2F_REQUIRE(gt_dtype == WM2F_U8 || gt_dtype == WM2F_I32, "%s: GT map must be uint8 or int32", who);
  if (C > kScMaxC || G > kScMaxIds) {
    set_error("%s: at most %d classes and %d listed ids per image (got %d, %d)", who, kScMaxC, kScMaxIds, C, G);
    return WM2F_EUNSUPPORTED;
  }
  // about 1024 blocks in all, at least 4096 pixels each
  int64_t per_img = ceil_div64(1024, B);
  const int64_t max_chunks = ceil_div64(n_pixels, 4096);
  per_img = per_img < max_chunks ? per_img : max_chunks;
  if (per_img < 1) per_img = 1;
  const int64_t chunk = ceil_div64(ceil_div64(n_pixels, per_img), kScStep) * kScStep;
  const dim3 grid((unsigned)ceil_div64(n_pixels, chunk), B);
  const bool lds = C <= kScLdsMaxC;
  const size_t psz = pred_dtype == WM2F_I64 ? 8 : (pred_dtype == WM2F_I32 ? 4 : 1);
  const size_t gsz = gt_dtype == WM2F_I32 ? 4 : 1;
  const size_t palign = psz * kScPix > 16 ? 16 : psz * kScPix, galign = gsz * kScPix;
  const bool vec = n_pixels % kScPix == 0 && reinterpret_cast<uintptr_t>(pred) % palign == 0 &&
                   reinterpret_cast<uintptr_t>(gt) % galign == 0;
  const size_t shm = ((size_t)2 * G + (lds ? (size_t)C * C : 0)) * sizeof(int32_t);
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* cf = reinterpret_cast<unsigned long long*>(conf);
  unsigned long long* no = reinterpret_cast<unsigned long long*>(n_out_of_range);
  const auto with_gt = [&](auto* p) {  // p: pred as the type it holds
    if (gt_dtype == WM2F_U8)
      launch_confusion(vec, lds, grid, shm, s, p, (const uint8_t*)gt, gt_ids, gt_cls, n_ids, cf, no, n_pixels, G, C,
                       ignore_index, background_label, chunk);
    else
      launch_confusion(vec, lds, grid, shm, s, p, (const int32_t*)gt, gt_ids, gt_cls, n_ids, cf, no, n_pixels, G, C,
                       ignore_index, background_label, chunk);
  };
  if (pred_dtype == WM2F_I64) with_gt((const int64_t*)pred);
  else if (pred_dtype == WM2F_I32) with_gt((const int32_t*)pred);
  else with_gt((const uint8_t*)pred);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
