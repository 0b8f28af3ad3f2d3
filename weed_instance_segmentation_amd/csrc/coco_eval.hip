// Segmentation mAP on the device: the hot part of torchmetrics' MeanAveragePrecision(iou_type="segm") as the
// reference's models/metrics.py::test_with_metrics uses it (pycocotools COCOeval.evaluate on binary masks).
// The semantics are written out in DESIGN.md section 11; oracle/coco_eval.py restates them in plain loops.
//
//   labelmap_pairs : joint histogram (P+1) x (G+1) of a prediction id map and a GT raw-id map, per image.  Row 0 is
//                    "no prediction", column 0 "no accepted GT id".  Intersections are the inner bins, areas the
//                    row / column sums.  One read of the two maps: HBM-bound at 5 B/pixel (fp32 + uint8).
//   pack_bits / mask_pairs : the same intersections and areas for (D, H, W) and (G, H, W) mask stacks, which may
//                    overlap: pack to bits (one wave ballot per 64 pixels), then AND + popcount over 8 x 8 pair tiles.
//   coco_match     : the greedy COCO matching, one 64-lane workgroup per image, a lane per (area range, IoU threshold).
//                    coco_match_min is the same walk with a second (inter, area, area) triple: the IoU of a pair is the
//                    smaller of the two quotients (Boundary AP: mask IoU and boundary IoU).
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kPcThreads = 256;
constexpr int kPcMaxIds = 4096;       // accepted GT ids per image, kept in LDS for the binary search
constexpr int kPcLdsBins = 12288;     // 48 KiB LDS histogram; larger (P+1)(G+1) goes to global atomics
constexpr int kPcUnroll = 4;
constexpr int kMatchMaxG = 512;       // GT per image in LDS (see wm2f.h)
constexpr int kMatchMaxD = 1024;      // detections per image in LDS (see wm2f.h)
constexpr int kMatchMaxLanes = 64;    // area ranges x thresholds

__device__ __forceinline__ int pred_row(float v, int P) {
  // the post-processor writes ids as exact small floats; anything else is "no prediction".  A rule of its own, on the
  // float and not on its bits (labelmap.h's map_id_below): the prediction arrives typed, and P may exceed 2^24
  return (v >= 0.f && v < (float)P && v == floorf(v)) ? (int)v + 1 : 0;
}
__device__ __forceinline__ int pred_row(int32_t v, int P) { return (v >= 0 && v < P) ? v + 1 : 0; }

__device__ __forceinline__ int gt_col(int32_t v, const int32_t* ids, int n) { return list_row(v, ids, n) + 1; }

// grid (chunks, B), 256 threads.  hist (B, P+1, G+1) cleared by the host side.  The (0, 0) bin -- background on both
// maps, most of an image -- is never counted per pixel: each block adds the number of pixels it skipped once.
template <typename PT, typename GT, bool kLds>
__global__ __launch_bounds__(kPcThreads) void labelmap_pairs_kernel(const PT* __restrict__ pred, const GT* __restrict__ gt,
                                                                   const int32_t* __restrict__ gt_ids,
                                                                   const int32_t* __restrict__ n_ids,
                                                                   int32_t* __restrict__ hist, int64_t n, int P, int G,
                                                                   int64_t chunk) {
  extern __shared__ int32_t smem[];
  int32_t* ids = smem;
  int32_t* bins = smem + G;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int nb = (P + 1) * (G + 1);
  const int ng = n_ids[b] < G ? n_ids[b] : G;
  for (int j = tid; j < ng; j += kPcThreads) ids[j] = gt_ids[(int64_t)b * G + j];
  if (kLds)
    for (int j = tid; j < nb; j += kPcThreads) bins[j] = 0;
  __syncthreads();
  int32_t* hb = hist + (int64_t)b * nb;
  const PT* pb = pred + (int64_t)b * n;
  const GT* gb = gt + (int64_t)b * n;
  const int64_t start = (int64_t)blockIdx.x * chunk;
  const int64_t end = start + chunk < n ? start + chunk : n;
  int skipped = 0;
  for (int64_t base = start; base < end; base += kPcThreads * kPcUnroll) {  // uniform trip count: ballots below
    PT pv[kPcUnroll];
    GT gv[kPcUnroll];
#pragma unroll
    for (int u = 0; u < kPcUnroll; ++u) {
      const int64_t i = base + u * kPcThreads + tid;
      pv[u] = i < end ? pb[i] : PT(-1);
      gv[u] = i < end ? gb[i] : GT(0);
    }
#pragma unroll
    for (int u = 0; u < kPcUnroll; ++u) {
      const int64_t i = base + u * kPcThreads + tid;
      int bin = -1;
      if (i < end) {
        bin = pred_row(pv[u], P) * (G + 1) + gt_col((int32_t)gv[u], ids, ng);
        if (bin == 0) {
          ++skipped;
          bin = -1;
        }
      }
      // a wave inside one instance pair hits one bin: one add of the lane count instead of 64 conflicting atomics
      const int first = __shfl(bin, 0, 64);
      const bool same = bin == first;
      const unsigned long long m = __ballot(same);
      int* tgt = kLds ? bins : hb;
      if (same) {
        if (lane == 0 && first > 0) atomicAdd(tgt + first, (int)__popcll(m));
      } else if (bin > 0) {
        atomicAdd(tgt + bin, 1);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) skipped += __shfl_xor(skipped, o, 64);
  if (lane == 0 && skipped) atomicAdd(hb, skipped);
  if (kLds) {
    __syncthreads();
    for (int j = tid; j < nb; j += kPcThreads)
      if (bins[j]) atomicAdd(hb + j, bins[j]);
  }
}

// grid (ceil(pairs / (4 * kPackPairsPerWave)), M), 256 threads: word w of mask m = pixels [32w, 32w + 32).
constexpr int kPackPairsPerWave = 16;
__global__ __launch_bounds__(256) void pack_bits_kernel(const uint8_t* __restrict__ masks, uint32_t* __restrict__ bits,
                                                        int32_t* __restrict__ area, int64_t n, int64_t words) {
  const int m = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint8_t* src = masks + (int64_t)m * n;
  uint32_t* dst = bits + (int64_t)m * words;
  const int64_t npairs = (words + 1) / 2;
  const int64_t p0 = ((int64_t)blockIdx.x * 4 + wave) * kPackPairsPerWave;
  int cnt = 0;
  uint8_t v[kPackPairsPerWave];
#pragma unroll
  for (int k = 0; k < kPackPairsPerWave; ++k) {
    const int64_t i = (p0 + k) * 64 + lane;
    v[k] = (p0 + k < npairs && i < n) ? src[i] : 0;
  }
#pragma unroll
  for (int k = 0; k < kPackPairsPerWave; ++k) {
    const unsigned long long bal = __ballot(v[k] != 0);
    const int64_t p = p0 + k;
    if (lane == 0 && p < npairs) {
      dst[2 * p] = (uint32_t)bal;
      if (2 * p + 1 < words) dst[2 * p + 1] = (uint32_t)(bal >> 32);
      cnt += __popcll(bal);
    }
  }
  if (lane == 0 && cnt) atomicAdd(area + m, cnt);
}

// grid (ceil(D/8), ceil(G/8), splits), 256 threads: inter[d][g] += popcount(a_d & b_g) over this split's words.
constexpr int kTile = 8;
__global__ __launch_bounds__(256) void mask_pairs_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ bb,
                                                         int32_t* __restrict__ inter, int D, int G, int64_t words,
                                                         int64_t wsplit) {
  __shared__ int red[4][kTile * kTile];
  const int d0 = blockIdx.x * kTile, g0 = blockIdx.y * kTile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w0 = (int64_t)blockIdx.z * wsplit;
  const int64_t w1 = w0 + wsplit < words ? w0 + wsplit : words;
  int acc[kTile][kTile];
#pragma unroll
  for (int i = 0; i < kTile; ++i)
#pragma unroll
    for (int j = 0; j < kTile; ++j) acc[i][j] = 0;
  for (int64_t w = w0 + threadIdx.x; w < w1; w += 256) {
    uint32_t av[kTile], bv[kTile];
#pragma unroll
    for (int i = 0; i < kTile; ++i) {
      av[i] = d0 + i < D ? a[(int64_t)(d0 + i) * words + w] : 0u;
      bv[i] = g0 + i < G ? bb[(int64_t)(g0 + i) * words + w] : 0u;
    }
#pragma unroll
    for (int i = 0; i < kTile; ++i)
#pragma unroll
      for (int j = 0; j < kTile; ++j) acc[i][j] += __popc(av[i] & bv[j]);
  }
#pragma unroll
  for (int i = 0; i < kTile; ++i)
#pragma unroll
    for (int j = 0; j < kTile; ++j) {
      int s = acc[i][j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (lane == 0) red[wave][i * kTile + j] = s;
    }
  __syncthreads();
  if (threadIdx.x < kTile * kTile) {
    const int i = threadIdx.x / kTile, j = threadIdx.x % kTile;
    const int s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (s && d0 + i < D && g0 + j < G) atomicAdd(inter + (int64_t)(d0 + i) * G + g0 + j, s);
  }
}

struct MatchArgs {
  const int32_t* inter;      // (B, D, G)
  const int32_t* det_area;   // (B, D)
  const int32_t* gt_area;    // (B, G)
  const int32_t* det_label;  // (B, D)
  const int32_t* gt_label;   // (B, G)
  const int32_t* det_order;  // (B, D)
  const int32_t* n_det;      // (B)
  const int32_t* n_gt;       // (B)
  const double* iou_thr;     // (T)
  const double* area_rng;    // (A, 2)
  int32_t* det_rank;         // (B, D)
  uint8_t* det_matched;      // (B, A, T, D)
  uint8_t* det_ignored;      // (B, A, T, D)
  uint8_t* gt_ignored;       // (B, A, G)
  int D, G, T, A, max_det;
  const int32_t* inter2;     // kMin only: the second triple, shapes as the first
  const int32_t* det_area2;
  const int32_t* gt_area2;
};

// one 64-lane workgroup per image.  LDS: the image's detections (score order, label, area, rank), its GT sorted by
// (label, index) -- each category's GT contiguous and in input order -- one fp64 IoU row, and a matched flag per
// (lane, GT).  The walk is latency-bound, so nothing on its path reads global memory: the next detection's intersection
// row is loaded into registers while the current one is walked.
// kMin: a second intersection row in registers and the second areas of the GT and the detections in LDS (4 B each); the
// IoU row holds min(inter / union, inter2 / union2).  Area ranges, labels, order and ranks come from the first triple.
constexpr int kRowRegs = kMatchMaxG / 64;
template <bool kMin>
__global__ __launch_bounds__(64) void coco_match_kernel(MatchArgs p) {
  extern __shared__ __align__(8) unsigned char msmem[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int D = p.D, G = p.G, T = p.T, A = p.A, AT = A * T;
  const int nd = p.n_det[b] < D ? p.n_det[b] : D, ng = p.n_gt[b] < G ? p.n_gt[b] : G;
  double* iou = reinterpret_cast<double*>(msmem);
  int32_t* s_area = reinterpret_cast<int32_t*>(iou + G);
  int32_t* s_label = s_area + G;
  int32_t* s_idx = s_label + G;
  int32_t* d_order = s_idx + G;  // detection index at score position k (only real detections: nv of them)
  int32_t* d_label = d_order + D;
  int32_t* d_area = d_label + D;
  int32_t* d_rank = d_area + D;
  int32_t* s_area2 = d_rank + D;                 // kMin only: G
  int32_t* d_area2 = s_area2 + (kMin ? G : 0);   // kMin only: D
  uint8_t* matched = reinterpret_cast<uint8_t*>(d_area2 + (kMin ? D : 0));
  const int32_t* glab = p.gt_label + (int64_t)b * G;
  const int32_t* garea = p.gt_area + (int64_t)b * G;
  const int32_t* order = p.det_order + (int64_t)b * D;
  int32_t* tmp_label = reinterpret_cast<int32_t*>(iou);  // the IoU row is not in use yet
  for (int g = lane; g < ng; g += 64) tmp_label[g] = glab[g];
  __syncthreads();
  for (int g = lane; g < ng; g += 64) {  // stable counting rank by (label, index)
    const int lg = tmp_label[g];
    int pos = 0;
    for (int h = 0; h < ng; ++h) {
      const int lh = tmp_label[h];
      pos += (lh < lg) || (lh == lg && h < g);
    }
    s_area[pos] = garea[g];
    s_label[pos] = lg;
    s_idx[pos] = g;
    if (kMin) s_area2[pos] = p.gt_area2[(int64_t)b * G + g];
  }
  for (int j = lane; j < AT * ng; j += 64) matched[j] = 0;
  for (int j = lane; j < A * G; j += 64) {
    const int a = j / G, g = j - a * G;
    const double ag = (double)(g < ng ? garea[g] : 0);
    p.gt_ignored[(int64_t)b * A * G + j] = g < ng && (ag < p.area_rng[2 * a] || ag > p.area_rng[2 * a + 1]);
  }
  // the real detections in score order (padding indices >= nd dropped), then each one's rank within its category
  int nv = 0;
  for (int k0 = 0; k0 < D; k0 += 64) {
    const int d = k0 + lane < D ? order[k0 + lane] : -1;
    const bool ok = d >= 0 && d < nd;
    const unsigned long long m = __ballot(ok);
    if (ok) {
      const int k = nv + __popcll(m & ((1ull << lane) - 1ull));
      d_order[k] = d;
      d_label[k] = p.det_label[(int64_t)b * D + d];
      d_area[k] = p.det_area[(int64_t)b * D + d];
      if (kMin) d_area2[k] = p.det_area2[(int64_t)b * D + d];
    }
    nv += __popcll(m);
  }
  __syncthreads();
  for (int k = lane; k < nv; k += 64) {
    const int l = d_label[k];
    int r = 0;
    for (int k2 = 0; k2 < k; ++k2) r += d_label[k2] == l;
    d_rank[k] = r;
  }
  for (int d = nd + lane; d < D; d += 64) p.det_rank[(int64_t)b * D + d] = -1;  // padding; real ones below
  const bool active = lane < AT;
  const int a = active ? lane / T : 0, t = active ? lane - (lane / T) * T : 0;
  const double lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1];
  const double thr = p.iou_thr[t];
  const int64_t fbase = ((int64_t)(b * A + a) * T + t) * D;
  uint8_t* my = matched + lane * ng;
  if (active)  // padding detections: no flags
    for (int d = nd; d < D; ++d) {
      p.det_matched[fbase + d] = 0;
      p.det_ignored[fbase + d] = 0;
    }
  __syncthreads();
  int row[kRowRegs];
  int row2[kMin ? kRowRegs : 1];
  auto load_row = [&](int k) {
    const int64_t off = ((int64_t)b * D + d_order[k]) * G;
#pragma unroll
    for (int j = 0; j < kRowRegs; ++j) {
      const int pos = lane + 64 * j;
      row[j] = pos < ng ? p.inter[off + s_idx[pos]] : 0;
      if constexpr (kMin) row2[j] = pos < ng ? p.inter2[off + s_idx[pos]] : 0;
    }
  };
  if (nv > 0 && ng > 0) load_row(0);
  for (int k = 0; k < nv; ++k) {
    const int d = d_order[k], r = d_rank[k], lab = d_label[k], ad = d_area[k];
    const int ad2 = kMin ? d_area2[k] : 0;
    if (lane == 0) p.det_rank[(int64_t)b * D + d] = r;
    if (r >= p.max_det) {
      if (active) {
        p.det_matched[fbase + d] = 0;
        p.det_ignored[fbase + d] = 0;
      }
      if (k + 1 < nv && ng > 0) load_row(k + 1);
      continue;
    }
    __syncthreads();  // the previous detection's walk is done with iou[]
#pragma unroll
    for (int j = 0; j < kRowRegs; ++j) {
      const int pos = lane + 64 * j;
      if (pos < ng) {
        const int x = row[j];
        double q = x == 0 ? 0.0 : (double)x / ((double)ad + (double)s_area[pos] - (double)x);
        if constexpr (kMin) {
          const int x2 = row2[j];
          const double q2 = x2 == 0 ? 0.0 : (double)x2 / ((double)ad2 + (double)s_area2[pos] - (double)x2);
          q = q2 < q ? q2 : q;
        }
        iou[pos] = q;
      }
    }
    if (k + 1 < nv && ng > 0) load_row(k + 1);  // in flight during the walk
    __syncthreads();
    if (!active) continue;
    int s = 0, e = ng;  // the category's GT range in sorted order
    {
      int lo_i = 0, hi_i = ng;
      while (lo_i < hi_i) { const int mid = (lo_i + hi_i) >> 1; if (s_label[mid] < lab) lo_i = mid + 1; else hi_i = mid; }
      s = lo_i;
      hi_i = ng;
      while (lo_i < hi_i) { const int mid = (lo_i + hi_i) >> 1; if (s_label[mid] <= lab) lo_i = mid + 1; else hi_i = mid; }
      e = lo_i;
    }
    double best = thr < 1.0 - 1e-10 ? thr : 1.0 - 1e-10;
    int m = -1;
    bool m_ign = false;
    // one pass over the range takes the non-ignored GT (want_ign = false), a second one -- only while no non-ignored GT
    // matched -- the ignored ones.  LDS reads go out 8 at a time: the walk is a chain of LDS round trips otherwise.
    auto walk = [&](bool want_ign) {
      for (int j0 = s; j0 < e; j0 += 8) {
        double v[8];
        int ar[8];
        uint8_t mk[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = j0 + u < e ? j0 + u : e - 1;
          v[u] = iou[j];
          ar[u] = s_area[j];
          mk[u] = my[j];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (j0 + u >= e) break;
          const double ag = (double)ar[u];
          if ((ag < lo || ag > hi) != want_ign || mk[u]) continue;
          if (v[u] < best) continue;
          best = v[u];
          m = j0 + u;
          m_ign = want_ign;
        }
      }
    };
    walk(false);
    if (m < 0) walk(true);
    uint8_t dm = 0, di;
    if (m >= 0) {
      my[m] = 1;
      dm = 1;
      di = m_ign;
    } else {
      di = (double)ad < lo || (double)ad > hi;
    }
    p.det_matched[fbase + d] = dm;
    p.det_ignored[fbase + d] = di;
  }
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_labelmap_pair_counts(const void* pred_map, int pred_dtype, const void* gt_map, int gt_dtype,
                                         const int32_t* gt_ids, const int32_t* n_ids, int32_t* hist, int B,
                                         int64_t n_pixels, int P, int G, void* stream) {
  const char* who = "wm2f_labelmap_pair_counts";
  WM2F_REQUIRE(pred_map && gt_map && gt_ids && n_ids && hist, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && B < 65536 && n_pixels > 0 && P >= 0 && G >= 0, "%s: bad size", who);
  WM2F_REQUIRE(pred_dtype == WM2F_F32 || pred_dtype == WM2F_I32, "%s: prediction map must be fp32 or int32", who);
  WM2F_REQUIRE(gt_dtype == WM2F_U8 || gt_dtype == WM2F_I32, "%s: GT map must be uint8 or int32", who);
  if (G > kPcMaxIds) {
    set_error("%s: %d GT ids per image, at most %d", who, G, kPcMaxIds);
    return WM2F_EUNSUPPORTED;
  }
  const int64_t nb = (int64_t)(P + 1) * (G + 1);
  WM2F_REQUIRE(nb < (int64_t)1 << 30, "%s: histogram too large", who);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(hist, 0, (size_t)(B * nb) * sizeof(int32_t), s) != hipSuccess) {
    set_error("%s: clearing the histogram failed", who);
    return WM2F_ELAUNCH;
  }
  // about 1024 blocks in all, at least 4096 pixels each
  int64_t per_img = ceil_div64(1024, B);
  const int64_t max_chunks = ceil_div64(n_pixels, 4096);
  per_img = per_img < max_chunks ? per_img : max_chunks;
  if (per_img < 1) per_img = 1;
  const int64_t chunk = ceil_div64(ceil_div64(n_pixels, per_img), kPcThreads * kPcUnroll) * kPcThreads * kPcUnroll;
  const dim3 grid((unsigned)ceil_div64(n_pixels, chunk), B);
  const bool lds = nb <= kPcLdsBins;
  const size_t shm = (size_t)(G + (lds ? nb : 0)) * sizeof(int32_t);
  const auto launch = [&](auto* pred, auto* gt) {  // the two maps as the types they hold
    using PT = std::remove_const_t<std::remove_pointer_t<decltype(pred)>>;
    using GT = std::remove_const_t<std::remove_pointer_t<decltype(gt)>>;
    if (lds)
      hipLaunchKernelGGL((labelmap_pairs_kernel<PT, GT, true>), grid, dim3(kPcThreads), shm, s, pred, gt, gt_ids, n_ids, hist,
                         n_pixels, P, G, chunk);
    else
      hipLaunchKernelGGL((labelmap_pairs_kernel<PT, GT, false>), grid, dim3(kPcThreads), shm, s, pred, gt, gt_ids, n_ids, hist,
                         n_pixels, P, G, chunk);
  };
  if (pred_dtype == WM2F_F32 && gt_dtype == WM2F_U8) launch((const float*)pred_map, (const uint8_t*)gt_map);
  else if (pred_dtype == WM2F_F32) launch((const float*)pred_map, (const int32_t*)gt_map);
  else if (gt_dtype == WM2F_U8) launch((const int32_t*)pred_map, (const uint8_t*)gt_map);
  else launch((const int32_t*)pred_map, (const int32_t*)gt_map);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int64_t wm2f_mask_pair_counts_workspace(int D, int G, int64_t n_pixels) {
  if (D < 0 || G < 0 || n_pixels <= 0) return -1;
  return (int64_t)(D + G) * ceil_div64(n_pixels, 32) * (int64_t)sizeof(uint32_t);
}

extern "C" int wm2f_mask_pair_counts(const uint8_t* det_masks, const uint8_t* gt_masks, int32_t* inter, int32_t* det_area,
                                     int32_t* gt_area, void* workspace, int D, int G, int64_t n_pixels, void* stream) {
  const char* who = "wm2f_mask_pair_counts";
  WM2F_REQUIRE(workspace && (inter || D == 0 || G == 0), "%s: null pointer", who);
  WM2F_REQUIRE((det_masks && det_area) || D == 0, "%s: null detection pointer", who);
  WM2F_REQUIRE((gt_masks && gt_area) || G == 0, "%s: null GT pointer", who);
  WM2F_REQUIRE(D >= 0 && G >= 0 && D < 65536 && G < 65536 && D + G > 0 && n_pixels > 0 && n_pixels < ((int64_t)1 << 31),
               "%s: bad size", who);
  hipStream_t s = (hipStream_t)stream;
  const int64_t words = ceil_div64(n_pixels, 32);
  uint32_t* abits = (uint32_t*)workspace;
  uint32_t* gbits = abits + (int64_t)D * words;
  bool ok = true;
  if (D) ok &= hipMemsetAsync(det_area, 0, (size_t)D * sizeof(int32_t), s) == hipSuccess;
  if (G) ok &= hipMemsetAsync(gt_area, 0, (size_t)G * sizeof(int32_t), s) == hipSuccess;
  if (D && G) ok &= hipMemsetAsync(inter, 0, (size_t)D * G * sizeof(int32_t), s) == hipSuccess;
  if (!ok) {
    set_error("%s: clearing the outputs failed", who);
    return WM2F_ELAUNCH;
  }
  const int64_t npairs = (words + 1) / 2;
  const unsigned pack_blocks = (unsigned)ceil_div64(npairs, 4 * kPackPairsPerWave);
  if (D)
    hipLaunchKernelGGL(pack_bits_kernel, dim3(pack_blocks, D), dim3(256), 0, s, det_masks, abits, det_area, n_pixels, words);
  if (G)
    hipLaunchKernelGGL(pack_bits_kernel, dim3(pack_blocks, G), dim3(256), 0, s, gt_masks, gbits, gt_area, n_pixels, words);
  if (D && G) {
    const int td = ceil_div(D, kTile), tg = ceil_div(G, kTile);
    int64_t splits = ceil_div64(1024, (int64_t)td * tg);
    const int64_t max_splits = ceil_div64(words, 1024);
    splits = splits < max_splits ? splits : max_splits;
    if (splits < 1) splits = 1;
    const int64_t wsplit = ceil_div64(words, splits);
    hipLaunchKernelGGL(mask_pairs_kernel, dim3(td, tg, (unsigned)ceil_div64(words, wsplit)), dim3(256), 0, s, abits, gbits,
                       inter, D, G, words, wsplit);
  }
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

// both entry points; inter2 == nullptr selects the plain kernel
static int coco_match_launch(const char* who, bool two, const int32_t* inter, const int32_t* det_area,
                             const int32_t* gt_area, const int32_t* inter2, const int32_t* det_area2,
                             const int32_t* gt_area2, const int32_t* det_label, const int32_t* gt_label,
                             const int32_t* det_order, const int32_t* n_det, const int32_t* n_gt,
                             const double* iou_thresholds, const double* area_ranges, int32_t* det_rank,
                             uint8_t* det_matched, uint8_t* det_ignored, uint8_t* gt_ignored, int B, int D, int G, int T,
                             int A, int max_det, void* stream) {
  WM2F_REQUIRE(det_area && det_label && det_order && n_det && n_gt && iou_thresholds && area_ranges && det_rank &&
                   det_matched && det_ignored,
               "%s: null pointer", who);
  WM2F_REQUIRE(G == 0 || (inter && gt_area && gt_label && gt_ignored), "%s: null GT pointer", who);
  WM2F_REQUIRE(!two || (det_area2 && (G == 0 || (inter2 && gt_area2))), "%s: null pointer in the second triple", who);
  WM2F_REQUIRE(B > 0 && B < 65536 && D > 0 && G >= 0 && T > 0 && A > 0 && max_det > 0, "%s: bad size", who);
  if (A * T > kMatchMaxLanes || G > kMatchMaxG || D > kMatchMaxD) {
    set_error("%s: needs area ranges x thresholds <= %d, at most %d GT and %d detections per image (got %d x %d, %d, %d)",
              who, kMatchMaxLanes, kMatchMaxG, kMatchMaxD, A, T, G, D);
    return WM2F_EUNSUPPORTED;
  }
  MatchArgs a{inter, det_area, gt_area, det_label, gt_label, det_order, n_det, n_gt, iou_thresholds, area_ranges,
              det_rank, det_matched, det_ignored, gt_ignored, D, G, T, A, max_det, inter2, det_area2, gt_area2};
  const size_t shm = (size_t)G * (sizeof(double) + 3 * sizeof(int32_t)) + (size_t)D * 4 * sizeof(int32_t) + (size_t)A * T * G +
                     (two ? (size_t)(G + D) * sizeof(int32_t) : 0);
  if (two) hipLaunchKernelGGL(coco_match_kernel<true>, dim3(B), dim3(64), shm, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(coco_match_kernel<false>, dim3(B), dim3(64), shm, (hipStream_t)stream, a);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_coco_match(const int32_t* inter, const int32_t* det_area, const int32_t* gt_area,
                               const int32_t* det_label, const int32_t* gt_label, const int32_t* det_order,
                               const int32_t* n_det, const int32_t* n_gt, const double* iou_thresholds,
                               const double* area_ranges, int32_t* det_rank, uint8_t* det_matched, uint8_t* det_ignored,
                               uint8_t* gt_ignored, int B, int D, int G, int T, int A, int max_det, void* stream) {
  return coco_match_launch("wm2f_coco_match", false, inter, det_area, gt_area, nullptr, nullptr, nullptr, det_label, gt_label,
                           det_order, n_det, n_gt, iou_thresholds, area_ranges, det_rank, det_matched, det_ignored, gt_ignored,
                           B, D, G, T, A, max_det, stream);
}

extern "C" int wm2f_coco_match_min(const int32_t* inter, const int32_t* det_area, const int32_t* gt_area,
                                   const int32_t* inter2, const int32_t* det_area2, const int32_t* gt_area2,
                                   const int32_t* det_label, const int32_t* gt_label, const int32_t* det_order,
                                   const int32_t* n_det, const int32_t* n_gt, const double* iou_thresholds,
                                   const double* area_ranges, int32_t* det_rank, uint8_t* det_matched,
                                   uint8_t* det_ignored, uint8_t* gt_ignored, int B, int D, int G, int T, int A,
                                   int max_det, void* stream) {
  return coco_match_launch("wm2f_coco_match_min", true, inter, det_area, gt_area, inter2, det_area2, gt_area2, det_label,
                           gt_label, det_order, n_det, n_gt, iou_thresholds, area_ranges, det_rank, det_matched, det_ignored,
                           gt_ignored, B, D, G, T, A, max_det, stream);
}
