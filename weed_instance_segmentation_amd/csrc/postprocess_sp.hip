// Device side of Mask2FormerImageProcessor.post_process_semantic_segmentation and
// post_process_panoptic_segmentation (transformers 5.15.0 models/mask2former/image_processing_mask2former.py:550-625,
// :748-841 with compute_segments :167-224).  DESIGN section 18.
//
// Semantic: S = einsum("bqc,bqhw->bchw", softmax(cls)[..., :-1], sigmoid(bilinear_384(logits))), bilinearly resized to
// the target size, argmax over classes.  Panoptic: the kept queries' sigmoid(bilinear_384(logits)), bilinearly resized
// to the target size, times the query's score; argmax over kept queries; per query the pixel counts that decide which
// segments survive; then the map is relabelled with the segment ids the host assigned from those counts.
//   semantic_scores        : S (B, C, gh, gw) fp32, one pass over the logits
//   semantic_resize_argmax : per target pixel the bilinear sample of every class of S, first-max argmax -> int64 map;
//                            optionally the resized scores (C, Ho, Wo)
//   panoptic_probs         : G (B, K, gh, gw) fp32 = sigmoid(bilinear_384(logits)) of the kept queries
//   panoptic_segments      : per target pixel v_k = bilinear(G_k) * score_k, first-max argmax k -> int32 map; per k the
//                            count of v_k >= mask_threshold and the count of pixels k owns (integer, deterministic)
//   panoptic_relabel       : map[p] = table[map[p]] (the host's k -> segment id, 0 for rejected queries)
// Streaming passes over small inputs; no roofline claim is made for them.
#include "common.h"
#include "postprocess_grid.h"

namespace wm2f {
namespace {

constexpr int kSemClassChunk = 8;  // class sums held in registers per pass over the queries
constexpr int kSegPixelsPerThread = 8;

// torch's CPU sigmoid: 1 / (1 + exp(-x)), with the accurate expf
__device__ __forceinline__ float sigmoidf_ref(float x) { return 1.f / (1.f + expf(-x)); }

// one thread per grid pixel; blockIdx.y = image.  The class probabilities of one chunk of classes sit in LDS
// (Q * kSemClassChunk floats); each chunk re-evaluates the Q bilinear samples (one chunk for C <= 8).
__global__ __launch_bounds__(256) void semantic_scores_kernel(const float* __restrict__ logits,
                                                              const float* __restrict__ probs, float* __restrict__ S,
                                                              int Q, int C, Grid g) {
  extern __shared__ float cp[];  // [Q][kSemClassChunk]
  const int b = blockIdx.y;
  const int n = g.gh * g.gw;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  const int gy = valid ? i / g.gw : 0, gx = valid ? i - gy * g.gw : 0;
  const float* lb = logits + (int64_t)b * Q * g.h * g.w;
  const float* pb = probs + (int64_t)b * Q * C;
  for (int c0 = 0; c0 < C; c0 += kSemClassChunk) {
    const int cn = C - c0 < kSemClassChunk ? C - c0 : kSemClassChunk;
    __syncthreads();
    for (int t = threadIdx.x; t < Q * kSemClassChunk; t += blockDim.x) {
      const int q = t / kSemClassChunk, j = t - q * kSemClassChunk;
      cp[t] = j < cn ? pb[q * C + c0 + j] : 0.f;
    }
    __syncthreads();
    if (!valid) continue;
    float acc[kSemClassChunk];
#pragma unroll
    for (int j = 0; j < kSemClassChunk; ++j) acc[j] = 0.f;
    for (int q = 0; q < Q; ++q) {  // ascending q, as the einsum's reduction
      const float s = sigmoidf_ref(grid_logit(lb + (int64_t)q * g.h * g.w, g, gy, gx));
#pragma unroll
      for (int j = 0; j < kSemClassChunk; ++j) acc[j] = fmaf(cp[q * kSemClassChunk + j], s, acc[j]);
    }
    float* out = S + ((int64_t)b * C + c0) * n + i;
    for (int j = 0; j < cn; ++j) out[(int64_t)j * n] = acc[j];
  }
}

// rows[j] = the image of output slot j (one launch per distinct target size).  Grid g: h, w = S's grid, gh, gw = target.
__global__ __launch_bounds__(256) void semantic_resize_argmax_kernel(const float* __restrict__ S,
                                                                     const int32_t* __restrict__ rows,
                                                                     int64_t* __restrict__ seg, float* __restrict__ out_scores,
                                                                     int C, Grid g) {
  const int j = blockIdx.y;
  const int64_t n = (int64_t)g.gh * g.gw;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int Y = i / g.gw, X = i - Y * g.gw;
  const int64_t plane = (int64_t)g.h * g.w;
  const float* sb = S + (int64_t)rows[j] * C * plane;
  float best = 0.f;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    const float v = grid_logit(sb + c * plane, g, Y, X);
    if (out_scores) out_scores[((int64_t)j * C + c) * n + i] = v;
    if (c == 0 || v > best) {  // first max wins
      best = v;
      arg = c;
    }
  }
  seg[(int64_t)j * n + i] = arg;
}

// one thread per grid pixel; blockIdx.y = b * K + k; slots k >= n_kept[b] are skipped (never read later)
__global__ __launch_bounds__(256) void panoptic_probs_kernel(const float* __restrict__ logits,
                                                             const int32_t* __restrict__ kept_q,
                                                             const int32_t* __restrict__ n_kept, float* __restrict__ G,
                                                             int Q, int K, Grid g) {
  const int bk = blockIdx.y, b = bk / K, k = bk - b * K;
  if (k >= n_kept[b]) return;
  const int n = g.gh * g.gw;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int gy = i / g.gw, gx = i - gy * g.gw;
  const float* p = logits + ((int64_t)b * Q + kept_q[bk]) * g.h * g.w;
  G[(int64_t)bk * n + i] = sigmoidf_ref(grid_logit(p, g, gy, gx));
}

// blockIdx.y = output slot j (image rows[j]); every thread handles kSegPixelsPerThread pixels of the block's tile.
// Grid g: h, w = G's grid, gh, gw = target.  counts (B, K, 2) int32, zeroed by the caller: [0] = #(v_k >= mask_thr),
// [1] = #pixels whose argmax is k.  LDS counters per block, then one global atomicAdd per (block, k, counter) != 0.
__global__ __launch_bounds__(256) void panoptic_segments_kernel(const float* __restrict__ G,
                                                                const int32_t* __restrict__ rows,
                                                                const int32_t* __restrict__ n_kept,
                                                                const float* __restrict__ scores, int32_t* __restrict__ seg,
                                                                int32_t* __restrict__ counts, int K, Grid g,
                                                                float mask_threshold) {
  extern __shared__ int cnt[];  // [K][2]
  const int j = blockIdx.y, b = rows[j];
  const int nk = n_kept[b];
  for (int t = threadIdx.x; t < 2 * nk; t += blockDim.x) cnt[t] = 0;
  __syncthreads();
  const int64_t n = (int64_t)g.gh * g.gw;
  const int64_t plane = (int64_t)g.h * g.w;
  const float* gb = G + (int64_t)b * K * plane;
  const float* sc = scores + (int64_t)b * K;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t base = (int64_t)blockIdx.x * blockDim.x * kSegPixelsPerThread;
  for (int r = 0; r < kSegPixelsPerThread; ++r) {
    const int64_t i = base + (int64_t)r * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    const int Y = valid ? (int)(i / g.gw) : 0, X = valid ? (int)(i - (int64_t)Y * g.gw) : 0;
    float best = 0.f;
    int arg = 0;
    for (int k = 0; k < nk; ++k) {
      const float v = __fmul_rn(grid_logit(gb + k * plane, g, Y, X), sc[k]);  // resize, then weigh: two roundings
      if (k == 0 || v > best) {  // first max wins
        best = v;
        arg = k;
      }
      const uint64_t above = __ballot(valid && v >= mask_threshold);
      if (lane == 0 && above) atomicAdd(&cnt[2 * k], __popcll(above));
    }
    if (valid) {
      atomicAdd(&cnt[2 * arg + 1], 1);
      seg[(int64_t)j * n + i] = arg;
    }
  }
  __syncthreads();
  int32_t* cb = counts + (int64_t)b * K * 2;
  for (int t = threadIdx.x; t < 2 * nk; t += blockDim.x)
    if (cnt[t]) atomicAdd(&cb[t], cnt[t]);
}

// seg (nrows, n) holds argmax indices k < n_kept[rows[j]]; table (B, K) int32
__global__ __launch_bounds__(256) void panoptic_relabel_kernel(int32_t* __restrict__ seg, const int32_t* __restrict__ rows,
                                                               const int32_t* __restrict__ table, int K, int64_t n) {
  const int j = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t* p = seg + (int64_t)j * n + i;
  *p = table[(int64_t)rows[j] * K + *p];
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_semantic_scores(const void* mask_logits, const void* class_probs, void* scores, int B, int Q, int C,
                                    int h, int w, int gh, int gw, void* stream) {
  const char* who = "wm2f_semantic_scores";
  WM2F_REQUIRE(mask_logits && class_probs && scores, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && B < 65536 && Q > 0 && Q <= 4096 && C > 0, "%s: bad size", who);
  Grid g;
  if (int rc = make_grid(g, h, w, gh, gw, who)) return rc;
  const size_t lds = (size_t)Q * kSemClassChunk * sizeof(float);
  hipLaunchKernelGGL(semantic_scores_kernel, dim3(ceil_div(gh * gw, 256), B), dim3(256), lds, (hipStream_t)stream,
                     (const float*)mask_logits, (const float*)class_probs, (float*)scores, Q, C, g);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_semantic_resize_argmax(const void* scores, const int32_t* rows, int nrows, void* segmentation,
                                           void* out_scores, int C, int gh, int gw, int Ho, int Wo, void* stream) {
  const char* who = "wm2f_semantic_resize_argmax";
  WM2F_REQUIRE(scores && rows && segmentation, "%s: null pointer", who);
  WM2F_REQUIRE(nrows > 0 && nrows < 65536 && C > 0 && Ho > 0 && Wo > 0 && (int64_t)Ho * Wo < INT32_MAX, "%s: bad size",
               who);
  Grid g;
  if (int rc = make_grid(g, gh, gw, Ho, Wo, who)) return rc;
  hipLaunchKernelGGL(semantic_resize_argmax_kernel, dim3(ceil_div(Ho * Wo, 256), nrows), dim3(256), 0, (hipStream_t)stream,
                     (const float*)scores, rows, (int64_t*)segmentation, (float*)out_scores, C, g);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_panoptic_probs(const void* mask_logits, const int32_t* kept_q, const int32_t* n_kept, void* probs, int B,
                                   int Q, int K, int h, int w, int gh, int gw, void* stream) {
  const char* who = "wm2f_panoptic_probs";
  WM2F_REQUIRE(mask_logits && kept_q && n_kept && probs, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && Q > 0 && K > 0 && K <= Q && (int64_t)B * K < 65536, "%s: bad size", who);
  Grid g;
  if (int rc = make_grid(g, h, w, gh, gw, who)) return rc;
  hipLaunchKernelGGL(panoptic_probs_kernel, dim3(ceil_div(gh * gw, 256), B * K), dim3(256), 0, (hipStream_t)stream,
                     (const float*)mask_logits, kept_q, n_kept, (float*)probs, Q, K, g);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_panoptic_segments(const void* probs, const int32_t* rows, const int32_t* n_kept, const void* scores,
                                      int32_t* segmentation, int32_t* counts, int nrows, int K, int gh, int gw, int Ho,
                                      int Wo, float mask_threshold, void* stream) {
  const char* who = "wm2f_panoptic_segments";
  WM2F_REQUIRE(probs && rows && n_kept && scores && segmentation && counts, "%s: null pointer", who);
  WM2F_REQUIRE(nrows > 0 && nrows < 65536 && K > 0 && K <= 4096 && Ho > 0 && Wo > 0 && (int64_t)Ho * Wo < INT32_MAX,
               "%s: bad size", who);
  Grid g;
  if (int rc = make_grid(g, gh, gw, Ho, Wo, who)) return rc;
  const size_t lds = (size_t)K * 2 * sizeof(int);
  hipLaunchKernelGGL(panoptic_segments_kernel, dim3(ceil_div(Ho * Wo, 256 * kSegPixelsPerThread), nrows), dim3(256), lds,
                     (hipStream_t)stream, (const float*)probs, rows, n_kept, (const float*)scores, segmentation, counts, K,
                     g, mask_threshold);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_panoptic_relabel(int32_t* segmentation, const int32_t* rows, const int32_t* table, int nrows, int K,
                                     int64_t n_pixels, void* stream) {
  const char* who = "wm2f_panoptic_relabel";
  WM2F_REQUIRE(segmentation && rows && table, "%s: null pointer", who);
  WM2F_REQUIRE(nrows > 0 && nrows < 65536 && K > 0 && n_pixels > 0 && n_pixels < INT32_MAX, "%s: bad size", who);
  hipLaunchKernelGGL(panoptic_relabel_kernel, dim3((unsigned)ceil_div64(n_pixels, 256), nrows), dim3(256), 0,
                     (hipStream_t)stream, segmentation, rows, table, K, n_pixels);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
