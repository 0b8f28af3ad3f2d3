// 1x1 convolution in NCHW at fp32 accuracy on the bf16 matrix cores ("split-bf16"):
//     y_b (N, P) = epilogue( W (N, K) . x_b[:, sampled p] (K, P) ),   P = Ho * Wo,  pixel p = (ho, wo) reads (s ho, s wo)
// for the ResNet bottlenecks' conv1 / conv3 / projection shortcut and the pixel decoder's input projections, adapter_1 and
// mask_projection (inference; BatchNorm folded into W and the bias by the caller).
//
// Arithmetic: that of token_gemm_split.hip -- both operands written as three bf16 pieces (h clamped to the largest finite
// bf16), the six products h.h, h.m, m.h, h.l, l.h, m.m summed in fp32 on v_mfma_f32_16x16x32_bf16 per k-step and the
// k-step sums added to the accumulator in order.
// The sequence of MFMAs an output element sees does not depend on the tile configuration, the batch or the other pixels,
// so results are bit-identical run to run and for any sub-batch.
//
// Layout of the work:
//   * W is split once per weight version by wm2f_token_linear_split_weight (fragment order [k-step][row tile][piece][lane]
//     [8 bf16]); a workgroup streams the NT-row panel of each k-step into a two-slot LDS ring by LDS-DMA (1 KiB pieces);
//   * W is the A operand (rows = output channels n), x the B operand (columns = pixels p).  A lane (j, g) of a B fragment
//     needs channels 8g .. 8g + 7 of pixel j: NCHW is channel-strided, so the lane loads them as 8 dwords, one per channel;
//     the 16 lanes of one g read 16 consecutive pixels (64 contiguous bytes at stride 1), and the wave's two column tiles
//     the full 128 bytes.  Each element is split once per wave in registers (no LDS staging);
//   * a workgroup of 8 waves owns an (NT channels) x (PT pixels) tile of one image, WN waves along n and 8 / WN along p;
//     a wave holds NRT row tiles x 2 column tiles of accumulators.  Configurations come from kCfg below, chosen per shape
//     by the host (fewest workgroup rounds on the device, weighted by the wave's work per k-step);
//   * epilogue in the store: lane (j, g) holds channels 4g .. 4g + 3 of pixel j, stored as dwords, 64 contiguous bytes per
//     channel row and wave-instruction.  Pixels p >= P (ragged tail) read zeros and store nothing.
//
// GroupNorm on either side (group_norm.h): the STATS instances also reduce the group statistics of what they
// store (input projections, adapter_1), the NORM instance normalises its operand as it loads it (mask_projection).  The
// stored output of a STATS instance is bit for bit that of the plain one; "no atomics" holds for the output, the
// statistics are added into an fp64 workspace with one atomic pair per (workgroup, group).
//
// Two sources (the DUAL instances): a bottleneck's conv3 and its projection shortcut as ONE GEMM over the
// concatenated K,  y = relu([W1 | W2] . [x1 ; x2 sampled] + bias).  The k-steps of source 1 come first, then those of
// source 2, each from its own split weight (the split is k-step major, so the two splits laid end to end ARE the split of
// [W1 | W2]) and its own image; the source of a k-step is chosen with wave-uniform selects.
#include <type_traits>

#include "common.h"
#include "group_norm.h"

namespace wm2f {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x8 = __attribute__((ext_vector_type(8))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kCT = 2;        // column tiles (16 pixels each) per wave
constexpr int kKStep = 32;    // K of one v_mfma_f32_16x16x32_bf16
constexpr int kFrag = 1024;   // bytes of one A fragment piece (64 lanes x 8 bf16)
constexpr unsigned kOob = 0x80000000u;
constexpr float kBf16Max = 3.38953139e38f;  // largest finite bf16, 0x7F7F

// epilogues, fixed at compile time
enum : int { kRaw = 0, kBias = 1, kBiasRelu = 2, kBiasResRelu = 3 };

// the first P pieces of the three-piece split (the pieces past P are left untouched and never read)
template <int P>
__device__ __forceinline__ void split3(const f32x8 x, bf16x8& h, bf16x8& m, bf16x8& l) {
  f32x8 xc;
#pragma unroll
  for (int i = 0; i < 8; ++i) xc[i] = __builtin_amdgcn_fmed3f(x[i], -kBf16Max, kBf16Max);
  if constexpr (P == 1) {  // no residual piece carries an inf or a NaN on: x * 0 (0, or NaN) keeps h non-finite with x
#pragma unroll
    for (int i = 0; i < 8; ++i) xc[i] = __builtin_fmaf(x[i], 0.f, xc[i]);
  }
  h = __builtin_convertvector(xc, bf16x8);
  if constexpr (P >= 2) {
    const f32x8 r1 = x - __builtin_convertvector(h, f32x8);
    m = __builtin_convertvector(r1, bf16x8);
    if constexpr (P >= 3) {
      const f32x8 r2 = r1 - __builtin_convertvector(m, f32x8);
      l = __builtin_convertvector(r2, bf16x8);
    }
  }
}

struct C1Args {
  const float *x, *bias, *residual;
  const void* ws;
  float* out;
  int K, N;
  int Hi, Wi, Wo, P, stride;
  // STATS: the group statistics of the stored output, stats[(b G + g) 2 + {0, 1}] += (sum, sum of squares); cpg = N / G
  double* stats;
  int G, cpg;
  // NORM: x is read as act(GroupNorm_nG(x) * ngamma + nbeta) from the filled workspace nstats (stride 1)
  const double* nstats;
  const float *ngamma, *nbeta;
  float neps;
  int nG, nrelu;
};

// DUAL: source 1 is (x, ws, K) above, read at stride 1 (Hi x Wi is the output map); source 2 follows it in K
struct C1DualArgs : C1Args {
  const float* x2;
  const void* ws2;
  int K2, H2, W2, stride2;
};

__device__ __forceinline__ void c1_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// NRT row tiles per wave, WN waves along n: a workgroup tile is NT = WN * NRT * 16 channels by PT = (8 / WN) * 32 pixels.
// STATS: the epilogue also reduces the group statistics of what it stores (gn_tile_stats; cpg in {4, 8, 16}).
// NORM: every loaded element becomes act(scale[b][k] x + shift[b][k]) before the split, the K pairs computed once per
// workgroup into LDS behind the ring (gn_affine / gn_apply: the bits group_norm_apply_kernel writes).
// P = the pieces of each operand that take part: 3 = all six products, 2 = h and m (m.h, h.m, h.h), 1 = h
// alone (h.h).  The split weight is the three-piece one at every P; the ring holds the first P pieces of each row tile.
// DUAL: k-steps 0 .. K / 32 - 1 read (ws, x), the next K2 / 32 read (ws2, x2 sampled at stride2); + bias + ReLU only.
template <int NRT, int WN, int EPI, bool STATS = false, bool NORM = false, int P = 3, bool DUAL = false>
__global__ __launch_bounds__(kThreads) void conv1x1_split_kernel(std::conditional_t<DUAL, C1DualArgs, C1Args> a) {
  static_assert(P >= 1 && P <= 3, "one, two or three pieces");
  static_assert(!DUAL || (EPI == kBiasRelu && !STATS && !NORM), "two sources: + bias + ReLU, no GroupNorm on either side");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [2][NT / 16][P][64][16 B] (+ NORM: [2][K] floats)
  constexpr int kRowTiles = WN * NRT;
  constexpr int kPanelBytes = kRowTiles * P * kFrag;
  constexpr int kPieces = kRowTiles * P;
  constexpr int kPT = (kWaves / WN) * kCT * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave % WN, wp = wave / WN;
  const int g = lane >> 4, j = lane & 15;
  const int nb = blockIdx.x, b = blockIdx.z;
  const int n_wg = nb * kRowTiles * 16;            // first channel of the workgroup
  const int p_w = blockIdx.y * kPT + wp * kCT * 16;  // first pixel of the wave
  const int n_ks1 = a.K / kKStep;  // k-steps of the (first) source
  int n_ks = n_ks1;
  if constexpr (DUAL) n_ks += a.K2 / kKStep;
  const int HWi = a.Hi * a.Wi;

  // per-image buffers (each below 2 GiB: checked by the host)
  const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.ws, 0, a.N * a.K * 6, 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)(a.x + (int64_t)b * a.K * HWi), 0, a.K * HWi * 4, 0x00020000);

  // source offset of this lane's pixel in each column tile (channel 8g of the k-step added per load)
  unsigned xo[kCT];
#pragma unroll
  for (int c = 0; c < kCT; ++c) {
    const int p = p_w + c * 16 + j;
    const int ho = p / a.Wo, wo = p - ho * a.Wo;
    xo[c] = p < a.P ? (unsigned)(((8 * g) * HWi + a.stride * (ho * a.Wi + wo)) * 4) : kOob;
  }
  const unsigned ch_bytes = (unsigned)HWi * 4;

  // DUAL: the same three things for the second source -- per-image resources, pixel offsets, channel stride
  __amdgpu_buffer_rsrc_t w2_rs = w_rs, x2_rs = x_rs;
  unsigned xo2[kCT] = {kOob, kOob};
  unsigned ch_bytes2 = ch_bytes;
  if constexpr (DUAL) {
    const int HW2 = a.H2 * a.W2;
    w2_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.ws2, 0, a.N * a.K2 * 6, 0x00020000);
    x2_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.x2 + (int64_t)b * a.K2 * HW2), 0, a.K2 * HW2 * 4, 0x00020000);
#pragma unroll
    for (int c = 0; c < kCT; ++c) {
      const int p = p_w + c * 16 + j;
      const int ho = p / a.Wo, wo = p - ho * a.Wo;
      xo2[c] = p < a.P ? (unsigned)(((8 * g) * HW2 + a.stride2 * (ho * a.W2 + wo)) * 4) : kOob;
    }
    ch_bytes2 = (unsigned)HW2 * 4;
  }

  float* ntab = reinterpret_cast<float*>(smem + 2 * kPanelBytes);  // NORM: scale[K], shift[K] of image b
  if (NORM) {
    const int ncpg = a.K / a.nG;
    const double n = (double)ncpg * (double)HWi;
    for (int c = tid; c < a.K; c += kThreads) {
      const GnAffine f = gn_affine(a.nstats, b * a.nG + c / ncpg, n, a.neps, a.ngamma[c], a.nbeta[c]);
      ntab[c] = f.scale;
      ntab[a.K + c] = f.shift;
    }
    __syncthreads();
  }

  f32x8 xr[kCT];
  // ring slot ks & 1 and xr <- k-step ksl of the source (wr, xs, po, cb)
  auto issue_from = [&](int ks, int ksl, const __amdgpu_buffer_rsrc_t wr, const __amdgpu_buffer_rsrc_t xs, const unsigned (&po)[kCT],
                        unsigned cb) {
    unsigned char* dst = smem + (ks & 1) * kPanelBytes;
    const int src = (ksl * (a.N / 16) + n_wg / 16) * 3 * kFrag;
    for (int f = wave; f < kPieces; f += kWaves) {
      const int fs = P == 3 ? f : (f / P) * 3 + f % P;  // ring piece f = piece f % P of row tile f / P
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_ptr_t)(dst + f * kFrag), 16, lane * 16, src + fs * kFrag, 0, 0);
    }
    const unsigned kb = (unsigned)(ksl * kKStep) * cb;
#pragma unroll
    for (int c = 0; c < kCT; ++c) {
      const unsigned o = po[c] == kOob ? kOob : po[c] + kb;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        xr[c][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xs, o, i * cb, 0));
    }
  };
  auto issue = [&](int ks) {
    if constexpr (DUAL) {  // wave-uniform selects and one load sequence: no branch around the x loads (§13.3)
      const bool second = ks >= n_ks1;
      const unsigned po[kCT] = {second ? xo2[0] : xo[0], second ? xo2[1] : xo[1]};
      issue_from(ks, second ? ks - n_ks1 : ks, second ? w2_rs : w_rs, second ? x2_rs : x_rs, po, second ? ch_bytes2 : ch_bytes);
    } else {
      issue_from(ks, ks, w_rs, x_rs, xo, ch_bytes);
    }
  };

  issue(0);
  c1_barrier();

  f32x4 acc[NRT][kCT];
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
    for (int c = 0; c < kCT; ++c) acc[rt][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int ks = 0; ks < n_ks; ++ks) {
    bf16x8 bh[kCT], bm[kCT], bl[kCT];
    if (NORM) {  // channels 32 ks + 8 g .. + 7; the columns of pixels p >= P are never stored, their value is free
      const f32x8 sc = *reinterpret_cast<const f32x8*>(ntab + ks * kKStep + 8 * g);
      const f32x8 sh = *reinterpret_cast<const f32x8*>(ntab + a.K + ks * kKStep + 8 * g);
#pragma unroll
      for (int c = 0; c < kCT; ++c)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const GnAffine f = {sc[i], sh[i]};
          xr[c][i] = a.nrelu ? gn_apply_relu(xr[c][i], f) : gn_apply(xr[c][i], f);
        }
    }
#pragma unroll
    for (int c = 0; c < kCT; ++c) split3<P>(xr[c], bh[c], bm[c], bl[c]);
    if (ks + 1 < n_ks) issue(ks + 1);  // the next step's loads fly under this step's MFMAs

    const unsigned char* panel = smem + (ks & 1) * kPanelBytes + wn * NRT * P * kFrag;
    auto read_a = [&](bf16x8 (&dst)[3], int rt) {
#pragma unroll
      for (int p = 0; p < P; ++p) dst[p] = *reinterpret_cast<const bf16x8*>(panel + (rt * P + p) * kFrag + lane * 16);
    };
    // the six products of one (row tile, column tile), the small terms first, summed from zero and added to the
    // accumulator once per k-step: the accumulator takes K / 32 roundings, not 6 K / 32 (at K = 2048 the six MFMAs
    // straight into it measured 2.6x the error of the fp32 library convolution against fp64)
    auto six = [&](f32x4 acc_in, const bf16x8 (&av)[3], int cc) {
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
      if constexpr (P == 3) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], bm[cc], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[2], bh[cc], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bl[cc], c, 0, 0, 0);
      }
      if constexpr (P >= 2) {  // P = 2: m.h, h.m, h.h, the order they have in the six-product chain
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], bh[cc], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bm[cc], c, 0, 0, 0);
      }
      return acc_in + __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bh[cc], c, 0, 0, 0);
    };
    bf16x8 av[2][3];
    read_a(av[0], 0);
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
      if (rt + 1 < NRT) read_a(av[(rt + 1) & 1], rt + 1);
      __builtin_amdgcn_sched_barrier(0);
      acc[rt][0] = six(acc[rt][0], av[rt & 1], 0);
      acc[rt][1] = six(acc[rt][1], av[rt & 1], 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    c1_barrier();  // step ks + 1's panel and x have landed; every wave is done with slot ks & 1
  }

  // ---- epilogue: lane (j, g) holds, per row tile rt and column tile c, channels n0 + rt*16 + 4g .. +3 of pixel p_w + 16c + j
  const int64_t img = (int64_t)b * a.N * a.P;
  const __amdgpu_buffer_rsrc_t o_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.out + img), 0, a.N * a.P * 4, 0x00020000);
  __amdgpu_buffer_rsrc_t r_rs = o_rs;
  if (EPI == kBiasResRelu) r_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.residual + img), 0, a.N * a.P * 4, 0x00020000);
  const int n0 = n_wg + wn * NRT * 16 + 4 * g;
  float gs[NRT], gss[NRT];  // STATS: this lane's sum and sum of squares per row tile
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt) {
    gs[rt] = gss[rt] = 0.f;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (EPI != kRaw) {
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[e] = a.bias[n0 + rt * 16 + e];
    }
#pragma unroll
    for (int c = 0; c < kCT; ++c) {
      const int p = p_w + c * 16 + j;
      const unsigned ro = p < a.P ? (unsigned)(((n0 + rt * 16) * a.P + p) * 4) : kOob;
      const unsigned rs = (unsigned)a.P * 4;
      float rv[4] = {0.f, 0.f, 0.f, 0.f};
      if (EPI == kBiasResRelu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) rv[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_rs, ro, e * rs, 0));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[rt][c][e];
        if (EPI != kRaw) v += bv[e];
        if (EPI == kBiasResRelu) v += rv[e];
        if (EPI == kBiasRelu || EPI == kBiasResRelu) v = v < 0.f ? 0.f : v;  // a NaN stays a NaN
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), o_rs, ro, e * rs, 0);
        if (STATS && p < a.P) {
          gs[rt] += v;
          gss[rt] = fmaf(v, v, gss[rt]);
        }
      }
    }
  }
  if (STATS) gn_tile_stats<NRT, WN, kWaves>(gs, gss, smem, a.stats, b * a.G, n_wg, a.cpg, tid);
}

// The configurations, (NRT, WN): workgroup tile NT x PT = (WN NRT 16) x (8 / WN x 32).  The LDS ring is 2 x NT x 64 P B.
struct Cfg {
  int nrt, wn;
};
constexpr Cfg kCfg[] = {{16, 1}, {8, 2}, {4, 4}, {8, 1}, {4, 1}};
constexpr int kNumCfg = sizeof(kCfg) / sizeof(kCfg[0]);

// The instances: the four epilogues; the statistics on raw and + bias; the normalised operand on + bias.
enum : int { kPlain = 0, kStats = 1, kNorm = 2 };

template <int NRT, int WN, int P>
void (*pick_epi(int epi, int opt))(C1Args) {
  if (opt == kStats)
    return epi == kRaw ? conv1x1_split_kernel<NRT, WN, kRaw, true, false, P> : conv1x1_split_kernel<NRT, WN, kBias, true, false, P>;
  if (opt == kNorm) return conv1x1_split_kernel<NRT, WN, kBias, false, true, P>;
  switch (epi) {
    case kRaw: return conv1x1_split_kernel<NRT, WN, kRaw, false, false, P>;
    case kBias: return conv1x1_split_kernel<NRT, WN, kBias, false, false, P>;
    case kBiasRelu: return conv1x1_split_kernel<NRT, WN, kBiasRelu, false, false, P>;
    default: return conv1x1_split_kernel<NRT, WN, kBiasResRelu, false, false, P>;
  }
}

template <int P>
void (*pick_cfg(int ci, int epi, int opt))(C1Args) {
  switch (ci) {
    case 0: return pick_epi<16, 1, P>(epi, opt);
    case 1: return pick_epi<8, 2, P>(epi, opt);
    case 2: return pick_epi<4, 4, P>(epi, opt);
    case 3: return pick_epi<8, 1, P>(epi, opt);
    default: return pick_epi<4, 1, P>(epi, opt);
  }
}

// The two-source instances: every configuration and piece count, + bias + ReLU.
template <int P>
void (*pick_dual_cfg(int ci))(C1DualArgs) {
  switch (ci) {
    case 0: return conv1x1_split_kernel<16, 1, kBiasRelu, false, false, P, true>;
    case 1: return conv1x1_split_kernel<8, 2, kBiasRelu, false, false, P, true>;
    case 2: return conv1x1_split_kernel<4, 4, kBiasRelu, false, false, P, true>;
    case 3: return conv1x1_split_kernel<8, 1, kBiasRelu, false, false, P, true>;
    default: return conv1x1_split_kernel<4, 1, kBiasRelu, false, false, P, true>;
  }
}

void (*pick_dual(int ci, int pieces))(C1DualArgs) {
  return pieces == 3 ? pick_dual_cfg<3>(ci) : (pieces == 2 ? pick_dual_cfg<2>(ci) : pick_dual_cfg<1>(ci));
}

void (*pick_kernel(int ci, int epi, int opt, int pieces))(C1Args) {
  return pieces == 3 ? pick_cfg<3>(ci, epi, opt) : (pieces == 2 ? pick_cfg<2>(ci, epi, opt) : pick_cfg<1>(ci, epi, opt));
}

// The configuration of a shape: fewest rounds of workgroups over the CUs (one 8-wave workgroup per CU) times the wave's
// work per k-step (NRT row tiles, plus a fixed share for the barrier, the x loads and the split); ties go to the wider NT.
int choose_cfg(int N, int P, int B, int n_cu) {
  int best = -1;
  int64_t best_cost = 0;
  for (int i = 0; i < kNumCfg; ++i) {
    const int nt = kCfg[i].wn * kCfg[i].nrt * 16, pt = (kWaves / kCfg[i].wn) * kCT * 16;
    if (N % nt) continue;
    const int64_t wgs = (int64_t)(N / nt) * ceil_div(P, pt) * B;
    const int64_t cost = ceil_div64(wgs, n_cu) * (kCfg[i].nrt + 4);
    if (best < 0 || cost < best_cost) best = i, best_cost = cost;
  }
  return best;
}

int cu_count(int* n_cu) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  static int cached[64] = {0};
  if (dev < 0 || dev >= 64) return -1;
  if (cached[dev] == 0) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
    cached[dev] = prop.multiProcessorCount;
  }
  *n_cu = cached[dev];
  return 0;
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_conv1x1_split_config(int N, int P, int B, int n_cu) {
  if (N <= 0 || P <= 0 || B <= 0 || n_cu <= 0) return -1;
  return choose_cfg(N, P, B, n_cu);
}

// The GroupNorm options of wm2f_conv1x1_split_gn_fwd (all zero: wm2f_conv1x1_split_fwd)
struct C1Gn {
  void* stats_out;
  int G_out;
  const void *nstats, *ngamma, *nbeta;
  int nG;
  float neps;
  int nrelu;
};

static int conv1x1_launch(const char* who, const void* x, const void* w_split, const void* bias, const void* residual, void* out,
                          const C1Gn& gn, int B, int K, int N, int Hi, int Wi, int stride, int relu, int config, int pieces,
                          void* stream) {
  WM2F_REQUIRE(pieces >= 1 && pieces <= 3, "%s: pieces = %d (1, 2 and 3 are built)", who, pieces);
  WM2F_REQUIRE(x && w_split && out, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && K > 0 && N > 0 && Hi > 0 && Wi > 0, "%s: non-positive size", who);
  WM2F_REQUIRE(K % kKStep == 0 && N % 64 == 0, "%s: K = %d must be a multiple of %d and N = %d of 64", who, K, kKStep, N);
  WM2F_REQUIRE(stride == 1 || stride == 2, "%s: stride %d (1 and 2 are built)", who, stride);
  const int Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1;
  const int64_t P = (int64_t)Ho * Wo;
  WM2F_REQUIRE((int64_t)K * Hi * Wi * 4 < (1ll << 31) && (int64_t)N * P * 4 < (1ll << 31),
               "%s: one image of x / out must stay below 2 GiB (32-bit buffer offsets)", who);
  WM2F_REQUIRE((int64_t)N * K * 6 < (1ll << 31), "%s: the split weight must stay below 2 GiB", who);
  WM2F_REQUIRE(!residual || (bias && relu), "%s: the residual epilogue is bias + residual + ReLU", who);
  WM2F_REQUIRE(!relu || bias, "%s: the ReLU epilogues carry a bias", who);
  const int opt = gn.stats_out ? kStats : (gn.nstats ? kNorm : kPlain);
  if (opt == kStats) {
    WM2F_REQUIRE(!gn.nstats, "%s: the statistics output and the normalised operand are not built together", who);
    WM2F_REQUIRE(!relu && !residual, "%s: the statistics epilogue is built for raw and + bias", who);
    WM2F_REQUIRE(gn.G_out > 0 && N % gn.G_out == 0 && gn_epilogue_cpg(N / gn.G_out),
                 "%s: N = %d in %d groups: the epilogue reduces groups of 4, 8 or 16 channels", who, N, gn.G_out);
  }
  if (opt == kNorm) {
    WM2F_REQUIRE(gn.ngamma && gn.nbeta, "%s: the normalised operand needs gamma and beta", who);
    WM2F_REQUIRE(bias && !relu && !residual, "%s: the normalised operand is built for the + bias epilogue", who);
    WM2F_REQUIRE(stride == 1, "%s: the normalised operand reads every pixel (stride 1)", who);
    WM2F_REQUIRE(gn.nG > 0 && K % gn.nG == 0, "%s: K = %d is not a multiple of %d groups", who, K, gn.nG);
    WM2F_REQUIRE(K <= 2048, "%s: the scale / shift table holds K <= 2048 channels, K = %d", who, K);
  }
  int n_cu = 0;
  if (cu_count(&n_cu) != 0) {
    set_error("%s: cannot query the device", who);
    return WM2F_ELAUNCH;
  }
  WM2F_REQUIRE(config >= -1 && config < kNumCfg, "%s: configuration %d out of range", who, config);
  const int ci = config >= 0 ? config : choose_cfg(N, (int)P, B, n_cu);
  WM2F_REQUIRE(ci >= 0 && N % (kCfg[ci].wn * kCfg[ci].nrt * 16) == 0, "%s: no configuration %d for N = %d", who, ci, N);
  const int epi = residual ? kBiasResRelu : (relu ? kBiasRelu : (bias ? kBias : kRaw));
  const int nt = kCfg[ci].wn * kCfg[ci].nrt * 16, pt = (kWaves / kCfg[ci].wn) * kCT * 16;
  C1Args a;
  a.x = (const float*)x;
  a.ws = w_split;
  a.bias = (const float*)bias;
  a.residual = (const float*)residual;
  a.out = (float*)out;
  a.K = K;
  a.N = N;
  a.Hi = Hi;
  a.Wi = Wi;
  a.Wo = Wo;
  a.P = (int)P;
  a.stride = stride;
  a.stats = (double*)gn.stats_out;
  a.G = opt == kStats ? gn.G_out : 1;
  a.cpg = opt == kStats ? N / gn.G_out : 4;
  a.nstats = (const double*)gn.nstats;
  a.ngamma = (const float*)gn.ngamma;
  a.nbeta = (const float*)gn.nbeta;
  a.neps = gn.neps;
  a.nG = opt == kNorm ? gn.nG : 1;
  a.nrelu = gn.nrelu;
  const size_t lds = (size_t)2 * (nt / 16) * pieces * kFrag + (opt == kNorm ? (size_t)2 * K * sizeof(float) : 0);
  void (*kfn)(C1Args) = pick_kernel(ci, epi, opt, pieces);
  // per call: the attribute belongs to the current device
  hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    set_error("%s: cannot raise dynamic LDS to %zu: %s", who, lds, hipGetErrorString(e));
    return WM2F_ELAUNCH;
  }
  if (opt == kStats) {
    e = hipMemsetAsync(gn.stats_out, 0, sizeof(double) * 2 * B * gn.G_out, (hipStream_t)stream);
    WM2F_REQUIRE(e == hipSuccess, "%s: memset failed: %s", who, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kfn, dim3(N / nt, ceil_div((int)P, pt), B), dim3(kThreads), lds, (hipStream_t)stream, a);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_conv1x1_split_fwd(const void* x, const void* w_split, const void* bias, const void* residual, void* out,
                                      int B, int K, int N, int Hi, int Wi, int stride, int relu, int config, void* stream) {
  const C1Gn none = {nullptr, 0, nullptr, nullptr, nullptr, 0, 0.f, 0};
  return conv1x1_launch("wm2f_conv1x1_split_fwd", x, w_split, bias, residual, out, none, B, K, N, Hi, Wi, stride, relu, config,
                        3, stream);
}

extern "C" int wm2f_conv1x1_split_fwd_p(const void* x, const void* w_split, const void* bias, const void* residual, void* out,
                                        int B, int K, int N, int Hi, int Wi, int stride, int relu, int config, int pieces,
                                        void* stream) {
  const C1Gn none = {nullptr, 0, nullptr, nullptr, nullptr, 0, 0.f, 0};
  return conv1x1_launch("wm2f_conv1x1_split_fwd_p", x, w_split, bias, residual, out, none, B, K, N, Hi, Wi, stride, relu, config,
                        pieces, stream);
}

extern "C" int wm2f_conv1x1_split_gn_fwd(const void* x, const void* w_split, const void* bias, void* out, void* stats_out,
                                         int G_out, const void* norm_stats, const void* norm_gamma, const void* norm_beta,
                                         int norm_G, float norm_eps, int norm_relu, int B, int K, int N, int Hi, int Wi,
                                         int stride, int config, void* stream) {
  const char* who = "wm2f_conv1x1_split_gn_fwd";
  WM2F_REQUIRE(stats_out || norm_stats, "%s: neither a statistics output nor a normalised operand", who);
  const C1Gn gn = {stats_out, G_out, norm_stats, norm_gamma, norm_beta, norm_G, norm_eps, norm_relu ? 1 : 0};
  return conv1x1_launch(who, x, w_split, bias, nullptr, out, gn, B, K, N, Hi, Wi, stride, 0, config, 3, stream);
}

extern "C" int wm2f_conv1x1_split_gn_fwd_p(const void* x, const void* w_split, const void* bias, void* out, void* stats_out,
                                           int G_out, const void* norm_stats, const void* norm_gamma, const void* norm_beta,
                                           int norm_G, float norm_eps, int norm_relu, int B, int K, int N, int Hi, int Wi,
                                           int stride, int config, int pieces, void* stream) {
  const char* who = "wm2f_conv1x1_split_gn_fwd_p";
  WM2F_REQUIRE(stats_out || norm_stats, "%s: neither a statistics output nor a normalised operand", who);
  const C1Gn gn = {stats_out, G_out, norm_stats, norm_gamma, norm_beta, norm_G, norm_eps, norm_relu ? 1 : 0};
  return conv1x1_launch(who, x, w_split, bias, nullptr, out, gn, B, K, N, Hi, Wi, stride, 0, config, pieces, stream);
}

extern "C" int wm2f_conv1x1_split_dual_fwd_p(const void* x1, const void* ws1, const void* x2, const void* ws2, const void* bias,
                                             void* out, int B, int K1, int K2, int N, int Ho, int Wo, int H2, int W2, int stride2,
                                             int config, int pieces, void* stream) {
  const char* who = "wm2f_conv1x1_split_dual_fwd_p";
  WM2F_REQUIRE(pieces >= 1 && pieces <= 3, "%s: pieces = %d (1, 2 and 3 are built)", who, pieces);
  WM2F_REQUIRE(x1 && ws1 && x2 && ws2 && bias && out, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && K1 > 0 && K2 > 0 && N > 0 && Ho > 0 && Wo > 0 && H2 > 0 && W2 > 0, "%s: non-positive size", who);
  WM2F_REQUIRE(K1 % kKStep == 0 && K2 % kKStep == 0 && N % 64 == 0,
               "%s: K1 = %d and K2 = %d must be multiples of %d and N = %d of 64", who, K1, K2, kKStep, N);
  WM2F_REQUIRE(stride2 == 1 || stride2 == 2, "%s: stride2 %d (1 and 2 are built)", who, stride2);
  WM2F_REQUIRE((H2 - 1) / stride2 + 1 == Ho && (W2 - 1) / stride2 + 1 == Wo,
               "%s: x2 (%d, %d) at stride %d does not sample onto the (%d, %d) output map", who, H2, W2, stride2, Ho, Wo);
  const int64_t P = (int64_t)Ho * Wo;
  WM2F_REQUIRE((int64_t)K1 * P * 4 < (1ll << 31) && (int64_t)K2 * H2 * W2 * 4 < (1ll << 31) && (int64_t)N * P * 4 < (1ll << 31),
               "%s: one image of x1 / x2 / out must stay below 2 GiB (32-bit buffer offsets)", who);
  WM2F_REQUIRE((int64_t)N * K1 * 6 < (1ll << 31) && (int64_t)N * K2 * 6 < (1ll << 31),
               "%s: each split weight must stay below 2 GiB", who);
  int n_cu = 0;
  if (cu_count(&n_cu) != 0) {
    set_error("%s: cannot query the device", who);
    return WM2F_ELAUNCH;
  }
  WM2F_REQUIRE(config >= -1 && config < kNumCfg, "%s: configuration %d out of range", who, config);
  const int ci = config >= 0 ? config : choose_cfg(N, (int)P, B, n_cu);  // the one-source rule: K plays no part in it
  WM2F_REQUIRE(ci >= 0 && N % (kCfg[ci].wn * kCfg[ci].nrt * 16) == 0, "%s: no configuration %d for N = %d", who, ci, N);
  const int nt = kCfg[ci].wn * kCfg[ci].nrt * 16, pt = (kWaves / kCfg[ci].wn) * kCT * 16;
  C1DualArgs a;
  a.x = (const float*)x1;
  a.ws = ws1;
  a.bias = (const float*)bias;
  a.residual = nullptr;
  a.out = (float*)out;
  a.K = K1;
  a.N = N;
  a.Hi = Ho;
  a.Wi = Wo;
  a.Wo = Wo;
  a.P = (int)P;
  a.stride = 1;
  a.stats = nullptr;
  a.G = 1;
  a.cpg = 4;
  a.nstats = nullptr;
  a.ngamma = a.nbeta = nullptr;
  a.neps = 0.f;
  a.nG = 1;
  a.nrelu = 0;
  a.x2 = (const float*)x2;
  a.ws2 = ws2;
  a.K2 = K2;
  a.H2 = H2;
  a.W2 = W2;
  a.stride2 = stride2;
  const size_t lds = (size_t)2 * (nt / 16) * pieces * kFrag;
  void (*kfn)(C1DualArgs) = pick_dual(ci, pieces);
  // per call: the attribute belongs to the current device
  hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    set_error("%s: cannot raise dynamic LDS to %zu: %s", who, lds, hipGetErrorString(e));
    return WM2F_ELAUNCH;
  }
  hipLaunchKernelGGL(kfn, dim3(N / nt, ceil_div((int)P, pt), B), dim3(kThreads), lds, (hipStream_t)stream, a);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
