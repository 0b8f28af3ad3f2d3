// 3x3 convolution, padding 1, in NCHW at fp32 accuracy on the bf16 matrix cores ("split-bf16"):
//     y_b (N, P) = epilogue( W (N, 9 Cin) . im2col(x_b) (9 Cin, P) ),   P = Ho * Wo,  stride s in {1, 2},
//     column k = (3 dy + dx) Cin + c of pixel p = (ho, wo) reads x_b[c, s ho + dy - 1, s wo + dx - 1] (zero outside the map)
// for the ResNet bottlenecks' conv2 (BatchNorm folded into W and the bias by the caller, bias + ReLU in the store) and the
// pixel decoder's FPN layer_1 (raw, with the GroupNorm statistics of the output from the epilogue: DESIGN §33; the
// normalisation and the ReLU happen in mask_projection's operand load).
//
// Arithmetic: that of conv1x1_split.hip -- both operands written as three bf16 pieces (h clamped to the largest finite
// bf16), the six products of a k-step summed from zero on v_mfma_f32_16x16x32_bf16, small terms first, and that sum added
// to the accumulator with one fp32 add.  No split-K: the sequence of MFMAs an output element sees does not depend on the
// tile configuration, the batch or the other pixels, so results are bit-identical run to run, for any sub-batch and under
// every configuration.
//
// Layout of the work:
//   * W is reordered tap-major (N, 3, 3, Cin) and split once per weight version by wm2f_token_linear_split_weight on its
//     (N, 9 Cin) view, so a 32-deep k-step is one tap and 32 consecutive channels: the A panel of a k-step is the 1x1
//     kernel's panel, streamed by LDS-DMA into a two-slot LDS ring;
//   * the B fragment is the 1x1 kernel's NCHW loader with each lane's source pixel shifted by (dy - 1, dx - 1).  A lane
//     keeps, per column tile, the offset of its pixel's window corner and a 9-bit mask of the taps that land inside the
//     map; a tap outside the map (a padded row or column, or a pixel of the ragged tail) reads from the out-of-range
//     offset, so the buffer load returns zero.  A row outside the map cannot be left to the buffer's range check: row
//     Hi of channel c is row 0 of channel c + 1;
//   * the k-steps run channel block outer, tap inner, so the nine shifted windows of one block are read back to back
//     (the same lines, from the vector L1).  Each element is split in registers once per tap (no LDS staging: DESIGN §15
//     counts the vector instructions against the MFMAs);
//   * a workgroup of 8 waves owns an (NT channels) x (PT pixels) tile of one image, WN waves along n and 8 / WN along p;
//     the tile table and the host's rule are those of the 1x1 kernel, ties broken towards WN = 1;
//   * epilogue in the store: lane (j, g) holds channels 4g .. 4g + 3 of pixel j, stored as dwords.
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
enum : int { kRaw = 0, kBias = 1, kBiasRelu = 2 };

// the fp32 values of eight bf16 read from their packed pairs: one shift or mask each (a plain conversion back from bf16
// compiles to a second v_cvt_pk_bf16_f32 per element plus a shift)
__device__ __forceinline__ f32x8 widen(const bf16x8 v) {
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
  const u32x4 w = __builtin_bit_cast(u32x4, v);
  f32x8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r[2 * i] = __builtin_bit_cast(float, w[i] << 16);
    r[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u);
  }
  return r;
}

// the split of conv1x1_split.hip, the same bits: its first P pieces (the pieces past P are left untouched and never read)
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
    const f32x8 r1 = x - widen(h);
    m = __builtin_convertvector(r1, bf16x8);
    if constexpr (P >= 3) {
      const f32x8 r2 = r1 - widen(m);
      l = __builtin_convertvector(r2, bf16x8);
    }
  }
}

struct C3Args {
  const float *x, *bias;
  const void* ws;
  float* out;
  int Cin, N;
  int Hi, Wi, Wo, P, stride;
  // STATS: the group statistics of the stored output, stats[(b G + g) 2 + {0, 1}] += (sum, sum of squares); cpg = N / G
  double* stats;
  int G, cpg;
};

__device__ __forceinline__ void c3_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// NRT row tiles per wave, WN waves along n: a workgroup tile is NT = WN * NRT * 16 channels by PT = (8 / WN) * 32 pixels.
// STATS: the epilogue also reduces the group statistics of what it stores (gn_tile_stats; cpg in {4, 8, 16}).
// P = the pieces of each operand that take part: 3 = all six products, 2 = h and m (m.h, h.m, h.h), 1 = h
// alone (h.h).  The split weight is the three-piece one at every P; the ring holds the first P pieces of each row tile.
template <int NRT, int WN, int EPI, bool STATS = false, int P = 3>
__global__ __launch_bounds__(kThreads) void conv3x3_split_kernel(C3Args a) {
  static_assert(P >= 1 && P <= 3, "one, two or three pieces");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [2][NT / 16][P][64][16 B]
  constexpr int kRowTiles = WN * NRT;
  constexpr int kPanelBytes = kRowTiles * P * kFrag;
  constexpr int kPieces = kRowTiles * P;
  constexpr int kPT = (kWaves / WN) * kCT * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave % WN, wp = wave / WN;
  const int g = lane >> 4, j = lane & 15;
  const int nb = blockIdx.x, b = blockIdx.z;
  const int n_wg = nb * kRowTiles * 16;              // first channel of the workgroup
  const int p_w = blockIdx.y * kPT + wp * kCT * 16;  // first pixel of the wave
  const int n_cb = a.Cin / kKStep;                   // channel blocks per tap
  const int n_ks = 9 * n_cb;
  const int HWi = a.Hi * a.Wi;

  // per-image buffers (each below 2 GiB: checked by the host)
  const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.ws, 0, a.N * 9 * a.Cin * 6, 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)(a.x + (int64_t)b * a.Cin * HWi), 0, a.Cin * HWi * 4, 0x00020000);

  // per column tile: the byte offset of this lane's window corner (s ho - 1, s wo - 1) in channel 8g (negative at the top
  // or left border; only the taps inside the map are ever added to it), and the taps inside the map, bit 3 dy + dx
  int xo[kCT];
  unsigned tap_ok[kCT];
#pragma unroll
  for (int c = 0; c < kCT; ++c) {
    const int p = p_w + c * 16 + j;
    const int ho = p / a.Wo, wo = p - ho * a.Wo;
    const int hi = a.stride * ho - 1, wi = a.stride * wo - 1;
    xo[c] = ((8 * g) * HWi + hi * a.Wi + wi) * 4;
    unsigned m = 0;
    if (p < a.P) {
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
          if ((unsigned)(hi + dy) < (unsigned)a.Hi && (unsigned)(wi + dx) < (unsigned)a.Wi) m |= 1u << (3 * dy + dx);
    }
    tap_ok[c] = m;
  }
  const unsigned ch_bytes = (unsigned)HWi * 4;

  f32x8 xr[kCT];
  // k-step it = 9 cb + tap: channels 32 cb .. 32 cb + 31 of tap (dy, dx); its A panel is k-step tap * n_cb + cb of the split W
  auto issue = [&](int it) {
    const int cb = it / 9, tap = it - 9 * cb;
    const int dy = tap / 3, dx = tap - 3 * dy;
    unsigned char* dst = smem + (it & 1) * kPanelBytes;
    const int src = ((tap * n_cb + cb) * (a.N / 16) + n_wg / 16) * 3 * kFrag;
    for (int f = wave; f < kPieces; f += kWaves) {
      const int fs = P == 3 ? f : (f / P) * 3 + f % P;  // ring piece f = piece f % P of row tile f / P
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (lds_ptr_t)(dst + f * kFrag), 16, lane * 16, src + fs * kFrag, 0, 0);
    }
    const int kb = (cb * kKStep * HWi + dy * a.Wi + dx) * 4;
#pragma unroll
    for (int c = 0; c < kCT; ++c) {
      const unsigned o = (tap_ok[c] >> tap) & 1u ? (unsigned)(xo[c] + kb) : kOob;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        xr[c][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(x_rs, o, i * ch_bytes, 0));
    }
  };

  issue(0);
  c3_barrier();

  f32x4 acc[NRT][kCT];
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
    for (int c = 0; c < kCT; ++c) acc[rt][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int it = 0; it < n_ks; ++it) {
    bf16x8 bh[kCT], bm[kCT], bl[kCT];
#pragma unroll
    for (int c = 0; c < kCT; ++c) split3<P>(xr[c], bh[c], bm[c], bl[c]);
    if (it + 1 < n_ks) issue(it + 1);  // the next step's loads fly under this step's MFMAs

    const unsigned char* panel = smem + (it & 1) * kPanelBytes + wn * NRT * P * kFrag;
    auto read_a = [&](bf16x8 (&dst)[3], int rt) {
#pragma unroll
      for (int p = 0; p < P; ++p) dst[p] = *reinterpret_cast<const bf16x8*>(panel + (rt * P + p) * kFrag + lane * 16);
    };
    // the six products of one (row tile, column tile), the small terms first, summed from zero and added to the
    // accumulator once per k-step (conv1x1_split.hip)
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
    c3_barrier();  // step it + 1's panel and x have landed; every wave is done with slot it & 1
  }

  // ---- epilogue: lane (j, g) holds, per row tile rt and column tile c, channels n0 + rt*16 + 4g .. +3 of pixel p_w + 16c + j
  const int64_t img = (int64_t)b * a.N * a.P;
  const __amdgpu_buffer_rsrc_t o_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.out + img), 0, a.N * a.P * 4, 0x00020000);
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
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[rt][c][e];
        if (EPI != kRaw) v += bv[e];
        if (EPI == kBiasRelu) v = v < 0.f ? 0.f : v;  // a NaN stays a NaN
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

template <int NRT, int WN, int P>
void (*pick_epi(int epi, bool stats))(C3Args) {
  if (stats) return conv3x3_split_kernel<NRT, WN, kRaw, true, P>;  // the statistics are built on the raw epilogue
  switch (epi) {
    case kRaw: return conv3x3_split_kernel<NRT, WN, kRaw, false, P>;
    case kBias: return conv3x3_split_kernel<NRT, WN, kBias, false, P>;
    default: return conv3x3_split_kernel<NRT, WN, kBiasRelu, false, P>;
  }
}

template <int P>
void (*pick_cfg(int ci, int epi, bool stats))(C3Args) {
  switch (ci) {
    case 0: return pick_epi<16, 1, P>(epi, stats);
    case 1: return pick_epi<8, 2, P>(epi, stats);
    case 2: return pick_epi<4, 4, P>(epi, stats);
    case 3: return pick_epi<8, 1, P>(epi, stats);
    default: return pick_epi<4, 1, P>(epi, stats);
  }
}

void (*pick_kernel(int ci, int epi, bool stats, int pieces))(C3Args) {
  return pieces == 3 ? pick_cfg<3>(ci, epi, stats) : (pieces == 2 ? pick_cfg<2>(ci, epi, stats) : pick_cfg<1>(ci, epi, stats));
}

// The configuration of a shape: fewest rounds of workgroups over the CUs (one 8-wave workgroup per CU) times the wave's
// work per k-step (NRT row tiles, plus a fixed share for the barrier, the x loads and the split), the 1x1 kernel's rule;
// ties go to the fewest waves along n, since every wave along n loads and splits the same nine shifted windows again
// ((8, 1) over (8, 2) measured 185 against 199 us at 256 channels on 64^2, (4, 1) over (4, 4) 238 against 272 us at 512
// on 32^2, B = 8), then to the wider NT.
int choose_cfg(int N, int P, int B, int n_cu) {
  int best = -1;
  int64_t best_cost = 0;
  for (int i = 0; i < kNumCfg; ++i) {
    const int nt = kCfg[i].wn * kCfg[i].nrt * 16, pt = (kWaves / kCfg[i].wn) * kCT * 16;
    if (N % nt) continue;
    const int64_t wgs = (int64_t)(N / nt) * ceil_div(P, pt) * B;
    const int64_t cost = ceil_div64(wgs, n_cu) * (kCfg[i].nrt + 4);
    if (best < 0 || cost < best_cost || (cost == best_cost && kCfg[i].wn < kCfg[best].wn)) best = i, best_cost = cost;
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

extern "C" int wm2f_conv3x3_split_config(int N, int P, int B, int n_cu) {
  if (N <= 0 || P <= 0 || B <= 0 || n_cu <= 0) return -1;
  return choose_cfg(N, P, B, n_cu);
}

// stats_out != NULL: the group statistics of the (raw) output in G_out groups (wm2f_conv3x3_split_stats_fwd)
static int conv3x3_launch(const char* who, const void* x, const void* w_split, const void* bias, void* out, void* stats_out,
                          int G_out, int B, int Cin, int N, int Hi, int Wi, int stride, int relu, int config, int pieces,
                          void* stream) {
  WM2F_REQUIRE(pieces >= 1 && pieces <= 3, "%s: pieces = %d (1, 2 and 3 are built)", who, pieces);
  WM2F_REQUIRE(x && w_split && out, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && Cin > 0 && N > 0 && Hi > 0 && Wi > 0, "%s: non-positive size", who);
  WM2F_REQUIRE(Cin % kKStep == 0 && N % 64 == 0, "%s: Cin = %d must be a multiple of %d and N = %d of 64", who, Cin, kKStep, N);
  WM2F_REQUIRE(stride == 1 || stride == 2, "%s: stride %d (1 and 2 are built)", who, stride);
  const int Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1;
  const int64_t P = (int64_t)Ho * Wo;
  WM2F_REQUIRE((int64_t)Cin * Hi * Wi * 4 < (1ll << 31) && (int64_t)N * P * 4 < (1ll << 31),
               "%s: one image of x / out must stay below 2 GiB (32-bit buffer offsets)", who);
  WM2F_REQUIRE((int64_t)N * 9 * Cin * 6 < (1ll << 31), "%s: the split weight must stay below 2 GiB", who);
  WM2F_REQUIRE(!relu || bias, "%s: the ReLU epilogue carries a bias", who);
  if (stats_out) {
    WM2F_REQUIRE(!bias && !relu, "%s: the statistics epilogue is built for the raw output", who);
    WM2F_REQUIRE(G_out > 0 && N % G_out == 0 && gn_epilogue_cpg(N / G_out),
                 "%s: N = %d in %d groups: the epilogue reduces groups of 4, 8 or 16 channels", who, N, G_out);
  }
  int n_cu = 0;
  if (cu_count(&n_cu) != 0) {
    set_error("%s: cannot query the device", who);
    return WM2F_ELAUNCH;
  }
  WM2F_REQUIRE(config >= -1 && config < kNumCfg, "%s: configuration %d out of range", who, config);
  const int ci = config >= 0 ? config : choose_cfg(N, (int)P, B, n_cu);
  WM2F_REQUIRE(ci >= 0 && N % (kCfg[ci].wn * kCfg[ci].nrt * 16) == 0, "%s: no configuration %d for N = %d", who, ci, N);
  const int epi = relu ? kBiasRelu : (bias ? kBias : kRaw);
  const int nt = kCfg[ci].wn * kCfg[ci].nrt * 16, pt = (kWaves / kCfg[ci].wn) * kCT * 16;
  C3Args a;
  a.x = (const float*)x;
  a.ws = w_split;
  a.bias = (const float*)bias;
  a.out = (float*)out;
  a.Cin = Cin;
  a.N = N;
  a.Hi = Hi;
  a.Wi = Wi;
  a.Wo = Wo;
  a.P = (int)P;
  a.stride = stride;
  a.stats = (double*)stats_out;
  a.G = stats_out ? G_out : 1;
  a.cpg = stats_out ? N / G_out : 4;
  const size_t lds = (size_t)2 * (nt / 16) * pieces * kFrag;
  void (*kfn)(C3Args) = pick_kernel(ci, epi, stats_out != nullptr, pieces);
  // per call: the attribute belongs to the current device
  hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    set_error("%s: cannot raise dynamic LDS to %zu: %s", who, lds, hipGetErrorString(e));
    return WM2F_ELAUNCH;
  }
  if (stats_out) {
    e = hipMemsetAsync(stats_out, 0, sizeof(double) * 2 * B * G_out, (hipStream_t)stream);
    WM2F_REQUIRE(e == hipSuccess, "%s: memset failed: %s", who, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kfn, dim3(N / nt, ceil_div((int)P, pt), B), dim3(kThreads), lds, (hipStream_t)stream, a);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_conv3x3_split_fwd(const void* x, const void* w_split, const void* bias, void* out, int B, int Cin, int N,
                                      int Hi, int Wi, int stride, int relu, int config, void* stream) {
  return conv3x3_launch("wm2f_conv3x3_split_fwd", x, w_split, bias, out, nullptr, 0, B, Cin, N, Hi, Wi, stride, relu, config,
                        3, stream);
}

extern "C" int wm2f_conv3x3_split_fwd_p(const void* x, const void* w_split, const void* bias, void* out, int B, int Cin, int N,
                                        int Hi, int Wi, int stride, int relu, int config, int pieces, void* stream) {
  return conv3x3_launch("wm2f_conv3x3_split_fwd_p", x, w_split, bias, out, nullptr, 0, B, Cin, N, Hi, Wi, stride, relu, config,
                        pieces, stream);
}

extern "C" int wm2f_conv3x3_split_stats_fwd(const void* x, const void* w_split, void* out, void* stats_out, int G_out, int B,
                                            int Cin, int N, int Hi, int Wi, int stride, int config, void* stream) {
  const char* who = "wm2f_conv3x3_split_stats_fwd";
  WM2F_REQUIRE(stats_out, "%s: null pointer", who);
  return conv3x3_launch(who, x, w_split, nullptr, out, stats_out, G_out, B, Cin, N, Hi, Wi, stride, 0, config, 3, stream);
}

extern "C" int wm2f_conv3x3_split_stats_fwd_p(const void* x, const void* w_split, void* out, void* stats_out, int G_out, int B,
                                              int Cin, int N, int Hi, int Wi, int stride, int config, int pieces, void* stream) {
  const char* who = "wm2f_conv3x3_split_stats_fwd_p";
  WM2F_REQUIRE(stats_out, "%s: null pointer", who);
  return conv3x3_launch(who, x, w_split, nullptr, out, stats_out, G_out, B, Cin, N, Hi, Wi, stride, 0, config, pieces, stream);
}
