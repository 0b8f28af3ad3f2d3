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
//     (the same lines, from the vector L1).  Each element is split in registers once per tap; conv3x3_staged_kernel, the
//     second kernel of this file, splits it once per channel block into LDS instead (stride 1, WN = 1: DESIGN §15);
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
  int tiles_w;  // the staged route: pixel tiles across the map
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
// ABL != 0: timing ablations of the profiling build, whose OUTPUTS ARE NOT VALID (include/wm2f_prof.h, WM2F_C3_ABL): they
// price what the nine taps of a channel block repeat.  kAblSplit splits x at tap 0 of each channel block only and feeds
// those pieces to taps 1 .. 8 (whose x loads are still issued and waited for); kAblLoads also drops the x loads of taps
// 1 .. 8.  The production library instantiates ABL = 0 alone.
enum : int { kAblSplit = 1, kAblLoads = 2 };
template <int NRT, int WN, int EPI, bool STATS = false, int P = 3, int ABL = 0>
__global__ __launch_bounds__(kThreads) void conv3x3_split_kernel(C3Args a) {
  static_assert(P >= 1 && P <= 3, "one, two or three pieces");
  static_assert(ABL == 0 || P == 3, "the ablations are built for three pieces");
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
    if (ABL == kAblLoads && tap != 0) return;
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

  bf16x8 kh[kCT], km[kCT], kl[kCT];  // ABL: the pieces of the block's tap 0
  for (int it = 0; it < n_ks; ++it) {
    bf16x8 bh[kCT], bm[kCT], bl[kCT];
    if (ABL == 0 || it % 9 == 0) {
#pragma unroll
      for (int c = 0; c < kCT; ++c) split3<P>(xr[c], bh[c], bm[c], bl[c]);
      if constexpr (ABL != 0) {
#pragma unroll
        for (int c = 0; c < kCT; ++c) kh[c] = bh[c], km[c] = bm[c], kl[c] = bl[c];
      }
    } else {
#pragma unroll
      for (int c = 0; c < kCT; ++c) {
        bh[c] = kh[c], bm[c] = km[c], bl[c] = kl[c];
        if constexpr (ABL == kAblSplit) asm volatile("" ::"v"(xr[c]));  // the loads of this tap stay
      }
    }
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

// ---- the staged route: stride 1, WN = 1.  The direct kernel above loads and splits every x element once per
// tap, nine times per channel block; here a workgroup's 256 pixels are a kTH x kTW tile of the map, and per channel block
// the tile plus a one-pixel halo is split ONCE and kept in LDS, [piece][g][halo pixel][16 B], behind the A ring.  The B
// fragment of a tap is then a 16-byte LDS read at a constant pixel offset, (dy kHW + dx) * 16 B.
//   * lane map: wave w owns row w of the tile as two column tiles of 16 pixels; lane (j, g) holds pixel j and channels
//     8g .. 8g + 7, as above, so the MFMAs, their order and the epilogue are the direct kernel's and so are the bits;
//   * staging item s = g kHalo + (halo pixel) of kStageItems, items s = r 512 + tid in kStageRounds rounds: consecutive
//     lanes load consecutive pixels of a halo row and write consecutive 16-byte slots (piece stride 4 kHalo 16 B).  A halo
//     pixel outside the map is NOT fetched (row Hi of channel c is row 0 of channel c + 1; its offset is the out-of-range
//     one and the load returns zero), and is stored as zeros: the padding of the convolution.  Pixels of a ragged tile
//     are halo pixels outside the map to their neighbours, and their own outputs are not stored;
//   * pipeline: one staged tile.  The loads of block cb + 1 are issued into registers at taps 0, 3 and 6 of block cb (one
//     round each) and waited for by the vmcnt(0) of the k-step barriers; after the barrier of tap 8 every wave is done
//     with the tile, the workgroup splits and writes the next one, and a second barrier publishes it;
//   * every barrier is reached by all eight waves: no wave leaves before the epilogue, whatever its pixels, and the only
//     guards are around the LDS stores of the items past kStageItems and around the global stores.
constexpr int kTH = 8, kTW = 32;
constexpr int kHW = kTW + 2, kHalo = (kTH + 2) * kHW;  // 34 columns, 340 halo pixels
constexpr int kStageItems = 4 * kHalo;                 // (g, halo pixel)
constexpr int kStageRounds = (kStageItems + kThreads - 1) / kThreads;
constexpr int kStagePiece = kStageItems * 16;          // bytes of one piece of the staged tile
static_assert(kTH == kWaves && kTW == kCT * 16, "a wave owns one row of the tile");

template <int NRT, int EPI, bool STATS = false, int P = 3>
__global__ __launch_bounds__(kThreads) void conv3x3_staged_kernel(C3Args a) {
  static_assert(P >= 1 && P <= 3, "one, two or three pieces");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [2][NRT][P][64][16 B], [P][4][kHalo][16 B]
  constexpr int kPanelBytes = NRT * P * kFrag;
  constexpr int kPieces = NRT * P;
  unsigned char* const tile = smem + 2 * kPanelBytes;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, j = lane & 15;
  const int nb = blockIdx.x, b = blockIdx.z;
  const int n_wg = nb * NRT * 16;
  const int ty = blockIdx.y / a.tiles_w, tx = blockIdx.y - ty * a.tiles_w;
  const int h0 = ty * kTH, w0 = tx * kTW;  // the tile's first pixel
  const int n_cb = a.Cin / kKStep;
  const int HWi = a.Hi * a.Wi;

  const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.ws, 0, a.N * 9 * a.Cin * 6, 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)(a.x + (int64_t)b * a.Cin * HWi), 0, a.Cin * HWi * 4, 0x00020000);

  // this lane's staging items: the byte offset of (channel 8g, halo pixel) in block 0, or the out-of-range offset
  unsigned so[kStageRounds];
#pragma unroll
  for (int r = 0; r < kStageRounds; ++r) {
    const int s = r * kThreads + tid;
    const int sg = s / kHalo, hp = s - sg * kHalo;
    const int hy = hp / kHW, hx = hp - hy * kHW;
    const int hi = h0 - 1 + hy, wi = w0 - 1 + hx;
    const bool ok = s < kStageItems && (unsigned)hi < (unsigned)a.Hi && (unsigned)wi < (unsigned)a.Wi;
    so[r] = ok ? (unsigned)(((8 * sg) * HWi + hi * a.Wi + wi) * 4) : kOob;
  }
  const unsigned ch_bytes = (unsigned)HWi * 4;

  f32x8 xs[kStageRounds];
  auto stage_load = [&](int r, int cb) {  // r is a constant after unrolling
    const unsigned o = so[r] != kOob ? so[r] + (unsigned)(cb * kKStep) * ch_bytes : kOob;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      xs[r][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(x_rs, o, i * ch_bytes, 0));
  };
  auto stage_write = [&]() {
#pragma unroll
    for (int r = 0; r < kStageRounds; ++r) {
      bf16x8 pc[3];
      split3<P>(xs[r], pc[0], pc[1], pc[2]);
      const int s = r * kThreads + tid;
      if (s < kStageItems) {
#pragma unroll
        for (int p = 0; p < P; ++p) *reinterpret_cast<bf16x8*>(tile + p * kStagePiece + s * 16) = pc[p];
      }
    }
  };
  // k-step it = 9 cb + tap: the A panel is k-step tap * n_cb + cb of the split W (the direct kernel's)
  auto issue_a = [&](int it, int cb, int tap) {
    unsigned char* dst = smem + (it & 1) * kPanelBytes;
    const int src = ((tap * n_cb + cb) * (a.N / 16) + n_wg / 16) * 3 * kFrag;
    for (int f = wave; f < kPieces; f += kWaves) {
      const int fs = P == 3 ? f : (f / P) * 3 + f % P;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (lds_ptr_t)(dst + f * kFrag), 16, lane * 16, src + fs * kFrag, 0, 0);
    }
  };

  issue_a(0, 0, 0);
#pragma unroll
  for (int r = 0; r < kStageRounds; ++r) stage_load(r, 0);
  c3_barrier();
  stage_write();
  __syncthreads();

  f32x4 acc[NRT][kCT];
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
    for (int c = 0; c < kCT; ++c) acc[rt][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // this lane's B fragment of tap (0, 0): halo pixel (wave, 16 c + j) of g, c = 0
  const unsigned char* const bsrc = tile + (g * kHalo + wave * kHW + j) * 16;
  int it = 0;
#pragma unroll 1
  for (int cb = 0; cb < n_cb; ++cb) {
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap, ++it) {
      const int dy = tap / 3, dx = tap - 3 * dy;
      bf16x8 bf[kCT][3];
#pragma unroll
      for (int c = 0; c < kCT; ++c)
#pragma unroll
        for (int p = 0; p < P; ++p)
          bf[c][p] = *reinterpret_cast<const bf16x8*>(bsrc + (dy * kHW + dx) * 16 + c * 256 + p * kStagePiece);
      const bool last = tap == 8 && cb + 1 == n_cb;
      if (!last) issue_a(it + 1, tap == 8 ? cb + 1 : cb, tap == 8 ? 0 : tap + 1);
      if (cb + 1 < n_cb) {  // the next block's x, a round at taps 0, 3 and 6
#pragma unroll
        for (int r = 0; r < kStageRounds; ++r)
          if (tap == 3 * r) stage_load(r, cb + 1);
      }

      const unsigned char* panel = smem + (it & 1) * kPanelBytes;
      auto read_a = [&](bf16x8 (&dst)[3], int rt) {
#pragma unroll
        for (int p = 0; p < P; ++p) dst[p] = *reinterpret_cast<const bf16x8*>(panel + (rt * P + p) * kFrag + lane * 16);
      };
      // the six products of the direct kernel, in its order (bf[..][0 / 1 / 2] = h / m / l)
      auto six = [&](f32x4 acc_in, const bf16x8 (&av)[3], int cc) {
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
        if constexpr (P == 3) {
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], bf[cc][1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[2], bf[cc][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bf[cc][2], c, 0, 0, 0);
        }
        if constexpr (P >= 2) {
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], bf[cc][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bf[cc][1], c, 0, 0, 0);
        }
        return acc_in + __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bf[cc][0], c, 0, 0, 0);
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
      c3_barrier();  // step it + 1's panel and the x loads issued so far have landed; every wave is done with slot it & 1
    }
    if (cb + 1 < n_cb) {  // after tap 8's barrier every wave is done with the staged tile
      stage_write();
      __syncthreads();
    }
  }

  // ---- epilogue, the direct kernel's: lane (j, g) holds channels n0 + rt*16 + 4g .. +3 of pixel (h0 + wave, w0 + 16c + j)
  const int64_t img = (int64_t)b * a.N * a.P;
  const __amdgpu_buffer_rsrc_t o_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.out + img), 0, a.N * a.P * 4, 0x00020000);
  const int n0 = n_wg + 4 * g;
  const int ho = h0 + wave;
  float gs[NRT], gss[NRT];
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
      const int wo = w0 + c * 16 + j;
      const bool live = ho < a.Hi && wo < a.Wi;
      const unsigned ro = live ? (unsigned)(((n0 + rt * 16) * a.P + ho * a.Wi + wo) * 4) : kOob;
      const unsigned rs = (unsigned)a.P * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[rt][c][e];
        if (EPI != kRaw) v += bv[e];
        if (EPI == kBiasRelu) v = v < 0.f ? 0.f : v;  // a NaN stays a NaN
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), o_rs, ro, e * rs, 0);
        if (STATS && live) {
          gs[rt] += v;
          gss[rt] = fmaf(v, v, gss[rt]);
        }
      }
    }
  }
  if (STATS) gn_tile_stats<NRT, 1, kWaves>(gs, gss, smem, a.stats, b * a.G, n_wg, a.cpg, tid);
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

template <int NRT, int P>
void (*pick_staged_epi(int epi, bool stats))(C3Args) {
  if (stats) return conv3x3_staged_kernel<NRT, kRaw, true, P>;
  switch (epi) {
    case kRaw: return conv3x3_staged_kernel<NRT, kRaw, false, P>;
    case kBias: return conv3x3_staged_kernel<NRT, kBias, false, P>;
    default: return conv3x3_staged_kernel<NRT, kBiasRelu, false, P>;
  }
}

template <int P>
void (*pick_staged_cfg(int ci, int epi, bool stats))(C3Args) {
  switch (kCfg[ci].nrt) {  // a WN = 1 entry
    case 16: return pick_staged_epi<16, P>(epi, stats);
    case 8: return pick_staged_epi<8, P>(epi, stats);
    default: return pick_staged_epi<4, P>(epi, stats);
  }
}

void (*pick_staged(int ci, int epi, bool stats, int pieces))(C3Args) {
  return pieces == 3 ? pick_staged_cfg<3>(ci, epi, stats)
                     : (pieces == 2 ? pick_staged_cfg<2>(ci, epi, stats) : pick_staged_cfg<1>(ci, epi, stats));
}

#ifdef WM2F_PROFILING
// the timing ablations (OUTPUTS NOT VALID): three pieces, no statistics
template <int NRT, int WN>
void (*pick_abl_epi(int epi, int abl))(C3Args) {
  if (abl == kAblSplit) {
    switch (epi) {
      case kRaw: return conv3x3_split_kernel<NRT, WN, kRaw, false, 3, kAblSplit>;
      case kBias: return conv3x3_split_kernel<NRT, WN, kBias, false, 3, kAblSplit>;
      default: return conv3x3_split_kernel<NRT, WN, kBiasRelu, false, 3, kAblSplit>;
    }
  }
  switch (epi) {
    case kRaw: return conv3x3_split_kernel<NRT, WN, kRaw, false, 3, kAblLoads>;
    case kBias: return conv3x3_split_kernel<NRT, WN, kBias, false, 3, kAblLoads>;
    default: return conv3x3_split_kernel<NRT, WN, kBiasRelu, false, 3, kAblLoads>;
  }
}

void (*pick_abl(int ci, int epi, int abl))(C3Args) {
  switch (ci) {
    case 0: return pick_abl_epi<16, 1>(epi, abl);
    case 1: return pick_abl_epi<8, 2>(epi, abl);
    case 2: return pick_abl_epi<4, 4>(epi, abl);
    case 3: return pick_abl_epi<8, 1>(epi, abl);
    default: return pick_abl_epi<4, 1>(epi, abl);
  }
}
#endif

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

// ---- the route of a launch: 0 the direct kernel, 1 the staged kernel
constexpr int kLdsLimit = 163840;  // LDS of one gfx950 workgroup; a launch is also checked against the device's own limit

int staged_lds(int nrt, int pieces) { return pieces * (2 * nrt * kFrag + kStagePiece); }

int64_t staged_tiles(int Hi, int Wi) { return (int64_t)ceil_div(Hi, kTH) * ceil_div(Wi, kTW); }

// the staged kernel is built for entry ci at this shape
bool staged_applies(int ci, int Hi, int Wi, int stride, int pieces, int lds_limit) {
  return stride == 1 && kCfg[ci].wn == 1 && staged_lds(kCfg[ci].nrt, pieces) <= lds_limit && staged_tiles(Hi, Wi) <= 65535;
}

// The auto rule (profiles/r15_conv3x3_staged_sites.jsonl): staged where it applies and
//   * the map is whole tiles, as at every measured site: the staged kernel then has exactly the direct kernel's workgroups.
//     A ragged map has more tiles than 256-pixel runs, each with a halo, and was not measured: it stays direct;
//   * the entry is not NRT 4 with more than one round of workgroups: two direct NRT 4 workgroups share a CU (117 VGPRs,
//     24 KiB of LDS) and one's prologue and epilogue run under the other's k-loop; the staged tile (88 KiB with the ring)
//     leaves room for one.  This rests on two sites, 64 -> 64 on 256^2, B = 8 (eight rounds: 222 us direct, 248 us staged)
//     and 512 -> 512 on 32^2 (one round: 224 against 176 us); elsewhere it is an extrapolation, and it misses the gain a
//     forced (4, 1) entry measured at the 256-channel sites, which the tile rule never picks there.
bool staged_pays(int ci, int N, int Hi, int Wi, int B, int n_cu) {
  if (Hi % kTH || Wi % kTW) return false;
  const int64_t wgs = (int64_t)(N / (kCfg[ci].nrt * 16)) * B * staged_tiles(Hi, Wi);
  return !(kCfg[ci].nrt == 4 && wgs > n_cu);
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

// the LDS one workgroup may ask for on the current device
int lds_max(int* bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  static int cached[64] = {0};
  if (dev < 0 || dev >= 64) return -1;
  if (cached[dev] == 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0) return -1;
    cached[dev] = v;
  }
  *bytes = cached[dev];
  return 0;
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_conv3x3_split_config(int N, int P, int B, int n_cu) {
  if (N <= 0 || P <= 0 || B <= 0 || n_cu <= 0) return -1;
  return choose_cfg(N, P, B, n_cu);
}

// Pure host function: the route (0 direct, 1 staged) and, in *entry, the tile-table entry the auto rule takes for a shape
// on a device of n_cu CUs; -1 for arguments no launch accepts.
extern "C" int wm2f_conv3x3_split_route(int N, int Hi, int Wi, int stride, int B, int n_cu, int pieces, int* entry) {
  if (N <= 0 || N % 64 || Hi <= 0 || Wi <= 0 || (stride != 1 && stride != 2) || B <= 0 || n_cu <= 0 || pieces < 1 || pieces > 3)
    return -1;
  const int64_t P = (int64_t)((Hi - 1) / stride + 1) * ((Wi - 1) / stride + 1);
  if (P >= (1ll << 31)) return -1;
  const int ci = choose_cfg(N, (int)P, B, n_cu);
  if (ci < 0) return -1;
  if (entry) *entry = ci;
  return staged_applies(ci, Hi, Wi, stride, pieces, kLdsLimit) && staged_pays(ci, N, Hi, Wi, B, n_cu) ? 1 : 0;
}

// stats_out != NULL: the group statistics of the (raw) output in G_out groups (wm2f_conv3x3_split_stats_fwd)
// route: -1 the auto rule, 0 the direct kernel, 1 the staged kernel (refused where it does not apply)
static int conv3x3_launch(const char* who, const void* x, const void* w_split, const void* bias, void* out, void* stats_out,
                          int G_out, int B, int Cin, int N, int Hi, int Wi, int stride, int relu, int config, int pieces,
                          int route, void* stream) {
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
  WM2F_REQUIRE(route >= -1 && route <= 1, "%s: route %d (-1 auto, 0 direct, 1 staged)", who, route);
  int lds_limit = kLdsLimit;
  // the device's own limit is asked for only where the staged kernel is a candidate
  if (route != 0 && staged_applies(ci, Hi, Wi, stride, pieces, kLdsLimit) && lds_max(&lds_limit) != 0) {
    set_error("%s: cannot query the device", who);
    return WM2F_ELAUNCH;
  }
  const bool applies = staged_applies(ci, Hi, Wi, stride, pieces, lds_limit < kLdsLimit ? lds_limit : kLdsLimit);
  WM2F_REQUIRE(route != 1 || applies,
               "%s: the staged route is built for stride 1 on a WN = 1 entry within %d B of LDS (stride %d, entry %d, %d B)", who,
               lds_limit, stride, ci, staged_lds(kCfg[ci].nrt, pieces));
  const bool staged = route == 1 || (route < 0 && applies && staged_pays(ci, N, Hi, Wi, B, n_cu));
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
  a.tiles_w = ceil_div(Wi, kTW);
  const size_t lds = staged ? (size_t)staged_lds(kCfg[ci].nrt, pieces) : (size_t)2 * (nt / 16) * pieces * kFrag;
  void (*kfn)(C3Args) = staged ? pick_staged(ci, epi, stats_out != nullptr, pieces) : pick_kernel(ci, epi, stats_out != nullptr, pieces);
#ifdef WM2F_PROFILING
  if (!staged) {  // WM2F_C3_ABL = 1 / 2: split at tap 0 of a channel block only / and no x loads at taps 1 .. 8 (OUTPUTS NOT VALID)
    const char* ea = getenv("WM2F_C3_ABL");
    const int abl = ea ? atoi(ea) : 0;
    WM2F_REQUIRE(abl == 0 || abl == kAblSplit || abl == kAblLoads, "%s: WM2F_C3_ABL = %d is not built (1 and 2 are)", who, abl);
    WM2F_REQUIRE(abl == 0 || (pieces == 3 && !stats_out), "%s: WM2F_C3_ABL is built for three pieces without statistics", who);
    if (abl) kfn = pick_abl(ci, epi, abl);
  }
#endif
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
  const int grid_y = staged ? (int)staged_tiles(Hi, Wi) : ceil_div((int)P, pt);
  hipLaunchKernelGGL(kfn, dim3(N / nt, grid_y, B), dim3(kThreads), lds, (hipStream_t)stream, a);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_conv3x3_split_fwd(const void* x, const void* w_split, const void* bias, void* out, int B, int Cin, int N,
                                      int Hi, int Wi, int stride, int relu, int config, void* stream) {
  return conv3x3_launch("wm2f_conv3x3_split_fwd", x, w_split, bias, out, nullptr, 0, B, Cin, N, Hi, Wi, stride, relu, config,
                        3, -1, stream);
}

extern "C" int wm2f_conv3x3_split_fwd_p(const void* x, const void* w_split, const void* bias, void* out, int B, int Cin, int N,
                                        int Hi, int Wi, int stride, int relu, int config, int pieces, void* stream) {
  return conv3x3_launch("wm2f_conv3x3_split_fwd_p", x, w_split, bias, out, nullptr, 0, B, Cin, N, Hi, Wi, stride, relu, config,
                        pieces, -1, stream);
}

extern "C" int wm2f_conv3x3_split_stats_fwd(const void* x, const void* w_split, void* out, void* stats_out, int G_out, int B,
                                            int Cin, int N, int Hi, int Wi, int stride, int config, void* stream) {
  const char* who = "wm2f_conv3x3_split_stats_fwd";
  WM2F_REQUIRE(stats_out, "%s: null pointer", who);
  return conv3x3_launch(who, x, w_split, nullptr, out, stats_out, G_out, B, Cin, N, Hi, Wi, stride, 0, config, 3, -1, stream);
}

extern "C" int wm2f_conv3x3_split_stats_fwd_p(const void* x, const void* w_split, void* out, void* stats_out, int G_out, int B,
                                              int Cin, int N, int Hi, int Wi, int stride, int config, int pieces, void* stream) {
  const char* who = "wm2f_conv3x3_split_stats_fwd_p";
  WM2F_REQUIRE(stats_out, "%s: null pointer", who);
  return conv3x3_launch(who, x, w_split, nullptr, out, stats_out, G_out, B, Cin, N, Hi, Wi, stride, 0, config, pieces, -1, stream);
}

// the same with the route of the launch: -1 the auto rule (the entry points above), 0 the direct kernel, 1 the staged kernel
extern "C" int wm2f_conv3x3_split_fwd_r(const void* x, const void* w_split, const void* bias, void* out, int B, int Cin, int N,
                                        int Hi, int Wi, int stride, int relu, int config, int pieces, int route, void* stream) {
  return conv3x3_launch("wm2f_conv3x3_split_fwd_r", x, w_split, bias, out, nullptr, 0, B, Cin, N, Hi, Wi, stride, relu, config,
                        pieces, route, stream);
}

extern "C" int wm2f_conv3x3_split_stats_fwd_r(const void* x, const void* w_split, void* out, void* stats_out, int G_out, int B,
                                              int Cin, int N, int Hi, int Wi, int stride, int config, int pieces, int route,
                                              void* stream) {
  const char* who = "wm2f_conv3x3_split_stats_fwd_r";
  WM2F_REQUIRE(stats_out, "%s: null pointer", who);
  return conv3x3_launch(who, x, w_split, nullptr, out, stats_out, G_out, B, Cin, N, Hi, Wi, stride, 0, config, pieces, route, stream);
}
