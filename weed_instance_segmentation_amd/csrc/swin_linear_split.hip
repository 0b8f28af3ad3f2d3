// The Swin backbone's Linears at fp32 accuracy on the bf16 matrix cores ("split-bf16"):
//     out (M, N) = epilogue( x (M, K) . W (N, K)^T + bias )
// for every width of a Swin model (96, 128, 192 times a power of two, N and K up to 6144) and the three epilogues of a
// Swin block: bias, bias + exact GELU, bias + residual; the bias epilogue can write the merged q | k | v projection as
// three tensors.
//
// The arithmetic is token_gemm_split.hip's: x is split into P bf16 pieces in registers, W comes split
// by wm2f_token_linear_split_weight, a 32-deep k-step is P (P + 1) / 2 v_mfma_f32_16x16x32_bf16 in the order m.m, l.h,
// h.l, m.h, h.m, h.h (W piece first), and the products are CHAINED into the accumulator: every MFMA takes the running
// sum as its C operand, k-step after k-step from k = 0, starting from +0.  The bias is added to the finished sum.
//
// Layout of the work.  The token kernel gives a workgroup all N features of its tokens; here N reaches 6144, so the
// tiling is 2-D: one workgroup per (token tile x feature tile), not persistent.
//   * a feature tile is NRT row tiles of 16 features; in wm2f_token_linear_split_weight's order
//     [k-step][row tile][piece][lane][8 bf16] the (feature tile, k-step) panel is NRT * 3 KiB of contiguous bytes.  The
//     last feature tile may be partial in whole row tiles: only its live row tiles are loaded and stored;
//   * every wave issues its share of the NEXT k-step's panel by LDS-DMA (1 KiB pieces, the first P pieces of each row
//     tile) into the other half of a two-panel ring, together with its own x loads of that step, then computes the
//     current one: one `s_waitcnt vmcnt(0)` + barrier per k-step;
//   * x is the B operand, loaded as fp32 (lane (j, g): token j, channels 8g .. 8g + 7 of the k-step) and split in
//     registers.  A wave owns CT column tiles of 16 tokens against the whole feature tile: each A fragment read from LDS
//     feeds CT chains.  The waves of a workgroup take consecutive token ranges;
//   * the tile table (kCfg) has a 256-token and a 64-token workgroup, each 128 and 96 features wide: 128 divides Swin-B's
//     widths, 96 those of Swin-T and Swin-L, and the 64-token tiles give stages 3 and 4 (4096 B and 1024 B tokens) enough
//     workgroups to fill the CUs without split-K (32-token tiles were measured and were not faster);
//   * workgroup ids are dealt to the XCDs round robin; xcd_contiguous_id turns them into ranges that are contiguous per
//     XCD, and inside a range the feature tile runs fastest: the workgroups that share an XCD's L2 read the same x rows.
// Every output has one MFMA sequence, fixed by (K, P) alone: the same bits under every tile shape, M and row position.
#include "common.h"

namespace wm2f {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x8 = __attribute__((ext_vector_type(8))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int kKStep = 32;    // K of one v_mfma_f32_16x16x32_bf16
constexpr int kFrag = 1024;   // bytes of one A fragment piece (64 lanes x 8 bf16)
constexpr unsigned kOob = 0x80000000u;
constexpr float kBf16Max = 3.38953139e38f;  // largest finite bf16, 0x7F7F

// The first P pieces of the three-piece split, as token_gemm_split.hip states it: h from x clamped to the largest finite
// bf16, the residual pieces from the unclamped x, so that an inf or a NaN stays one
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

struct SlArgs {
  const float *x, *bias, *residual;
  const void* ws;
  float* out[3];
  int64_t M;
  int K, N;
  int epilogue;  // 0 bias, 1 bias + GELU, 2 bias + residual
  int n3;        // features per output buffer: N, or N / 3 for the three-way output
  int n_ft;      // feature tiles
  int n_wg;      // token tiles x feature tiles
  int per_xcd;   // workgroup ids per XCD of the launch grid
};

struct SlCfg {
  int nrt, waves, ct;
};
// The tile table: a workgroup is (waves * ct * 16) tokens x (nrt * 16) features.
constexpr SlCfg kCfg[] = {{8, 8, 2}, {6, 8, 2}, {8, 4, 1}, {6, 4, 1}};
constexpr int kNumCfg = sizeof(kCfg) / sizeof(kCfg[0]);

__device__ __forceinline__ void sl_barrier() {  // this wave's vector memory has landed, then the workgroup's
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), the builtin: token_gemm_split.hip, sg_wait_vm
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// exact GELU on the fp32 value, F.gelu's default: 0.5 v (1 + erf(v / sqrt 2))
__device__ __forceinline__ float gelu_erf(float v) { return v * 0.5f * (1.f + erff(v * 0.70710678118654752440f)); }

template <int NRT, int WAVES, int CT, int P>
__global__ __launch_bounds__(WAVES * 64) void swin_linear_split_kernel(SlArgs a) {
  static_assert(P >= 1 && P <= 3, "one, two or three pieces");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [2][NRT][P][64][16 B], then the tile's bias
  constexpr int kPanelBytes = NRT * P * kFrag;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wg = xcd_contiguous_id(blockIdx.x, a.per_xcd);
  if (wg >= a.n_wg) return;  // workgroup-uniform: the grid is rounded up to whole XCD rounds
  const int tt = wg / a.n_ft, ft = wg - tt * a.n_ft;
  const int nrt_all = a.N / 16;
  const int rt0 = ft * NRT;
  const int nrt_live = nrt_all - rt0 < NRT ? nrt_all - rt0 : NRT;  // the last feature tile may be partial
  const int n0 = rt0 * 16;
  const int n_ks = a.K / kKStep;
  const int g = lane >> 4, j = lane & 15;

  float* bias_s = reinterpret_cast<float*>(smem + 2 * kPanelBytes);
  for (int i = tid; i < NRT * 16; i += WAVES * 64) bias_s[i] = (a.bias && i < nrt_live * 16) ? a.bias[n0 + i] : 0.f;

  const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.ws, 0, a.N * a.K * 6, 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)(a.M * a.K * 4), 0x00020000);

  // this wave's column tiles: tokens tok0 + 16 c + j; a tile that starts at or past M is dead (wave-uniform)
  const int64_t tok0 = ((int64_t)tt * WAVES + wave) * (CT * 16);
  const int64_t left = a.M - tok0;
  const int n_live = left <= 0 ? 0 : (left > 16 * (CT - 1) ? CT : (int)((left + 15) / 16));

  // issue the loads of k-step ks: this wave's pieces of the W panel (LDS-DMA into ring slot ks & 1) and its x of that step
  f32x8 xr[CT];
  auto issue = [&](int ks) {
    unsigned char* dst = smem + (ks & 1) * kPanelBytes;
    const int src = (ks * nrt_all + rt0) * 3 * kFrag;
    for (int f = wave; f < nrt_live * P; f += WAVES) {
      const int fs = P == 3 ? f : (f / P) * 3 + f % P;  // ring piece f = piece f % P of row tile f / P
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (lds_ptr_t)(dst + f * kFrag), 16, lane * 16, src + fs * kFrag, 0, 0);
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int64_t t = tok0 + 16 * c + j;
      const unsigned xo = t < a.M ? (unsigned)((t * a.K + ks * kKStep + 8 * g) * 4) : kOob;
      const f32x4 lo = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, xo, 0, 0));
      const f32x4 hi = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, xo, 16, 0));
      xr[c] = (f32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
  };

  issue(0);
  sl_barrier();  // (also publishes bias_s)

  f32x4 acc[NRT][CT];
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[rt][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int ks = 0; ks < n_ks; ++ks) {
    bf16x8 bh[CT], bm[CT], bl[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < n_live) split3<P>(xr[c], bh[c], bm[c], bl[c]);  // wave-uniform; a dead tile's pieces are never read
    if (ks + 1 < n_ks) issue(ks + 1);  // the next step's loads fly under this step's MFMAs

    const unsigned char* panel = smem + (ks & 1) * kPanelBytes;
    auto read_a = [&](bf16x8 (&dst)[3], int rt) {
#pragma unroll
      for (int p = 0; p < P; ++p) dst[p] = *reinterpret_cast<const bf16x8*>(panel + (rt * P + p) * kFrag + lane * 16);
    };
    // the products of one (row tile, column tile), chained into the accumulator; the small terms first
    auto chain = [&](f32x4 c, const bf16x8 (&av)[3], int cc) -> f32x4 {
      if constexpr (P == 3) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], bm[cc], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[2], bh[cc], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bl[cc], c, 0, 0, 0);
      }
      if constexpr (P >= 2) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], bh[cc], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bm[cc], c, 0, 0, 0);
      }
      return __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bh[cc], c, 0, 0, 0);
    };
    // A dead row tile of a partial feature tile runs its chains on whatever the ring holds there: its accumulators are
    // never stored, and the loop stays one straight line.  A dead column tile is skipped by a wave-uniform branch.
    if (n_live > 0) {
      bf16x8 av[2][3];
      read_a(av[0], 0);
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
        if (rt + 1 < NRT) read_a(av[(rt + 1) & 1], rt + 1);
        __builtin_amdgcn_sched_barrier(0);
        acc[rt][0] = chain(acc[rt][0], av[rt & 1], 0);
        if constexpr (CT > 1) {
          if (n_live > 1) acc[rt][1] = chain(acc[rt][1], av[rt & 1], 1);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    sl_barrier();  // step ks + 1's panel and x have landed; every wave is done with slot ks & 1
  }

  // ---- epilogue.  Lane (j, g) holds, per row tile rt and column tile c, features n0 + rt*16 + 4g .. +3 of token
  //      tok0 + 16 c + j.  A row tile lies inside one output buffer (n3 % 16 == 0).
  const int out_bytes = (int)(a.M * a.n3 * 4);
  const __amdgpu_buffer_rsrc_t r_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.residual, 0, a.epilogue == 2 ? (int)(a.M * a.N * 4) : 0, 0x00020000);
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    if (c < n_live) {  // wave-uniform
      const int64_t tk = tok0 + 16 * c + j;
      const bool tok_ok = tk < a.M;
      if (a.epilogue == 2) {
        f32x4 rv[NRT];
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
          const unsigned ro = (tok_ok && rt < nrt_live) ? (unsigned)((tk * a.N + n0 + rt * 16 + 4 * g) * 4) : kOob;
          rv[rt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_rs, ro, 0, 0));
        }
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) acc[rt][c] = (acc[rt][c] + *reinterpret_cast<const f32x4*>(bias_s + rt * 16 + 4 * g)) + rv[rt];
      } else {
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
          f32x4 v = acc[rt][c] + *reinterpret_cast<const f32x4*>(bias_s + rt * 16 + 4 * g);
          if (a.epilogue == 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = gelu_erf(v[e]);
          }
          acc[rt][c] = v;
        }
      }
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
        const int f0 = n0 + rt * 16;
        const int which = f0 / a.n3;  // wave-uniform
        float* ob = which == 0 ? a.out[0] : (which == 1 ? a.out[1] : a.out[2]);
        const __amdgpu_buffer_rsrc_t o_rs = __builtin_amdgcn_make_buffer_rsrc((void*)ob, 0, out_bytes, 0x00020000);
        const unsigned oo = (tok_ok && rt < nrt_live) ? (unsigned)((tk * a.n3 + (f0 - which * a.n3) + 4 * g) * 4) : kOob;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[rt][c]), o_rs, oo, 0, 0);
      }
    }
  }
}

using sl_kernel_t = void (*)(SlArgs);

template <int P>
sl_kernel_t sl_pick(int cfg) {
  switch (cfg) {
    case 0: return swin_linear_split_kernel<8, 8, 2, P>;
    case 1: return swin_linear_split_kernel<6, 8, 2, P>;
    case 2: return swin_linear_split_kernel<8, 4, 1, P>;
    default: return swin_linear_split_kernel<6, 4, 1, P>;
  }
}

// The host's choice, from the per-site lines of profiles/swin_linear_bench.jsonl.
// Tokens: the 256-token workgroup when its grid gives every CU a workgroup, the 64-token one below that (stage 3 and 4
// at B = 1: the 64-token entries are the fastest on every such line).
// Width: the table's width that leaves the fewest dead row tiles in the last feature tile (128 divides 128 2^i, 96
// divides 96 2^i and 192 2^i).  Where both leave none, the 64-token class takes 96 at every level, and the 256-token
// class takes 96 at three pieces -- the 256 x 128 tile then needs 138 registers and one workgroup fits a CU, the
// 256 x 96 tile 122 and two fit -- and 128 at one or two pieces.  Nothing depends on K.
int choose_cfg(int64_t M, int N, int pieces, int n_cu) {
  const int dead128 = ceil_div(N, 128) * 128 - N, dead96 = ceil_div(N, 96) * 96 - N;
  const int tn = dead96 < dead128 ? 96 : 128;  // on a tie: the width the 256-token class would take at one or two pieces
  const bool big = ceil_div64(M, 256) * ceil_div(N, dead96 <= dead128 ? 96 : 128) >= n_cu;
  if (dead96 == dead128) return big ? (pieces == 3 ? 1 : 0) : 3;
  return (big ? 0 : 2) + (tn == 96 ? 1 : 0);
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

extern "C" int wm2f_swin_linear_split_configs(void) { return kNumCfg; }

extern "C" int wm2f_swin_linear_split_config(int64_t M, int N, int pieces, int n_cu) {
  if (M <= 0 || N <= 0 || N % 16 || pieces < 1 || pieces > 3 || n_cu <= 0) return -1;
  return choose_cfg(M, N, pieces, n_cu);
}

extern "C" int wm2f_swin_linear_split_fwd_p(const void* x, const void* w_split, const void* bias, const void* residual,
                                            void* out0, void* out1, void* out2, int64_t M, int K, int N, int epilogue,
                                            int n_out, int config, int pieces, void* stream) {
  const char* who = "wm2f_swin_linear_split_fwd_p";
  // sizes first, pointers after: a caller can ask about sizes alone
  WM2F_REQUIRE(pieces >= 1 && pieces <= 3, "%s: pieces = %d (1, 2 and 3 are built)", who, pieces);
  WM2F_REQUIRE(M > 0 && K > 0 && N > 0, "%s: non-positive size", who);
  WM2F_REQUIRE(K % kKStep == 0 && N % 16 == 0, "%s: K = %d must be a multiple of %d and N = %d of 16", who, K, kKStep, N);
  WM2F_REQUIRE(epilogue >= 0 && epilogue <= 2, "%s: epilogue = %d (0 bias, 1 bias + GELU, 2 bias + residual)", who, epilogue);
  WM2F_REQUIRE(n_out == 1 || n_out == 3, "%s: n_out = %d (1 or 3)", who, n_out);
  WM2F_REQUIRE(n_out == 1 || (N % 3 == 0 && (N / 3) % 16 == 0 && epilogue == 0),
               "%s: n_out = 3 needs N / 3 = %d a multiple of 16 and the bias epilogue", who, N / 3);
  WM2F_REQUIRE(config >= -1 && config < kNumCfg, "%s: config = %d outside the table of %d (-1: the host's choice)", who, config, kNumCfg);
  WM2F_REQUIRE(M * (int64_t)K * 4 < (1ll << 31) && M * (int64_t)N * 4 < (1ll << 31), "%s: x / out / residual must stay below 2 GiB (32-bit buffer offsets)", who);
  WM2F_REQUIRE((int64_t)N * K * 6 < (1ll << 31), "%s: the split weight must stay below 2 GiB", who);
  WM2F_REQUIRE((epilogue == 2) == (residual != nullptr), "%s: the residual comes with epilogue 2, and only with it", who);
  WM2F_REQUIRE(x && w_split && out0 && (n_out == 1 || (out1 && out2)), "%s: null pointer", who);
  WM2F_REQUIRE(!residual || residual != out0, "%s: out0 may not alias the residual", who);
  const uintptr_t al = (uintptr_t)x | (uintptr_t)w_split | (uintptr_t)bias | (uintptr_t)residual | (uintptr_t)out0 |
                       (uintptr_t)out1 | (uintptr_t)out2;
  WM2F_REQUIRE(al % 16 == 0, "%s: every pointer must be 16-byte aligned", who);
  int n_cu = 0;
  if (cu_count(&n_cu) != 0) {
    set_error("%s: cannot query the device", who);
    return WM2F_ELAUNCH;
  }
  const int cfg = config >= 0 ? config : choose_cfg(M, N, pieces, n_cu);
  const SlCfg& c = kCfg[cfg];
  SlArgs a;
  a.x = (const float*)x;
  a.ws = w_split;
  a.bias = (const float*)bias;
  a.residual = (const float*)residual;
  a.out[0] = (float*)out0;
  a.out[1] = (float*)(n_out == 3 ? out1 : out0);
  a.out[2] = (float*)(n_out == 3 ? out2 : out0);
  a.M = M;
  a.K = K;
  a.N = N;
  a.epilogue = epilogue;
  a.n3 = N / n_out;
  a.n_ft = ceil_div(N, c.nrt * 16);
  const int64_t n_wg = ceil_div64(M, c.waves * c.ct * 16) * a.n_ft;
  WM2F_REQUIRE(n_wg < (1ll << 30), "%s: too many workgroups", who);
  a.n_wg = (int)n_wg;
  a.per_xcd = ceil_div(a.n_wg, kNumXcd);
  const int grid = a.per_xcd * kNumXcd;
  const size_t lds = (size_t)2 * c.nrt * pieces * kFrag + (size_t)c.nrt * 16 * sizeof(float);
  sl_kernel_t kfn = pieces == 3 ? sl_pick<3>(cfg) : (pieces == 2 ? sl_pick<2>(cfg) : sl_pick<1>(cfg));
  hipLaunchKernelGGL(kfn, dim3(grid), dim3(c.waves * 64), lds, (hipStream_t)stream, a);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
