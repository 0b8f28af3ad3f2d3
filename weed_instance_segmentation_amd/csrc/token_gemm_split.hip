// Token GEMM of the pixel decoder at fp32 accuracy on the bf16 matrix cores ("split-bf16"):
//     out (M, N) = epilogue( x (M, K) . W (N, K)^T + bias )
// with the epilogues of token_gemm.hip (bias, ReLU, residual + LayerNorm, + pos second output, feature-group-major output).
//
// The split.  Every fp32 operand is written as three bf16 pieces, a = h + m + l, each the round-to-nearest
// bf16 of what the previous pieces leave: h = bf16(a), m = bf16(a - h), l = bf16(a - h - m).  Both differences are exact in
// fp32, |m| <= 2^-8 |a|, |l| <= 2^-16 |a|, and l takes the last <= 8 significant bits exactly, so h + m + l == a for every
// a of magnitude >= 2^-110 (below it the pieces fall under bf16's subnormal step 2^-133).  A product x w is accumulated as
// the six terms h.h + h.m + m.h + h.l + l.h + m.m, each product of two bf16 values exact in fp32; the three left out (m.l,
// l.m, l.l) are bounded by 2^-23 |x w| and are of order 2^-28 |x w| on typical data -- an fp32 GEMM in accuracy: the
// tests hold it to twice the error of the fp32-MFMA kernel (token_gemm.hip) against an fp64 reference.
// Non-finite values: h is taken from x clamped to the largest finite bf16 (an RNE bf16 of |x| near FLT_MAX is inf, and
// inf - inf between the pieces would turn a finite input into NaN); an inf or NaN input still makes its residual
// pieces inf / NaN, so every output a non-finite input touches is non-finite.  The one difference from fp32: such an
// output is NaN where an fp32 GEMM may give +-inf (inf - inf inside the pieces).
//
// Layout of the work (MI355X: 256 CUs, 160 KiB LDS, v_mfma_f32_16x16x32_bf16 = 16 cycles, 8 of them blocking vector issue):
//   * W is split ONCE per weight version (wm2f_token_linear_split_weight) into fragment order
//     [k-step (K/32)][row tile (N/16)][piece h|m|l][lane][8 bf16]: a (row tile, k-step) A fragment of one piece is 1 KiB of
//     contiguous bytes, lane-linear, and one k-step's panel of a feature slice is contiguous;
//   * one persistent workgroup per CU, 8 waves (2 per SIMD, 256 registers each), no loader wave: every wave issues its
//     share of the NEXT k-step's panel by LDS-DMA (1 KiB pieces) into the other half of a two-panel ring, together with its
//     own x loads of the next k-step, then computes the current one; one `s_waitcnt vmcnt(0)` + barrier per k-step, and
//     no other wait for vector memory between a k-step's LDS-DMA issue and its first MFMA (sg_wait_vm below);
//   * a CU owns a contiguous range of 16-token column tiles, its waves split it as evenly as tiles allow, and a wave walks
//     its share two column tiles (32 tokens) per turn: each A fragment read from LDS feeds 2 x 6 MFMAs (3 ds_read_b128 per
//     12 MFMAs of 16 cycles: a quarter of the LDS array's 256 B/clk); a wave with an odd share has one live tile in its
//     last turn and then runs the one tile's split and six-MFMA chains only (a wave-uniform branch), so the turn costs
//     one tile: at the encoder's 42 tiles per CU the busiest SIMD runs 11 tile-steps, and project_kv, one tile per wave,
//     half the MFMAs it ran before;
//   * x is the B operand, loaded as fp32 (lane (j, g): token j, channels 8g .. 8g + 7 of the k-step) and split in
//     registers once per element and feature slice; a wave owns ALL N features of its tokens when N <= 288, so the
//     LayerNorm of a token is a reduction inside the wave.  N = 1024 (fc1) runs as four 256-wide slices one after the
//     other on the same tokens, so the slices' x re-reads hit the caches, not HBM.
//   * the LayerNorm epilogue keeps two batches of residual rows, then of pos rows, in flight (in the registers the x loads
//     of the next step, issued behind it, leave free), so its waits for memory overlap instead of following one another.
// Roofline: bf16 MFMA, 6 x 2 M N K flop against 2.5 PFLOP/s; HBM: x once, out once (+ residual, + pos).  Measured
// (timing ablations of the profiling build): no site is MFMA-bound -- without its MFMAs a launch is 8-15 %
// faster, without its epilogue stores 13-26 %; a k-step waits on its memory path (x, the panel every CU re-reads per
// k-step and turn), and the epilogue's stores and loads come on top.  Keeping the bias epilogues' stores in flight across
// the barrier, and walking odd workgroups half a turn out of phase, were built and measured there and are not kept.
// token_ffn_split_kernel below runs the encoder's fc1 and fc2 as one kernel on the same tiling.
#include "common.h"

namespace wm2f {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x8 = __attribute__((ext_vector_type(8))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int kSgWaves = 8;
constexpr int kSgThreads = kSgWaves * 64;
constexpr int kSgCT = 2;      // column tiles (16 tokens each) per wave and turn
constexpr int kKStep = 32;    // K of one v_mfma_f32_16x16x32_bf16
constexpr int kFrag = 1024;   // bytes of one A fragment piece (64 lanes x 8 bf16)
constexpr unsigned kOob = 0x80000000u;
constexpr float kBf16Max = 3.38953139e38f;  // largest finite bf16, 0x7F7F

// The first P pieces of the three-piece split (P = 3: all of it; the pieces past P are left untouched and never read)
template <int P = 3>
__device__ __forceinline__ void split3(const f32x8 x, bf16x8& h, bf16x8& m, bf16x8& l) {
  f32x8 xc;
#pragma unroll
  for (int i = 0; i < 8; ++i) xc[i] = __builtin_amdgcn_fmed3f(x[i], -kBf16Max, kBf16Max);
  if constexpr (P == 1) {  // no residual piece carries an inf or a NaN on: x * 0 (0, or NaN) keeps h non-finite with x
#pragma unroll
    for (int i = 0; i < 8; ++i) xc[i] = __builtin_fmaf(x[i], 0.f, xc[i]);
  }
  // vector conversions: v_cvt_pk_bf16_f32 (RNE, a NaN stays a NaN); bf16 -> f32 is exact
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

__global__ __launch_bounds__(256) void split_weight_kernel(const float* __restrict__ w, bf16x8* __restrict__ ws, int N, int K) {
  const int kg_n = K / 8;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over (feature n, group of 8 channels)
  if (i >= N * kg_n) return;
  const int n = i / kg_n, kg = i - n * kg_n;
  const f32x4* src = reinterpret_cast<const f32x4*>(w + (int64_t)n * K + kg * 8);
  const f32x4 lo = src[0], hi = src[1];
  const f32x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  bf16x8 h, m, l;
  split3(v, h, m, l);
  const int ks = kg >> 2, g = kg & 3, rt = n >> 4, lane = (n & 15) + 16 * g;
  const int64_t base = ((int64_t)ks * (N / 16) + rt) * 3 * 64 + lane;
  ws[base] = h;
  ws[base + 64] = m;
  ws[base + 128] = l;
}

// The row map of the fused feed-forward kernel (token_ffn_split_kernel): the weight row that sits at row
// position n of the split.  Inside every 32-row block, position (row tile 2i + h, row 4g + e) holds row 8g + 4h + e of
// the block, so that registers e = 0 .. 3 of the C tiles 2i and 2i + 1 are, in lane group g, k = 32i + 8g .. + 7 in
// natural order: the B fragment of the next product's k-step i.  A permutation of each 32-row block.
__host__ __device__ constexpr int ffn_row_of(int n) {
  return (n & ~31) + 8 * ((n >> 2) & 3) + 4 * ((n >> 4) & 1) + (n & 3);
}

// split_weight_kernel with the rows in another order: row position n of the split holds row ffn_row_of(n) of w
__global__ __launch_bounds__(256) void split_weight_rows_kernel(const float* __restrict__ w, bf16x8* __restrict__ ws, int N, int K) {
  const int kg_n = K / 8;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over (row position n, group of 8 channels)
  if (i >= N * kg_n) return;
  const int n = i / kg_n, kg = i - n * kg_n;
  const f32x4* src = reinterpret_cast<const f32x4*>(w + (int64_t)ffn_row_of(n) * K + kg * 8);
  const f32x4 lo = src[0], hi = src[1];
  const f32x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  bf16x8 h, m, l;
  split3(v, h, m, l);
  const int ks = kg >> 2, g = kg & 3, rt = n >> 4, lane = (n & 15) + 16 * g;
  const int64_t base = ((int64_t)ks * (N / 16) + rt) * 3 * 64 + lane;
  ws[base] = h;
  ws[base + 64] = m;
  ws[base + 128] = l;
}

struct SgArgs {
  const float *x, *bias, *residual, *gamma, *beta, *pos;
  const void* ws;
  float *out, *out_pos;
  int64_t M;
  int K, N, relu;
  int out_group;  // 0: out (M, N) row-major; G > 0: out (N / G, M, G)
  int64_t pos_rows;
  float eps;
  int tiles_total;  // ceil(M / 16)
};

// The k-step's wait for this wave's vector memory: s_waitcnt vmcnt(0), expcnt and lgkmcnt left at their maxima.  It is
// the builtin, not inline asm: the compiler's own wait insertion then knows the counter is drained and adds no wait of
// its own between a k-step's LDS-DMA issue and its first MFMA (it did, vmcnt(3) / vmcnt(1) in front of the x loads, when
// the wait was hidden in asm: in hardware those waited for the LDS-DMA pieces just issued).
__device__ __forceinline__ void sg_wait_vm() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0x0F70);
}

__device__ __forceinline__ void sg_barrier() {
  sg_wait_vm();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// The LayerNorm epilogue's loads, template parameter PIPE: residual batches double-buffered, and the pos
// batch of a row-tile pair loaded before the stores of the pair before it.  The product library is compiled with
// PIPE = true alone; the profiling build also carries the serial epilogue (WM2F_TGS_OPT=0) and the timing ablations ABL
// (WM2F_TGS_ABL: 1 no epilogue stores, 2 no epilogue loads, 4 no MFMAs -- OUTPUTS NOT VALID), include/wm2f_prof.h.
constexpr int kAblStores = 1, kAblLoads = 2, kAblMfma = 4;

// NRT = row tiles of one feature slice (16: N = 256 and the 256-wide slices of N = 1024; 18: N = 288).
// EPI = the epilogue, fixed at compile time (one LayerNorm epilogue inside the k-step loop beside the others spilled):
// 0 = bias (+ ReLU) row-major, 1 = bias (+ ReLU) feature-group major, 2 = bias + residual + LayerNorm (+ pos)
// P = the pieces of each operand that take part: 3 = all six products, 2 = h and m (m.h, h.m, h.h), 1 = h
// alone (h.h).  The split weight is the three-piece one at every P; the ring holds the first P pieces of each row tile.
template <int NRT, int EPI, bool PIPE = true, int ABL = 0, int P = 3>
__global__ __launch_bounds__(kSgThreads) void token_gemm_split_kernel(SgArgs a) {
  static_assert(P >= 1 && P <= 3, "one, two or three pieces");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [2][NRT][P][64][16 B], then bias | gamma | beta
  constexpr int kPanelBytes = NRT * P * kFrag;
  constexpr int kPieces = NRT * P;
  constexpr int CT = kSgCT;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_cu = gridDim.x, cu = blockIdx.x;
  const int t0 = (int)(((int64_t)a.tiles_total * cu) / n_cu), t1 = (int)(((int64_t)a.tiles_total * (cu + 1)) / n_cu);
  const int n_t = t1 - t0;
  const int n_ks = a.K / kKStep;
  const int n_sl = a.N / (NRT * 16);
  const int share_max = (n_t + kSgWaves - 1) / kSgWaves;
  const int n_iter = (share_max + CT - 1) / CT;
  const int spt = n_sl * n_ks;  // k-steps per turn
  const int n_q = n_iter * spt;
  float* vec = reinterpret_cast<float*>(smem + 2 * kPanelBytes);
  for (int i = tid; i < 3 * a.N; i += kSgThreads) {
    const int which = i / a.N, f = i - which * a.N;
    const float* srcv = which == 0 ? a.bias : (which == 1 ? a.gamma : a.beta);
    vec[i] = srcv ? srcv[f] : 0.f;
  }
  __syncthreads();
  if (n_q == 0) return;  // workgroup-uniform

  const int base = n_t / kSgWaves, extra = n_t % kSgWaves;
  const int w0 = t0 + wave * base + (wave < extra ? wave : extra);
  const int w1 = w0 + base + (wave < extra ? 1 : 0);
  const int g = lane >> 4, j = lane & 15;
  const int nrt_all = a.N / 16;
  const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.ws, 0, a.N * a.K * 6, 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)(a.M * a.K * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t o_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.out, 0, (int)(a.M * a.N * 4), 0x00020000);

  // issue the loads of k-step q: this wave's pieces of the W panel (LDS-DMA into ring slot q & 1) and its x of that step
  f32x8 xr[CT];
  auto issue = [&](int q) {
    const int it = q / spt, r = q - it * spt, sl = r / n_ks, ks = r - sl * n_ks;
    unsigned char* dst = smem + (q & 1) * kPanelBytes;
    const int src = (ks * nrt_all + sl * NRT) * 3 * kFrag;
    for (int f = wave; f < kPieces; f += kSgWaves) {
      const int fs = P == 3 ? f : (f / P) * 3 + f % P;  // ring piece f = piece f % P of row tile f / P
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (lds_ptr_t)(dst + f * kFrag), 16, lane * 16, src + fs * kFrag, 0, 0);
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int tile = w0 + CT * it + c;
      const int64_t t = (int64_t)tile * 16 + j;
      const unsigned xo = (tile < w1 && t < a.M) ? (unsigned)((t * a.K + ks * kKStep + 8 * g) * 4) : kOob;
      const f32x4 lo = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, xo, 0, 0));
      const f32x4 hi = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, xo, 16, 0));
      xr[c] = (f32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
  };

  issue(0);
  sg_barrier();  // (also publishes vec)

  f32x4 acc[NRT][CT];
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[rt][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int q = 0; q < n_q; ++q) {
    const int it = q / spt, r = q - it * spt, sl = r / n_ks, ks = r - sl * n_ks;
    const int ct0 = w0 + CT * it;
    const int n_live = ct0 >= w1 ? 0 : (ct0 + 1 >= w1 ? 1 : 2);  // wave-uniform
    bf16x8 bh[CT], bm[CT], bl[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < n_live) split3<P>(xr[c], bh[c], bm[c], bl[c]);  // wave-uniform; a dead tile's pieces are never read
    // the next step's loads fly under this step's MFMAs -- except before a LayerNorm epilogue, where their 16 registers
    // made the epilogue spill: there they are issued after it
    const bool late = EPI == 2 && ks + 1 == n_ks;
    if (q + 1 < n_q && !late) issue(q + 1);

    const unsigned char* panel = smem + (q & 1) * kPanelBytes;
    auto read_a = [&](bf16x8 (&dst)[3], int rt) {
#pragma unroll
      for (int p = 0; p < P; ++p) dst[p] = *reinterpret_cast<const bf16x8*>(panel + (rt * P + p) * kFrag + lane * 16);
    };
    // the six products of one (row tile, column tile); the small terms first
    auto six = [&](f32x4 c, const bf16x8 (&av)[3], int cc) -> f32x4 {
      if (ABL & kAblMfma) {  // timing ablation: three multiply-adds keep the LDS reads and the split alive
        c[0] += __builtin_bit_cast(f32x4, av[0])[0] * __builtin_bit_cast(f32x4, bl[cc])[0];
        c[1] += __builtin_bit_cast(f32x4, av[1])[1] * __builtin_bit_cast(f32x4, bm[cc])[1];
        c[2] += __builtin_bit_cast(f32x4, av[2])[2] * __builtin_bit_cast(f32x4, bh[cc])[2];
        return c;
      }
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
    // a turn with one live column tile skips the second tile's split and its six-MFMA chains by a wave-uniform branch
    // inside the one unrolled loop (a separate one-tile loop beside this one made the compiler spill the accumulators);
    // the dead tile's accumulators stay zero and nothing of it is stored.  A live tile's MFMA sequence is the same either way
    if (n_live > 0) {
      bf16x8 av[2][3];
      read_a(av[0], 0);
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
        if (rt + 1 < NRT) read_a(av[(rt + 1) & 1], rt + 1);
        __builtin_amdgcn_sched_barrier(0);
        acc[rt][0] = six(acc[rt][0], av[rt & 1], 0);
        if (n_live > 1) acc[rt][1] = six(acc[rt][1], av[rt & 1], 1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    if (ks + 1 == n_ks) {
      // ---- epilogue of feature slice sl.  Lane (j, g) holds, per row tile rt and column tile c, features
      //      n0 + rt*16 + 4g .. +3 of token (ct0 + c)*16 + j.
      const int n0 = sl * NRT * 16;
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        __builtin_amdgcn_sched_barrier(0);
        if (c < n_live) {  // wave-uniform
          const int64_t tk = (int64_t)(ct0 + c) * 16 + j;
          const bool tok_ok = tk < a.M;
          const unsigned row_o = tok_ok ? (unsigned)((tk * a.N + n0) * 4) : kOob;
          // timing ablation "no epilogue stores": a condition that is never true at run time keeps the values alive
          const bool st = !(ABL & kAblStores) || a.tiles_total < 0;
#pragma unroll
          for (int rt = 0; rt < NRT; ++rt) {
            f32x4 v = acc[rt][c] + *reinterpret_cast<const f32x4*>(vec + n0 + rt * 16 + 4 * g);
            if (a.relu) v = __builtin_elementwise_max(v, (f32x4){0.f, 0.f, 0.f, 0.f});
            acc[rt][c] = v;
          }
          if (EPI == 2) {  // LayerNorm over the token's N features (n_sl == 1): this lane's NRT * 4 values, then the 4 lane groups
            // this lane's 4 features of row tile 0; a row tile's 64 bytes go into the instruction's offset field (the
            // same addresses as row_o + (rt * 16 + 4 * g) * 4 in one register per store cost 15 registers and spilled)
            const unsigned row_g = tok_ok ? row_o + (unsigned)(16 * g) : kOob;
            constexpr int kEB = 2;  // row tiles per batch of epilogue loads (4 spilled beside the accumulators of two column tiles)
            if (a.residual && !(ABL & kAblLoads)) {
              const __amdgpu_buffer_rsrc_t r_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.residual, 0, (int)(a.M * a.N * 4), 0x00020000);
              if (PIPE) {
                // two batches in the registers the late-issued x loads leave free: batch b + 1 flies while b is added
                f32x4 rv[2][kEB];
#pragma unroll
                for (int i = 0; i < kEB; ++i)
                  rv[0][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_rs, row_g, i * 64, 0));
#pragma unroll
                for (int h0 = 0; h0 < NRT; h0 += kEB) {
                  const int b = (h0 / kEB) & 1;
                  if (h0 + kEB < NRT) {
#pragma unroll
                    for (int i = 0; i < kEB; ++i)
                      rv[b ^ 1][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_rs, row_g, (h0 + kEB + i) * 64, 0));
                  }
#pragma unroll
                  for (int i = 0; i < kEB; ++i) acc[h0 + i][c] += rv[b][i];
                  __builtin_amdgcn_sched_barrier(0);
                }
              } else {
#pragma unroll
                for (int h0 = 0; h0 < NRT; h0 += kEB) {
                  f32x4 rv[kEB];
#pragma unroll
                  for (int i = 0; i < kEB; ++i)
                    rv[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_rs, row_g, (h0 + i) * 64, 0));
#pragma unroll
                  for (int i = 0; i < kEB; ++i) acc[h0 + i][c] += rv[i];
                  __builtin_amdgcn_sched_barrier(0);  // one batch of residual rows in registers at a time
                }
              }
            }
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
              const f32x4 v = acc[rt][c];
              s1 += (v[0] + v[1]) + (v[2] + v[3]);
              s2 += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
            }
            s1 += __shfl_xor(s1, 16, 64);
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 16, 64);
            s2 += __shfl_xor(s2, 32, 64);
            const float inv_n = 1.f / (float)a.N;
            const float mean = s1 * inv_n;
            float var = s2 * inv_n - mean * mean;
            var = var < 0.f ? 0.f : var;
            const float rstd = rsqrtf(var + a.eps);
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
              const int f0 = rt * 16 + 4 * g;
              const f32x4 gm = *reinterpret_cast<const f32x4*>(vec + a.N + f0), bt = *reinterpret_cast<const f32x4*>(vec + 2 * a.N + f0);
              acc[rt][c] = (acc[rt][c] - mean) * rstd * gm + bt;
            }
            const bool pipe_pos = PIPE && a.out_pos;  // then `out` is stored pair by pair between the pos loads
            if (st && !pipe_pos) {
#pragma unroll
              for (int rt = 0; rt < NRT; ++rt)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[rt][c]), o_rs, row_g, rt * 64, 0);
            }
            if (a.out_pos) {  // the next layer's hidden + pos
              const __amdgpu_buffer_rsrc_t p_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.pos, 0, (int)(a.pos_rows * a.N * 4), 0x00020000);
              const __amdgpu_buffer_rsrc_t q_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.out_pos, 0, (int)(a.M * a.N * 4), 0x00020000);
              const unsigned prow = tok_ok ? (unsigned)(((tk % a.pos_rows) * a.N + 4 * g) * 4) : kOob;
              const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
              if (PIPE) {
                // the pos rows of pair h0 + 2 are loaded before the stores of pair h0: the wait for a pos batch then
                // covers the stores of the pair before, issued a whole batch earlier, never the ones just issued
                f32x4 pv[2][kEB];
#pragma unroll
                for (int i = 0; i < kEB; ++i)
                  pv[0][i] = (ABL & kAblLoads) ? zero4 : __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(p_rs, prow, i * 64, 0));
#pragma unroll
                for (int h0 = 0; h0 < NRT; h0 += kEB) {
                  const int b = (h0 / kEB) & 1;
                  if (h0 + kEB < NRT) {
#pragma unroll
                    for (int i = 0; i < kEB; ++i)
                      pv[b ^ 1][i] = (ABL & kAblLoads) ? zero4 : __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(p_rs, prow, (h0 + kEB + i) * 64, 0));
                  }
                  if (st) {
#pragma unroll
                    for (int i = 0; i < kEB; ++i)
                      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[h0 + i][c]), o_rs, row_g, (h0 + i) * 64, 0);
#pragma unroll
                    for (int i = 0; i < kEB; ++i)
                      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, (ABL & kAblLoads) ? acc[h0 + i][c] : acc[h0 + i][c] + pv[b][i]), q_rs, row_g, (h0 + i) * 64, 0);
                  }
                  __builtin_amdgcn_sched_barrier(0);
                }
              } else {
#pragma unroll
                for (int h0 = 0; h0 < NRT; h0 += kEB) {
                  f32x4 pv[kEB];
#pragma unroll
                  for (int i = 0; i < kEB; ++i)
                    pv[i] = (ABL & kAblLoads) ? zero4 : __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(p_rs, prow, (h0 + i) * 64, 0));
                  if (st) {
#pragma unroll
                    for (int i = 0; i < kEB; ++i)
                      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, (ABL & kAblLoads) ? acc[h0 + i][c] : acc[h0 + i][c] + pv[i]), q_rs, row_g, (h0 + i) * 64, 0);
                  }
                }
              }
            }
          } else if (!st) {
            // timing ablation: nothing is stored
          } else if (EPI == 1) {
            // feature-group-major output (N / G, M, G); a lane's 4 consecutive features stay inside one group (G % 4 == 0)
            const unsigned G = (unsigned)a.out_group;
            const unsigned grp_bytes = (unsigned)(a.M * G * 4);
            const unsigned tok_o = tok_ok ? (unsigned)(tk * G * 4) : kOob;
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
              const unsigned f0 = (unsigned)(n0 + rt * 16 + 4 * g);
              const unsigned grp = f0 / G;
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[rt][c]), o_rs, tok_o + grp * grp_bytes + (f0 - grp * G) * 4, 0, 0);
            }
          } else {
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt)
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[rt][c]), o_rs, row_o + (unsigned)((rt * 16 + 4 * g) * 4), 0, 0);
          }
        }
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) acc[rt][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
    if (q + 1 < n_q && late) issue(q + 1);
    sg_barrier();  // step q + 1's panel and x have landed; every wave is done with slot q & 1
  }
}

// ---- The encoder's feed-forward pair in one kernel:
//     out (M, 256) = LayerNorm(relu(x (M, 256) . W1 (F, 256)^T + b1) . W2 (256, F)^T + b2 + residual), out_pos = out + pos
// The (M, F) intermediate never leaves the registers.  The tiling and the arithmetic are the kernel's above: one persistent
// workgroup per CU, 8 waves, the 48 KiB W panels by LDS-DMA into the two-slot ring, x split in registers, six products per
// k-step in the same MFMA order, a wave owns all features of its tokens.  A wave takes ONE column tile per turn: acc1 (a
// 256-wide slice of the hidden features) and acc2 (the 256 outputs) are 64 registers each.  Per slice s of the F / 256:
//   * 8 k-steps of fc1 into acc1 -- W1's rows of slice s in the order of ffn_row_of (wm2f_token_linear_split_weight_rows),
//     x loaded as above;  + b1 (read through the same map), ReLU;
//   * 8 k-steps of fc2 into acc2 -- panels 8s .. 8s + 7 of the plain split of W2; step i takes its B operand from
//     acc1[2i] and acc1[2i + 1]: lane (j, g) of a C tile holds rows 4g .. 4g + 3 of column j, a B fragment wants
//     k = 8g .. 8g + 7 of column j, and the row map makes those eight registers k = 32i + 8g .. + 7 in natural order.  No
//     x load; the steps stay unrolled (a runtime index into acc1 would put it in scratch).
// After the last slice the LayerNorm epilogue above (PIPE) runs on acc2.  Every MFMA sees the operands of the two-launch
// route in the same k positions and the same order, so the outputs are its bits.  ABL: kAblStores, kAblMfma (profiling build).
struct FfnArgs {
  const float *x, *b1, *b2, *residual, *gamma, *beta, *pos;
  const void *w1s, *w2s;
  float *out, *out_pos;
  int64_t M;
  int F;
  int64_t pos_rows;
  float eps;
  int tiles_total;  // ceil(M / 16)
};

template <int ABL = 0, int P = 3>
__global__ __launch_bounds__(kSgThreads) void token_ffn_split_kernel(FfnArgs a) {
  constexpr int NRT = 16, D = 256, NKS = D / kKStep;  // K of fc1 = N of fc2 = 256; 8 k-steps per slice in either product
  static_assert(P >= 1 && P <= 3, "one, two or three pieces");
  constexpr int kPanelBytes = NRT * P * kFrag;
  constexpr int kPieces = NRT * P;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [2][NRT][P][64][16 B], then b1 | b2 | gamma | beta
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_cu = gridDim.x, cu = blockIdx.x;
  const int t0 = (int)(((int64_t)a.tiles_total * cu) / n_cu), t1 = (int)(((int64_t)a.tiles_total * (cu + 1)) / n_cu);
  const int n_t = t1 - t0;
  const int n_sl = a.F / D;
  const int nrt1 = a.F / 16;
  const int n_iter = (n_t + kSgWaves - 1) / kSgWaves;  // turns: one column tile per wave and turn
  float* vec = reinterpret_cast<float*>(smem + 2 * kPanelBytes);
  for (int i = tid; i < a.F + 3 * D; i += kSgThreads) {
    const int r = i - a.F;
    vec[i] = r < 0 ? a.b1[i] : (r < D ? a.b2[r] : (r < 2 * D ? a.gamma[r - D] : a.beta[r - 2 * D]));
  }
  __syncthreads();
  if (n_iter == 0) return;  // workgroup-uniform

  const int base = n_t / kSgWaves, extra = n_t % kSgWaves;
  const int w0 = t0 + wave * base + (wave < extra ? wave : extra);
  const int w1 = w0 + base + (wave < extra ? 1 : 0);
  const int g = lane >> 4, j = lane & 15;
  const __amdgpu_buffer_rsrc_t w1_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.w1s, 0, a.F * D * 6, 0x00020000);
  const __amdgpu_buffer_rsrc_t w2_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.w2s, 0, a.F * D * 6, 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)(a.M * D * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t o_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.out, 0, (int)(a.M * D * 4), 0x00020000);

  // this wave's pieces of one panel (48 KiB at P = 3: the first P pieces of each row tile), by LDS-DMA into ring slot `slot`
  auto issue_w = [&](const __amdgpu_buffer_rsrc_t rs, int src, int slot) {
    unsigned char* dst = smem + slot * kPanelBytes;
    for (int f = wave; f < kPieces; f += kSgWaves) {
      const int fs = P == 3 ? f : (f / P) * 3 + f % P;  // ring piece f = piece f % P of row tile f / P
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(dst + f * kFrag), 16, lane * 16, src + fs * kFrag, 0, 0);
    }
  };
  // panel (slice sl, k-step ks) of W1: row tiles 16 sl .. + 15 of k-step ks;  panel (sl, i) of W2: k-step 8 sl + i
  auto w1_src = [&](int sl, int ks) { return (ks * nrt1 + sl * NRT) * 3 * kFrag; };
  auto w2_src = [&](int sl, int i) { return (sl * NKS + i) * NRT * 3 * kFrag; };
  f32x8 xr;
  auto issue_x = [&](int tile, int ks) {
    const int64_t t = (int64_t)tile * 16 + j;
    const unsigned xo = (tile < w1 && t < a.M) ? (unsigned)((t * D + ks * kKStep + 8 * g) * 4) : kOob;
    const f32x4 lo = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, xo, 0, 0));
    const f32x4 hi = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, xo, 16, 0));
    xr = (f32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
  // one k-step of one column tile: the 16 row tiles of the panel in `slot` against the pieces of the B fragment, into acc;
  // the six products in the order of token_gemm_split_kernel, the small terms first
  auto k_step = [&](f32x4 (&acc)[NRT], int slot, const bf16x8 bh, const bf16x8 bm, const bf16x8 bl) {
    const unsigned char* panel = smem + slot * kPanelBytes;
    auto read_a = [&](bf16x8 (&dst)[3], int rt) {
#pragma unroll
      for (int p = 0; p < P; ++p) dst[p] = *reinterpret_cast<const bf16x8*>(panel + (rt * P + p) * kFrag + lane * 16);
    };
    bf16x8 av[2][3];
    read_a(av[0], 0);
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
      if (rt + 1 < NRT) read_a(av[(rt + 1) & 1], rt + 1);
      __builtin_amdgcn_sched_barrier(0);
      f32x4 c = acc[rt];
      const bf16x8(&v)[3] = av[rt & 1];
      if (ABL & kAblMfma) {  // timing ablation: three multiply-adds keep the LDS reads and the split alive
        c[0] += __builtin_bit_cast(f32x4, v[0])[0] * __builtin_bit_cast(f32x4, bl)[0];
        c[1] += __builtin_bit_cast(f32x4, v[1])[1] * __builtin_bit_cast(f32x4, bm)[1];
        c[2] += __builtin_bit_cast(f32x4, v[2])[2] * __builtin_bit_cast(f32x4, bh)[2];
      } else {
        if constexpr (P == 3) {
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v[1], bm, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v[2], bh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v[0], bl, c, 0, 0, 0);
        }
        if constexpr (P >= 2) {
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v[1], bh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v[0], bm, c, 0, 0, 0);
        }
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v[0], bh, c, 0, 0, 0);
      }
      acc[rt] = c;
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  issue_w(w1_rs, w1_src(0, 0), 0);
  issue_x(w0, 0);
  sg_barrier();  // (also publishes vec)

  f32x4 acc1[NRT], acc2[NRT];
  for (int it = 0; it < n_iter; ++it) {
    const int tile = w0 + it;
    const bool live = tile < w1;  // wave-uniform; a dead wave still loads its share of every panel and meets every barrier
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) acc2[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int sl = 0; sl < n_sl; ++sl) {
      const bool more = sl + 1 < n_sl;
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) acc1[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      // ---- fc1: acc1 = W1[rows of slice sl] . x; a slice is 16 steps, so step ks sits in ring slot ks & 1
#pragma unroll 1
      for (int ks = 0; ks < NKS; ++ks) {
        bf16x8 bh, bm, bl;
        if (live) split3<P>(xr, bh, bm, bl);
        // every fc1 step issues a panel and an x load, without a branch (a step without the x load made the compiler wait
        // for the panel it had just issued): the last one takes fc2's first panel and the x of the next fc1 step there
        // will be, k-step 0 of this tile again or, after the last slice, of the next turn's tile
        const bool last = ks + 1 == NKS;
        issue_w(last ? w2_rs : w1_rs, last ? w2_src(sl, 0) : w1_src(sl, ks + 1), (ks + 1) & 1);
        issue_x(last && !more ? tile + 1 : tile, last ? 0 : ks + 1);
        if (live) k_step(acc1, ks & 1, bh, bm, bl);
        sg_barrier();
      }
      // + b1, ReLU: position (row tile rt = 2i + h, rows 4g .. 4g + 3) holds hidden features 256 sl + 32i + 8g + 4h .. + 3
      if (live) {
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
          const f32x4 v = acc1[rt] + *reinterpret_cast<const f32x4*>(vec + sl * D + 32 * (rt >> 1) + 8 * g + 4 * (rt & 1));
          // max(v, 0) is v_max_f32, which answers 0 for a NaN; the NaN is put back, so that a non-finite token stays
          // non-finite through the ReLU (every other value keeps the bits of the max)
          f32x4 m = __builtin_elementwise_max(v, (f32x4){0.f, 0.f, 0.f, 0.f});
#pragma unroll
          for (int e = 0; e < 4; ++e) m[e] = v[e] != v[e] ? v[e] : m[e];
          acc1[rt] = m;
        }
      }
      // ---- fc2: acc2 += W2[:, 256 sl + 32i .. + 31] . relu(...), step i in ring slot i & 1
#pragma unroll
      for (int i = 0; i < NKS; ++i) {
        bf16x8 bh, bm, bl;
        if (live) {
          const f32x4 lo = acc1[2 * i], hi = acc1[2 * i + 1];
          split3<P>((f32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}, bh, bm, bl);
        }
        if (i + 1 < NKS) {
          issue_w(w2_rs, w2_src(sl, i + 1), (i + 1) & 1);
        } else if (more) {
          issue_w(w1_rs, w1_src(sl + 1, 0), 0);
        }  // the last step of a turn issues nothing: the next turn's first panel follows the epilogue
        if (live) k_step(acc2, i & 1, bh, bm, bl);
        if (i + 1 < NKS || more) sg_barrier();
      }
    }

    // ---- bias + residual + LayerNorm (+ pos) on acc2: the epilogue of token_gemm_split_kernel<16, 2, true>, one column
    //      tile.  Lane (j, g) holds, per row tile rt, features rt*16 + 4g .. +3 of token tile*16 + j.
    __builtin_amdgcn_sched_barrier(0);
    if (live) {
      const int64_t tk = (int64_t)tile * 16 + j;
      const bool tok_ok = tk < a.M;
      const unsigned row_g = tok_ok ? (unsigned)((tk * D + 4 * g) * 4) : kOob;  // a row tile's 64 bytes go into the offset field
      const bool st = !(ABL & kAblStores) || a.tiles_total < 0;  // "no epilogue stores": never true at run time
      constexpr int kEB = 2;  // row tiles per batch of epilogue loads
      const float* b2v = vec + a.F;
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) acc2[rt] = acc2[rt] + *reinterpret_cast<const f32x4*>(b2v + rt * 16 + 4 * g);
      {
        const __amdgpu_buffer_rsrc_t r_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.residual, 0, (int)(a.M * D * 4), 0x00020000);
        f32x4 rv[2][kEB];  // batch b + 1 flies while b is added
#pragma unroll
        for (int i = 0; i < kEB; ++i)
          rv[0][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_rs, row_g, i * 64, 0));
#pragma unroll
        for (int h0 = 0; h0 < NRT; h0 += kEB) {
          const int b = (h0 / kEB) & 1;
          if (h0 + kEB < NRT) {
#pragma unroll
            for (int i = 0; i < kEB; ++i)
              rv[b ^ 1][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_rs, row_g, (h0 + kEB + i) * 64, 0));
          }
#pragma unroll
          for (int i = 0; i < kEB; ++i) acc2[h0 + i] += rv[b][i];
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
        const f32x4 v = acc2[rt];
        s1 += (v[0] + v[1]) + (v[2] + v[3]);
        s2 += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
      }
      s1 += __shfl_xor(s1, 16, 64);
      s1 += __shfl_xor(s1, 32, 64);
      s2 += __shfl_xor(s2, 16, 64);
      s2 += __shfl_xor(s2, 32, 64);
      const float inv_n = 1.f / (float)D;
      const float mean = s1 * inv_n;
      float var = s2 * inv_n - mean * mean;
      var = var < 0.f ? 0.f : var;
      const float rstd = rsqrtf(var + a.eps);
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
        const int f0 = rt * 16 + 4 * g;
        const f32x4 gm = *reinterpret_cast<const f32x4*>(b2v + D + f0), bt = *reinterpret_cast<const f32x4*>(b2v + 2 * D + f0);
        acc2[rt] = (acc2[rt] - mean) * rstd * gm + bt;
      }
      if (!a.out_pos) {
        if (st) {
#pragma unroll
          for (int rt = 0; rt < NRT; ++rt)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc2[rt]), o_rs, row_g, rt * 64, 0);
        }
      } else {  // the next layer's hidden + pos: the pos rows of pair h0 + 2 are loaded before the stores of pair h0
        const __amdgpu_buffer_rsrc_t p_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.pos, 0, (int)(a.pos_rows * D * 4), 0x00020000);
        const __amdgpu_buffer_rsrc_t q_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.out_pos, 0, (int)(a.M * D * 4), 0x00020000);
        const unsigned prow = tok_ok ? (unsigned)(((tk % a.pos_rows) * D + 4 * g) * 4) : kOob;
        f32x4 pv[2][kEB];
#pragma unroll
        for (int i = 0; i < kEB; ++i)
          pv[0][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(p_rs, prow, i * 64, 0));
#pragma unroll
        for (int h0 = 0; h0 < NRT; h0 += kEB) {
          const int b = (h0 / kEB) & 1;
          if (h0 + kEB < NRT) {
#pragma unroll
            for (int i = 0; i < kEB; ++i)
              pv[b ^ 1][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(p_rs, prow, (h0 + kEB + i) * 64, 0));
          }
          if (st) {
#pragma unroll
            for (int i = 0; i < kEB; ++i)
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc2[h0 + i]), o_rs, row_g, (h0 + i) * 64, 0);
#pragma unroll
            for (int i = 0; i < kEB; ++i)
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc2[h0 + i] + pv[b][i]), q_rs, row_g, (h0 + i) * 64, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    if (it + 1 < n_iter) issue_w(w1_rs, w1_src(0, 0), 0);
    sg_barrier();  // the next turn's first panel has landed; every wave is done with both slots
  }
}

using sg_kernel_t = void (*)(SgArgs);

// the instance of (N == 288, epilogue) with P pieces; PIPE applies to the LayerNorm epilogue alone
template <bool PIPE, int ABL, int P = 3>
sg_kernel_t sg_pick(bool n288, int epi) {
  if (n288) return epi == 2 ? token_gemm_split_kernel<18, 2, PIPE, ABL, P> : (epi == 1 ? token_gemm_split_kernel<18, 1, true, ABL, P> : token_gemm_split_kernel<18, 0, true, ABL, P>);
  return epi == 2 ? token_gemm_split_kernel<16, 2, PIPE, ABL, P> : (epi == 1 ? token_gemm_split_kernel<16, 1, true, ABL, P> : token_gemm_split_kernel<16, 0, true, ABL, P>);
}

int device_cu_count(int* n_cu) {
  static int cached = 0;
  if (cached == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
    cached = prop.multiProcessorCount;
  }
  *n_cu = cached;
  return 0;
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_token_linear_split_weight(const void* w, void* w_split, int N, int K, void* stream) {
  const char* who = "wm2f_token_linear_split_weight";
  WM2F_REQUIRE(w && w_split, "%s: null pointer", who);
  WM2F_REQUIRE(N > 0 && K > 0 && N % 16 == 0 && K % kKStep == 0, "%s: N = %d must be a multiple of 16 and K = %d of %d", who, N, K, kKStep);
  WM2F_REQUIRE((int64_t)N * K * 6 < (1ll << 31), "%s: the split weight must stay below 2 GiB", who);
  const int total = N * (K / 8);
  hipLaunchKernelGGL(split_weight_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)w,
                     (bf16x8*)w_split, N, K);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_token_linear_split_weight_rows(const void* w, void* w_split, int N, int K, int row_order, void* stream) {
  const char* who = "wm2f_token_linear_split_weight_rows";
  WM2F_REQUIRE(row_order == WM2F_ROWS_NATURAL || row_order == WM2F_ROWS_FFN, "%s: row_order = %d (0: natural, 1: the fused feed-forward's)", who, row_order);
  if (row_order == WM2F_ROWS_NATURAL) return wm2f_token_linear_split_weight(w, w_split, N, K, stream);
  WM2F_REQUIRE(w && w_split, "%s: null pointer", who);
  WM2F_REQUIRE(N > 0 && K > 0 && N % 32 == 0 && K % kKStep == 0, "%s: N = %d and K = %d must be multiples of %d", who, N, K, kKStep);
  WM2F_REQUIRE((int64_t)N * K * 6 < (1ll << 31), "%s: the split weight must stay below 2 GiB", who);
  const int total = N * (K / 8);
  hipLaunchKernelGGL(split_weight_rows_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)w,
                     (bf16x8*)w_split, N, K);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_token_ffn_row(int n) { return n >= 0 ? ffn_row_of(n) : -1; }

// pieces = P of the kernel (3: wm2f_token_ffn_split_fwd)
static int token_ffn_launch(const char* who, const void* x, const void* w1_split, const void* b1, const void* w2_split,
                            const void* b2, const void* residual, const void* ln_gamma, const void* ln_beta, const void* pos,
                            void* out, void* out_plus_pos, int64_t M, int K, int F, int N, int64_t pos_rows, float eps,
                            int pieces, void* stream) {
  WM2F_REQUIRE(pieces >= 1 && pieces <= 3, "%s: pieces = %d (1, 2 and 3 are built)", who, pieces);
  WM2F_REQUIRE(x && w1_split && b1 && w2_split && b2 && out, "%s: null pointer", who);
  WM2F_REQUIRE(residual && ln_gamma && ln_beta, "%s: the residual and the LayerNorm (gamma and beta) are part of the kernel", who);
  WM2F_REQUIRE(M > 0, "%s: non-positive size", who);
  WM2F_REQUIRE(K == 256 && N == 256, "%s: K = %d, N = %d (256 and 256 are built)", who, K, N);
  WM2F_REQUIRE(F == 256 || F == 512 || F == 768 || F == 1024, "%s: F = %d is not built (256, 512, 768 and 1024 are)", who, F);
  WM2F_REQUIRE(M * (int64_t)256 * 4 < (1ll << 31), "%s: x / out must stay below 2 GiB (32-bit buffer offsets)", who);
  WM2F_REQUIRE((pos == nullptr) == (out_plus_pos == nullptr), "%s: pos and out_plus_pos come together", who);
  WM2F_REQUIRE(!pos || (pos_rows > 0 && pos_rows * (int64_t)256 * 4 < (1ll << 31)), "%s: pos needs pos_rows >= 1 and must stay below 2 GiB", who);
  int n_cu = 0;
  if (device_cu_count(&n_cu) != 0) {
    set_error("%s: cannot query the device", who);
    return WM2F_ELAUNCH;
  }
  FfnArgs a;
  a.x = (const float*)x;
  a.w1s = w1_split;
  a.w2s = w2_split;
  a.b1 = (const float*)b1;
  a.b2 = (const float*)b2;
  a.residual = (const float*)residual;
  a.gamma = (const float*)ln_gamma;
  a.beta = (const float*)ln_beta;
  a.pos = (const float*)pos;
  a.out = (float*)out;
  a.out_pos = (float*)out_plus_pos;
  a.M = M;
  a.F = F;
  a.pos_rows = pos_rows;
  a.eps = eps;
  a.tiles_total = (int)ceil_div64(M, 16);
  int grid = n_cu;
  if (grid > a.tiles_total) grid = a.tiles_total;
  const size_t lds = (size_t)2 * 16 * pieces * kFrag + (size_t)(F + 3 * 256) * sizeof(float);
  void (*kfn)(FfnArgs) = pieces == 3 ? token_ffn_split_kernel<0> : (pieces == 2 ? token_ffn_split_kernel<0, 2> : token_ffn_split_kernel<0, 1>);
#ifdef WM2F_PROFILING
  {  // WM2F_FFN_ABL = 1 / 4: the kernel without its epilogue stores / without its MFMAs (OUTPUTS NOT VALID)
    const char* ea = getenv("WM2F_FFN_ABL");
    const int abl = ea ? atoi(ea) : 0;
    WM2F_REQUIRE(abl == 0 || abl == 1 || abl == 4, "%s: WM2F_FFN_ABL = %d is not built (1 and 4 are)", who, abl);
    WM2F_REQUIRE(pieces == 3 || abl == 0, "%s: WM2F_FFN_ABL is built for three pieces", who);
    if (abl == 1) kfn = token_ffn_split_kernel<kAblStores>;
    if (abl == 4) kfn = token_ffn_split_kernel<kAblMfma>;
  }
#endif
  hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    set_error("%s: cannot raise dynamic LDS to %zu: %s", who, lds, hipGetErrorString(e));
    return WM2F_ELAUNCH;
  }
  hipLaunchKernelGGL(kfn, dim3(grid), dim3(kSgThreads), lds, (hipStream_t)stream, a);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_token_ffn_split_fwd(const void* x, const void* w1_split, const void* b1, const void* w2_split, const void* b2,
                                        const void* residual, const void* ln_gamma, const void* ln_beta, const void* pos,
                                        void* out, void* out_plus_pos, int64_t M, int K, int F, int N, int64_t pos_rows,
                                        float eps, void* stream) {
  return token_ffn_launch("wm2f_token_ffn_split_fwd", x, w1_split, b1, w2_split, b2, residual, ln_gamma, ln_beta, pos, out,
                          out_plus_pos, M, K, F, N, pos_rows, eps, 3, stream);
}

extern "C" int wm2f_token_ffn_split_fwd_p(const void* x, const void* w1_split, const void* b1, const void* w2_split,
                                          const void* b2, const void* residual, const void* ln_gamma, const void* ln_beta,
                                          const void* pos, void* out, void* out_plus_pos, int64_t M, int K, int F, int N,
                                          int64_t pos_rows, float eps, int pieces, void* stream) {
  return token_ffn_launch("wm2f_token_ffn_split_fwd_p", x, w1_split, b1, w2_split, b2, residual, ln_gamma, ln_beta, pos, out,
                          out_plus_pos, M, K, F, N, pos_rows, eps, pieces, stream);
}

// pieces = P of the kernel (3: wm2f_token_linear_split_fwd)
static int token_split_launch(const char* who, const void* x, const void* w_split, const void* bias, const void* residual,
                              const void* ln_gamma, const void* ln_beta, const void* pos, void* out, void* out_plus_pos,
                              int64_t M, int K, int N, int relu, int64_t pos_rows, float eps, int out_group, int pieces,
                              void* stream) {
  WM2F_REQUIRE(pieces >= 1 && pieces <= 3, "%s: pieces = %d (1, 2 and 3 are built)", who, pieces);
  WM2F_REQUIRE(x && w_split && bias && out, "%s: null pointer", who);
  WM2F_REQUIRE(M > 0 && K > 0 && N > 0, "%s: non-positive size", who);
  WM2F_REQUIRE(N == 256 || N == 288 || N == 512 || N == 768 || N == 1024,
               "%s: N = %d is not built (256, 288 and multiples of 256 up to 1024 are)", who, N);
  WM2F_REQUIRE(K % kKStep == 0, "%s: K = %d must be a multiple of %d", who, K, kKStep);
  WM2F_REQUIRE(M * (int64_t)K * 4 < (1ll << 31) && M * (int64_t)N * 4 < (1ll << 31), "%s: x / out must stay below 2 GiB (32-bit buffer offsets)", who);
  WM2F_REQUIRE((int64_t)N * K * 6 < (1ll << 31), "%s: the split weight must stay below 2 GiB", who);
  WM2F_REQUIRE(pos_rows * (int64_t)N * 4 < (1ll << 31), "%s: pos must stay below 2 GiB", who);
  WM2F_REQUIRE((ln_gamma == nullptr) == (ln_beta == nullptr), "%s: LayerNorm needs both gamma and beta", who);
  WM2F_REQUIRE(!ln_gamma || N <= 288, "%s: the LayerNorm epilogue needs N <= 288 (one feature slice per token)", who);
  WM2F_REQUIRE(!residual || ln_gamma, "%s: the residual belongs to the LayerNorm epilogue", who);
  WM2F_REQUIRE(!out_plus_pos || (pos && ln_gamma && pos_rows > 0), "%s: out_plus_pos needs pos, pos_rows and the LayerNorm epilogue", who);
  WM2F_REQUIRE(out_group == 0 || (out_group > 0 && out_group % 4 == 0 && N % out_group == 0 && !ln_gamma),
               "%s: out_group = %d must divide N, be a multiple of 4 and exclude the LayerNorm epilogue", who, out_group);
  int n_cu = 0;
  if (device_cu_count(&n_cu) != 0) {
    set_error("%s: cannot query the device", who);
    return WM2F_ELAUNCH;
  }
  SgArgs a;
  a.x = (const float*)x;
  a.ws = w_split;
  a.bias = (const float*)bias;
  a.residual = (const float*)residual;
  a.gamma = (const float*)ln_gamma;
  a.beta = (const float*)ln_beta;
  a.pos = (const float*)pos;
  a.out = (float*)out;
  a.out_pos = (float*)out_plus_pos;
  a.M = M;
  a.K = K;
  a.N = N;
  a.relu = relu;
  a.out_group = out_group;
  a.pos_rows = pos_rows;
  a.eps = eps;
  a.tiles_total = (int)ceil_div64(M, 16);
  int grid = n_cu;
  if (grid > a.tiles_total) grid = a.tiles_total;
  const int nrt = N == 288 ? 18 : 16;
  const size_t lds = (size_t)2 * nrt * pieces * kFrag + (size_t)3 * N * sizeof(float);
  const int epi = ln_gamma ? 2 : (out_group > 0 ? 1 : 0);
  sg_kernel_t kfn = pieces == 3 ? sg_pick<true, 0>(N == 288, epi)
                                : (pieces == 2 ? sg_pick<true, 0, 2>(N == 288, epi) : sg_pick<true, 0, 1>(N == 288, epi));
#ifdef WM2F_PROFILING
  {  // WM2F_TGS_OPT = 0: the LayerNorm epilogue with its loads one batch at a time, as before §13.2 (valid outputs, the
     // same bits); WM2F_TGS_ABL = 1 / 2 / 4: the shipped kernel without epilogue stores / epilogue loads / MFMAs
     // (OUTPUTS NOT VALID)
    const char* eo = getenv("WM2F_TGS_OPT");
    const char* ea = getenv("WM2F_TGS_ABL");
    const int abl = ea ? atoi(ea) : 0;
    WM2F_REQUIRE(pieces == 3 || (!eo && abl == 0), "%s: WM2F_TGS_OPT / WM2F_TGS_ABL are built for three pieces", who);
    if (abl != 0) {
      WM2F_REQUIRE(abl == 1 || abl == 2 || abl == 4, "%s: WM2F_TGS_ABL = %d is not built (1, 2, 4 are)", who, abl);
      WM2F_REQUIRE(!eo, "%s: WM2F_TGS_ABL ablates the shipped kernel only (unset WM2F_TGS_OPT)", who);
      kfn = abl == 1 ? sg_pick<true, 1>(N == 288, epi) : (abl == 2 ? sg_pick<true, 2>(N == 288, epi) : sg_pick<true, 4>(N == 288, epi));
    } else if (eo) {
      const int opt = atoi(eo);
      WM2F_REQUIRE(opt == 0 || opt == 1, "%s: WM2F_TGS_OPT = %d is not built (0 and 1 are)", who, opt);
      if (opt == 0) kfn = sg_pick<false, 0>(N == 288, epi);
    }
  }
#endif
  hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    set_error("%s: cannot raise dynamic LDS to %zu: %s", who, lds, hipGetErrorString(e));
    return WM2F_ELAUNCH;
  }
  hipLaunchKernelGGL(kfn, dim3(grid), dim3(kSgThreads), lds, (hipStream_t)stream, a);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_token_linear_split_fwd(const void* x, const void* w_split, const void* bias, const void* residual,
                                           const void* ln_gamma, const void* ln_beta, const void* pos, void* out,
                                           void* out_plus_pos, int64_t M, int K, int N, int relu, int64_t pos_rows, float eps,
                                           int out_group, void* stream) {
  return token_split_launch("wm2f_token_linear_split_fwd", x, w_split, bias, residual, ln_gamma, ln_beta, pos, out, out_plus_pos,
                            M, K, N, relu, pos_rows, eps, out_group, 3, stream);
}

extern "C" int wm2f_token_linear_split_fwd_p(const void* x, const void* w_split, const void* bias, const void* residual,
                                             const void* ln_gamma, const void* ln_beta, const void* pos, void* out,
                                             void* out_plus_pos, int64_t M, int K, int N, int relu, int64_t pos_rows, float eps,
                                             int out_group, int pieces, void* stream) {
  return token_split_launch("wm2f_token_linear_split_fwd_p", x, w_split, bias, residual, ln_gamma, ln_beta, pos, out,
                            out_plus_pos, M, K, N, relu, pos_rows, eps, out_group, pieces, stream);
}
