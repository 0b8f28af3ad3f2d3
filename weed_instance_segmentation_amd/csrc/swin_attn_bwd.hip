// Backward of the Swin backbone's shifted-window attention (include/wm2f.h: wm2f_swin_window_attn_bwd), the mirror of
// swin_attn.hip under the same geometry contract.  Work unit: one (image, window, head) "pair"; the workgroup split is the
// forward's (ws 4: 4 pairs x 1 wave, ws 7: 1 pair x 4 waves, ws 12: 1 pair x 3 waves).  Every real token belongs to one window,
// so a pair owns all of its queries AND all of its keys: grad_q / grad_k / grad_v are complete inside the workgroup and leave
// with plain vector stores; nothing of size L x L goes to HBM.
//
// Per pair the window's K, V, Q and dO rows are gathered once into LDS (padding keys: k_pad / v_pad; padding queries: zero dO
// and lse = +inf, which makes their P, dP, delta and dS exactly 0), then two passes recompute S with the forward's arithmetic:
//   pass A, a wave owns 16 QUERIES (C column = query, rows = keys, the forward's layout) and holds their whole score column:
//     S^T = K Q^T, dP^T = V dO^T, P = exp(S - lse), delta = sum_keys P dP, dS = P (dP - delta)
//     dQ^T = K^T dS^T (dS^T is already the B operand); dS is also summed into the wave's relative-offset bins (LDS)
//   pass B, a wave owns 16 KEYS (C column = key, rows = queries) and walks the query tiles, one tile live at a time:
//     S = Q K^T, dP = dO V^T, P, dS with pass A's delta;  dV^T += dO^T P,  dK^T += Q^T dS  (P / dS are the B operands)
// S is computed twice so that no accumulator tile is ever transposed: 2 x the cheapest product instead of an L x L round trip
// through LDS.  delta comes from P and dP, not from the saved output: no extra read, and in the bf16 form the saved output is
// rounded to bf16 while P and dP are fp32 here.
//
// Bias-table gradient: for one key the 16 queries of a tile fall into 16 different offsets, so the lanes of ONE lane group g
// never collide; the four groups add in turn (ds_add_f32 into the wave's own bin array; one wave's LDS operations complete in
// program order), the waves' arrays are added in wave order, the pair's (2 ws - 1)^2 sums go to the workspace and a second
// kernel adds the pairs in a fixed order.  dK / dV of padding slots (the k / v Linear's bias gradient) take the same road.
// No float atomics to global memory; every sum has one order, so two runs give the same bits.
//
// fp32 form: v_mfma_f32_16x16x4_f32.  bf16 form: v_mfma_f32_16x16x16_bf16, fp32 S / P / dS / accumulators, P and dS rounded to
// bf16 once where they become MFMA operands; Q, K and dO are also stored transposed in LDS (the A operands of the products
// that contract over slots).
#include "common.h"

#include <type_traits>

namespace wm2f {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));

constexpr int kInvalidKey = 1 << 30;  // slot table flag: a slot beyond L (the tile padding inside the kernel)
constexpr int kRedSlices = 16;        // reduce kernel: pair slices per output, added in slice order

template <int WS>
struct SwinBwdGeom {
  static constexpr int L = WS * WS, LT = (L + 15) / 16, LP = LT * 16;
  static constexpr int NB = (2 * WS - 1) * (2 * WS - 1), NBP = (NB + 3) / 4 * 4;
  static constexpr int PAIRS = WS == 4 ? 4 : 1;
  static constexpr int WPP = WS == 4 ? 1 : (WS == 7 ? 4 : 3);  // waves per pair
};

template <int WS, int D, int PAIRS, int WPP>
struct alignas(16) SwinBwdSmemF32 {
  static constexpr int LP = SwinBwdGeom<WS>::LP, NBP = SwinBwdGeom<WS>::NBP;
  float k[PAIRS][LP][D + 4];  // + 4: rows 16 bytes apart in the bank row
  float v[PAIRS][LP][D + 4];
  float q[PAIRS][LP][D + 4];
  float go[PAIRS][LP][D + 4];
  float bias[PAIRS][NBP];
  float bins[PAIRS][WPP][NBP];
  float padacc[PAIRS][WPP][2 * D];
  float lse[PAIRS][LP];    // +inf: not a real query
  float delta[PAIRS][LP];
  int kinfo[PAIRS][LP];    // i * (2 ws - 1) + j  |  region << 16  |  kInvalidKey
  int tok[PAIRS][LP];      // token index in the image, -1 = padding token, -2 = no slot
};

template <int WS, int D, int PAIRS, int WPP>
struct alignas(16) SwinBwdSmemBf16 {
  static constexpr int LP = SwinBwdGeom<WS>::LP, NBP = SwinBwdGeom<WS>::NBP;
  uint16_t k[PAIRS][LP][D + 8];
  uint16_t v[PAIRS][LP][D + 8];
  uint16_t q[PAIRS][LP][D + 8];
  uint16_t go[PAIRS][LP][D + 8];
  uint16_t kt[PAIRS][D][LP + 8];   // transposed: [d][slot]
  uint16_t qt[PAIRS][D][LP + 8];
  uint16_t got[PAIRS][D][LP + 8];
  float bias[PAIRS][NBP];
  float bins[PAIRS][WPP][NBP];
  float padacc[PAIRS][WPP][2 * D];
  float lse[PAIRS][LP];
  float delta[PAIRS][LP];
  int kinfo[PAIRS][LP];
  int tok[PAIRS][LP];
};

// C[4 g + r][n] = sum_d a_row(4 g + r)[d] * b_row(n)[d]: `a` / `b` are THIS lane's rows (row index lane & 15) of the A / B
// operand.  The lane group g takes the same d of both rows, so any split of d over (g, step) is a valid contraction.
template <int D>
__device__ __forceinline__ f32x4 dot_rows(const float* a, const float* b, int g) {
  constexpr int DK = D / 4;
  f32x4 c = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < DK; t += 4) {
    const float4 x = *reinterpret_cast<const float4*>(a + DK * g + t);
    const float4 y = *reinterpret_cast<const float4*>(b + DK * g + t);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, y.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, y.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, y.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, y.w, c, 0, 0, 0);
  }
  return c;
}

template <int D>
__device__ __forceinline__ f32x4 dot_rows(const uint16_t* a, const uint16_t* b, int g) {
  f32x4 c = (f32x4){0.f, 0.f, 0.f, 0.f};
  if constexpr (D == 32) {
    const s16x8 x = *reinterpret_cast<const s16x8*>(a + 8 * g), y = *reinterpret_cast<const s16x8*>(b + 8 * g);
    c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_shufflevector(x, x, 0, 1, 2, 3),
                                                  __builtin_shufflevector(y, y, 0, 1, 2, 3), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_shufflevector(x, x, 4, 5, 6, 7),
                                                  __builtin_shufflevector(y, y, 4, 5, 6, 7), c, 0, 0, 0);
  } else {
    c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(*reinterpret_cast<const s16x4*>(a + 4 * g),
                                                  *reinterpret_cast<const s16x4*>(b + 4 * g), c, 0, 0, 0);
  }
  return c;
}

__device__ __forceinline__ s16x4 pack_bf16(f32x4 x) {
  bf16x4_t p;
#pragma unroll
  for (int r = 0; r < 4; ++r) p[r] = (__bf16)x[r];
  return __builtin_bit_cast(s16x4, p);
}

template <typename T, int WS, int D>
__global__ __launch_bounds__(SwinBwdGeom<WS>::PAIRS* SwinBwdGeom<WS>::WPP* kWave) void swin_window_attn_bwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ k_pad,
    const T* __restrict__ v_pad, const float* __restrict__ bias_table, const float* __restrict__ lse,
    const T* __restrict__ grad_out, T* __restrict__ grad_q, T* __restrict__ grad_k, T* __restrict__ grad_v,
    float* __restrict__ part_bias, float* __restrict__ part_pad, int H, int W, int heads, int shift, int nWy, int nWx,
    int total_pairs, float scale) {
  using G = SwinBwdGeom<WS>;
  constexpr bool BF16 = std::is_same<T, uint16_t>::value;
  constexpr int L = G::L, LT = G::LT, LP = G::LP, NB = G::NB, NBP = G::NBP, PAIRS = G::PAIRS, WPP = G::WPP;
  constexpr int NT = WPP * kWave;  // threads of one pair
  constexpr int DT = D / 16;       // 16-row tiles of a transposed (d-major) result
  constexpr int R = 2 * WS - 1;
  using Smem = typename std::conditional<BF16, SwinBwdSmemBf16<WS, D, PAIRS, WPP>, SwinBwdSmemF32<WS, D, PAIRS, WPP>>::type;
  __shared__ Smem sm;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, n = lane & 15;
  const int pl = wave / WPP;             // pair of this wave inside the workgroup
  const int wv = wave - pl * WPP;        // wave inside the pair
  const int tp = threadIdx.x - pl * NT;  // thread inside the pair
  int pair = blockIdx.x * PAIRS + pl;
  const bool live = pair < total_pairs;  // idle waves of the last ws 4 workgroup replay the last pair and store nothing
  if (!live) pair = total_pairs - 1;
  const int head = pair % heads;
  const int wb = pair / heads;
  const int nW = nWy * nWx;
  const int win = wb % nW, b = wb / nW;
  const int wy = win / nWx, wx = win - wy * nWx;
  const int Hp = nWy * WS, Wp = nWx * WS;
  const int E = heads * D;
  const int64_t img = (int64_t)b * H * W;
  const float* lse_row = lse + ((int64_t)b * heads + head) * H * W;

  // ---- slot tables, the head's bias column, cleared bins
  for (int s = tp; s < LP; s += NT) {
    int tk = -2, info = kInvalidKey;
    if (s < L) {
      const int i = s / WS, j = s - i * WS;
      const int r = wy * WS + i, c = wx * WS + j;  // rolled-frame coordinates
      int region = 0;
      if (shift > 0) region = 3 * ((r >= Hp - WS) + (r >= Hp - shift)) + ((c >= Wp - WS) + (c >= Wp - shift));
      int py = r + shift, px = c + shift;
      if (py >= Hp) py -= Hp;
      if (px >= Wp) px -= Wp;
      tk = (py < H && px < W) ? py * W + px : -1;
      info = (i * R + j) | (region << 16);
    }
    sm.tok[pl][s] = tk;
    sm.kinfo[pl][s] = info;
    sm.lse[pl][s] = tk >= 0 ? lse_row[tk] : INFINITY;
  }
  for (int t = tp; t < NB; t += NT) sm.bias[pl][t] = bias_table[(int64_t)t * heads + head];
  for (int t = tp; t < WPP * NBP; t += NT) (&sm.bins[pl][0][0])[t] = 0.f;
  __syncthreads();

  // ---- gather the window's K, V, Q, dO rows: by token, 16 bytes per lane
  if constexpr (!BF16) {
    constexpr int CH = D / 4;
    for (int idx = tp; idx < LP * CH; idx += NT) {
      const int s = idx / CH, c = idx - s * CH;
      const int tk = sm.tok[pl][s];
      float4 kx = make_float4(0.f, 0.f, 0.f, 0.f), vx = kx, qx = kx, gx = kx;
      if (tk >= 0) {
        const int64_t off = (img + tk) * E + head * D + 4 * c;
        kx = *reinterpret_cast<const float4*>(k + off);
        vx = *reinterpret_cast<const float4*>(v + off);
        qx = *reinterpret_cast<const float4*>(q + off);
        gx = *reinterpret_cast<const float4*>(grad_out + off);
      } else if (tk == -1) {
        if (k_pad != nullptr) kx = *reinterpret_cast<const float4*>(k_pad + head * D + 4 * c);
        if (v_pad != nullptr) vx = *reinterpret_cast<const float4*>(v_pad + head * D + 4 * c);
      }
      *reinterpret_cast<float4*>(&sm.k[pl][s][4 * c]) = kx;
      *reinterpret_cast<float4*>(&sm.v[pl][s][4 * c]) = vx;
      *reinterpret_cast<float4*>(&sm.q[pl][s][4 * c]) = qx;
      *reinterpret_cast<float4*>(&sm.go[pl][s][4 * c]) = gx;
    }
  } else {
    constexpr int CH = D / 8;
    for (int idx = tp; idx < LP * CH; idx += NT) {
      const int s = idx / CH, c = idx - s * CH;
      const int tk = sm.tok[pl][s];
      s16x8 kx = (s16x8){0, 0, 0, 0, 0, 0, 0, 0}, vx = kx, qx = kx, gx = kx;
      if (tk >= 0) {
        const int64_t off = (img + tk) * E + head * D + 8 * c;
        kx = *reinterpret_cast<const s16x8*>(k + off);
        vx = *reinterpret_cast<const s16x8*>(v + off);
        qx = *reinterpret_cast<const s16x8*>(q + off);
        gx = *reinterpret_cast<const s16x8*>(grad_out + off);
      } else if (tk == -1) {
        if (k_pad != nullptr) kx = *reinterpret_cast<const s16x8*>(k_pad + head * D + 8 * c);
        if (v_pad != nullptr) vx = *reinterpret_cast<const s16x8*>(v_pad + head * D + 8 * c);
      }
      *reinterpret_cast<s16x8*>(&sm.k[pl][s][8 * c]) = kx;
      *reinterpret_cast<s16x8*>(&sm.v[pl][s][8 * c]) = vx;
      *reinterpret_cast<s16x8*>(&sm.q[pl][s][8 * c]) = qx;
      *reinterpret_cast<s16x8*>(&sm.go[pl][s][8 * c]) = gx;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        sm.kt[pl][8 * c + e][s] = (uint16_t)kx[e];
        sm.qt[pl][8 * c + e][s] = (uint16_t)qx[e];
        sm.got[pl][8 * c + e][s] = (uint16_t)gx[e];
      }
    }
  }
  __syncthreads();

  // ---- pass A: the wave's query tiles.  dQ, delta, bias bins
  for (int qt = wv; qt < LT; qt += WPP) {
    const int qs = 16 * qt + n;            // < LP
    const int qtok = sm.tok[pl][qs];
    const int qinfo = sm.kinfo[pl][qs];    // a slot beyond L: offset 0, never used with a non-zero dS
    const int qoff = (qinfo & 0xffff) + (WS - 1) * R + (WS - 1);
    const int qreg = (qinfo >> 16) & 0xff;
    const float qlse = sm.lse[pl][qs];

    f32x4 s[LT], dp[LT];
    float dsum = 0.f;
#pragma unroll
    for (int kt = 0; kt < LT; ++kt) {
      s[kt] = dot_rows<D>(&sm.k[pl][16 * kt + n][0], &sm.q[pl][qs][0], g);
      dp[kt] = dot_rows<D>(&sm.v[pl][16 * kt + n][0], &sm.go[pl][qs][0], g);
      const int4 ki = *reinterpret_cast<const int4*>(&sm.kinfo[pl][16 * kt + 4 * g]);
      const int kin[4] = {ki.x, ki.y, ki.z, ki.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int info = kin[r];
        float bm = sm.bias[pl][qoff - (info & 0xffff)];
        if (((info >> 16) & 0xff) != qreg) bm += -100.0f;
        float x = s[kt][r] * scale + bm;
        if (info & kInvalidKey) x = -INFINITY;
        const float p = __expf(x - qlse);
        s[kt][r] = p;
        dsum += p * dp[kt][r];
      }
    }
    dsum += __shfl_xor(dsum, 16, kWave);
    dsum += __shfl_xor(dsum, 32, kWave);
    if (g == 0) sm.delta[pl][qs] = dsum;
#pragma unroll
    for (int kt = 0; kt < LT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) s[kt][r] *= dp[kt][r] - dsum;  // dS^T

    if (part_bias != nullptr) {
      float* bins = &sm.bins[pl][wv][0];
#pragma unroll 1
      for (int gg = 0; gg < 4; ++gg) {
        if (g == gg) {
#pragma unroll
          for (int kt = 0; kt < LT; ++kt) {
            const int4 ki = *reinterpret_cast<const int4*>(&sm.kinfo[pl][16 * kt + 4 * g]);
            const int kin[4] = {ki.x, ki.y, ki.z, ki.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) atomicAdd(&bins[qoff - (kin[r] & 0xffff)], s[kt][r]);
          }
        }
      }
    }

    f32x4 dq[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i) dq[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < LT; ++kt) {
      if constexpr (!BF16) {
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            dq[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(sm.k[pl][16 * kt + 4 * g + t][16 * i + n], s[kt][t], dq[i], 0, 0, 0);
      } else {
        const s16x4 db = pack_bf16(s[kt]);
#pragma unroll
        for (int i = 0; i < DT; ++i)
          dq[i] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
              *reinterpret_cast<const s16x4*>(&sm.kt[pl][16 * i + n][16 * kt + 4 * g]), db, dq[i], 0, 0, 0);
      }
    }
    // dQ^T: column = query n, rows d = 16 i + 4 g + r -> 4 consecutive channels of the query's own token
    if (live && qtok >= 0) {
      T* gp = grad_q + (img + qtok) * E + head * D + 4 * g;
#pragma unroll
      for (int i = 0; i < DT; ++i) {
        const f32x4 x = dq[i] * scale;
        if constexpr (!BF16) *reinterpret_cast<float4*>(gp + 16 * i) = make_float4(x[0], x[1], x[2], x[3]);
        else *reinterpret_cast<s16x4*>(gp + 16 * i) = pack_bf16(x);
      }
    }
  }
  __syncthreads();

  // ---- pass B: the wave's key tiles.  dK, dV and their sums over padding slots
  f32x4 padk[DT], padv[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) padk[i] = padv[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int kt = wv; kt < LT; kt += WPP) {
    const int ks = 16 * kt + n;
    const int ktok = sm.tok[pl][ks];
    const int kinf = sm.kinfo[pl][ks];
    const int koff = kinf & 0xffff, kreg = (kinf >> 16) & 0xff;
    const bool kvalid = !(kinf & kInvalidKey);
    f32x4 dk[DT], dv[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i) dk[i] = dv[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int qt = 0; qt < LT; ++qt) {
      f32x4 p = dot_rows<D>(&sm.q[pl][16 * qt + n][0], &sm.k[pl][ks][0], g);    // S: column = key, rows = queries
      f32x4 ds = dot_rows<D>(&sm.go[pl][16 * qt + n][0], &sm.v[pl][ks][0], g);  // dP
      const int4 qi = *reinterpret_cast<const int4*>(&sm.kinfo[pl][16 * qt + 4 * g]);
      const float4 ql = *reinterpret_cast<const float4*>(&sm.lse[pl][16 * qt + 4 * g]);
      const float4 qd = *reinterpret_cast<const float4*>(&sm.delta[pl][16 * qt + 4 * g]);
      const int qin[4] = {qi.x, qi.y, qi.z, qi.w};
      const float qls[4] = {ql.x, ql.y, ql.z, ql.w}, qde[4] = {qd.x, qd.y, qd.z, qd.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int info = qin[r];
        float bm = sm.bias[pl][(info & 0xffff) + (WS - 1) * R + (WS - 1) - koff];
        if (((info >> 16) & 0xff) != kreg) bm += -100.0f;
        float x = p[r] * scale + bm;
        if (!kvalid) x = -INFINITY;
        const float e = __expf(x - qls[r]);
        p[r] = e;
        ds[r] = e * (ds[r] - qde[r]);
      }
      if constexpr (!BF16) {
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            dv[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(sm.go[pl][16 * qt + 4 * g + t][16 * i + n], p[t], dv[i], 0, 0, 0);
            dk[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(sm.q[pl][16 * qt + 4 * g + t][16 * i + n], ds[t], dk[i], 0, 0, 0);
          }
      } else {
        const s16x4 pb = pack_bf16(p), db = pack_bf16(ds);
#pragma unroll
        for (int i = 0; i < DT; ++i) {
          dv[i] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
              *reinterpret_cast<const s16x4*>(&sm.got[pl][16 * i + n][16 * qt + 4 * g]), pb, dv[i], 0, 0, 0);
          dk[i] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
              *reinterpret_cast<const s16x4*>(&sm.qt[pl][16 * i + n][16 * qt + 4 * g]), db, dk[i], 0, 0, 0);
        }
      }
    }
    // dK^T / dV^T: column = key n, rows d = 16 i + 4 g + r
    const int64_t krow = (img + (ktok >= 0 ? ktok : 0)) * E + head * D + 4 * g;
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const f32x4 xk = dk[i] * scale, xv = dv[i];
      if (live && ktok >= 0) {
        if constexpr (!BF16) {
          *reinterpret_cast<float4*>(grad_k + krow + 16 * i) = make_float4(xk[0], xk[1], xk[2], xk[3]);
          *reinterpret_cast<float4*>(grad_v + krow + 16 * i) = make_float4(xv[0], xv[1], xv[2], xv[3]);
        } else {
          *reinterpret_cast<s16x4*>(grad_k + krow + 16 * i) = pack_bf16(xk);
          *reinterpret_cast<s16x4*>(grad_v + krow + 16 * i) = pack_bf16(xv);
        }
      }
      if (part_pad != nullptr) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float a = ktok == -1 ? xk[r] : 0.f, c = ktok == -1 ? xv[r] : 0.f;
#pragma unroll
          for (int m = 1; m < 16; m <<= 1) {
            a += __shfl_xor(a, m, kWave);
            c += __shfl_xor(c, m, kWave);
          }
          padk[i][r] += a;
          padv[i][r] += c;
        }
      }
    }
  }
  if (part_pad != nullptr && n == 0) {
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sm.padacc[pl][wv][16 * i + 4 * g + r] = padk[i][r];
        sm.padacc[pl][wv][D + 16 * i + 4 * g + r] = padv[i][r];
      }
  }
  __syncthreads();

  // ---- the pair's partial sums: waves added in wave order
  if (live) {
    if (part_bias != nullptr) {
      for (int t = tp; t < NB; t += NT) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < WPP; ++w) a += sm.bins[pl][w][t];
        part_bias[(int64_t)pair * NB + t] = a;
      }
    }
    if (part_pad != nullptr) {
      for (int t = tp; t < 2 * D; t += NT) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < WPP; ++w) a += sm.padacc[pl][w][t];
        part_pad[(int64_t)pair * 2 * D + t] = a;
      }
    }
  }
}

// out(head, t) = sum over the nwb (image, window) units of part[(unit * heads + head) * n + t]: kRedSlices interleaved
// slices per output, each added in unit order, then the slices in slice order.  mode 0: the bias table, out0[t * heads +
// head].  mode 1: t = which * D + d, (which ? out1 : out0)[head * D + d], either may be null.
__global__ __launch_bounds__(64 * kRedSlices) void swin_bwd_reduce_kernel(const float* __restrict__ part,
                                                                          float* __restrict__ out0, float* __restrict__ out1,
                                                                          int nwb, int heads, int n, int D, int mode) {
  __shared__ float red[kRedSlices][64];
  const int t = blockIdx.x * 64 + threadIdx.x, head = blockIdx.y, sl = threadIdx.y;
  float a = 0.f;
  if (t < n)
    for (int u = sl; u < nwb; u += kRedSlices) a += part[((int64_t)u * heads + head) * n + t];
  red[sl][threadIdx.x] = a;
  __syncthreads();
  if (sl == 0 && t < n) {
    float x = 0.f;
#pragma unroll
    for (int i = 0; i < kRedSlices; ++i) x += red[i][threadIdx.x];
    if (mode == 0) {
      out0[(int64_t)t * heads + head] = x;
    } else {
      float* o = t < D ? out0 : out1;
      if (o != nullptr) o[head * D + (t < D ? t : t - D)] = x;
    }
  }
}

template <typename T, int WS, int D>
void launch_swin_bwd(const void* q, const void* k, const void* v, const void* k_pad, const void* v_pad, const void* bias_table,
                     const void* lse, const void* grad_out, void* grad_q, void* grad_k, void* grad_v, float* part_bias,
                     float* part_pad, int H, int W, int heads, int shift, int nWy, int nWx, int total_pairs, hipStream_t st) {
  using G = SwinBwdGeom<WS>;
  const float scale = 1.0f / sqrtf((float)D);
  hipLaunchKernelGGL((swin_window_attn_bwd_kernel<T, WS, D>), dim3(ceil_div(total_pairs, G::PAIRS)),
                     dim3(G::PAIRS * G::WPP * kWave), 0, st, (const T*)q, (const T*)k, (const T*)v, (const T*)k_pad,
                     (const T*)v_pad, (const float*)bias_table, (const float*)lse, (const T*)grad_out, (T*)grad_q, (T*)grad_k,
                     (T*)grad_v, part_bias, part_pad, H, W, heads, shift, nWy, nWx, total_pairs, scale);
}

bool swin_bwd_built(int ws, int D) { return (ws == 4 || ws == 7 || ws == 12) && (D == 16 || D == 32); }

}  // namespace

}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_swin_window_attn_bwd_workspace(int B, int H, int W, int heads, int D, int ws) {
  if (B <= 0 || H <= 0 || W <= 0 || heads <= 0 || !swin_bwd_built(ws, D)) return 0;
  const int64_t pairs = (int64_t)B * ceil_div(H, ws) * ceil_div(W, ws) * heads;
  const int64_t nb = (int64_t)(2 * ws - 1) * (2 * ws - 1);
  return pairs * (nb + 2 * D) * (int64_t)sizeof(float);
}

extern "C" int wm2f_swin_window_attn_bwd(const void* q, const void* k, const void* v, const void* k_pad, const void* v_pad,
                                         const void* bias_table, const void* lse, const void* grad_out, void* grad_q,
                                         void* grad_k, void* grad_v, void* grad_k_pad, void* grad_v_pad, void* grad_bias_table,
                                         void* workspace, int B, int H, int W, int heads, int D, int ws, int shift, int dtype,
                                         void* stream) {
  const char* who = "wm2f_swin_window_attn_bwd";
  WM2F_REQUIRE(q && k && v && bias_table && lse && grad_out && grad_q && grad_k && grad_v, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && heads > 0, "%s: non-positive size", who);
  WM2F_REQUIRE(ws > 0 && shift >= 0 && shift < ws, "%s: shift %d outside [0, window %d)", who, shift, ws);
  WM2F_REQUIRE(dtype == WM2F_F32 || dtype == WM2F_BF16, "%s: dtype %d", who, dtype);
  const bool want_pad = grad_k_pad != nullptr || grad_v_pad != nullptr, want_bias = grad_bias_table != nullptr;
  WM2F_REQUIRE(workspace != nullptr || !(want_pad || want_bias), "%s: null workspace", who);
  const uintptr_t al = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
                       reinterpret_cast<uintptr_t>(grad_out) | reinterpret_cast<uintptr_t>(grad_q) |
                       reinterpret_cast<uintptr_t>(grad_k) | reinterpret_cast<uintptr_t>(grad_v) |
                       reinterpret_cast<uintptr_t>(k_pad) | reinterpret_cast<uintptr_t>(v_pad) |
                       reinterpret_cast<uintptr_t>(workspace);
  const int nWy = ceil_div(H, ws), nWx = ceil_div(W, ws);
  const int64_t pairs = (int64_t)B * nWy * nWx * heads;
  if (!swin_bwd_built(ws, D) || heads > 65535 || (al & 15) != 0 || pairs >= (int64_t(1) << 31) ||
      (int64_t)H * W >= (int64_t(1) << 31)) {
    set_error("%s: built for window 4 / 7 / 12, head_dim 16 / 32, 16-byte aligned operands (got window %d, head_dim %d)", who,
              ws, D);
    return WM2F_EUNSUPPORTED;
  }
  const int nb = (2 * ws - 1) * (2 * ws - 1);
  float* part_bias = want_bias ? (float*)workspace : nullptr;
  float* part_pad = want_pad ? (float*)workspace + pairs * nb : nullptr;
  hipStream_t st = (hipStream_t)stream;
#define WM2F_SB(Tv, WSv, Dv)                                                                                              \
  launch_swin_bwd<Tv, WSv, Dv>(q, k, v, k_pad, v_pad, bias_table, lse, grad_out, grad_q, grad_k, grad_v, part_bias, part_pad, \
                               H, W, heads, shift, nWy, nWx, (int)pairs, st)
#define WM2F_SB_D(Tv, WSv)             \
  do {                                 \
    if (D == 32) WM2F_SB(Tv, WSv, 32); \
    else WM2F_SB(Tv, WSv, 16);         \
  } while (0)
#define WM2F_SB_WS(Tv)                  \
  do {                                  \
    if (ws == 4) WM2F_SB_D(Tv, 4);      \
    else if (ws == 7) WM2F_SB_D(Tv, 7); \
    else WM2F_SB_D(Tv, 12);             \
  } while (0)
  if (dtype == WM2F_F32) WM2F_SB_WS(float);
  else WM2F_SB_WS(uint16_t);
#undef WM2F_SB_WS
#undef WM2F_SB_D
#undef WM2F_SB
  WM2F_CHECK_LAUNCH(who);
  const int nwb = B * nWy * nWx;
  if (want_bias) {
    hipLaunchKernelGGL(swin_bwd_reduce_kernel, dim3(ceil_div(nb, 64), heads), dim3(64, kRedSlices), 0, st, part_bias,
                       (float*)grad_bias_table, (float*)nullptr, nwb, heads, nb, D, 0);
    WM2F_CHECK_LAUNCH(who);
  }
  if (want_pad) {
    hipLaunchKernelGGL(swin_bwd_reduce_kernel, dim3(ceil_div(2 * D, 64), heads), dim3(64, kRedSlices), 0, st, part_pad,
                       (float*)grad_k_pad, (float*)grad_v_pad, nwb, heads, 2 * D, D, 1);
    WM2F_CHECK_LAUNCH(who);
  }
  return WM2F_OK;
}
