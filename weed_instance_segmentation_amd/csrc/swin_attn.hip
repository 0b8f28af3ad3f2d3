// Shifted-window attention of the Swin backbone, inference forward (include/wm2f.h: wm2f_swin_window_attn_fwd).
// One launch replaces, per Swin layer, what transformers' modeling_swin.py:401-468, :486-505, :553-626 spell as
//     pad -> roll -> window partition -> q k^T * D^-1/2 + relative-position bias (+ shift mask) -> softmax -> p v
//         -> window reverse -> roll back -> crop.
// q, k, v and out stay in IMAGE order (B, H*W, heads*D), exactly as the three Linears write them: pad, roll and
// partition are index arithmetic in the loader, and the (windows, heads, L, L) score tensor never exists.
//
// Work unit: one (image, window, head) "pair".  A workgroup takes PAIRS of them, WPP waves each:
//   ws  4  (L =  16, 1 key tile ): 4 pairs x 1 wave       -- consecutive pairs are the heads of one window
//   ws  7  (L =  49, 4 key tiles): 1 pair  x 4 waves, one 16-query tile per wave
//   ws 12  (L = 144, 9 key tiles): 1 pair  x 3 waves, three query tiles per wave
// Per pair the window's K and V rows are gathered ONCE into LDS (a head's D values of a token are one contiguous segment),
// together with the head's column of the bias table and two small per-slot tables (token index; bias offset + shift
// region).  A wave then holds the whole score column block of its 16 queries in registers -- no key split, no online
// rescale, no merge kernel:
//   S^T = K Q^T      A = K tile [key][d] from LDS, B = Q^T [d][query] from global -> C: column = query (lane & 15),
//                    rows = keys 4 g + r of the tile: already the B operand of the second product (as masked_xattn.hip)
//   softmax over all LT tiles of the column (two 16-lane-row shuffles), fp32
//   O^T = V^T P^T    A = V^T [d][key] from LDS, B = P^T
// fp32 form: v_mfma_f32_16x16x4_f32 (exact fp32 products).  bf16 form: v_mfma_f32_16x16x16_bf16, S / softmax / O in
// fp32, P rounded to bf16 once; V is stored TRANSPOSED in LDS by the loader so that the A operand of the second product
// is one 8-byte read.
//
// LDS per workgroup (bytes): fp32 D = 32: ws 12 44.7 K, ws 7 19.6 K, ws 4 19.8 K;  bf16 D = 32: ws 12 24.5 K.
#include "common.h"

#include <type_traits>

namespace wm2f {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));

constexpr int kInvalidKey = 1 << 30;  // slot table flag: a key slot beyond L (the tile padding inside the kernel)

template <int WS>
struct SwinGeom {
  static constexpr int L = WS * WS, LT = (L + 15) / 16, LP = LT * 16;
  static constexpr int NB = (2 * WS - 1) * (2 * WS - 1), NBP = (NB + 3) / 4 * 4;
  static constexpr int PAIRS = WS == 4 ? 4 : 1;
  static constexpr int WPP = WS == 4 ? 1 : (WS == 7 ? 4 : 3);  // waves per pair
};

template <int WS, int D, int PAIRS>
struct alignas(16) SwinSmemF32 {
  float k[PAIRS][SwinGeom<WS>::LP][D + 4];  // + 4: rows 16 bytes apart in the bank row (K: b128 reads down 16 rows)
  float v[PAIRS][SwinGeom<WS>::LP][D + 4];
  float bias[PAIRS][SwinGeom<WS>::NBP];
  int kinfo[PAIRS][SwinGeom<WS>::LP];  // i * (2 ws - 1) + j  |  region << 16  |  kInvalidKey
  int tok[PAIRS][SwinGeom<WS>::LP];    // token index in the image, -1 = padding token, -2 = no slot
};

template <int WS, int D, int PAIRS>
struct alignas(16) SwinSmemBf16 {
  uint16_t k[PAIRS][SwinGeom<WS>::LP][D + 8];
  uint16_t vt[PAIRS][D][SwinGeom<WS>::LP + 8];  // V transposed: [d][key]
  float bias[PAIRS][SwinGeom<WS>::NBP];
  int kinfo[PAIRS][SwinGeom<WS>::LP];
  int tok[PAIRS][SwinGeom<WS>::LP];
};

// TRAIN: the same forward, also writing the log-sum-exp of every real query's row to lse (B, heads, H*W) for the backward
// (swin_attn_bwd.hip).
template <typename T, int WS, int D, bool TRAIN>
__global__ __launch_bounds__(SwinGeom<WS>::PAIRS* SwinGeom<WS>::WPP* kWave) void swin_window_attn_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ k_pad,
    const T* __restrict__ v_pad, const float* __restrict__ bias_table, T* __restrict__ out, float* __restrict__ lse, int H,
    int W, int heads, int shift, int nWy, int nWx, int total_pairs, float scale) {
  using G = SwinGeom<WS>;
  constexpr bool BF16 = std::is_same<T, uint16_t>::value;
  constexpr int L = G::L, LT = G::LT, LP = G::LP, NB = G::NB, PAIRS = G::PAIRS, WPP = G::WPP;
  constexpr int NT = WPP * kWave;  // threads of one pair
  constexpr int DT = D / 16;       // 16-row tiles of O^T
  constexpr int R = 2 * WS - 1;
  using Smem = typename std::conditional<BF16, SwinSmemBf16<WS, D, PAIRS>, SwinSmemF32<WS, D, PAIRS>>::type;
  __shared__ Smem sm;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, n = lane & 15;
  const int pl = wave / WPP;                    // pair of this wave inside the workgroup
  const int tp = threadIdx.x - pl * NT;         // thread inside the pair
  int pair = blockIdx.x * PAIRS + pl;
  const bool live = pair < total_pairs;         // the last workgroup of the ws 4 form may carry idle waves: they replay
  if (!live) pair = total_pairs - 1;            // the last pair (every barrier is reached) and store nothing
  const int head = pair % heads;
  const int wb = pair / heads;
  const int nW = nWy * nWx;
  const int win = wb % nW, b = wb / nW;
  const int wy = win / nWx, wx = win - wy * nWx;
  const int Hp = nWy * WS, Wp = nWx * WS;
  const int E = heads * D;
  const int64_t img = (int64_t)b * H * W;

  // ---- slot tables and the head's bias column
  for (int s = tp; s < LP; s += NT) {
    int tk = -2, info = kInvalidKey;
    if (s < L) {
      const int i = s / WS, j = s - i * WS;
      const int r = wy * WS + i, c = wx * WS + j;  // rolled-frame coordinates
      int region = 0;
      if (shift > 0) region = 3 * ((r >= Hp - WS) + (r >= Hp - shift)) + ((c >= Wp - WS) + (c >= Wp - shift));
      int py = r + shift, px = c + shift;  // padded-frame position the slot's token comes from (and goes back to)
      if (py >= Hp) py -= Hp;
      if (px >= Wp) px -= Wp;
      tk = (py < H && px < W) ? py * W + px : -1;
      info = (i * R + j) | (region << 16);
    }
    sm.tok[pl][s] = tk;
    sm.kinfo[pl][s] = info;
  }
  for (int t = tp; t < NB; t += NT) sm.bias[pl][t] = bias_table[(int64_t)t * heads + head];
  __syncthreads();

  // ---- gather K and V of the window: by token, 16 bytes per lane, consecutive lanes on one token's segment
  if constexpr (!BF16) {
    constexpr int CH = D / 4;
    for (int idx = tp; idx < LP * CH; idx += NT) {
      const int key = idx / CH, c = idx - key * CH;
      const int tk = sm.tok[pl][key];
      float4 kx = make_float4(0.f, 0.f, 0.f, 0.f), vx = kx;
      if (tk >= 0) {
        const int64_t off = (img + tk) * E + head * D + 4 * c;
        kx = *reinterpret_cast<const float4*>(k + off);
        vx = *reinterpret_cast<const float4*>(v + off);
      } else if (tk == -1) {  // a padding token: a zero row through the Linears = their bias (zeros without one)
        if (k_pad != nullptr) kx = *reinterpret_cast<const float4*>(k_pad + head * D + 4 * c);
        if (v_pad != nullptr) vx = *reinterpret_cast<const float4*>(v_pad + head * D + 4 * c);
      }
      *reinterpret_cast<float4*>(&sm.k[pl][key][4 * c]) = kx;
      *reinterpret_cast<float4*>(&sm.v[pl][key][4 * c]) = vx;
    }
  } else {
    constexpr int CH = D / 8;
    for (int idx = tp; idx < LP * CH; idx += NT) {
      const int key = idx / CH, c = idx - key * CH;
      const int tk = sm.tok[pl][key];
      s16x8 kx = (s16x8){0, 0, 0, 0, 0, 0, 0, 0}, vx = kx;
      if (tk >= 0) {
        const int64_t off = (img + tk) * E + head * D + 8 * c;
        kx = *reinterpret_cast<const s16x8*>(k + off);
        vx = *reinterpret_cast<const s16x8*>(v + off);
      } else if (tk == -1) {
        if (k_pad != nullptr) kx = *reinterpret_cast<const s16x8*>(k_pad + head * D + 8 * c);
        if (v_pad != nullptr) vx = *reinterpret_cast<const s16x8*>(v_pad + head * D + 8 * c);
      }
      *reinterpret_cast<s16x8*>(&sm.k[pl][key][8 * c]) = kx;
#pragma unroll
      for (int e = 0; e < 8; ++e) sm.vt[pl][8 * c + e][key] = (uint16_t)vx[e];
    }
  }
  __syncthreads();

  // ---- the wave's query tiles
  for (int qt = wave - pl * WPP; qt < LT; qt += WPP) {
    const int qs = 16 * qt + n;
    const int qsc = qs < L ? qs : L - 1;  // a column beyond L replays the last slot; never stored
    const int qtok = qs < L ? sm.tok[pl][qs] : -2;
    const int qinfo = sm.kinfo[pl][qsc];
    const int qoff = (qinfo & 0xffff) + (WS - 1) * R + (WS - 1);
    const int qreg = (qinfo >> 16) & 0xff;
    const int64_t qrow = (img + (qtok >= 0 ? qtok : 0)) * E + head * D;  // padding queries read token 0; never stored

    f32x4 s[LT];
    if constexpr (!BF16) {
      constexpr int DK = D / 4;  // k-steps: lane group g owns d = DK g .. DK g + DK - 1 (K and Q alike)
      float qf[DK];
#pragma unroll
      for (int t = 0; t < DK; t += 4) {
        const float4 x = *reinterpret_cast<const float4*>(q + qrow + DK * g + t);
        qf[t] = x.x; qf[t + 1] = x.y; qf[t + 2] = x.z; qf[t + 3] = x.w;
      }
#pragma unroll
      for (int kt = 0; kt < LT; ++kt) {
        float kf[DK];
#pragma unroll
        for (int t = 0; t < DK; t += 4) {
          const float4 x = *reinterpret_cast<const float4*>(&sm.k[pl][16 * kt + n][DK * g + t]);
          kf[t] = x.x; kf[t + 1] = x.y; kf[t + 2] = x.z; kf[t + 3] = x.w;
        }
        s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < DK; ++t) s[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[t], qf[t], s[kt], 0, 0, 0);
      }
    } else if constexpr (D == 32) {
      // lane (n, g) holds d = 8 g .. 8 g + 7 of its row: elements 0..3 feed MFMA step 0, 4..7 step 1 (K and Q alike)
      const s16x8 qx = *reinterpret_cast<const s16x8*>(q + qrow + 8 * g);
      const s16x4 q0 = __builtin_shufflevector(qx, qx, 0, 1, 2, 3), q1 = __builtin_shufflevector(qx, qx, 4, 5, 6, 7);
#pragma unroll
      for (int kt = 0; kt < LT; ++kt) {
        const s16x8 kx = *reinterpret_cast<const s16x8*>(&sm.k[pl][16 * kt + n][8 * g]);
        const s16x4 k0 = __builtin_shufflevector(kx, kx, 0, 1, 2, 3), k1 = __builtin_shufflevector(kx, kx, 4, 5, 6, 7);
        s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        s[kt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(k0, q0, s[kt], 0, 0, 0);
        s[kt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(k1, q1, s[kt], 0, 0, 0);
      }
    } else {
      const s16x4 q0 = *reinterpret_cast<const s16x4*>(q + qrow + 4 * g);
#pragma unroll
      for (int kt = 0; kt < LT; ++kt) {
        const s16x4 k0 = *reinterpret_cast<const s16x4*>(&sm.k[pl][16 * kt + n][4 * g]);
        s[kt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(k0, q0, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      }
    }

    // ---- scale, relative-position bias, shift mask; softmax over the whole column
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < LT; ++kt) {
      const int4 ki = *reinterpret_cast<const int4*>(&sm.kinfo[pl][16 * kt + 4 * g]);
      const int kin[4] = {ki.x, ki.y, ki.z, ki.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int info = kin[r];
        float bm = sm.bias[pl][qoff - (info & 0xffff)];
        if (((info >> 16) & 0xff) != qreg) bm += -100.0f;
        float x = s[kt][r] * scale + bm;
        if (info & kInvalidKey) x = -INFINITY;
        s[kt][r] = x;
        mx = fmaxf(mx, x);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, kWave));
    mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));  // finite: slot 0 of every window is a real key slot
    float lsum = 0.f;
    f32x4 o[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i) o[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if constexpr (!BF16) {
#pragma unroll
      for (int kt = 0; kt < LT; ++kt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __expf(s[kt][r] - mx);
          s[kt][r] = p;
          lsum += p;
        }
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            o[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(sm.v[pl][16 * kt + 4 * g + t][16 * i + n], s[kt][t], o[i], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int kt = 0; kt < LT; ++kt) {
        bf16x4_t pk;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pk[r] = (__bf16)__expf(s[kt][r] - mx);
          lsum += (float)pk[r];  // the sum of what the second product really multiplies by
        }
        const s16x4 pb = __builtin_bit_cast(s16x4, pk);
#pragma unroll
        for (int i = 0; i < DT; ++i) {
          const s16x4 va = *reinterpret_cast<const s16x4*>(&sm.vt[pl][16 * i + n][16 * kt + 4 * g]);
          o[i] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(va, pb, o[i], 0, 0, 0);
        }
      }
    }
    lsum += __shfl_xor(lsum, 16, kWave);
    lsum += __shfl_xor(lsum, 32, kWave);
    const float inv = 1.f / lsum;

    // ---- O^T: column = query n, rows d = 16 i + 4 g + r -> 4 consecutive channels of the query's own token
    if (live && qtok >= 0) {
      if constexpr (TRAIN) {
        if (g == 0) lse[((int64_t)b * heads + head) * H * W + qtok] = mx + logf(lsum);  // the accurate log: an error here is a normalisation error of every P of the row
      }
      T* op = out + qrow + 4 * g;
#pragma unroll
      for (int i = 0; i < DT; ++i) {
        if constexpr (!BF16) {
          *reinterpret_cast<float4*>(op + 16 * i) = make_float4(o[i][0] * inv, o[i][1] * inv, o[i][2] * inv, o[i][3] * inv);
        } else {
          bf16x4_t ob;
#pragma unroll
          for (int r = 0; r < 4; ++r) ob[r] = (__bf16)(o[i][r] * inv);
          *reinterpret_cast<s16x4*>(op + 16 * i) = __builtin_bit_cast(s16x4, ob);
        }
      }
    }
  }
}

template <typename T, int WS, int D>
void launch_swin(const void* q, const void* k, const void* v, const void* k_pad, const void* v_pad, const void* bias_table,
                 void* out, void* lse, int H, int W, int heads, int shift, int nWy, int nWx, int total_pairs, hipStream_t st) {
  using G = SwinGeom<WS>;
  const float scale = 1.0f / sqrtf((float)D);
  const dim3 grid(ceil_div(total_pairs, G::PAIRS)), block(G::PAIRS * G::WPP * kWave);
  if (lse != nullptr)
    hipLaunchKernelGGL((swin_window_attn_kernel<T, WS, D, true>), grid, block, 0, st, (const T*)q, (const T*)k, (const T*)v,
                       (const T*)k_pad, (const T*)v_pad, (const float*)bias_table, (T*)out, (float*)lse, H, W, heads, shift,
                       nWy, nWx, total_pairs, scale);
  else
    hipLaunchKernelGGL((swin_window_attn_kernel<T, WS, D, false>), grid, block, 0, st, (const T*)q, (const T*)k, (const T*)v,
                       (const T*)k_pad, (const T*)v_pad, (const float*)bias_table, (T*)out, (float*)nullptr, H, W, heads,
                       shift, nWy, nWx, total_pairs, scale);
}

// Argument checks and dispatch of both exported forwards; lse == nullptr is the inference form.
int swin_fwd(const char* who, const void* q, const void* k, const void* v, const void* k_pad, const void* v_pad,
             const void* bias_table, void* out, void* lse, int B, int H, int W, int heads, int D, int ws, int shift, int dtype,
             void* stream) {
  WM2F_REQUIRE(q && k && v && bias_table && out, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && heads > 0, "%s: non-positive size", who);
  WM2F_REQUIRE(ws > 0 && shift >= 0 && shift < ws, "%s: shift %d outside [0, window %d)", who, shift, ws);
  WM2F_REQUIRE(dtype == WM2F_F32 || dtype == WM2F_BF16, "%s: dtype %d", who, dtype);
  const uintptr_t al = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
                       reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(k_pad) | reinterpret_cast<uintptr_t>(v_pad);
  const int nWy = ceil_div(H, ws), nWx = ceil_div(W, ws);
  const int64_t pairs = (int64_t)B * nWy * nWx * heads;
  if ((ws != 4 && ws != 7 && ws != 12) || (D != 16 && D != 32) || heads > 65535 || (al & 15) != 0 ||
      pairs >= (int64_t(1) << 31) || (int64_t)H * W >= (int64_t(1) << 31)) {
    set_error("%s: built for window 4 / 7 / 12, head_dim 16 / 32, 16-byte aligned operands (got window %d, head_dim %d)", who,
              ws, D);
    return WM2F_EUNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
#define WM2F_SW(Tv, WSv, Dv) \
  launch_swin<Tv, WSv, Dv>(q, k, v, k_pad, v_pad, bias_table, out, lse, H, W, heads, shift, nWy, nWx, (int)pairs, st)
#define WM2F_SW_D(Tv, WSv)       \
  do {                           \
    if (D == 32) WM2F_SW(Tv, WSv, 32); \
    else WM2F_SW(Tv, WSv, 16);   \
  } while (0)
#define WM2F_SW_WS(Tv)                 \
  do {                                 \
    if (ws == 4) WM2F_SW_D(Tv, 4);     \
    else if (ws == 7) WM2F_SW_D(Tv, 7); \
    else WM2F_SW_D(Tv, 12);            \
  } while (0)
  if (dtype == WM2F_F32) WM2F_SW_WS(float);
  else WM2F_SW_WS(uint16_t);
#undef WM2F_SW_WS
#undef WM2F_SW_D
#undef WM2F_SW
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

}  // namespace

}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_swin_window_attn_fwd(const void* q, const void* k, const void* v, const void* k_pad, const void* v_pad,
                                         const void* bias_table, void* out, int B, int H, int W, int heads, int D, int ws,
                                         int shift, int dtype, void* stream) {
  return swin_fwd("wm2f_swin_window_attn_fwd", q, k, v, k_pad, v_pad, bias_table, out, nullptr, B, H, W, heads, D, ws, shift,
                  dtype, stream);
}

extern "C" int wm2f_swin_window_attn_train_fwd(const void* q, const void* k, const void* v, const void* k_pad,
                                               const void* v_pad, const void* bias_table, void* out, void* lse, int B, int H,
                                               int W, int heads, int D, int ws, int shift, int dtype, void* stream) {
  WM2F_REQUIRE(lse != nullptr, "wm2f_swin_window_attn_train_fwd: null lse");
  return swin_fwd("wm2f_swin_window_attn_train_fwd", q, k, v, k_pad, v_pad, bias_table, out, lse, B, H, W, heads, D, ws, shift,
                  dtype, stream);
}
