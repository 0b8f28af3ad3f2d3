// The ResNet stem in one kernel, at fp32 accuracy on the bf16 matrix cores ("split-bf16"):
//     out (B, 64, Hp, Wp) = MaxPool2d(3, stride 2, pad 1)( ReLU( conv7x7(x (B, Cin, Hi, Wi), W (64, Cin, 7, 7), stride 2, pad 3) + bias ) )
//     Hc = (Hi - 1) / 2 + 1,  Hp = (Hc - 1) / 2 + 1   (likewise W)
// as an implicit GEMM  conv_b (64, Hc Wc) = W (64, K) . im2col(x_b) (K, Hc Wc),  K = 160, where tap (c, ky, kx) of conv pixel
// (cy, cx) reads x_b[c, 2 cy - 3 + ky, 2 cx - 3 + kx] (zero outside the image).  The raw convolution never reaches memory: it
// is pooled in the accumulator registers, and bias + ReLU are applied to the pooled value (max commutes with the
// monotone bias + ReLU).
//
// K order (ops.stem_weight_columns builds it before the split).  A lane's B fragment is 8 consecutive columns, so column
// 8 G + i, i < 7, is tap (c, ky, kx) = (G / 7, G % 7, i) -- group G is one kernel row: 7 consecutive floats of one input
// row -- for the first min(7 Cin, 20) kernel rows.  With Cin = 3 the 21st row (c, ky) = (2, 6) rides in the eighth
// columns: column 8 G + 7 is its tap kx = G for G < 7.  Every other column is padding: W is zero there and the kernel
// feeds zeros, so that a non-finite input cannot meet a zero weight.  k-steps that hold only padding are left out
// (2, 4, 5 k-steps for Cin = 1, 2, 3).
//
// Arithmetic: that of conv3x3_split.hip -- both operands written as three bf16 pieces (h clamped to the largest finite
// bf16), the six products of a k-step summed from zero on v_mfma_f32_16x16x32_bf16, small terms first, and that sum added
// to the accumulator with one fp32 add.  No split-K, no atomics: the sequence of MFMAs a conv pixel sees depends on Cin
// alone (k-steps that hold only padding are left out), not on its position, the batch, the grid or how rows are shared
// out, so results are bit-identical run to run, for any sub-batch and any grid.
//
// Layout of the work:
//   * the whole split W (wm2f_token_linear_split_weight of the (64, 160) zero-padded OIHW view) sits in LDS for the
//     kernel's lifetime, 12 KiB per k-step: no ring and no barrier after the first;
//   * a WAVE, not the workgroup, owns a unit of work: a strip of 15 pooled columns by Rc pooled rows of one image.  It
//     walks the strip's conv rows top to bottom, one row of 32 conv pixels (two 16-pixel column tiles, conv columns
//     30 s - 1 .. 30 s + 30 of strip s) per step.  Lane (j, g) of column tile t holds conv column 30 s - 1 + 16 t + j:
//     the horizontal 3-max is two DPP moves inside the 16-lane row (plus one lane taken from the other tile), the
//     vertical 3-max runs over the steps in 32 carried registers.  Pooled columns sit at the odd conv-local columns
//     1, 3 .. 29, so 32 conv columns give 15 pooled ones (30 of 32 conv pixels are unique); rows are recomputed only at
//     the first row of a unit;
//   * the wave keeps the input rows of its strip, 69 columns x Cin planes, in a private 8-row ring in LDS (row iy in
//     slot iy mod 8, 256 floats per slot).  A conv row reads 7 rows; the 2 new rows of the next step are fetched into
//     registers under this step's MFMAs and written after its reads (LDS operations of one wave stay in order), so no
//     barrier is ever needed.  Ring addresses wrap with one AND, and a kernel row is one address: a k-step's B fragments
//     of both column tiles (the second is the first + 128 bytes) cost one v_add, one v_and_or, six ds_read_b64 and two
//     ds_read_b32 (planes are 70 columns apart to keep the 8-byte alignment);
//   * B fragments (lane (j, g): pixel j, k = 32 ks + 8 g .. + 7) are split in registers;
//   * conv columns outside the map start their accumulators at -inf (PyTorch's pool padding), conv rows outside it are
//     never computed.  fmax drops a NaN, so non-finiteness travels beside the values: one accumulator register per
//     pixel times zero (0 or NaN; by the split kernels' contract every channel of a pixel is non-finite together) is
//     pooled with adds and added to the outputs.
#include "common.h"

namespace wm2f {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x8 = __attribute__((ext_vector_type(8))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x2 = __attribute__((ext_vector_type(2))) float;
typedef __attribute__((address_space(3))) const float* lds_cf_t;
typedef __attribute__((address_space(3))) const f32x2* lds_cf2_t;
typedef __attribute__((address_space(3))) unsigned char* lds_u8_t;

constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kN = 64;             // output channels
constexpr int kRT = kN / 16;       // row tiles
constexpr int kKPad = 160;         // K of the split weight
constexpr int kFrag = 1024;        // bytes of one A fragment piece (64 lanes x 8 bf16)
constexpr int kStripP = 15;        // pooled columns of a strip
constexpr int kStripW = 69;        // input columns of a strip: 2 * 31 + 7
constexpr int kPlaneF = 70;        // floats between the planes of a ring slot
constexpr int kRowF = 256;         // floats of a ring slot (Cin * 70 <= 210 used)
constexpr int kRingBytes = 8 * kRowF * 4;
constexpr unsigned kRingMask = kRingBytes - 1;
constexpr int kWOff = kWaves * kRingBytes;
// the bias behind the first P pieces of the split W; the bytes of dynamic LDS
constexpr int stem_bias_off(int P) { return kWOff + (kKPad / 32) * kRT * P * kFrag; }
constexpr int stem_lds(int P) { return stem_bias_off(P) + kN * 4; }
constexpr unsigned kOob = 0x80000000u;
constexpr float kBf16Max = 3.38953139e38f;  // largest finite bf16, 0x7F7F

// DPP controls: lane j of a 16-lane row takes lane j - 1 (lane 0 keeps `old`) / lane (j + 1) mod 16
constexpr int kRowShr1 = 0x111;
constexpr int kRowRor15 = 0x12F;

template <int CTRL>
__device__ __forceinline__ float dpp(float old, float src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src),
                                                                CTRL, 0xf, 0xf, false));
}

// the fp32 values of eight bf16 read from their packed pairs (conv3x3_split.hip)
__device__ __forceinline__ f32x8 widen(const bf16x8 v) {
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

struct StemArgs {
  const float *x, *bias;
  const void* ws;
  float* out;
  int Hi, Wi, Hc, Wc, Hp, Wp;
  int S;       // strips per pooled row
  int Rc;      // pooled rows of a unit
  int nchunk;  // units per strip column
  int units;   // B * nchunk * S
};

// P = the pieces of each operand that take part: 3 = all six products, 2 = h and m (m.h, h.m, h.h), 1 = h
// alone (h.h).  The split weight is the three-piece one at every P; LDS holds the first P pieces of each row tile.
template <int CIN, int P = 3>
__global__ __launch_bounds__(kThreads) void stem7x7_pool_kernel(StemArgs a) {
  static_assert(P >= 1 && P <= 3, "one, two or three pieces");
  extern __shared__ __attribute__((aligned(8192))) unsigned char smem[];  // [8 rings][8 slots][256 f32] | W | bias
  constexpr int kPanelP = kRT * P * kFrag;  // bytes of one k-step of W in LDS
  constexpr int kBiasOff = stem_bias_off(P);
  constexpr int NG = 7 * CIN < 20 ? 7 * CIN : 20;  // kernel rows held as groups of 8 columns
  constexpr int NKS = (NG + 3) / 4;                // k-steps that hold any
  constexpr int N7 = 7 * CIN > 20 ? 7 : 0;         // groups whose eighth column is a tap of kernel row 20
  constexpr int NIT = (kPlaneF * CIN + 63) / 64;   // 64-lane pieces of a ring row
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, j = lane & 15;

  // the split W and the bias, once per workgroup
  {
    const u32x4* src = reinterpret_cast<const u32x4*>(a.ws);
    u32x4* dst = reinterpret_cast<u32x4*>(smem + kWOff);
    for (int i = tid; i < NKS * kPanelP / 16; i += kThreads) {
      const int f = i >> 6;  // LDS piece f = piece f % P of (k-step, row tile) f / P
      dst[i] = src[P == 3 ? i : (((f / P) * 3 + f % P) << 6) + (i & 63)];
    }
    if (tid < kN) reinterpret_cast<float*>(smem + kBiasOff)[tid] = a.bias[tid];
  }
  __syncthreads();

  unsigned char* ring = smem + wave * kRingBytes;
  const unsigned ring_lds = (unsigned)(uintptr_t)(lds_u8_t)ring;  // a multiple of the ring's size: OR-ed into wrapped offsets

  // byte offset in the ring of this lane's kernel row of k-step ks (group G = 4 ks + g), before the row slot and the wrap,
  // and of its tap of kernel row 20
  unsigned kj[NKS], kj7 = 0;
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int G = 4 * ks + g;
    kj[ks] = (unsigned)(((G % 7) * kRowF + (G / 7) * kPlaneF + 2 * j) * 4);
  }
  if (N7) kj7 = (unsigned)((6 * kRowF + 2 * kPlaneF + 2 * j) * 4);  // + 4 G per k-step
  const int HWi = a.Hi * a.Wi;
  const int n_w = gridDim.x * kWaves;
  for (int u = blockIdx.x * kWaves + wave; u < a.units; u += n_w) {
    const int s = u % a.S, t_ = u / a.S;
    const int ch = t_ % a.nchunk, b = t_ / a.nchunk;
    const int r0 = ch * a.Rc, r1 = min(r0 + a.Rc, a.Hp);
    const int cy_s = max(2 * r0 - 1, 0), cy_e = min(2 * r1 - 1, a.Hc - 1);
    const int x0 = 60 * s - 5;  // input column of ring column 0: 2 (30 s - 1) - 3

    // per-image buffers (each below 2 GiB: checked by the host)
    const __amdgpu_buffer_rsrc_t x_rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(a.x + (int64_t)b * CIN * HWi), 0, CIN * HWi * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t o_rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.out + (int64_t)b * kN * a.Hp * a.Wp), 0, kN * a.Hp * a.Wp * 4, 0x00020000);

    // ring column e = lane + 64 it is plane e / 69, input column x0 + e % 69; columns outside the image (and past the
    // planes) load zero through the buffer's range check
    unsigned xb[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int e = lane + 64 * it;
      const int c = e / kPlaneF, ix = x0 + e - kPlaneF * c;
      xb[it] = (c < CIN && e - kPlaneF * c < kStripW && (unsigned)ix < (unsigned)a.Wi) ? (unsigned)((c * HWi + ix) * 4) : kOob;
    }
    // a row outside the image cannot be left to the range check (row Hi of plane c is row 0 of plane c + 1)
    float pre[2][NIT];
    auto fetch = [&](int iy) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const bool row_ok = (unsigned)(iy + r) < (unsigned)a.Hi;
        const unsigned ro = (unsigned)((iy + r) * a.Wi * 4);
#pragma unroll
        for (int it = 0; it < NIT; ++it)
          pre[r][it] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(x_rs, row_ok ? xb[it] + ro : kOob, 0, 0));
      }
    };
    auto stash = [&](int iy) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int it = 0; it < NIT; ++it)
          *reinterpret_cast<float*>(ring + ((((iy + r) & 7) * kRowF) + lane + 64 * it) * 4) = pre[r][it];
    };

    // is the conv column of this lane in column tile t, 30 s - 1 + 16 t + j, inside the map
    bool cok[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) cok[t] = (unsigned)(30 * s - 1 + 16 * t + j) < (unsigned)a.Wc;

    // rows 2 cy_s - 4 .. 2 cy_s + 3: the first conv row's seven and one the ring overwrites before it is read
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      fetch(2 * cy_s - 4 + 2 * q);
      stash(2 * cy_s - 4 + 2 * q);
    }

    f32x4 carry[kRT][2];
    float fcarry[2] = {0.f, 0.f};
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
      for (int t = 0; t < 2; ++t) carry[rt][t] = (f32x4){-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};

#pragma unroll 1
    for (int cy = cy_s; cy <= cy_e; ++cy) {
      const bool more = cy < cy_e;
      if (more) fetch(2 * cy + 4);  // the next row's two new input rows fly under this row's MFMAs

      const unsigned rowbase = (unsigned)(((2 * cy - 3) & 7) * kRowF * 4);
      auto gather = [&](int ks, f32x8 (&xr)[2]) {
        const unsigned at = ((rowbase + kj[ks]) & kRingMask) | ring_lds;
        const bool row_ok = 4 * ks + g < NG;  // false only in the last k-step of Cin < 3
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
          for (int p = 0; p < 3; ++p) {
            const f32x2 v = *(lds_cf2_t)(uintptr_t)(at + 128 * t + 8 * p);
            xr[t][2 * p] = v[0];
            xr[t][2 * p + 1] = v[1];
          }
          xr[t][6] = *(lds_cf_t)(uintptr_t)(at + 128 * t + 24);
          xr[t][7] = 0.f;
          if (4 * ks + 3 >= NG) {
#pragma unroll
            for (int i = 0; i < 7; ++i) xr[t][i] = row_ok ? xr[t][i] : 0.f;
          }
        }
        if (4 * ks < N7) {
          const unsigned a7 = ((rowbase + kj7 + 16 * ks + 4 * g) & kRingMask) | ring_lds;
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const float v = *(lds_cf_t)(uintptr_t)(a7 + 128 * t);
            xr[t][7] = (4 * ks + 3 < N7 || 4 * ks + g < N7) ? v : 0.f;
          }
        }
      };

      f32x4 acc[kRT][2];
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const float c0 = cok[t] ? 0.f : -__builtin_inff();  // a column outside the map never wins a pool window
          acc[rt][t] = (f32x4){c0, c0, c0, c0};
        }

      f32x8 xr[2];
      gather(0, xr);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        bf16x8 bh[2], bm[2], bl[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) split3<P>(xr[t], bh[t], bm[t], bl[t]);
        if (ks + 1 < NKS) gather(ks + 1, xr);

        const unsigned char* panel = smem + kWOff + ks * kPanelP;
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
        bf16x8 av[3];
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) {
          read_a(av, rt);
          __builtin_amdgcn_sched_barrier(0);
          acc[rt][0] = six(acc[rt][0], av, 0);
          acc[rt][1] = six(acc[rt][1], av, 1);
          __builtin_amdgcn_sched_barrier(0);
        }
      }

      // ---- pool.  Lane (j, g) holds channels rt * 16 + 4 g .. + 3 of conv column 30 s - 1 + 16 t + j of conv row cy.
      // Horizontal: the 3-max of a lane and its two neighbours (lane 15 of tile 0 takes lane 0 of tile 1); vertical:
      // pooled row r is conv rows 2 r - 1, 2 r, 2 r + 1, so an even row joins the carried odd row and an odd row closes
      // the window and becomes the next one's first row.
      const bool odd = cy & 1;
      const int r = cy >> 1;
      const bool emit = odd ? r >= r0 : cy == a.Hc - 1;
      const bool is15 = j == 15;
      auto hsum = [&](float v0, float v1, float& h0, float& h1, auto op) {
        const float l0 = dpp<kRowShr1>(v0, v0), l1 = dpp<kRowShr1>(v1, v1);
        const float n0 = dpp<kRowRor15>(v0, v0), n1 = dpp<kRowRor15>(v1, v1);
        h0 = op(op(v0, l0), is15 ? n1 : n0);
        h1 = op(op(v1, l1), n1);
      };
      auto fmax2 = [](float p, float q) { return __builtin_fmaxf(p, q); };
      auto fadd2 = [](float p, float q) { return p + q; };

      float fo[2];
      {
        float fh0, fh1;
        hsum(cok[0] ? acc[0][0][0] * 0.f : 0.f, cok[1] ? acc[0][1][0] * 0.f : 0.f, fh0, fh1, fadd2);
        fo[0] = fcarry[0] + fh0;
        fo[1] = fcarry[1] + fh1;
        fcarry[0] = odd ? fh0 : fo[0];
        fcarry[1] = odd ? fh1 : fo[1];
      }
      const float* bias_l = reinterpret_cast<const float*>(smem + kBiasOff);
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt) {
        f32x4 o[2];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float h0, h1;
          hsum(acc[rt][0][e], acc[rt][1][e], h0, h1, fmax2);
          o[0][e] = __builtin_fmaxf(carry[rt][0][e], h0);
          o[1][e] = __builtin_fmaxf(carry[rt][1][e], h1);
          carry[rt][0][e] = odd ? h0 : o[0][e];
          carry[rt][1][e] = odd ? h1 : o[1][e];
        }
        if (emit) {
          const int n0 = rt * 16 + 4 * g;
          const f32x4 bv = *reinterpret_cast<const f32x4*>(bias_l + n0);
          const unsigned rs = (unsigned)(a.Hp * a.Wp * 4);
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            // the odd conv-local columns 1 .. 29 are the centres of pooled columns 15 s .. 15 s + 14
            const int pc = kStripP * s + ((16 * t + j - 1) >> 1);
            const bool centre = (j & 1) && 16 * t + j < 2 * kStripP && pc < a.Wp;
            const unsigned ro = centre ? (unsigned)(((n0 * a.Hp + r) * a.Wp + pc) * 4) : kOob;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float v = o[t][e] + bv[e];
              v = v < 0.f ? 0.f : v;  // a NaN stays a NaN
              v += fo[t];             // 0, or NaN where the window holds a non-finite conv pixel
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), o_rs, ro, e * rs, 0);
            }
          }
        }
      }

      if (more) stash(2 * cy + 4);  // after this row's reads: slot (2 cy + 5) mod 8 held row 2 cy - 3
    }
  }
}

// Pooled rows per unit: the fewest rounds of units over the waves times the conv rows of a unit (2 Rc + 1, plus about
// three rows' time to fill the ring), ties to the longer unit.
int choose_rows(int B, int S, int Hp, int n_waves) {
  int best = 1;
  int64_t best_cost = -1;
  for (int rc = 1; rc <= Hp; ++rc) {
    const int64_t units = (int64_t)B * S * ceil_div(Hp, rc);
    const int64_t cost = ceil_div64(units, n_waves) * (2 * rc + 4);
    if (best_cost < 0 || cost <= best_cost) best = rc, best_cost = cost;
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

// pieces = P of the kernel (3: wm2f_stem7x7_pool_fwd)
template <int P>
static void (*stem_pick(int Cin))(StemArgs) {
  return Cin == 1 ? stem7x7_pool_kernel<1, P> : Cin == 2 ? stem7x7_pool_kernel<2, P> : stem7x7_pool_kernel<3, P>;
}

static int stem_launch(const char* who, const void* x, const void* w_split, const void* bias, void* out, int B, int Cin, int N,
                       int Hi, int Wi, int grid, int pieces, void* stream) {
  WM2F_REQUIRE(pieces >= 1 && pieces <= 3, "%s: pieces = %d (1, 2 and 3 are built)", who, pieces);
  WM2F_REQUIRE(x && w_split && bias && out, "%s: null pointer", who);
  WM2F_REQUIRE(B > 0 && Hi > 0 && Wi > 0, "%s: non-positive size", who);
  WM2F_REQUIRE(Cin >= 1 && 49 * Cin <= kKPad, "%s: Cin = %d (1, 2 and 3 are built: 49 Cin <= %d)", who, Cin, kKPad);
  WM2F_REQUIRE(N == kN, "%s: N = %d (%d is built)", who, N, kN);
  WM2F_REQUIRE(grid <= 65536, "%s: grid = %d is too large", who, grid);
  const int Hc = (Hi - 1) / 2 + 1, Wc = (Wi - 1) / 2 + 1;
  const int Hp = (Hc - 1) / 2 + 1, Wp = (Wc - 1) / 2 + 1;
  WM2F_REQUIRE((int64_t)Cin * Hi * Wi * 4 < (1ll << 31) && (int64_t)N * Hp * Wp * 4 < (1ll << 31),
               "%s: one image of x / out must stay below 2 GiB (32-bit buffer offsets)", who);
  int n_cu = 0;
  if (cu_count(&n_cu) != 0) {
    set_error("%s: cannot query the device", who);
    return WM2F_ELAUNCH;
  }
  const int S = ceil_div(Wp, kStripP);
  WM2F_REQUIRE((int64_t)B * S * Hp < (1ll << 31), "%s: too many units of work", who);
  const int wgs0 = grid > 0 ? grid : n_cu;
  const int rc = choose_rows(B, S, Hp, wgs0 * kWaves);
  StemArgs a;
  a.x = (const float*)x;
  a.ws = w_split;
  a.bias = (const float*)bias;
  a.out = (float*)out;
  a.Hi = Hi;
  a.Wi = Wi;
  a.Hc = Hc;
  a.Wc = Wc;
  a.Hp = Hp;
  a.Wp = Wp;
  a.S = S;
  a.Rc = rc;
  a.nchunk = ceil_div(Hp, rc);
  a.units = B * a.nchunk * S;
  const int wgs = grid > 0 ? grid : min(n_cu, ceil_div(a.units, kWaves));
  void (*kfn)(StemArgs) = pieces == 3 ? stem_pick<3>(Cin) : (pieces == 2 ? stem_pick<2>(Cin) : stem_pick<1>(Cin));
  const int kLds = stem_lds(pieces);
  // per call: the attribute belongs to the current device
  hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
  if (e != hipSuccess) {
    set_error("%s: cannot raise dynamic LDS to %d: %s", who, kLds, hipGetErrorString(e));
    return WM2F_ELAUNCH;
  }
  hipLaunchKernelGGL(kfn, dim3(wgs), dim3(kThreads), kLds, (hipStream_t)stream, a);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_stem7x7_pool_fwd(const void* x, const void* w_split, const void* bias, void* out, int B, int Cin, int N,
                                     int Hi, int Wi, int grid, void* stream) {
  return stem_launch("wm2f_stem7x7_pool_fwd", x, w_split, bias, out, B, Cin, N, Hi, Wi, grid, 3, stream);
}

extern "C" int wm2f_stem7x7_pool_fwd_p(const void* x, const void* w_split, const void* bias, void* out, int B, int Cin, int N,
                                       int Hi, int Wi, int grid, int pieces, void* stream) {
  return stem_launch("wm2f_stem7x7_pool_fwd_p", x, w_split, bias, out, B, Cin, N, Hi, Wi, grid, pieces, stream);
}
