// GroupNorm pieces shared by the apply kernels (fused_elementwise.hip), the convolution epilogues that produce the group
// statistics and the 1x1 operand loader that applies the normalisation on the fly (conv1x1_split.hip, conv3x3_split.hip;
// DESIGN §33).  One definition of the affine map, so every consumer of one statistics workspace sees the same bits.
#pragma once
#include "common.h"

namespace wm2f {

// y = scale * x + shift for one channel of one image
struct GnAffine {
  float scale, shift;
};

// The affine map of channel c in group bg = b * G + g from the workspace stats[2 bg + {0, 1}] = (sum, sum of squares) over
// the group's n = cpg * H * W values: mean and variance in fp64, the variance clamped at 0, rstd rounded to float,
//     scale = rstd * gamma,   shift = beta - mean * scale.
// add_pre: the statistics are those of x + pre (a per-channel bias that no pass has added to x yet), so
//     shift = beta + (pre - mean) * scale.
__device__ __forceinline__ GnAffine gn_affine(const double* __restrict__ stats, int bg, double n, float eps, float gamma,
                                              float beta, bool add_pre = false, float pre = 0.f) {
  const double mean_d = stats[2 * bg] / n;
  double var_d = stats[2 * bg + 1] / n - mean_d * mean_d;
  var_d = var_d < 0.0 ? 0.0 : var_d;
  const float rstd = (float)(1.0 / sqrt(var_d + (double)eps));
  GnAffine a;
  a.scale = rstd * gamma;
  a.shift = add_pre ? fmaf(pre - (float)mean_d, a.scale, beta) : fmaf(-(float)mean_d, a.scale, beta);
  return a;
}

// one element: a single fused multiply-add, written out so that no translation unit can round it another way
__device__ __forceinline__ float gn_apply(float x, const GnAffine a) { return fmaf(x, a.scale, a.shift); }
__device__ __forceinline__ float gn_apply_relu(float x, const GnAffine a) { return fmaxf(fmaf(x, a.scale, a.shift), 0.f); }

// Group sizes whose groups lie inside one 16-channel row tile of the split convolutions' accumulator layout: the
// convolution epilogues produce the statistics for exactly these.
__host__ __device__ __forceinline__ bool gn_epilogue_cpg(int cpg) { return cpg == 4 || cpg == 8 || cpg == 16; }

// Sum of v over the 16 lanes of a DPP row (the lanes j = 0 .. 15 of one g in the MFMA accumulator layout); every lane of
// the row ends with the same value.  Four fp32 additions deep: lane pairs, quads, the two quads of a half row, the halves.
__device__ __forceinline__ float gn_row_sum16(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false));  // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, false));  // row_mirror
  return v;
}

// The group statistics of a split convolution's workgroup tile, called by every wave after its last k-step barrier (the
// A ring in `smem` is free).  Lane (j, g) hands in, per row tile rt, the fp32 sum and sum of squares of its 8 stored
// values (channels 16 rt + 4 g .. + 3 of its two pixels; zero for pixels of the ragged tail) in s[rt], ss[rt].
// Order: the 16 lanes of a g (gn_row_sum16), the g's that share a group (cpg 8: pairs, cpg 16: all four), the workgroup's
// waves along p through LDS (in fp64, in wave order), then one fp64 atomicAdd pair per (workgroup, group).
// red: [kWaves][NRT][4][2] floats at the start of smem.
template <int NRT, int WN, int kWaves>
__device__ __forceinline__ void gn_tile_stats(const float (&s)[NRT], const float (&ss)[NRT], unsigned char* smem, double* stats,
                                              int bG, int n_wg, int cpg, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, j = lane & 15;
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt) {
    float a = gn_row_sum16(s[rt]), q = gn_row_sum16(ss[rt]);
    if (cpg >= 8) {
      a += __shfl_xor(a, 16);
      q += __shfl_xor(q, 16);
    }
    if (cpg == 16) {
      a += __shfl_xor(a, 32);
      q += __shfl_xor(q, 32);
    }
    if (j == 0) {
      red[((wave * NRT + rt) * 4 + g) * 2] = a;
      red[((wave * NRT + rt) * 4 + g) * 2 + 1] = q;
    }
  }
  __syncthreads();
  // thread t < 4 WN NRT: row tile R = t / 4 of the workgroup (wave column R / NRT, its row tile R % NRT), lane row t % 4
  constexpr int kSlots = WN * NRT * 4;
  static_assert(kSlots <= kWaves * 64, "one thread per (row tile, g)");
  const int slot_g = tid & 3;
  if (tid < kSlots && slot_g % (cpg >> 2) == 0) {
    const int R = tid >> 2, wn = R / NRT, rt = R - wn * NRT;
    double a = 0.0, q = 0.0;
#pragma unroll
    for (int wp = 0; wp < kWaves / WN; ++wp) {
      const int w = wp * WN + wn;
      a += (double)red[((w * NRT + rt) * 4 + slot_g) * 2];
      q += (double)red[((w * NRT + rt) * 4 + slot_g) * 2 + 1];
    }
    const int grp = (n_wg + R * 16 + 4 * slot_g) / cpg;
    atomicAdd(stats + 2 * (bG + grp), a);
    atomicAdd(stats + 2 * (bG + grp) + 1, q);
  }
}

}  // namespace wm2f
