// Simple Copy-Paste on the device: instances of one image of a compact batch are cut out and pasted,
// shifted, onto another -- float32 pixels (B, C, H, W) and int32 id maps (B, H, W), out of place.  The rule is the contract
// comment of include/wm2f.h; tests/copy_paste_reference.py restates it in numpy.
//
// Three steps, each one entry point, none of which synchronises with the host:
//   select  (maps only)  per destination, the area of every selected source id in the whole source frame (`original`)
//                        and the part of it that arrives inside the destination's window (`landed`); a second, tiny
//                        kernel strikes from the LUT what does not land or lands less than min_visible of itself.
//   paste                one pass over the destination: map and pixels are read once and written once, the source map is
//                        read where a source pixel can arrive, the source pixels only where something is pasted.  The
//                        same pass counts every id of the destination before the paste and what the paste takes and adds.
//   prune   (maps only)  destination instances that kept less than min_visible of themselves become ignore_index.
// A thread owns four neighbouring pixels of a row (16-byte loads and stores) when W and the pointers allow; the source
// side is read as 16 bytes too when dx is a multiple of four, else pixel by pixel and only where pasted.  Otherwise the
// same kernels run with one pixel per thread.  The 256-entry LUT and the histograms live in LDS; a workgroup flushes its
// non-zero counts with integer atomics, so the areas are exact and the same from run to run.  Values outside 0 .. 254
// (ignore_index and everything else that is no id -- most of a field image) are not counted.
#include "common.h"

namespace wm2f {
namespace {

constexpr int kThreads = 256;       // = the LUT's length: thread t owns entry t of every table
constexpr int kIds = 256;
constexpr int kCpMaxImages = 32;    // destinations per launch: their descriptors travel as a kernel argument
constexpr int kItems = 8;           // quads (or pixels) a thread walks before the grid is made larger
constexpr int kMaxBlocksX = 2048;
constexpr int kMaxShift = 1 << 16;

struct CpDesc {
  int src, dy, dx, h, w;
};

struct CpArgs {
  CpDesc d[kCpMaxImages];
};

__device__ __forceinline__ bool is_id(int v) { return (unsigned)v < 255u; }

template <int VEC>
__device__ __forceinline__ void load_i(const int32_t* p, int (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const int4 q = *reinterpret_cast<const int4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
    v[0] = *p;
  }
}

template <int VEC>
__device__ __forceinline__ void store_i(int32_t* p, const int (&v)[VEC]) {
  if constexpr (VEC == 4)
    *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
  else
    *p = v[0];
}

template <int VEC>
__device__ __forceinline__ void load_u(const uint32_t* p, uint32_t (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
    v[0] = *p;
  }
}

template <int VEC>
__device__ __forceinline__ void store_u(uint32_t* p, const uint32_t (&v)[VEC]) {
  if constexpr (VEC == 4)
    *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
  else
    *p = v[0];
}

// adds the ids of v (where keep[i]) to an LDS histogram, one atomic per run of equal neighbours
template <int VEC>
__device__ __forceinline__ void hist_runs(int* hist, const int (&v)[VEC], const bool (&keep)[VEC], int step) {
  int cur = -1, cnt = 0;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    const int id = (keep[i] && is_id(v[i])) ? v[i] : -1;
    if (id != cur) {
      if (cur >= 0) atomicAdd(&hist[cur], cnt * step);
      cur = id, cnt = 0;
    }
    ++cnt;
  }
  if (cur >= 0) atomicAdd(&hist[cur], cnt * step);
}

__global__ __launch_bounds__(kThreads) void cp_zero_rows_kernel(int32_t* __restrict__ areas, int row0, int rows) {
  int32_t* a = areas + (int64_t)blockIdx.x * 3 * kIds + row0 * kIds;
  for (int i = threadIdx.x; i < rows * kIds; i += kThreads) a[i] = 0;
}

// step A, the counts: the workgroups of row blockIdx.y walk the map of that destination's SOURCE image
template <int VEC>
__global__ __launch_bounds__(kThreads) void cp_count_kernel(const int32_t* __restrict__ maps,
                                                            const int32_t* __restrict__ lut_in,
                                                            int32_t* __restrict__ areas, int32_t* __restrict__ landed,
                                                            const CpArgs args, int b0, int H, int W) {
  __shared__ int s_lut[kIds], s_orig[kIds], s_land[kIds];
  const CpDesc d = args.d[blockIdx.y];
  if (d.src < 0) return;  // block-uniform
  const int b = b0 + blockIdx.y, t = threadIdx.x;
  const int l = lut_in[(int64_t)b * kIds + t];
  s_lut[t] = (t < 255 && is_id(l)) ? l : -1;
  s_orig[t] = 0, s_land[t] = 0;
  __syncthreads();
  const int32_t* m = maps + (int64_t)d.src * H * W;
  const int wq = W / VEC, n = H * wq;
  for (int q = blockIdx.x * kThreads + t; q < n; q += gridDim.x * kThreads) {
    const int y = q / wq, x0 = (q - y * wq) * VEC;
    int v[VEC];
    load_i<VEC>(m + (int64_t)y * W + x0, v);
    const bool row_in = (unsigned)(y + d.dy) < (unsigned)d.h;
    bool sel[VEC], in[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      sel[i] = is_id(v[i]) && s_lut[v[i]] >= 0;
      in[i] = sel[i] && row_in && (unsigned)(x0 + i + d.dx) < (unsigned)d.w;
    }
    hist_runs<VEC>(s_orig, v, sel, 1);
    hist_runs<VEC>(s_land, v, in, 1);
  }
  __syncthreads();
  if (s_orig[t]) atomicAdd(&areas[((int64_t)b * 3 + 2) * kIds + t], s_orig[t]);
  if (s_land[t]) atomicAdd(&landed[(int64_t)b * kIds + t], s_land[t]);
}

// step A, the decision: one thread per LUT entry
__global__ __launch_bounds__(kThreads) void cp_strike_kernel(const int32_t* __restrict__ lut_in,
                                                             const int32_t* __restrict__ areas,
                                                             const int32_t* __restrict__ landed,
                                                             int32_t* __restrict__ lut_out, const CpArgs args, int b0,
                                                             int64_t num, int64_t den) {
  const int b = b0 + blockIdx.x, t = threadIdx.x;
  int l = lut_in[(int64_t)b * kIds + t];
  if (args.d[blockIdx.x].src < 0 || t == 255 || !is_id(l)) l = -1;
  if (l >= 0) {
    const int64_t orig = areas[((int64_t)b * 3 + 2) * kIds + t], land = landed[(int64_t)b * kIds + t];
    if (land == 0 || land * den < num * orig) l = -1;
  }
  lut_out[(int64_t)b * kIds + t] = l;
}

// step B: the workgroups of row blockIdx.y walk destination b0 + blockIdx.y
template <int VEC>
__global__ __launch_bounds__(kThreads) void cp_paste_kernel(const uint32_t* __restrict__ pix_in,
                                                            const int32_t* __restrict__ maps_in,
                                                            const int32_t* __restrict__ lut,
                                                            uint32_t* __restrict__ pix_out, int32_t* __restrict__ maps_out,
                                                            int32_t* __restrict__ areas, const CpArgs args, int b0, int C,
                                                            int H, int W) {
  __shared__ int s_lut[kIds], s_before[kIds], s_delta[kIds];
  const CpDesc d = args.d[blockIdx.y];
  const int b = b0 + blockIdx.y, t = threadIdx.x;
  const bool has = d.src >= 0;
  int l = has ? lut[(int64_t)b * kIds + t] : -1;
  s_lut[t] = (t < 255 && is_id(l)) ? l : -1;
  s_before[t] = 0, s_delta[t] = 0;
  __syncthreads();
  const int64_t plane = (int64_t)H * W;
  const int s = has ? d.src : b;
  const int32_t* md = maps_in + (int64_t)b * plane;
  const int32_t* ms = maps_in + (int64_t)s * plane;
  int32_t* mo = maps_out + (int64_t)b * plane;
  const uint32_t* pd = pix_in + (int64_t)b * C * plane;
  const uint32_t* ps = pix_in + (int64_t)s * C * plane;
  uint32_t* po = pix_out + (int64_t)b * C * plane;
  const bool vec_src = VEC == 4 && (d.dx & 3) == 0;  // the source quad is aligned as the destination's is
  const int wq = W / VEC, n = H * wq;
  for (int q = blockIdx.x * kThreads + t; q < n; q += gridDim.x * kThreads) {
    const int y = q / wq, x0 = (q - y * wq) * VEC;
    const int off = y * W + x0;
    int dv[VEC], ov[VEC];
    bool p[VEC], all_true[VEC];
    load_i<VEC>(md + off, dv);
#pragma unroll
    for (int i = 0; i < VEC; ++i) ov[i] = dv[i], p[i] = false, all_true[i] = true;
    const int ys = y - d.dy;
    const int soff = ys * W + x0 - d.dx;  // used only where the source position lies inside the frame
    if (has && y < d.h && (unsigned)ys < (unsigned)H) {
      if (vec_src) {
        if ((unsigned)(x0 - d.dx) < (unsigned)W) {  // W % 4 == 0: the whole quad is inside or outside
          int sv[VEC];
          load_i<VEC>(ms + soff, sv);
#pragma unroll
          for (int i = 0; i < VEC; ++i)
            if (x0 + i < d.w && is_id(sv[i]) && s_lut[sv[i]] >= 0) p[i] = true, ov[i] = s_lut[sv[i]];
        }
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          if (x0 + i < d.w && (unsigned)(x0 + i - d.dx) < (unsigned)W) {
            const int sv = ms[soff + i];
            if (is_id(sv) && s_lut[sv] >= 0) p[i] = true, ov[i] = s_lut[sv];
          }
        }
      }
    }
    store_i<VEC>(mo + off, ov);
    hist_runs<VEC>(s_before, dv, all_true, 1);
    bool any = false, all = true;
#pragma unroll
    for (int i = 0; i < VEC; ++i) any = any || p[i], all = all && p[i];
    if (any) {
      hist_runs<VEC>(s_delta, dv, p, -1);
      hist_runs<VEC>(s_delta, ov, p, 1);
    }
    for (int c = 0; c < C; ++c) {
      const int64_t co = (int64_t)c * plane;
      uint32_t v[VEC];
      if (!all) {
        load_u<VEC>(pd + co + off, v);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = 0u;
      }
      if (any) {
        if (vec_src) {
          uint32_t sp[VEC];
          load_u<VEC>(ps + co + soff, sp);
#pragma unroll
          for (int i = 0; i < VEC; ++i) v[i] = p[i] ? sp[i] : v[i];
        } else {
#pragma unroll
          for (int i = 0; i < VEC; ++i)
            if (p[i]) v[i] = ps[co + soff + i];
        }
      }
      store_u<VEC>(po + co + off, v);
    }
  }
  __syncthreads();
  const int before = s_before[t], delta = s_delta[t];
  if (before) atomicAdd(&areas[((int64_t)b * 3 + 0) * kIds + t], before);
  if (before + delta) atomicAdd(&areas[((int64_t)b * 3 + 1) * kIds + t], before + delta);
}

// step C: in place on the pasted maps
template <int VEC>
__global__ __launch_bounds__(kThreads) void cp_prune_kernel(int32_t* __restrict__ maps, const int32_t* __restrict__ areas,
                                                            int H, int W, int64_t num, int64_t den, int ignore_index) {
  __shared__ int s_kill[kIds];
  const int b = blockIdx.y, t = threadIdx.x;
  const int64_t before = areas[((int64_t)b * 3 + 0) * kIds + t], after = areas[((int64_t)b * 3 + 1) * kIds + t];
  s_kill[t] = t < 255 && after > 0 && after * den < num * before;
  __syncthreads();
  int32_t* m = maps + (int64_t)b * H * W;
  const int wq = W / VEC, n = H * wq;
  for (int q = blockIdx.x * kThreads + t; q < n; q += gridDim.x * kThreads) {
    int v[VEC];
    load_i<VEC>(m + (int64_t)q * VEC, v);
    bool changed = false;
#pragma unroll
    for (int i = 0; i < VEC; ++i)
      if (is_id(v[i]) && s_kill[v[i]]) v[i] = ignore_index, changed = true;
    if (changed) store_i<VEC>(m + (int64_t)q * VEC, v);
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_frame(const char* who, int B, int H, int W) {
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0, "%s: need B, H, W > 0, got %d, %d, %d", who, B, H, W);
  if (B > 65535 || H > WM2F_PRE_MAX_SIDE || W > WM2F_PRE_MAX_SIDE) {
    set_error("%s: B = %d, (H, W) = (%d, %d) exceed the built bounds (B <= 65535, sides <= %d)", who, B, H, W,
              WM2F_PRE_MAX_SIDE);
    return WM2F_EUNSUPPORTED;
  }
  return WM2F_OK;
}

int check_fraction(const char* who, int64_t num, int64_t den) {
  WM2F_REQUIRE(den >= 1 && den <= 1024 && num >= 0 && num <= den, "%s: min_visible = %lld / %lld, expected 0 <= num <= den <= 1024",
               who, (long long)num, (long long)den);
  return WM2F_OK;
}

// rows b0 .. b0 + n - 1 of the host descriptor, checked, as a kernel argument
int fill_args(const char* who, const int64_t* desc, int B, int H, int W, int b0, int n, CpArgs& a) {
  for (int i = 0; i < n; ++i) {
    const int b = b0 + i;
    const int64_t* r = desc + (int64_t)b * WM2F_COPY_PASTE_DESC_LEN;
    WM2F_REQUIRE(r[0] >= -1 && r[0] < B && r[0] != b, "%s: image %d: source = %lld, expected -1 or another image of the batch",
                 who, b, (long long)r[0]);
    WM2F_REQUIRE(r[1] >= -kMaxShift && r[1] <= kMaxShift && r[2] >= -kMaxShift && r[2] <= kMaxShift,
                 "%s: image %d: shift (%lld, %lld) outside +-%d", who, b, (long long)r[1], (long long)r[2], kMaxShift);
    WM2F_REQUIRE(r[3] >= 0 && r[3] <= H && r[4] >= 0 && r[4] <= W, "%s: image %d: window (%lld, %lld) outside the (%d, %d) frame",
                 who, b, (long long)r[3], (long long)r[4], H, W);
    a.d[i] = CpDesc{(int)r[0], (int)r[1], (int)r[2], (int)r[3], (int)r[4]};
  }
  return WM2F_OK;
}

unsigned blocks_x(int H, int W, int vec) {
  const int64_t n = (int64_t)H * (W / vec);
  const int64_t g = ceil_div64(n, (int64_t)kThreads * kItems);
  return (unsigned)(g < 1 ? 1 : (g > kMaxBlocksX ? kMaxBlocksX : g));
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int wm2f_copy_paste_select(const int32_t* maps, const int32_t* lut_in, int32_t* lut_out, int32_t* areas,
                                      int32_t* workspace, const int64_t* desc, int B, int H, int W, int64_t num,
                                      int64_t den, void* stream) {
  const char* who = "wm2f_copy_paste_select";
  WM2F_REQUIRE(maps && lut_in && lut_out && areas && workspace && desc, "%s: null pointer", who);
  int rc = check_frame(who, B, H, W);
  if (rc != WM2F_OK) return rc;
  rc = check_fraction(who, num, den);
  if (rc != WM2F_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = W % 4 == 0 && aligned16(maps);
  if (hipMemsetAsync(workspace, 0, (size_t)B * kIds * sizeof(int32_t), st) != hipSuccess) {
    set_error("%s: clearing the workspace failed", who);
    return WM2F_ELAUNCH;
  }
  hipLaunchKernelGGL(cp_zero_rows_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, areas, 2, 1);
  for (int b0 = 0; b0 < B; b0 += kCpMaxImages) {
    const int n = B - b0 < kCpMaxImages ? B - b0 : kCpMaxImages;
    CpArgs a = {};
    rc = fill_args(who, desc, B, H, W, b0, n, a);
    if (rc != WM2F_OK) return rc;
    if (vec)
      hipLaunchKernelGGL(cp_count_kernel<4>, dim3(blocks_x(H, W, 4), (unsigned)n), dim3(kThreads), 0, st, maps, lut_in, areas,
                         workspace, a, b0, H, W);
    else
      hipLaunchKernelGGL(cp_count_kernel<1>, dim3(blocks_x(H, W, 1), (unsigned)n), dim3(kThreads), 0, st, maps, lut_in, areas,
                         workspace, a, b0, H, W);
    hipLaunchKernelGGL(cp_strike_kernel, dim3((unsigned)n), dim3(kThreads), 0, st, lut_in, areas, workspace, lut_out, a, b0,
                       num, den);
  }
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_copy_paste(const float* pixels_in, const int32_t* maps_in, const int32_t* lut, float* pixels_out,
                               int32_t* maps_out, int32_t* areas, const int64_t* desc, int B, int C, int H, int W,
                               void* stream) {
  const char* who = "wm2f_copy_paste";
  WM2F_REQUIRE(pixels_in && maps_in && lut && pixels_out && maps_out && areas && desc, "%s: null pointer", who);
  int rc = check_frame(who, B, H, W);
  if (rc != WM2F_OK) return rc;
  WM2F_REQUIRE(C > 0 && C <= 1024, "%s: C = %d, expected 1 .. 1024", who, C);
  WM2F_REQUIRE((const void*)pixels_in != (const void*)pixels_out && maps_in != maps_out, "%s: the call is out of place", who);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = W % 4 == 0 && aligned16(pixels_in) && aligned16(pixels_out) && aligned16(maps_in) && aligned16(maps_out);
  hipLaunchKernelGGL(cp_zero_rows_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, areas, 0, 2);
  for (int b0 = 0; b0 < B; b0 += kCpMaxImages) {
    const int n = B - b0 < kCpMaxImages ? B - b0 : kCpMaxImages;
    CpArgs a = {};
    rc = fill_args(who, desc, B, H, W, b0, n, a);
    if (rc != WM2F_OK) return rc;
    const uint32_t* pin = reinterpret_cast<const uint32_t*>(pixels_in);
    uint32_t* pout = reinterpret_cast<uint32_t*>(pixels_out);
    if (vec)
      hipLaunchKernelGGL(cp_paste_kernel<4>, dim3(blocks_x(H, W, 4), (unsigned)n), dim3(kThreads), 0, st, pin, maps_in, lut,
                         pout, maps_out, areas, a, b0, C, H, W);
    else
      hipLaunchKernelGGL(cp_paste_kernel<1>, dim3(blocks_x(H, W, 1), (unsigned)n), dim3(kThreads), 0, st, pin, maps_in, lut,
                         pout, maps_out, areas, a, b0, C, H, W);
  }
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_copy_paste_prune(int32_t* maps, const int32_t* areas, int B, int H, int W, int64_t num, int64_t den,
                                     int ignore_index, void* stream) {
  const char* who = "wm2f_copy_paste_prune";
  WM2F_REQUIRE(maps && areas, "%s: null pointer", who);
  int rc = check_frame(who, B, H, W);
  if (rc != WM2F_OK) return rc;
  rc = check_fraction(who, num, den);
  if (rc != WM2F_OK) return rc;
  WM2F_REQUIRE(ignore_index < 0 || ignore_index > 254, "%s: ignore_index = %d is an instance id", who, ignore_index);
  if (num == 0) return WM2F_OK;  // nothing can fail after * den >= 0
  hipStream_t st = (hipStream_t)stream;
  if (W % 4 == 0 && aligned16(maps))
    hipLaunchKernelGGL(cp_prune_kernel<4>, dim3(blocks_x(H, W, 4), (unsigned)B), dim3(kThreads), 0, st, maps, areas, H, W, num,
                       den, ignore_index);
  else
    hipLaunchKernelGGL(cp_prune_kernel<1>, dim3(blocks_x(H, W, 1), (unsigned)B), dim3(kThreads), 0, st, maps, areas, H, W, num,
                       den, ignore_index);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
