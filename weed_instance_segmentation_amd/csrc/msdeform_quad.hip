// K1, streaming quad kernel: multi-scale deformable attention for the encoder's own shape
// (3 levels ordered coarse -> fine with sides 1 : 2 : 4 or close to it, 4 points, head_dim 32, queries == tokens).
// Same arithmetic as msdeform.hip / msdeform_tiled.hip (transformers modeling_mask2former.py:798-837,
// fused prologue :983-1002); this file changes WHO computes what and WHEN the windows arrive.
//
// What the LDS-window kernel (msdeform_tiled.hip) measured as its two limits, and the answer here:
//  1. Instruction issue in the gather: with 4 lanes per query every lane repeated the whole
//     coordinate / weight arithmetic of all 12 points (84 VALU per lane and point, 16 of them the
//     FMAs).  Here lane j of a query's quad owns point j of every level: it computes that point's
//     window address and four corner weights ONCE, and the quad shares them with DPP quad_perm
//     broadcasts (v_mov_b32_dpp, 5 per point) -- about 37 VALU per lane and point.
//  2. Staging and gather ran back to back (one 149.5-KiB workgroup per CU).  Here every thread
//     keeps the accumulators of its (up to 3) queries in registers, the LEVELS are the phases and
//     each level's window is its own __shared__ array: two loader waves keep the window of the
//     next phase in flight by LDS-DMA while the gather waves read the current one (below).
//  Bank conflicts: a quad reads 64 contiguous bytes per ds_read_b128 and the four quads of a
//  16-lane LDS group would all land on the same 16 banks (pixel stride 128 B); the quads alternate
//  which 64-B half of the pixel they read first, so they spread over all four 16-bank blocks.
//
// Window geometry is compile-time: tile 16 x 16 finest-level pixels, margin 4 -> 14^2, 18^2, 26^2
// pixels x 128 B = 25 + 41 + 85 KiB.
// Points whose 2 x 2 footprint leaves the window take the slow path (global loads), as before.
//
// Roofline: HBM, algorithmic bytes as msdeform.hip (550 502 400 B per launch at config 2).
#include "msdeform_tiled.h"
#include <type_traits>

// Cache-policy bits (gfx940+: 1 = sc0, 2 = nt, 16 = sc1) of the streaming kernel's three global streams: window DMA,
// operand rows, output rows.  Overridable at compile time for A/B builds (tools/kbench.py --lib).
#ifndef WM2F_DMA_AUX
#define WM2F_DMA_AUX 0
#endif
#ifndef WM2F_OP_AUX
#define WM2F_OP_AUX 0
#endif
#ifndef WM2F_ST_AUX
#define WM2F_ST_AUX 0
#endif

namespace wm2f {

namespace {

constexpr int kQF = 16, kQM = 4, kPasses = 3;
template <int LV> struct Win {
  static constexpr int side = (kQF >> (2 - LV)) + 2 * kQM + 2;  // 14, 18, 26
  static constexpr int npix = side * side;
  static constexpr int chunks = (npix + 7) / 8;                 // 1-KiB LDS-DMA pieces (8 pixels x 128 B): 25, 41, 85
};

struct QuadGeom {
  int W0, H0;  // coarsest level; in an exact pyramid level l is (H0 << l, W0 << l)
  int tiles_x, tiles_y;
  int start[3];
  int a_qstride, b_qstride;
  // any 3-level pyramid ordered coarse -> fine (sizes that are not multiples of 32 give 25x42 / 50x84 /
  // 100x167 ...): the level sizes, their reciprocals, and 1 / (2 W_fine), 1 / (2 H_fine) for the tile -> query arithmetic
  int W[3], H[3], exact;
  float inv_w[3], inv_h[3], inv_2wf, inv_2hf;
};

// MODE 7: the kernel with in-kernel time stamps (s_memtime), read back with wm2f_debug_stamps.  A profiling aid; no
// other mode touches this buffer.
// The stamp buffer -- the library's only device global -- and every ablation / stamped instantiation exist in the
// PROFILING build alone (libwm2f_prof.so, -DWM2F_PROFILING, include/wm2f_prof.h); the production library carries
// MODE 0 kernels only and no global mutable state.
#ifdef WM2F_PROFILING
constexpr int kStampSlots = 160, kStampGroups = 8192;  // 10 waves x 16 slots per workgroup
__device__ long long g_stamps[kStampGroups * kStampSlots];
#endif

template <int K>
__device__ __forceinline__ float bcast(float v) {  // value of lane K of this lane's quad
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), K * 0x55, 0xF, 0xF, true));
}
template <int K>
__device__ __forceinline__ int bcast(int v) {
  return __builtin_amdgcn_mov_dpp(v, K * 0x55, 0xF, 0xF, true);
}
__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true)));
  return fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true)));
}
__device__ __forceinline__ float quad_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
  return v + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));
}

constexpr int waitcnt_vm(int n) { return (n & 15) | (0x7 << 4) | (0xF << 8) | ((n >> 4) << 14); }  // vmcnt(n) only

// s_waitcnt vmcnt(N) that survives the compiler's own wait insertion.  While an LDS-DMA is pending,
// SIInsertWaitcnts answers ANY vmcnt need of the next instruction with vmcnt(0) (it treats the DMA
// as a flat access that may complete out of order) and folds that into a directly preceding wait.
// The s_nop needs nothing, so the counted wait is emitted as written and entered in the pass's
// scoreboard; the loads it covers are then known complete when their first user follows.
// Workgroup barrier without the memory-model fence of __syncthreads(): the fence makes the compiler
// drain vmcnt while LDS-DMA is pending.  What the fence would order is ordered here by hand: a
// window is read only behind the counted wait of every wave (wait_vm) plus this barrier, and the
// "memory" clobbers keep the compiler from moving LDS accesses across it.
__device__ __forceinline__ void wg_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(waitcnt_vm(N));
  asm volatile("s_nop 0");
  __builtin_amdgcn_sched_barrier(0);
}

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using u32x2q = __attribute__((ext_vector_type(2))) unsigned;
typedef __bf16 bf16x2q_t __attribute__((ext_vector_type(2)));
typedef float f32x2c_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_bf16_rne(float lo, float hi) {  // v_cvt_pk_bf16_f32
  const f32x2c_t v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2q_t));
}
using f32x4q = __attribute__((ext_vector_type(4))) float;

struct Acc {
  f32x2 a_lo, a_hi, b_lo, b_hi;  // first-read half (4 channels), second-read half
};

// Window requests: a wave-instruction (buffer_load_dwordx4 ... lds) moves 8 pixels x 128 B, lane-linear in LDS, through a
// descriptor of this (image, head, level) slab and a 32-bit byte offset per lane; a pixel outside the image gets an offset
// that fails the descriptor's range check, and the hardware then writes zeros to LDS (tools/probes/lds_dma_oob.hip) = zero
// padding.  Every loader issues a FIXED number of requests per window, so that its waits can count them; the few requests
// beyond the last piece fetch that last piece again (same bytes to the same place).
// (A separate landing pad for them would be cheaper on the memory side, but a conditional LDS-DMA
// into a second LDS object makes the compiler's LDS-DMA tracking give up and drain vmcnt to 0
// before the first window read -- measured on the ISA.)
constexpr unsigned kOobOffset = 0x80000000u;

// What a lane publishes to its quad for one (query, level): its point's top-left corner (byte offset
// in the window) and the four corner weights, attention weight folded in; zeros when the point is
// not inside the window (slow path) or the query slot is empty.
struct Prod {
  int addr;
  float w00, w01, w10, w11;
};

// `base`: the window's LDS byte address -- the published address is absolute and a consumer needs one add (its lane
// offset) per half.
template <int LV>
__device__ __forceinline__ Prod produce(float px, float py, float aw, int wx0, int wy0, bool valid, unsigned& slow,
                                        int base) {
  constexpr int WW = Win<LV>::side;
  const float x0f = floorf(px), y0f = floorf(py);
  const int xr = (int)x0f - wx0, yr = (int)y0f - wy0;
  const bool fast = ((unsigned)xr < (unsigned)(WW - 1)) & ((unsigned)yr < (unsigned)(WW - 1));
  const bool use = fast & valid;
  Prod p;
  p.addr = base + (use ? (yr * WW + xr) * 128 : 0);
  const float a = use ? aw : 0.f;
  slow |= (valid & !fast) ? (1u << LV) : 0u;
  const float fx1 = px - x0f, fy1 = py - y0f;
  const float a1 = a * fy1, a0 = a - a1;
  p.w01 = a0 * fx1;
  p.w00 = a0 - p.w01;
  p.w11 = a1 * fx1;
  p.w10 = a1 - p.w11;
  return p;
}

// The corner reads of one point: 8 x 16 B (2 halves x 4 corners).  ONE such buffer rolls through a phase: as soon as the
// FMA of corner i has issued, the read of the next point's corner i refills the same registers, so 7 to 8 reads stay in
// flight per wave at a cost of 32 registers (double-buffering whole points cost 72 and spilled).
struct Corners {
  float4 v[8];
};
typedef const __attribute__((address_space(3))) float4* lds_cf4_t;
struct PointAddr {  // where the quad reads a point, and its four corner weights
  int a1, a2;       // absolute LDS byte addresses of the first- and second-read half (the producer folded the window base in)
  float q[4];
};

template <int LV, int K>
__device__ __forceinline__ PointAddr point_addr(const Prod& p, int off1, int off2) {
  PointAddr a;
  const int ak = bcast<K>(p.addr);
  a.q[0] = bcast<K>(p.w00);
  a.q[1] = bcast<K>(p.w01);
  a.q[2] = bcast<K>(p.w10);
  a.q[3] = bcast<K>(p.w11);
  a.a1 = ak + off1;
  a.a2 = ak + off2;
  return a;
}

template <int LV, int I, int MODE>
__device__ __forceinline__ float4 read_corner(const PointAddr& a) {
  constexpr int WW = Win<LV>::side;
  constexpr int o = (I & 1) * 8 + ((I >> 1) & 1) * WW * 8;  // corner order: 00, 01, 10, 11 (float4 units)
  if (MODE == 4) {  // ablation: no LDS reads
    asm volatile("" ::"v"(a.a1), "v"(a.a2));
    return make_float4(a.q[0], a.q[1], a.q[2], a.q[3]);
  }
  // an LDS address held as an integer; the cast chain keeps the access a ds_read (address-space inference)
  const float4* gp = (const float4*)reinterpret_cast<lds_cf4_t>((size_t)((I < 4 ? a.a1 : a.a2) + o * 16));
  return *gp;
}

// One level for all kPasses queries of the lane: 12 points (pass t, producer lane k), see Corners.
template <int LV, int GI, int I, int MODE>
__device__ __forceinline__ void corner_steps(Acc& acc, Corners& cr, const PointAddr& cur, const PointAddr& nxt) {
  if constexpr (I < 8) {
    if (I < 4) pk_fma4(acc.a_lo, acc.a_hi, cur.q[I & 3], cr.v[I]);
    else pk_fma4(acc.b_lo, acc.b_hi, cur.q[I & 3], cr.v[I]);
    if constexpr (GI + 1 < kPasses * 4) cr.v[I] = read_corner<LV, I, MODE>(nxt);
    __builtin_amdgcn_sched_barrier(0);
    corner_steps<LV, GI, I + 1, MODE>(acc, cr, cur, nxt);
  }
}

template <int LV, int GI, int MODE>
__device__ __forceinline__ void pipe_step(Acc (&acc)[kPasses], const Prod (&pr)[kPasses], int off1, int off2, Corners& cr,
                                          const PointAddr& cur, bool skip_last) {
  if constexpr (GI < kPasses * 4) {
    if (GI == (kPasses - 1) * 4 && skip_last) return;  // wave-uniform: the last pass holds no query in this wave
    PointAddr nxt = cur;
    if constexpr (GI + 1 < kPasses * 4) nxt = point_addr<LV, (GI + 1) & 3>(pr[(GI + 1) >> 2], off1, off2);
    __builtin_amdgcn_sched_barrier(0);
    corner_steps<LV, GI, 0, MODE>(acc[GI >> 2], cr, cur, nxt);
    // Pin the sums here: the accumulators are only stored at the very end, and LLVM's code sinking otherwise
    // moves whole FMA chains down there (every corner then stays live across all three phases: 500+ spills).
    asm volatile("" : "+v"(acc[GI >> 2].a_lo), "+v"(acc[GI >> 2].a_hi), "+v"(acc[GI >> 2].b_lo), "+v"(acc[GI >> 2].b_hi));
    pipe_step<LV, GI + 1, MODE>(acc, pr, off1, off2, cr, nxt, skip_last);
  }
}

template <int LV, int I, int MODE>
__device__ __forceinline__ void first_reads(Corners& cr, const PointAddr& a) {
  if constexpr (I < 8) {
    cr.v[I] = read_corner<LV, I, MODE>(a);
    first_reads<LV, I + 1, MODE>(cr, a);
  }
}

template <int LV, int MODE>
__device__ __forceinline__ void gather_phase(const float4* win, Acc (&acc)[kPasses], const float (&px)[kPasses][3],
                                             const float (&py)[kPasses][3], const float (&wt)[kPasses][3],
                                             const bool (&valid)[kPasses], int wx0, int wy0, unsigned (&slow)[kPasses],
                                             int off1, int off2, bool skip_last) {
  Prod pr[kPasses];
  const int base = (int)(size_t)(lds_cf4_t)win;
#pragma unroll
  for (int t = 0; t < kPasses; ++t)
    pr[t] = produce<LV>(px[t][LV], py[t][LV], wt[t][LV], wx0, wy0, valid[t], slow[t], base);
  Corners cr;
  const PointAddr a0 = point_addr<LV, 0>(pr[0], off1, off2);
  first_reads<LV, 0, MODE>(cr, a0);
  __builtin_amdgcn_sched_barrier(0);
  pipe_step<LV, 0, MODE>(acc, pr, off1, off2, cr, a0, skip_last);
}

// Slow path for one point and 4 channels: per-corner image-bounds checks, corners from global memory.
__device__ __forceinline__ void quad_point_slow(float4& acc, const float* __restrict__ vlev, int Hl, int Wl,
                                                int row_stride, float x, float y, float aw) {
  if (!(x > -1.f && x < (float)Wl && y > -1.f && y < (float)Hl)) return;
  const float x0f = floorf(x), y0f = floorf(y);
  const int x0 = (int)x0f, y0 = (int)y0f;
  const float fx1 = x - x0f, fy1 = y - y0f, fx0 = 1.f - fx1, fy0 = 1.f - fy1;
  const bool xl = x0 >= 0, xr = x0 + 1 < Wl, yt = y0 >= 0, yb = y0 + 1 < Hl;
  const float* p00 = vlev + (int64_t)(y0 * Wl + x0) * row_stride;
  if (yt && xl) fma4s(acc, aw * fy0 * fx0, ld4g(p00));
  if (yt && xr) fma4s(acc, aw * fy0 * fx1, ld4g(p00 + row_stride));
  if (yb && xl) fma4s(acc, aw * fy1 * fx0, ld4g(p00 + (int64_t)Wl * row_stride));
  if (yb && xr) fma4s(acc, aw * fy1 * fx1, ld4g(p00 + (int64_t)(Wl + 1) * row_stride));
}

// =====================================================================================================
// Persistent workgroups, two loader waves.
//
// Issuing a tile's 168 LDS-DMA requests (accepted at the rate the memory side delivers, ~46 cycles each), the per-tile
// set-up and the barriers behind them need no gather wave -- with a workgroup per tile and every wave staging before it
// gathered they were 15.5k of a workgroup's 31.7k cycles (profiles/r01_k1_quad_stamps.json).  So:
//   * one workgroup per CU stays resident and walks over its tiles (grid = CUs, XCD-contiguous tile ranges).  The LDS is
//     busy for about half of a tile's 21k cycles, but a second, smaller workgroup per CU to fill the rest ran 18 % slower:
//     the request path, not the LDS, is what it runs into;
//   * waves 8 and 9 only move data: they keep the window of the NEXT phase in flight while waves 0-7 gather
//     the current one.  The three windows form the ring: under the coarse and the mid gather of tile n its fine window
//     is requested (in two parts), under the fine gather the coarse and mid windows of tile n + 1.  Hand-over is one
//     s_barrier per phase (10 waves), the loaders join it behind a counted vmcnt that covers exactly the window about
//     to be read;
//   * a loader's per-lane request offsets depend on (level, piece, lane) only: computed once into registers,
//     a request then costs one v_add (tile origin) -- plus a column test on tiles at the left / right image
//     border; rows above / below the image fail the descriptor's range check by themselves;
//   * the gather waves fetch the NEXT tile's locations / weights under the fine gather of the current one,
//     and their decode of "which query is mine" is cached while the tile shape (full / ragged) stays the same.
// The gather waves never see an LDS-DMA in their instruction stream, so the compiler's wait insertion needs
// no help there; the loaders never read LDS.
#ifndef WM2F_STREAM_GATHER_WAVES
#define WM2F_STREAM_GATHER_WAVES 8
#endif
constexpr int kGatherWaves = WM2F_STREAM_GATHER_WAVES;  // 8 or 10 (10: 3 waves on every SIMD at the same 168 registers; measured 3 % slower)
constexpr int kLoaders = 2, kStreamThreads = (kGatherWaves + kLoaders) * 64;
template <int LV> struct LWin {
  static constexpr int n = (Win<LV>::chunks + kLoaders - 1) / kLoaders;  // requests per loader: 13, 21, 43
};
static_assert(LWin<0>::n == 13 && LWin<1>::n == 21 && LWin<2>::n == 43, "vmcnt constants of the loader");

// MODE 7 stamps: the workgroup's SECOND tile (steady state); slots 0-9 by wave 0 (gather),
// 10-15 by wave 8 (loader).
#ifdef WM2F_PROFILING
#define WM2F_SSTAMP(slot, who)                                                                              \
  do { /* every wave of the role stamps its own row: [workgroup][wave][slot], second tile of the workgroup */ \
    if (MODE == 7 && k == 1 && lane == 0 && blockIdx.x < kStampGroups)                                      \
      g_stamps[blockIdx.x * kStampSlots + wave * 16 + (slot)] = (long long)__builtin_readcyclecounter();    \
  } while (0)
#else
#define WM2F_SSTAMP(slot, who) do { } while (0)
#endif

struct StreamGeom {
  QuadGeom q;
  int n_logical, per_xcd, wg_per_xcd;
  float inv_heads, inv_ntiles, inv_tiles_x;
  // a workgroup's next tile is `wg_per_xcd` ids further: (step_t tiles, step_h heads) with heads innermost -- or, in SLAB
  // order (tiles innermost: id = (image * heads + head) * n_tiles + tile), step_h slabs and step_t = (step_ty, step_tx) tiles
  int step_t, step_h, step_tx, step_ty;
  // unused (they steered a strip tile order that was removed: DESIGN.md 9.1); kept so that the kernel arguments stay where they were
  int unused_i[3];
  float unused_f[3];
  // layout of `value` in floats: pixel pitch, and the head / image strides -- (B, S, heads, 32) or head-major (heads, B, S, 32)
  int v_pix;
  long long v_head, v_img;
};

// exact floor(a / d) for 0 <= a < 2^22 with inv ~ 1/d (one correction step either way)
__device__ __forceinline__ int div_small(int a, int d, float inv) {
  int q = (int)(((float)a + 0.5f) * inv);
  int r = a - q * d;
  if (r < 0) { --q; r += d; }
  if (r >= d) { ++q; }
  return q;
}

struct TileId {
  int b, h, tx, ty;
};

// One tile (16 x 16 finest-level pixels) seen from level l: the queries whose reference point (q + 0.5) / n falls into
// the tile -- columns [qx0, qx0 + nqx), rows [qy0, qy0 + nqy) -- and the window origin, floor(first sampled pixel) - margin,
// where a reference point x in [tx 16 / W_f, (tx + 1) 16 / W_f) lands on pixel x W_l - 0.5 of level l.  In an exact
// 1 : 2 : 4 pyramid these are tx * f, f, tx * f - 1 - margin with f = 4 << l; in general they need a division per bound
// (exact float divisions: the host checks the operands stay below 2^22).
struct LevelTile {
  int wx0, wy0, qx0, qy0, nqx, nqy;
};
__device__ __forceinline__ void axis_tile(int t, int n, int nf, float inv_2nf, int& w0, int& q0, int& nq) {
  // first query at or beyond the tile's lower edge: q >= (2 t 16 n - nf) / (2 nf), rounded up (msdeform_tiled.h: q_lo)
  auto lo = [&](int tt) {
    const int a = 2 * tt * kQF * n - nf;
    if (a <= 0) return 0;
    const int v = div_small(a + 2 * nf - 1, 2 * nf, inv_2nf);
    return v > n ? n : v;
  };
  q0 = lo(t);
  nq = lo(t + 1) - q0;
  const int a = 2 * t * kQF * n - nf;  // floor(t 16 n / nf - 0.5) = floor(a / (2 nf)); a < 0 only for t = 0: -1
  w0 = (a < 0 ? -1 : div_small(a, 2 * nf, inv_2nf)) - kQM;
}
__device__ __forceinline__ LevelTile level_tile(const QuadGeom& g, int l, int tx, int ty) {
  LevelTile r;
  if (g.exact || l == 2) {
    const int fq = kQF >> (2 - l);
    r.qx0 = tx * fq;
    r.qy0 = ty * fq;
    r.wx0 = r.qx0 - 1 - kQM;
    r.wy0 = r.qy0 - 1 - kQM;
    const int nx = g.W[l] - r.qx0, ny = g.H[l] - r.qy0;
    r.nqx = nx < 0 ? 0 : (nx > fq ? fq : nx);
    r.nqy = ny < 0 ? 0 : (ny > fq ? fq : ny);
    return r;
  }
  axis_tile(tx, g.W[l], g.W[2], g.inv_2wf, r.wx0, r.qx0, r.nqx);
  axis_tile(ty, g.H[l], g.H[2], g.inv_2hf, r.wy0, r.qy0, r.nqy);
  return r;
}

// Position of a persistent workgroup in its tile sequence (all wave-uniform): image, head, and the tile's index within
// the image in WORK order.  One division chain at the start, then additions.
struct TileWalk {
  int b, h, tile, tx, ty;  // tx, ty: kept incrementally in raster order (no division on the per-tile path)
};
__device__ __forceinline__ void walk_xy(TileWalk& w, const StreamGeom& sg) {  // (tx, ty) of w.tile by division: start-up only
  w.ty = div_small(w.tile, sg.q.tiles_x, sg.inv_tiles_x);
  w.tx = w.tile - w.ty * sg.q.tiles_x;
}
template <bool SLAB>
__device__ __forceinline__ TileWalk walk_init(int id, const StreamGeom& sg, int heads) {
  TileWalk w;
  const int n_tiles = sg.q.tiles_x * sg.q.tiles_y;
  if (SLAB) {  // slab order: the tiles of one (image, head) slab are consecutive ids
    const int bh = div_small(id, n_tiles, sg.inv_ntiles);
    w.tile = id - bh * n_tiles;
    w.b = div_small(bh, heads, sg.inv_heads);
    w.h = bh - w.b * heads;
    walk_xy(w, sg);
    return w;
  }
  const int bt = div_small(id, heads, sg.inv_heads);
  w.h = id - bt * heads;
  w.b = div_small(bt, n_tiles, sg.inv_ntiles);
  w.tile = bt - w.b * n_tiles;
  walk_xy(w, sg);
  return w;
}
// Next tile of this workgroup: `step_h` heads and `step_t` tiles further.  The tile coordinates advance with a few scalar
// adds and compares per step (per-wave stamps: the division chains, the kernel-argument reloads they dragged in and the
// waits behind them had made this block 3 - 6 k cycles of a 21 k-cycle tile).
template <bool SLAB>
__device__ __forceinline__ void walk_step(TileWalk& w, const StreamGeom& sg, int heads) {
  const int n_tiles = sg.q.tiles_x * sg.q.tiles_y;
  if (SLAB) {  // tile = ty * tiles_x + tx stays true throughout: a wrap of the tile index is a wrap of ty
    w.tile += sg.step_t;
    w.tx += sg.step_tx;
    w.ty += sg.step_ty;
    w.h += sg.step_h;
    if (w.tx >= sg.q.tiles_x) {
      w.tx -= sg.q.tiles_x;
      ++w.ty;
    }
    if (w.tile >= n_tiles) {
      w.tile -= n_tiles;
      w.ty -= sg.q.tiles_y;
      ++w.h;
    }
    while (w.h >= heads) {
      w.h -= heads;
      ++w.b;
    }
    return;
  }
  int adv = sg.step_t;
  w.h += sg.step_h;
  if (w.h >= heads) {
    w.h -= heads;
    ++adv;
  }
  w.tile += adv;
  while (w.tile >= n_tiles) {
    w.tile -= n_tiles;
    ++w.b;
  }
  for (int i = 0; i < adv; ++i) {
    if (++w.tx == sg.q.tiles_x) {
      w.tx = 0;
      if (++w.ty == sg.q.tiles_y) w.ty = 0;
    }
  }
}
__device__ __forceinline__ TileId walk_tile(const TileWalk& w) {
  TileId t;
  t.b = w.b;
  t.h = w.h;
  t.tx = w.tx;
  t.ty = w.ty;
  return t;
}

template <int LV>
struct LoaderRegs {  // per-lane constants of one loader for one level
  unsigned rel[LWin<LV>::n];  // byte offset of this lane's 16 B relative to the window origin pixel
};

template <int LV>
__device__ __forceinline__ void loader_init(LoaderRegs<LV>& r, int ld, int Wl, int row_bytes, unsigned pix_lane,
                                            unsigned lane_part) {
  using W = Win<LV>;
#pragma unroll
  for (int i = 0; i < LWin<LV>::n; ++i) {
    int c = ld + kLoaders * i;
    c = c < W::chunks ? c : W::chunks - 1;
    const unsigned idx = (unsigned)(c * 8) + pix_lane;
    const unsigned wy = idx / (unsigned)W::side, wx = idx - wy * (unsigned)W::side;
    r.rel[i] = __umul24(__umul24(wy, (unsigned)Wl) + wx, (unsigned)row_bytes) + lane_part;
  }
}

// Requests [I0, I1) of this loader for one window.  tile_off = byte offset of the window origin pixel in the
// slab (negative above / left of the image); x_border: the window sticks out left or right.
typedef __attribute__((address_space(3))) float4* lds4_t;  // an LDS pointer that never passes through a generic one

template <int LV, int I0, int I1>
__device__ __forceinline__ void loader_issue(lds4_t win, const LoaderRegs<LV>& r, __amdgpu_buffer_rsrc_t slab, int ld,
                                             int tile_off, bool x_border, int wx0, int Wl, unsigned pix_lane) {
  using W = Win<LV>;
  static_assert(I0 >= 0 && I1 <= LWin<LV>::n, "request range");
  if (!x_border) {
#pragma unroll
    for (int i = I0; i < I1; ++i) {
      int c = ld + kLoaders * i;
      c = c < W::chunks ? c : W::chunks - 1;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(slab, (lptr_t)(win + c * 64), 16, (int)(r.rel[i] + (unsigned)tile_off), 0, 0, WM2F_DMA_AUX);
    }
  } else {
    // the columns are tile-invariant too, but 77 more live registers do not fit: recompute them per use (the
    // empty asm hides the value from loop-invariant code motion)
    asm volatile("" : "+v"(pix_lane));
#pragma unroll
    for (int i = I0; i < I1; ++i) {
      int c = ld + kLoaders * i;
      c = c < W::chunks ? c : W::chunks - 1;
      const unsigned idx = (unsigned)(c * 8) + pix_lane;
      const int x = wx0 + (int)(idx - (idx / (unsigned)W::side) * (unsigned)W::side);
      const unsigned off = ((unsigned)x < (unsigned)Wl) ? r.rel[i] + (unsigned)tile_off : kOobOffset;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(slab, (lptr_t)(win + c * 64), 16, (int)off, 0, 0, WM2F_DMA_AUX);
    }
  }
}

struct LoaderTile {  // wave-uniform per-tile values of the loaders
  __amdgpu_buffer_rsrc_t slab[3];
  int tile_off[3], wx0[3];
  bool x_border;
};

__device__ __forceinline__ LoaderTile loader_tile(const float* value, const StreamGeom& sg, const TileId& t, int S, int heads) {
  const QuadGeom& g = sg.q;
  const int row_stride = sg.v_pix, row_bytes = row_stride * 4;
  const float* vb = value + (int64_t)t.b * sg.v_img + (int64_t)t.h * sg.v_head;  // this head's slice
  LoaderTile lt;
  lt.x_border = false;
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const int Wl = g.W[l];
    const LevelTile lv = level_tile(g, l, t.tx, t.ty);
    lt.wx0[l] = lv.wx0;
    lt.tile_off[l] = (lv.wy0 * Wl + lv.wx0) * row_bytes;
    lt.x_border = lt.x_border || lv.wx0 < 0 || lv.wx0 + (l == 0 ? Win<0>::side : (l == 1 ? Win<1>::side : Win<2>::side)) > Wl;
    const int npx = g.W[l] * g.H[l];
    lt.slab[l] = __builtin_amdgcn_make_buffer_rsrc((void*)(vb + (int64_t)g.start[l] * row_stride), 0,
                                                   (npx - 1) * row_bytes + 128, 0x00020000);
  }
  return lt;
}

// What a gather lane knows about "its" queries for one tile SHAPE (the numbers of queries per level in the tile: the
// same for every interior tile of an exact pyramid), so that a tile costs a handful of instructions per pass instead of a
// decode:
//   q_rel     row * W_lq + col of the query inside its own level, relative to the tile's first query of that level
//   lq        the query's level (0 coarse .. 2 fine);   col, row   its position among the tile's queries of that level
// With the tile's per-level first query (3 scalars) the token is q_rel + first[lq] and the query's column qx0[lq] + col;
// its reference point (qx + 0.5) / W_lq lands on pixel ref * W_l - 0.5 of level l (HF:993-1002 with grid_sample's
// align_corners = False rule), to which the sampling offset is added.
// General pyramids: packed into one register per pass (the kernel sits at its 168-register cap):
// col | row << 8 | lq << 16 | valid << 31.
struct PassConst {
  unsigned code[kPasses];
  __device__ __forceinline__ int col(int t) const { return (int)(code[t] & 255u); }
  __device__ __forceinline__ int row(int t) const { return (int)((code[t] >> 8) & 255u); }
  __device__ __forceinline__ int lq(int t) const { return (int)((code[t] >> 16) & 3u); }
  __device__ __forceinline__ bool valid(int t) const { return (code[t] >> 31) != 0u; }
};
// Exact 1 : 2 : 4 pyramids (the encoder's own shape; the kernel template is instantiated for them separately: the general
// arithmetic cost the production shape 15 %, profiles/r02_kbench_k1_general_vs_exact.jsonl): a query's reference point sits
// at pixel (tx * 4 * 2^l) + (cxs * 2^l - 0.5) of level l with cxs = (col + 0.5) * 2^-lq -- integers and eighths, exact in
// fp32, so the sampling coordinate `that + offset` is rounded once.
struct PassConstExact {
  int q_rel[kPasses], lq[kPasses];
  float cxs[kPasses], cys[kPasses];
  bool valid[kPasses];
};

// OPT: compile-time form of what were run-time switches in the kernel argument.  As run-time fields they put both operand
// paths into the one production kernel: +29 % instructions, 60 more scalar spills, 69 kernel-argument reloads inside the tile
// loop, and 152 -> 166 us on the model's operands (tools/probes/k1_two_libs.py, bisected over the round's commits).
constexpr int kOptLanes = 1;        // lane-major operand rows (wm2f_msdeform_fused_lanes_fwd)
constexpr int kOptAllFull = 8;      // level sides are multiples of the tile: every tile has the full query counts
// SLAB order -- heads outermost.  An XCD's 32 workgroups walk the tiles of ONE (image, head) slab together (2.75 MB of value
// at config 2: it stays in the XCD's 4 MiB L2, so the window halos -- 3.6 x the slab at L2 level -- are fetched from HBM once)
// before the next head; needs head-major operand rows, otherwise a token's 1152-byte row is fetched once per head.  Without
// it: heads innermost, the tiles of an image in plain raster order (strip and Z orders were no faster: DESIGN.md 9.1).
constexpr int kOptSlab = 128;
// The training forward (wm2f_msdeform_rows_fwd): the [offsets | logits] rows are bf16 (the merged projection's output under
// bf16 autocast, read as it is); the output is stored as bf16 (what the output projection reads there).
constexpr int kOptRowsBf16 = 1024, kOptOutBf16 = 2048;

template <bool FUSED, int MODE, bool EXACT, int OPT>
__global__ __launch_bounds__(kStreamThreads, 1) void msdeform_stream_fwd_kernel(
    const float* __restrict__ value, const float* __restrict__ a_in, const float* __restrict__ b_in, float* __restrict__ out,
    StreamGeom sg, int S, int Q, int heads) {
  constexpr int D = 32, NL = 3, P = 4;
  constexpr bool kLanes = FUSED && (OPT & kOptLanes) != 0, kSlab = (OPT & kOptSlab) != 0;
  constexpr int kOpAux = WM2F_OP_AUX, kStAux = WM2F_ST_AUX;
  constexpr bool kRowsLp = FUSED && (OPT & kOptRowsBf16) != 0, kOutLp = (OPT & kOptOutBf16) != 0;
  constexpr int kRowEsz = kRowsLp ? 2 : 4;
  static_assert(!(kRowsLp && (OPT & kOptLanes)), "bf16 rows exist in the token-major [offsets | logits] form only");
  // Lane rows: the 36 floats of a (token, head) record come in 16-byte ALIGNED pieces -- [x0 y0 x1 y1] of lanes 0..3, then
  // [x2 y2 w0 w1] of lanes 0..3, then w2 of lanes 0..3 (include/wm2f.h) -- so that a lane's two dwordx4 loads are 16-byte
  // aligned (nine consecutive floats per lane, a 36-byte lane stride, measured 1 % slower in the model).
  constexpr bool kAligned = kLanes;
  constexpr bool kAllFull = EXACT && (OPT & kOptAllFull) != 0;
  constexpr int kLoaderWave0 = kGatherWaves, kGW = kGatherWaves;
  __shared__ __attribute__((aligned(16))) float4 win0[Win<0>::chunks * 64];
  __shared__ __attribute__((aligned(16))) float4 win1[Win<1>::chunks * 64];
  __shared__ __attribute__((aligned(16))) float4 win2[Win<2>::chunks * 64];
  const QuadGeom& g = sg.q;
  // this workgroup's tiles: ids first + k * stride, k < n_my (XCD-contiguous ranges, as xcd_contiguous_id)
  const int xcd = blockIdx.x % kNumXcd, lw = blockIdx.x / kNumXcd;
  const int range_end = min((xcd + 1) * sg.per_xcd, sg.n_logical) - xcd * sg.per_xcd;  // ids of this XCD: [0, range_end)
  const int n_my = lw < range_end ? (range_end - lw + sg.wg_per_xcd - 1) / sg.wg_per_xcd : 0;
  const int first = xcd * sg.per_xcd + lw;
  if (n_my <= 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row_stride = sg.v_pix, row_bytes = row_stride * 4;

  if (wave >= kLoaderWave0) {
    // ------------------------------------------------------------------ loader waves
    const int ld = wave - kLoaderWave0;
    const unsigned pix_lane = (unsigned)lane >> 3, lane_part = ((unsigned)lane & 7u) * 16u;  // a request moves 8 pixels x 128 B
    LoaderRegs<0> r0;
    LoaderRegs<1> r1;
    LoaderRegs<2> r2;
    loader_init<0>(r0, ld, g.W[0], row_bytes, pix_lane, lane_part);
    loader_init<1>(r1, ld, g.W[1], row_bytes, pix_lane, lane_part);
    loader_init<2>(r2, ld, g.W[2], row_bytes, pix_lane, lane_part);
    // Schedule (per loader; F = fine window split in two parts so that no phase carries much more than a third of
    // a tile's requests -- the requests are accepted at the memory side's pace, ~100 cycles each per loader, and
    // the gather waves wait for the loader at every barrier):
    //   under the coarse gather of tile k:  F(k) part A                      (26 requests)
    //   under the mid gather:               F(k) part B                      (17)
    //   under the fine gather:              coarse(k + 1), mid(k + 1)        (13 + 21)
    // (With coarse(k + 1) requested under the mid gather the loaders were the last to reach Bf(k) in every workgroup, 1.5k
    // cycles behind the gather waves (profiles/r02_k1_stream_stamps_*.json); the coarse window is not needed before
    // Bc(k + 1), a whole fine gather away.)
    constexpr int kFA = 26;
    TileWalk walk = walk_init<kSlab>(first, sg, heads);
    LoaderTile lt = loader_tile(value, sg, walk_tile(walk), S, heads);
    if (MODE != 5) loader_issue<0, 0, LWin<0>::n>((lds4_t)win0, r0, lt.slab[0], ld, lt.tile_off[0], lt.x_border, lt.wx0[0], g.W[0], pix_lane);
    __builtin_amdgcn_sched_barrier(0);
    if (MODE != 5) loader_issue<1, 0, LWin<1>::n>((lds4_t)win1, r1, lt.slab[1], ld, lt.tile_off[1], lt.x_border, lt.wx0[1], g.W[1], pix_lane);
    for (int k = 0; k < n_my; ++k) {
      const bool more = k + 1 < n_my;
      wait_vm<LWin<1>::n>();  // coarse(k) landed; mid(k) may still fly
      WM2F_SSTAMP(10, kLoaderWave0);
      wg_barrier();           // Bc(k): gather waves are done with fine(k-1)
      WM2F_SSTAMP(11, kLoaderWave0);
      if (MODE != 5) loader_issue<2, 0, kFA>((lds4_t)win2, r2, lt.slab[2], ld, lt.tile_off[2], lt.x_border, lt.wx0[2], g.W[2], pix_lane);
      WM2F_SSTAMP(12, kLoaderWave0);
      wait_vm<kFA>();  // mid(k) landed
      wg_barrier();    // Bm(k): gather waves are done with coarse(k)
      WM2F_SSTAMP(13, kLoaderWave0);
      if (MODE != 5) loader_issue<2, kFA, LWin<2>::n>((lds4_t)win2, r2, lt.slab[2], ld, lt.tile_off[2], lt.x_border, lt.wx0[2], g.W[2], pix_lane);
      wait_vm<0>();  // fine(k) landed
      WM2F_SSTAMP(14, kLoaderWave0);
      wg_barrier();  // Bf(k): gather waves are done with mid(k)
      WM2F_SSTAMP(15, kLoaderWave0);
      if (more) {
        walk_step<kSlab>(walk, sg, heads);
        lt = loader_tile(value, sg, walk_tile(walk), S, heads);
        __builtin_amdgcn_sched_barrier(0);
        if (MODE != 5) loader_issue<0, 0, LWin<0>::n>((lds4_t)win0, r0, lt.slab[0], ld, lt.tile_off[0], lt.x_border, lt.wx0[0], g.W[0], pix_lane);
        __builtin_amdgcn_sched_barrier(0);
        if (MODE != 5) loader_issue<1, 0, LWin<1>::n>((lds4_t)win1, r1, lt.slab[1], ld, lt.tile_off[1], lt.x_border, lt.wx0[1], g.W[1], pix_lane);
      }
    }
    return;
  }

  // -------------------------------------------------------------------- gather waves
  const int j = tid & 3, quad = lane >> 2;
  const int xq = (0x73261540 >> ((quad & 7) * 4)) & 7;  // quads 0..7 -> row positions 0,4,5,1,6,2,3,7
  const int slot = wave * 16 + (quad & 8) + xq;
  // Quad -> query and first-read half, chosen for the LDS banks.  A ds_read_b128 is served in 16-lane groups
  // {0-3,12-15,20-27} / {4-11,16-19,28-31}: quads {0,3,5,6} / {1,2,4,7} of each half-wave.  A quad reads 64 B =
  // one of four 16-bank blocks: block = 2 * (pixel & 1) + half.  Group mates that read the same half get
  // NEIGHBOURING queries of a tile row: for an offset field that varies slowly they sample the same pixel
  // (same address: broadcast) or adjacent pixels (other parity), the other pair reads the other half first,
  // so the four quads of a group fall in four different blocks.  (Independent random offsets still collide:
  // 1.75 LDS cycles per group on average, measured 1.71.)
  const int hq = (quad >> 2) & 1;  // which 64-B half of a pixel this quad reads first (a lane owns 4 + 4 channels)
  const int off1 = j * 16 + hq * 64, off2 = j * 16 + (1 - hq) * 64;
  const __amdgpu_buffer_rsrc_t a_rs = __builtin_amdgcn_make_buffer_rsrc((void*)a_in, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t b_rs = __builtin_amdgcn_make_buffer_rsrc((void*)b_in, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t out_rs = __builtin_amdgcn_make_buffer_rsrc((void*)out, 0, 0x7fffffff, 0x00020000);

  typename std::conditional<EXACT, PassConstExact, PassConst>::type pc;
  int shape_key = -1;  // packed (nqx, nqy) per level of the tile shape `pc` was built for
  // operands of a tile: raw loads + where they go
  struct Ops {
    float2 lc[kPasses][NL];
    float wt[kPasses][NL];
    int qrow[kPasses];  // b * Q + token
    bool valid[kPasses];
    int wx0[NL], wy0[NL], qx0[NL], qy0[NL], b, h, tx, ty;
  };
  // reference point of token q (HF:1127-1156): ((column + 0.5) / W_l, (row + 0.5) / H_l) of its own level (slow path only)
  auto ref_point = [&](int q, float& rx, float& ry) __attribute__((always_inline)) {
    const int l = (q >= g.start[1] ? 1 : 0) + (q >= g.start[2] ? 1 : 0);
    const int rel = q - (l == 2 ? g.start[2] : (l == 1 ? g.start[1] : 0));
    const int Wq = l == 2 ? g.W[2] : (l == 1 ? g.W[1] : g.W[0]);
    const float iw = l == 2 ? g.inv_w[2] : (l == 1 ? g.inv_w[1] : g.inv_w[0]), ih = l == 2 ? g.inv_h[2] : (l == 1 ? g.inv_h[1] : g.inv_h[0]);
    const int qy = (int)(((float)rel + 0.5f) * iw), r0 = rel - qy * Wq;
    const int qyc = r0 < 0 ? qy - 1 : (r0 >= Wq ? qy + 1 : qy);  // one correction step: rel can exceed 2^22 / W
    const int qx = rel - qyc * Wq;
    rx = ((float)qx + 0.5f) * iw;
    ry = ((float)qyc + 0.5f) * ih;
  };
  const int a_row = g.a_qstride * kRowEsz, b_row = g.b_qstride * kRowEsz;  // bytes per token in the two operand arrays (< 2^24: host)
  auto fetch = [&](const TileId& t) __attribute__((always_inline)) {
    Ops o;
    o.b = t.b;
    o.h = t.h;
    o.tx = t.tx;
    o.ty = t.ty;
    int nqx[NL], nqy[NL], qfirst[NL], key = 0;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      if constexpr (EXACT) {
        // (window origins are tx * fq - 1 - margin: recomputed where they are used instead of carried in `Ops` -- the
        // kernel's scalar registers are its scarcest resource: every per-tile scalar spilled is a v_readlane or, worse, a
        // kernel-argument reload with its wait on the tile's critical path)
        const int Wl = g.W0 << l, Hl = g.H0 << l, fq = kQF >> (2 - l);
        if (kAllFull) {  // level sides are multiples of the tile: every tile holds fq x fq queries of level l
          nqx[l] = nqy[l] = fq;
        } else {
          int nx = Wl - t.tx * fq, ny = Hl - t.ty * fq;
          nqx[l] = nx < 0 ? 0 : (nx > fq ? fq : nx);
          nqy[l] = ny < 0 ? 0 : (ny > fq ? fq : ny);
        }
        qfirst[l] = t.b * Q + g.start[l] + (t.ty * fq) * Wl + t.tx * fq;  // the tile's first token of level l
      } else {
        const LevelTile lv = level_tile(g, l, t.tx, t.ty);
        o.wx0[l] = lv.wx0;
        o.wy0[l] = lv.wy0;
        o.qx0[l] = lv.qx0;
        o.qy0[l] = lv.qy0;
        nqx[l] = lv.nqx;
        nqy[l] = lv.nqy;
        qfirst[l] = t.b * Q + g.start[l] + lv.qy0 * g.W[l] + lv.qx0;
      }
      key = key * 1024 + nqx[l] * 32 + nqy[l];
    }
    if (key != shape_key) {  // wave-uniform; interior tiles all share one shape
      shape_key = key;
      const int c1 = nqx[0] * nqy[0], c2 = c1 + nqx[1] * nqy[1], nq = c2 + nqx[2] * nqy[2];
#pragma unroll
      for (int t2 = 0; t2 < kPasses; ++t2) {
        // passes 0, 1: all 8 gather waves; the third pass of a full tile (80 queries) goes to waves 0-3 and 7:
        // the loaders share their SIMDs with waves (0, 4) and (1, 5) (waves go to SIMDs cyclically), so waves 4
        // and 5 -- and 6, whose SIMD then carries 3 + 2 passes -- stay at two passes
        // With 10 gather waves two passes cover 320 queries and wave 2 takes the last 16.
        const int w3 = kGW == 8 ? (wave < 4 ? wave : (wave == 7 ? 4 : 1 << 20)) : (wave == 2 ? 0 : 1 << 20);
        int qi = t2 < 2 ? slot + (kGW * 16) * t2 : 2 * (kGW * 16) + w3 * 16 + (quad & 8) + xq;
        const bool ok = qi < nq;
        if (!ok) qi = 0;  // an empty slot shadows the tile's first query (a real token: loads stay in range)
        const bool ge1 = qi >= c1, ge2 = qi >= c2;
        const int lq = (ge1 ? 1 : 0) + (ge2 ? 1 : 0);
        const int nx = ge2 ? nqx[2] : (ge1 ? nqx[1] : nqx[0]);
        const int loc_i = qi - (ge2 ? c2 : (ge1 ? c1 : 0));
        const int nxs = nx < 1 ? 1 : nx;
        const int ly_ = (int)(((float)loc_i + 0.5f) * __builtin_amdgcn_rcpf((float)nxs));  // exact: small integers
        const int lx_ = loc_i - ly_ * nxs;
        if constexpr (EXACT) {
          const float sc = ge2 ? 0.25f : (ge1 ? 0.5f : 1.f);
          pc.valid[t2] = ok;
          pc.lq[t2] = lq;
          pc.q_rel[t2] = (int)__umul24((unsigned)ly_, (unsigned)(g.W0 << lq)) + lx_;
          pc.cxs[t2] = ((float)lx_ + 0.5f) * sc;
          pc.cys[t2] = ((float)ly_ + 0.5f) * sc;
        } else {
          pc.code[t2] = (unsigned)lx_ | ((unsigned)ly_ << 8) | ((unsigned)lq << 16) | (ok ? 0x80000000u : 0u);
        }
      }
    }
#pragma unroll
    for (int t2 = 0; t2 < kPasses; ++t2) {
      int q;
      if constexpr (EXACT) {
        q = pc.q_rel[t2] + (pc.lq[t2] == 2 ? qfirst[2] : (pc.lq[t2] == 1 ? qfirst[1] : qfirst[0]));
        o.valid[t2] = pc.valid[t2];
      } else {
        const int lq = pc.lq(t2);
        q = (int)__umul24((unsigned)pc.row(t2), (unsigned)(lq == 2 ? g.W[2] : (lq == 1 ? g.W[1] : g.W[0]))) + pc.col(t2) +
            (lq == 2 ? qfirst[2] : (lq == 1 ? qfirst[1] : qfirst[0]));
        o.valid[t2] = pc.valid(t2);
      }
      o.qrow[t2] = q;
    }
    const int ah = (o.h * (NL * P * 2) + j * 2) * kRowEsz, bh = (o.h * (NL * P) + j) * kRowEsz;
#pragma unroll
    for (int t2 = 0; t2 < kPasses; ++t2) {
      int q = o.qrow[t2];
      if (MODE == 8) q = o.qrow[0] & ~1023;  // (profiling build, timing ablation: every operand load from one hot record -- same instructions, L2 latency)
      const int a_off = (int)__umul24((unsigned)q, (unsigned)a_row) + ah;
      const int b_off = (int)__umul24((unsigned)q, (unsigned)b_row) + bh;
      if (kLanes) {
        // lane rows (wm2f_msdeform_fused_lanes_fwd): the 36 numbers of head h form one 144-byte record -- a pass is 3 loads
        // (two 16-byte aligned dwordx4, one dword) whose quad footprint lies inside that record, instead of 6 loads
        // scattered over the token's 1152-byte row (16 quads x 6 loads x 8 waves queued
        // in the texture-address unit behind the loaders' traffic: the per-wave stamps showed 3.0k cycles for the older and
        // 5.5k for the younger wave of each SIMD in this fetch)
        // b_row is the HEAD stride of the lane-major array here (144 B inside a 1152-B token row, or a whole (B, Q, 36)
        // slab when the rows are stored head-major)
        const int rec = (int)__umul24((unsigned)q, (unsigned)a_row) + o.h * b_row;
        const int off = rec + (kAligned ? j * 16 : j * 36);
        f32x4q A = {0.f, 0.f, 0.f, 0.f}, Bq = {0.f, 0.f, 0.f, 0.f};
        if (MODE != 6) {  // (MODE 6, profiling build: timing ablation without the gather waves' loads and stores)
          A = __builtin_bit_cast(f32x4q, __builtin_amdgcn_raw_buffer_load_b128(a_rs, off, 0, kOpAux));
          Bq = __builtin_bit_cast(f32x4q, __builtin_amdgcn_raw_buffer_load_b128(a_rs, off + (kAligned ? 64 : 16), 0, kOpAux));
        }
        o.lc[t2][0] = make_float2(A.x, A.y);
        o.lc[t2][1] = make_float2(A.z, A.w);
        o.lc[t2][2] = make_float2(Bq.x, Bq.y);
        o.wt[t2][0] = Bq.z;
        o.wt[t2][1] = Bq.w;
        o.wt[t2][2] = MODE == 6 ? 0.f : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(a_rs, kAligned ? rec + 128 + j * 4 : off + 32, 0, kOpAux));
      } else {
#pragma unroll
        for (int l = 0; l < NL; ++l) {
          if constexpr (kRowsLp) {  // bf16 -> fp32 is a shift: exact
            const unsigned xy = __builtin_amdgcn_raw_buffer_load_b32(a_rs, a_off + l * (P * 2 * 2), 0, kOpAux);
            const unsigned lg = (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(b_rs, b_off + l * (P * 2), 0, kOpAux);
            o.lc[t2][l] = make_float2(__uint_as_float(xy << 16), __uint_as_float(xy & 0xffff0000u));
            o.wt[t2][l] = __uint_as_float(lg << 16);
          } else {
            o.lc[t2][l] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(a_rs, a_off + l * (P * 2 * 4), 0, kOpAux));
            o.wt[t2][l] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(b_rs, b_off + l * (P * 4), 0, kOpAux));
          }
        }
      }
    }
    return o;
  };

  TileWalk walk = walk_init<kSlab>(first, sg, heads);
  Ops nxt = fetch(walk_tile(walk));
  for (int k = 0; k < n_my; ++k) {
    Ops cur = nxt;
    WM2F_SSTAMP(0, 0);
    // ---- per-point pixel coordinates and (fused) softmax weights
    float px[kPasses][NL], py[kPasses][NL], wt[kPasses][NL];
#pragma unroll
    for (int t = 0; t < kPasses; ++t) {
#pragma unroll
      for (int l = 0; l < NL; ++l) wt[t][l] = cur.wt[t][l];
      if (FUSED) {  // softmax over the 12 logits of the quad (HF:986-991)
        const float mx = quad_max(fmaxf(fmaxf(wt[t][0], wt[t][1]), wt[t][2]));
        float s = 0.f;
#pragma unroll
        for (int l = 0; l < NL; ++l) {
          wt[t][l] = __expf(wt[t][l] - mx);
          s += wt[t][l];
        }
        const float inv = __builtin_amdgcn_rcpf(quad_sum(s));
#pragma unroll
        for (int l = 0; l < NL; ++l) wt[t][l] *= inv;
      }
      float refx = 0.f, refy = 0.f;
      if constexpr (FUSED && !EXACT) {  // the query's reference point (`pc` still describes this tile: the next fetch comes later)
        const int lq = pc.lq(t);
        const int qx = pc.col(t) + (lq == 2 ? cur.qx0[2] : (lq == 1 ? cur.qx0[1] : cur.qx0[0]));
        const int qy = pc.row(t) + (lq == 2 ? cur.qy0[2] : (lq == 1 ? cur.qy0[1] : cur.qy0[0]));
        refx = ((float)qx + 0.5f) * (lq == 2 ? g.inv_w[2] : (lq == 1 ? g.inv_w[1] : g.inv_w[0]));
        refy = ((float)qy + 0.5f) * (lq == 2 ? g.inv_h[2] : (lq == 1 ? g.inv_h[1] : g.inv_h[0]));
      }
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        if constexpr (FUSED && EXACT) {
          // loc = ref + off / (W, H); pixel = loc * (W, H) - 0.5 == ref * W - 0.5 + off, with ref * W - 0.5 taken
          // exactly: tile origin + (cxs * 2^l - 0.5)
          px[t][l] = ((float)(cur.tx << (l + 2)) + fmaf(pc.cxs[t], (float)(1 << l), -0.5f)) + cur.lc[t][l].x;
          py[t][l] = ((float)(cur.ty << (l + 2)) + fmaf(pc.cys[t], (float)(1 << l), -0.5f)) + cur.lc[t][l].y;
        } else if constexpr (FUSED) {
          px[t][l] = fmaf(refx, (float)g.W[l], -0.5f) + cur.lc[t][l].x;
          py[t][l] = fmaf(refy, (float)g.H[l], -0.5f) + cur.lc[t][l].y;
        } else {
          const float Wl = (float)g.W[l], Hl = (float)g.H[l];
          px[t][l] = ((2.f * cur.lc[t][l].x - 1.f + 1.f) * Wl - 1.f) * 0.5f;
          py[t][l] = ((2.f * cur.lc[t][l].y - 1.f + 1.f) * Hl - 1.f) * 0.5f;
        }
      }
    }
    Acc acc[kPasses];
    unsigned slow[kPasses];
#pragma unroll
    for (int t = 0; t < kPasses; ++t) {
      acc[t].a_lo = acc[t].a_hi = acc[t].b_lo = acc[t].b_hi = (f32x2){0.f, 0.f};
      slow[t] = 0;
    }
    const bool skip_last = __builtin_amdgcn_ballot_w64(cur.valid[kPasses - 1]) == 0;
    auto wx0_of = [&](int l) __attribute__((always_inline)) { return EXACT ? cur.tx * (kQF >> (2 - l)) - 1 - kQM : cur.wx0[l]; };
    auto wy0_of = [&](int l) __attribute__((always_inline)) { return EXACT ? cur.ty * (kQF >> (2 - l)) - 1 - kQM : cur.wy0[l]; };

    WM2F_SSTAMP(1, 0);
    wg_barrier();  // Bc(k)
    WM2F_SSTAMP(2, 0);
    gather_phase<0, MODE>(win0, acc, px, py, wt, cur.valid, wx0_of(0), wy0_of(0), slow, off1, off2, skip_last);
    WM2F_SSTAMP(3, 0);
    wg_barrier();  // Bm(k)
    WM2F_SSTAMP(4, 0);
    gather_phase<1, MODE>(win1, acc, px, py, wt, cur.valid, wx0_of(1), wy0_of(1), slow, off1, off2, skip_last);
    WM2F_SSTAMP(5, 0);
    wg_barrier();  // Bf(k)
    WM2F_SSTAMP(6, 0);
    if (k + 1 < n_my) {  // lands under the fine gather
      walk_step<kSlab>(walk, sg, heads);
      nxt = fetch(walk_tile(walk));
    }
    __builtin_amdgcn_sched_barrier(0);
    WM2F_SSTAMP(7, 0);
    gather_phase<2, MODE>(win2, acc, px, py, wt, cur.valid, wx0_of(2), wy0_of(2), slow, off1, off2, skip_last);
    WM2F_SSTAMP(8, 0);

    // ---- slow points (rare), then the stores
    const float* vb = value + (int64_t)cur.b * sg.v_img + (int64_t)cur.h * sg.v_head;
    const bool wave_slow = __builtin_amdgcn_ballot_w64((slow[0] | slow[1] | slow[2]) != 0) != 0;
#pragma unroll
    for (int t = 0; t < kPasses; ++t) {
      float4 r1 = make_float4(acc[t].a_lo.x, acc[t].a_lo.y, acc[t].a_hi.x, acc[t].a_hi.y);
      float4 r2 = make_float4(acc[t].b_lo.x, acc[t].b_lo.y, acc[t].b_hi.x, acc[t].b_hi.y);
      if (wave_slow && cur.valid[t]) {
        unsigned todo = (unsigned)bcast<0>((int)slow[t]) | ((unsigned)bcast<1>((int)slow[t]) << 3) |
                        ((unsigned)bcast<2>((int)slow[t]) << 6) | ((unsigned)bcast<3>((int)slow[t]) << 9);
        constexpr bool lm = kLanes;  // lane-major rows: point k2 of level l sits at [k2 * 9 + 2 * l], its logit at [k2 * 9 + 6 + l]
        // (element offsets: the rows are fp32, or bf16 in the training form)
        const int64_t ap_e = lm ? (int64_t)cur.qrow[t] * g.a_qstride + (int64_t)cur.h * g.b_qstride
                                : (int64_t)cur.qrow[t] * g.a_qstride + cur.h * (NL * P * 2);
        const int64_t bp_e = lm ? ap_e : (int64_t)cur.qrow[t] * g.b_qstride + cur.h * (NL * P);
        const float* b_base = lm ? a_in : b_in;
        auto row_a = [&](int i) __attribute__((always_inline)) {
          if constexpr (kRowsLp) return __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(a_in)[ap_e + i] << 16);
          else return a_in[ap_e + i];
        };
        auto row_b = [&](int i) __attribute__((always_inline)) {
          if constexpr (kRowsLp) return __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(b_base)[bp_e + i] << 16);
          else return b_base[bp_e + i];
        };
        // where point k2 of level l keeps its x (y follows) and its logit inside the 36-float record
        auto xy_at = [&](int k2, int l) __attribute__((always_inline)) {
          return kAligned ? (l < 2 ? k2 * 4 + 2 * l : 16 + k2 * 4) : (lm ? k2 * 9 + 2 * l : (l * P + k2) * 2);
        };
        auto logit_at = [&](int i) __attribute__((always_inline)) {  // i = l * P + k2
          const int k2 = i & 3, l = i >> 2;
          return kAligned ? row_b(l < 2 ? 16 + k2 * 4 + 2 + l : 32 + k2) : (lm ? row_b(k2 * 9 + 6 + l) : row_b(i));
        };
        float refx = 0.f, refy = 0.f, sm_max = 0.f, sm_inv = 1.f;
        if (FUSED && todo) {  // re-derive what the fast path no longer holds in registers
          ref_point(cur.qrow[t] - cur.b * Q, refx, refy);
          sm_max = logit_at(0);
          for (int i = 1; i < NL * P; ++i) sm_max = fmaxf(sm_max, logit_at(i));
          float ssum = 0.f;
          for (int i = 0; i < NL * P; ++i) ssum += __expf(logit_at(i) - sm_max);
          sm_inv = __builtin_amdgcn_rcpf(ssum);
        }
        while (todo) {  // bit (k2 * 3 + l): point k2 of level l
          const int i = __ffs(todo) - 1;
          todo &= todo - 1;
          const int k2 = i / 3, l = i - k2 * 3;
          const int Wl = l == 2 ? g.W[2] : (l == 1 ? g.W[1] : g.W[0]), Hl = l == 2 ? g.H[2] : (l == 1 ? g.H[1] : g.H[0]);
          const int st_l = l == 0 ? g.start[0] : (l == 1 ? g.start[1] : g.start[2]);
          const float lx = row_a(xy_at(k2, l)), ly = row_a(xy_at(k2, l) + 1);
          float aw = logit_at(l * P + k2), x, y;
          if (FUSED) {
            aw = __expf(aw - sm_max) * sm_inv;
            x = (refx * (float)Wl - 0.5f) + lx;
            y = (refy * (float)Hl - 0.5f) + ly;
          } else {
            x = ((2.f * lx - 1.f + 1.f) * (float)Wl - 1.f) * 0.5f;
            y = ((2.f * ly - 1.f + 1.f) * (float)Hl - 1.f) * 0.5f;
          }
          const float* vlev = vb + (int64_t)st_l * row_stride;
          quad_point_slow(r1, vlev + (off1 >> 2), Hl, Wl, row_stride, x, y, aw);
          quad_point_slow(r2, vlev + (off2 >> 2), Hl, Wl, row_stride, x, y, aw);
        }
      }
      const unsigned o_off = cur.valid[t] ? (unsigned)((cur.qrow[t] * heads + cur.h) * (D * (kOutLp ? 2 : 4))) : kOobOffset;
      if (MODE == 6) {  // keep the sums alive without a store
        asm volatile("" ::"v"(r1.x), "v"(r1.y), "v"(r1.z), "v"(r1.w), "v"(r2.x), "v"(r2.y), "v"(r2.z), "v"(r2.w));
        continue;
      }
      if constexpr (kOutLp) {  // round to nearest even, as a cast pass over the fp32 output would
        __builtin_amdgcn_raw_buffer_store_b64((u32x2q){pack_bf16_rne(r1.x, r1.y), pack_bf16_rne(r1.z, r1.w)}, out_rs, (int)(o_off + (off1 >> 1)), 0, kStAux);
        __builtin_amdgcn_raw_buffer_store_b64((u32x2q){pack_bf16_rne(r2.x, r2.y), pack_bf16_rne(r2.z, r2.w)}, out_rs, (int)(o_off + (off2 >> 1)), 0, kStAux);
        continue;
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, r1), out_rs, (int)(o_off + off1), 0, kStAux);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, r2), out_rs, (int)(o_off + off2), 0, kStAux);
    }
    WM2F_SSTAMP(9, 0);
  }
}

}  // namespace

// ------------------------------------------------------------------------------------ host side
// Streaming launch: one workgroup per CU.
template <bool FUSED>
int launch_stream(const void* value, const void* a, const void* b, void* out, const int32_t* level_hw, int B, int S,
                  int Q, int heads, int L, int P, void* stream, const char* who, bool* handled, int mode, int a_qstride,
                  int b_qstride, int lanes) {
  // mode: 0 the kernel that runs.  Profiling build: 4 without LDS reads, 7 stamped; on the lane-major rows 800 slab order,
  //       807 its stamped build, and its timing ablations (OUTPUTS NOT VALID) 814 no LDS reads, 815 no window DMA,
  //       816 no operand loads / stores, 820 operand loads from one hot record.  Any other mode: not handled.
  *handled = false;
#ifdef WM2F_PROFILING
  if (mode != 0 && mode != 4 && mode != 7 && mode != 800 && mode != 807 && !(mode >= 814 && mode <= 816) && mode != 820) return WM2F_OK;
#else
  if (mode != 0) return WM2F_OK;  // every other mode is an ablation or a stamped build: profiling library
#endif
  if (P != 4 || L != 3 || (int64_t)Q != S) return WM2F_OK;
  const int H0 = level_hw[0], W0 = level_hw[1];
  bool exact = true;
  int64_t tokens = 0;
  for (int l = 0; l < 3; ++l) {
    const int Hl = level_hw[2 * l], Wl = level_hw[2 * l + 1];
    if (Hl < 1 || Wl < 1) return WM2F_OK;
    if (Hl != (H0 << l) || Wl != (W0 << l)) exact = false;
    tokens += (int64_t)Hl * Wl;
  }
  if (tokens != S) return WM2F_OK;
  if (!exact) {
    // Any other coarse -> fine pyramid whose levels roughly double (input sizes that are not multiples of 32: 25x42 /
    // 50x84 / 100x167): a 16 x 16 tile of the finest level must hold at most 4+1, 8+1 queries per axis of the two coarser
    // levels (the slot count: 25 + 81 + 256 <= 384) and its sampling range must fit the compile-time windows; the float
    // divisions of the tile -> query arithmetic must stay exact (operands below 2^22).
    if (lanes || mode == 4 || mode == 7) return WM2F_OK;
    const int Wf = level_hw[5], Hf = level_hw[4];
    for (int l = 0; l < 2; ++l) {
      const int Hl = level_hw[2 * l], Wl = level_hw[2 * l + 1], fq = kQF >> (2 - l);
      if ((int64_t)kQF * Wl > (int64_t)(fq + 1) * Wf - Wl || (int64_t)kQF * Hl > (int64_t)(fq + 1) * Hf - Hl) return WM2F_OK;  // <= fq + 1 queries per axis
      if ((int64_t)kQF * Wl > (int64_t)fq * Wf + Wf || (int64_t)kQF * Hl > (int64_t)fq * Hf + Hf) return WM2F_OK;          // window: 16 W_l / W_f <= fq + 1
      if ((int64_t)2 * kQF * ((Wf + kQF - 1) / kQF + 1) * Wl + 2 * Wf >= (1 << 22) ||
          (int64_t)2 * kQF * ((Hf + kQF - 1) / kQF + 1) * Hl + 2 * Hf >= (1 << 22))
        return WM2F_OK;
    }
  }
  StreamGeom sg;
  QuadGeom& g = sg.q;
  g.W0 = W0;
  g.H0 = H0;
  g.exact = exact ? 1 : 0;
  int64_t start = 0;
  for (int l = 0; l < 3; ++l) {
    g.H[l] = level_hw[2 * l];
    g.W[l] = level_hw[2 * l + 1];
    g.inv_w[l] = 1.f / (float)g.W[l];
    g.inv_h[l] = 1.f / (float)g.H[l];
    g.start[l] = (int)start;
    start += (int64_t)g.H[l] * g.W[l];
  }
  g.inv_2wf = 1.f / (float)(2 * g.W[2]);
  g.inv_2hf = 1.f / (float)(2 * g.H[2]);
  g.tiles_x = (g.W[2] + kQF - 1) / kQF;
  g.tiles_y = (g.H[2] + kQF - 1) / kQF;
  g.a_qstride = a_qstride > 0 ? a_qstride : heads * L * P * 2;
  g.b_qstride = b_qstride > 0 ? b_qstride : heads * L * P;
  const int64_t n_logical = (int64_t)B * heads * g.tiles_x * g.tiles_y;
  const int64_t lim = 0x7fffffff;
  if (n_logical >= (1 << 22) || (int64_t)B * Q >= (1 << 24) || g.a_qstride * 4 >= (1 << 24) || (!(lanes & 1) && g.b_qstride * 4 >= (1 << 24)) || ((lanes & 1) && (int64_t)heads * g.b_qstride * 4 >= lim) ||
      (int64_t)B * Q * g.a_qstride * 4 >= lim || (!(lanes & 1) && (int64_t)B * Q * g.b_qstride * 4 >= lim) ||
      (int64_t)B * Q * heads * 32 * 4 >= lim || (int64_t)g.H[2] * g.W[2] >= (1 << 24) || heads * 32 * 4 >= (1 << 24) ||
      (int64_t)S * heads * 32 * 4 >= lim)
    return WM2F_OK;
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
      set_error("%s: cannot query the device", who);
      return WM2F_ELAUNCH;
    }
    n_cu = prop.multiProcessorCount;
  }
  int wg = n_cu - n_cu % kNumXcd;  // a multiple of the XCD count
  if (wg < kNumXcd) wg = kNumXcd;
  sg.n_logical = (int)n_logical;
  sg.per_xcd = (int)ceil_div64(n_logical, kNumXcd);
  sg.wg_per_xcd = wg / kNumXcd;
  if (sg.wg_per_xcd > sg.per_xcd) sg.wg_per_xcd = sg.per_xcd;
  wg = sg.wg_per_xcd * kNumXcd;
  sg.inv_heads = 1.f / (float)heads;
  sg.inv_ntiles = 1.f / (float)(g.tiles_x * g.tiles_y);
  sg.inv_tiles_x = 1.f / (float)g.tiles_x;
  sg.step_t = sg.wg_per_xcd / heads;
  sg.step_h = sg.wg_per_xcd % heads;
  sg.step_tx = sg.step_ty = 0;
  // slab order (lanes bit 2; profiling build: modes 800-820)
  const bool slab = exact && FUSED && (lanes & 1) && ((lanes & 4) || mode >= 800);
  if (slab) {
    const int n_tiles = g.tiles_x * g.tiles_y;
    sg.step_h = sg.wg_per_xcd / n_tiles;
    sg.step_t = sg.wg_per_xcd % n_tiles;
    sg.step_ty = sg.step_t / g.tiles_x;
    sg.step_tx = sg.step_t % g.tiles_x;
  }
  for (int i = 0; i < 3; ++i) sg.unused_i[i] = 0, sg.unused_f[i] = 0.f;
  const bool all_full = exact && g.W[2] % kQF == 0 && g.H[2] % kQF == 0;  // e.g. every input whose sides are multiples of 128
#ifdef WM2F_PROFILING
  // an instrument that is not built for this shape or these rows is not handled (never the plain kernel in its place)
  if ((mode >= 800 && (!slab || (mode != 800 && !all_full))) || (mode == 4 && (lanes & 1))) return WM2F_OK;
#endif
  const bool v_hm = (lanes & 2) != 0;  // value stored head-major, (heads, B, S, 32)
  sg.v_pix = v_hm ? 32 : heads * 32;
  sg.v_head = v_hm ? (long long)B * S * 32 : 32;
  sg.v_img = v_hm ? (long long)S * 32 : (long long)S * heads * 32;
  const bool ln = FUSED && (lanes & 1) != 0;
  auto kfn = ln ? msdeform_stream_fwd_kernel<FUSED, 0, true, kOptLanes> : msdeform_stream_fwd_kernel<FUSED, 0, true, 0>;
  if (all_full) kfn = ln ? msdeform_stream_fwd_kernel<FUSED, 0, true, kOptLanes | kOptAllFull> : msdeform_stream_fwd_kernel<FUSED, 0, true, kOptAllFull>;
  if constexpr (FUSED) if (slab) {
    kfn = all_full ? msdeform_stream_fwd_kernel<FUSED, 0, true, kOptLanes | kOptAllFull | kOptSlab> : msdeform_stream_fwd_kernel<FUSED, 0, true, kOptLanes | kOptSlab>;
#ifdef WM2F_PROFILING
    if (mode == 807) kfn = msdeform_stream_fwd_kernel<FUSED, 7, true, kOptLanes | kOptAllFull | kOptSlab>;
    // timing ablations of the slab-order kernel (OUTPUTS NOT VALID)
    if (mode == 814) kfn = msdeform_stream_fwd_kernel<FUSED, 4, true, kOptLanes | kOptAllFull | kOptSlab>;
    if (mode == 815) kfn = msdeform_stream_fwd_kernel<FUSED, 5, true, kOptLanes | kOptAllFull | kOptSlab>;
    if (mode == 816) kfn = msdeform_stream_fwd_kernel<FUSED, 6, true, kOptLanes | kOptAllFull | kOptSlab>;
    if (mode == 820) kfn = msdeform_stream_fwd_kernel<FUSED, 8, true, kOptLanes | kOptAllFull | kOptSlab>;
#endif
  }
  if (!exact) kfn = ln ? msdeform_stream_fwd_kernel<FUSED, 0, false, kOptLanes> : msdeform_stream_fwd_kernel<FUSED, 0, false, 0>;
  // lanes bits 3 / 4: bf16 [offsets | logits] rows / bf16 output (the training forward under bf16 autocast: both or neither)
  if constexpr (FUSED) if ((lanes & 24) == 24) {
    if (ln || slab || mode != 0) return WM2F_OK;
    kfn = !exact ? msdeform_stream_fwd_kernel<FUSED, 0, false, kOptRowsBf16 | kOptOutBf16>
                 : (all_full ? msdeform_stream_fwd_kernel<FUSED, 0, true, kOptAllFull | kOptRowsBf16 | kOptOutBf16>
                             : msdeform_stream_fwd_kernel<FUSED, 0, true, kOptRowsBf16 | kOptOutBf16>);
  } else if (lanes & 24) return WM2F_OK;
#ifdef WM2F_PROFILING
  if (mode == 4 && exact) kfn = msdeform_stream_fwd_kernel<FUSED, 4, true, 0>;
  if (mode == 7 && exact) kfn = ln ? msdeform_stream_fwd_kernel<FUSED, 7, true, kOptLanes> : msdeform_stream_fwd_kernel<FUSED, 7, true, 0>;
#endif
  hipLaunchKernelGGL(kfn, dim3(wg), dim3(kStreamThreads), 0, (hipStream_t)stream, (const float*)value, (const float*)a,
                     (const float*)b, (float*)out, sg, S, Q, heads);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: streaming launch failed: %s", who, hipGetErrorString(e));
    return WM2F_ELAUNCH;
  }
  *handled = true;
  return WM2F_OK;
}

template int launch_stream<false>(const void*, const void*, const void*, void*, const int32_t*, int, int, int, int, int,
                                  int, void*, const char*, bool*, int, int, int, int);
template int launch_stream<true>(const void*, const void*, const void*, void*, const int32_t*, int, int, int, int, int,
                                 int, void*, const char*, bool*, int, int, int, int);

}  // namespace wm2f

#ifdef WM2F_PROFILING
// Copy the MODE-7 time stamps (int64 [8192 workgroups][16 slots], s_memtime ticks) to host memory (include/wm2f_prof.h).
extern "C" int wm2f_debug_stamps(void* host_dst, int64_t n_bytes) {
  using namespace wm2f;
  WM2F_REQUIRE(host_dst && n_bytes > 0 && n_bytes <= (int64_t)sizeof(long long) * kStampGroups * kStampSlots,
               "wm2f_debug_stamps: bad destination / size");
  hipError_t e = hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(g_stamps), (size_t)n_bytes, 0, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    set_error("wm2f_debug_stamps: %s", hipGetErrorString(e));
    return WM2F_ELAUNCH;
  }
  return WM2F_OK;
}
#endif  // WM2F_PROFILING
