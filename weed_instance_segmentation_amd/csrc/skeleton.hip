// Skeletons of id maps on the device: Guo and Hall's two-sub-iteration parallel thinning of every
// instance at once, and per-instance sums over the skeleton (pixels, links, tips, junctions, widths).  The rule is
// written out in include/wm2f.h; tests/skeleton_reference.py restates it in numpy.
//
//   wm2f_labelmap_skeleton (2 + ceil(rounds / I) launches, I = per_launch)
//     skel_init    the counters of every image <- 0
//     skel_thin    a 256-thread workgroup owns a 64 x 64 tile of one image.  It loads the tile and a halo of 2 I pixels
//                  (rounded up to whole 4-cell words along x) into LDS as int16 cells (id or -1, four cells to a 64-bit
//                  word; outside the image: -1), runs up to 2 I sub-iterations there and stores the owned tile.  After
//                  sub-iteration t the cells at least t inside the loaded region are exact, so the owned tile is exact
//                  at the end; a sub-iteration only visits the cells that can still matter.  A thread owns whole words:
//                  it takes the decisions of its words into a register mask, then a barrier, then it rewrites the words
//                  it deleted from, then a barrier -- a sub-iteration is synchronous inside the tile as well.  The words
//                  are dealt out in patches of 16 x 16 cells, a patch to a wave at a time: a wave whose patch lies
//                  inside an instance or off every instance has nothing to evaluate.  After two sub-iterations in a
//                  row without a deletion the workgroup's image is final and it goes on to the store.  Deletions
//                  inside owned tiles are added to the image's counter of the iteration, the live pixels of the owned
//                  tile to the launch's counter: one integer atomic per workgroup and counter.
//                  The launches ping-pong between `out` and one workspace plane so that the last one writes `out`; the
//                  first decodes the typed map.  Launch l >= 2 returns at once when launch l - 1 deleted nothing in its
//                  image: that launch read one plane and wrote an equal copy to the other, so both hold the result.
//     skel_status  status rows from the counters
//   wm2f_labelmap_skeleton_stats (2 launches): clear; a thread per pixel, a skeleton pixel of a listed id looks at its
//                  eight neighbours and adds its terms to its id's row with 64-bit integer atomics -- one lane for the
//                  wave when the skeleton pixels among the wave's 64 belong to one id.
// Everything is integer, the atomics are add and max on integers: results are bit-identical from run to run.
#include "labelmap.h"

namespace wm2f {
namespace {

constexpr int kSkThreads = 256;
constexpr int kSkTile = 64;
constexpr int kSkMaxRounds = 1024;
constexpr int kSkDefaultPerLaunch = 4;         // per_launch = 0
constexpr int kSkCounters = 2 * kSkMaxRounds;  // per image: deletions of every iteration, live pixels after every launch
constexpr int kSkStatCols = 8;
constexpr unsigned long long kSkDead = ~0ull;  // a word of four dead cells

// the LDS image of a workgroup that runs up to I iterations: Ly rows of PW words, a word = 4 cells; word 0 and word
// PW - 1 of a row are guards that stay dead, so a word's left and right neighbours always exist
template <int I>
struct SkGeom {
  static constexpr int hy = 2 * I;
  static constexpr int hx = (hy + 3) / 4 * 4;
  static constexpr int Ly = kSkTile + 2 * hy;
  static constexpr int Lx = kSkTile + 2 * hx;
  static constexpr int SX = Lx / 4;  // words of a row that hold loaded cells
  static constexpr int PW = SX + 2;
  static constexpr int words = Ly * PW;
  // the words are dealt out in patches of 16 rows x 4 words (16 x 16 cells), a patch to a wave at a time, so that a
  // wave whose patch lies inside an instance, or off every instance, skips it as one
  static constexpr int PXN = (SX + 3) / 4;
  static constexpr int patches = (Ly + 15) / 16 * PXN;
  static constexpr int per_thread = (patches + kSkThreads / 64 - 1) / (kSkThreads / 64);
  // the row and the word of thread tid's k-th word; outside the image for a patch's overhang
  __device__ static __forceinline__ void word_of(int tid, int k, int& y, int& s) {
    const int c = k * (kSkThreads / 64) + (tid >> 6);
    const int py = c / PXN, px = c - py * PXN;
    y = py * 16 + ((tid & 63) >> 2);
    s = px * 4 + (tid & 3);
  }
};
static_assert(SkGeom<8>::per_thread * 4 <= 64, "a thread's decisions fit one 64-bit mask");

__host__ inline int64_t sk_round16(int64_t v) { return (v + 15) / 16 * 16; }
__host__ inline int64_t sk_plane_bytes(int B, int H, int W) { return sk_round16((int64_t)B * H * W * 4); }

__device__ __forceinline__ int sk_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ int sk_cell(unsigned long long w, int j) { return (int)((w >> (16 * j)) & 0xffffull); }

// grid ceil(B * kSkCounters / 256)
__global__ __launch_bounds__(kSkThreads) void skel_init_kernel(int32_t* __restrict__ cnt, int n) {
  const int i = blockIdx.x * kSkThreads + threadIdx.x;
  if (i < n) cnt[i] = 0;
}

// does the pixel with the neighbours p2 .. p9 (bit i - 2 of `p`: N, NE, E, SE, S, SW, W, NW) go in sub-iteration `par`
__device__ __forceinline__ bool sk_deletes(unsigned p, int par) {
  const unsigned p2 = p & 1u, p3 = (p >> 1) & 1u, p4 = (p >> 2) & 1u, p5 = (p >> 3) & 1u, p6 = (p >> 4) & 1u,
                 p7 = (p >> 5) & 1u, p8 = (p >> 6) & 1u, p9 = (p >> 7) & 1u;
  const unsigned C = ((p2 ^ 1u) & (p3 | p4)) + ((p4 ^ 1u) & (p5 | p6)) + ((p6 ^ 1u) & (p7 | p8)) + ((p8 ^ 1u) & (p9 | p2));
  const unsigned n1 = (p9 | p2) + (p3 | p4) + (p5 | p6) + (p7 | p8);
  const unsigned n2 = (p2 | p3) + (p4 | p5) + (p6 | p7) + (p8 | p9);
  const unsigned n = n1 < n2 ? n1 : n2;
  const unsigned m = par ? ((p2 | p3 | (p5 ^ 1u)) & p4) : ((p6 | p7 | (p9 ^ 1u)) & p8);
  return C == 1u && n >= 2u && n <= 3u && m == 0u;
}

// grid (ceil(W / 64), ceil(H / 64), B).  src: the typed map (launch 0) or a state plane (int32: id or -1, which decodes
// as an int32 map does).  Runs the iterations it0 .. it0 + iters - 1, iters <= I.
template <int DT, int I>
__global__ __launch_bounds__(kSkThreads) void skel_thin_kernel(const void* __restrict__ src, int32_t* __restrict__ dst,
                                                               int32_t* cnt, int H, int W, int N, int launch, int it0,
                                                               int iters, int vec_in, int vec_out) {
  using G = SkGeom<I>;
  using E = typename MapElem<DT>::type;
  __shared__ __align__(16) unsigned long long s_cell[G::words];
  __shared__ int s_del[I];
  __shared__ int s_live;
  const int tid = threadIdx.x, b = blockIdx.z;
  int32_t* del = cnt + b * kSkCounters;
  if (launch >= 2) {  // the quiet exit: the launch before this one ran I iterations and deleted nothing
    int prev = 0;
    for (int i = it0 - I; i < it0; ++i) prev |= del[i];
    if (prev == 0) return;
  }
  if (tid < I) s_del[tid] = 0;
  if (tid == 0) s_live = 0;

  // ---- load: every word of the image once, guards and everything outside the map dead
  const int gx0 = (int)blockIdx.x * kSkTile - G::hx, gy0 = (int)blockIdx.y * kSkTile - G::hy;
  const int64_t img = (int64_t)b * H * W;
  const E* in = reinterpret_cast<const E*>(src) + img;
#pragma unroll  // all of a thread's loads in flight before the first is used
  for (int w = tid; w < G::words; w += kSkThreads) {
    const int y = w / G::PW, sw = w - y * G::PW;
    const int gy = gy0 + y, gx = gx0 + (sw - 1) * 4;
    unsigned long long v = kSkDead;
    if (sw >= 1 && sw <= G::SX && gy >= 0 && gy < H && gx + 3 >= 0 && gx < W) {
      const E* p = in + (int64_t)gy * W + gx;
      uint32_t raw[4];
      int id[4];
      if (vec_in && gx >= 0) {  // W is a multiple of 4 and so is gx: the four pixels are inside
        load_map4<DT>(p, raw);
#pragma unroll
        for (int j = 0; j < 4; ++j) id[j] = map_id_below<DT>(raw[j], N);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) id[j] = (gx + j >= 0 && gx + j < W) ? map_id_below<DT>((uint32_t)p[j], N) : -1;
      }
      v = 0ull;
#pragma unroll
      for (int j = 0; j < 4; ++j) v |= (unsigned long long)((uint32_t)id[j] & 0xffffu) << (16 * j);
    }
    s_cell[w] = v;
  }
  __syncthreads();

  // ---- thin: sub-iteration t - 1 visits the cells at least t inside the loaded region
  int n_del = 0;  // this thread's deletions inside the owned tile in the running iteration
  int quiet = 0;  // the sub-iterations in a row in which no thread of the workgroup deleted
  for (int t = 1; t <= 2 * iters; ++t) {
    const int par = (t - 1) & 1;
    unsigned long long mask = 0ull;  // bit 4 k + j: cell j of this thread's k-th word goes
#pragma unroll
    for (int k = 0; k < G::per_thread; ++k) {
      int y, s;
      G::word_of(tid, k, y, s);
      if (y < t || y >= G::Ly - t || 4 * s + 3 < t || 4 * s >= G::Lx - t) continue;
      const unsigned long long* row = s_cell + y * G::PW + 1 + s;
      const unsigned long long mid = row[0];
      if (mid == kSkDead) continue;
      const unsigned long long up = row[-G::PW], dn = row[G::PW];
      int a[3][6];  // the rows above, of and below the word, from the cell left of it to the cell right of it
      a[0][0] = sk_cell(row[-G::PW - 1], 3);
      a[1][0] = sk_cell(row[-1], 3);
      a[2][0] = sk_cell(row[G::PW - 1], 3);
      a[0][5] = sk_cell(row[-G::PW + 1], 0);
      a[1][5] = sk_cell(row[1], 0);
      a[2][5] = sk_cell(row[G::PW + 1], 0);
      {  // the inside of an instance: all 18 cells carry one id, C = 0 everywhere
        const int c = sk_cell(mid, 0);
        const unsigned long long rep = (unsigned long long)c * 0x0001000100010001ull;
        if (mid == rep && up == rep && dn == rep && a[0][0] == c && a[1][0] == c && a[2][0] == c && a[0][5] == c &&
            a[1][5] == c && a[2][5] == c)
          continue;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[0][j + 1] = sk_cell(up, j);
        a[1][j + 1] = sk_cell(mid, j);
        a[2][j + 1] = sk_cell(dn, j);
      }
      const bool owned = y >= G::hy && y < G::hy + kSkTile && 4 * s >= G::hx && 4 * s < G::hx + kSkTile;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = a[1][j + 1];
        if (c == 0xffff) continue;
        const unsigned p = (unsigned)(a[0][j + 1] == c) | (unsigned)(a[0][j + 2] == c) << 1 | (unsigned)(a[1][j + 2] == c) << 2 |
                           (unsigned)(a[2][j + 2] == c) << 3 | (unsigned)(a[2][j + 1] == c) << 4 | (unsigned)(a[2][j] == c) << 5 |
                           (unsigned)(a[1][j] == c) << 6 | (unsigned)(a[0][j] == c) << 7;
        if (p != 0xffu && sk_deletes(p, par)) {
          mask |= 1ull << (4 * k + j);
          n_del += owned ? 1 : 0;
        }
      }
    }
    if (par) {  // the iteration's decisions are all taken: its count
      const int sum = sk_wave_sum(n_del);
      if ((tid & 63) == 0 && sum != 0) atomicAdd(&s_del[(t - 1) >> 1], sum);
      n_del = 0;
    }
    // every decision of the sub-iteration read the state at its start; and did any thread of the workgroup delete
    const int any = __syncthreads_or(mask != 0ull ? 1 : 0);
    if (!any) {
      // Two quiet sub-iterations in a row, one of each kind: the image did not change between them, and the later
      // ones visit a part of the same cells in the same state, so they delete nothing either.  The image is final.
      if (++quiet == 2) break;
      continue;  // nothing to write
    }
    quiet = 0;
    if (mask != 0ull) {
#pragma unroll
      for (int k = 0; k < G::per_thread; ++k) {
        const unsigned nib = (unsigned)(mask >> (4 * k)) & 15u;
        if (nib == 0u) continue;
        int y, s;
        G::word_of(tid, k, y, s);
        unsigned long long v = s_cell[y * G::PW + 1 + s];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((nib >> j) & 1u) v |= 0xffffull << (16 * j);
        s_cell[y * G::PW + 1 + s] = v;
      }
    }
    __syncthreads();
  }

  // ---- store the owned tile: 16 threads a row, 16 rows a pass
  int32_t* out = dst + img;
  int n_live = 0;
#pragma unroll
  for (int pass = 0; pass < kSkTile / 16; ++pass) {
    const int r = pass * 16 + (tid >> 4), q = tid & 15;
    const int gy = (int)blockIdx.y * kSkTile + r, gx = (int)blockIdx.x * kSkTile + 4 * q;
    if (gy >= H || gx >= W) continue;
    const unsigned long long v = s_cell[(G::hy + r) * G::PW + 1 + G::hx / 4 + q];
    int id[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      id[j] = (int)(int16_t)(uint16_t)sk_cell(v, j);
      n_live += id[j] >= 0 ? 1 : 0;  // a cell outside the map is dead
    }
    int32_t* o = out + (int64_t)gy * W + gx;
    if (vec_out) {
      *reinterpret_cast<int4*>(o) = make_int4(id[0], id[1], id[2], id[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (gx + j < W) o[j] = id[j];
    }
  }
  const int live = sk_wave_sum(n_live);
  if ((tid & 63) == 0 && live != 0) atomicAdd(&s_live, live);
  __syncthreads();
  if (tid < iters && s_del[tid] != 0) atomicAdd(del + it0 + tid, s_del[tid]);
  if (tid == 0 && s_live != 0) atomicAdd(del + kSkMaxRounds + launch, s_live);
}

// grid B: status[b] = [skeleton pixels, iterations that deleted something, deletions in iteration R, R]
__global__ __launch_bounds__(kSkThreads) void skel_status_kernel(const int32_t* __restrict__ cnt, int32_t* __restrict__ status,
                                                                 int rounds, int per) {
  __shared__ int s_busy, s_last;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int32_t* del = cnt + b * kSkCounters;
  if (tid == 0) {
    s_busy = 0;
    s_last = 0;
  }
  __syncthreads();
  int busy = 0, last = 0;
  for (int i = tid; i < rounds; i += kSkThreads) busy += del[i] != 0 ? 1 : 0;
  const int launches = ceil_div(rounds, per);
  for (int l = tid; l < launches; l += kSkThreads) {  // the launches that ran are 0, 1 and those after a busy one
    bool ran = l < 2;
    if (!ran) {
      int prev = 0;
      for (int i = (l - 1) * per; i < l * per; ++i) prev |= del[i];
      ran = prev != 0;
    }
    if (ran) last = l;
  }
  if (busy != 0) atomicAdd(&s_busy, busy);
  if (last != 0) atomicMax(&s_last, last);
  __syncthreads();
  if (tid == 0) {
    int32_t* st = status + b * 4;
    st[0] = del[kSkMaxRounds + s_last];
    st[1] = s_busy;
    st[2] = del[rounds - 1];
    st[3] = rounds;
  }
}

// grid (ceil(W / 64), ceil(H / 4), B), a thread per pixel
__global__ __launch_bounds__(kSkThreads) void skel_stats_kernel(const int32_t* __restrict__ skel, const int32_t* __restrict__ d2,
                                                                const int32_t* __restrict__ ids,
                                                                const int32_t* __restrict__ n_ids,
                                                                unsigned long long* __restrict__ stats, int H, int W, int N) {
  const int x = (int)blockIdx.x * 64 + (threadIdx.x & 63), y = (int)blockIdx.y * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.z;
  const int64_t img = (int64_t)b * H * W;
  const int32_t* m = skel + img;
  const bool inside = x < W && y < H;
  const int v = inside ? m[(int64_t)y * W + x] : -1;
  int r = -1;
  if (v >= 0) {
    if (ids == nullptr) {
      r = v < N ? v : -1;
    } else {
      int n = n_ids[b];
      n = n < 0 ? 0 : (n > N ? N : n);
      r = list_row(v, ids + (int64_t)b * N, n);
    }
  }
  const unsigned long long active = __ballot(r >= 0);
  if (active == 0ull) return;  // wave-uniform: no skeleton pixel of a listed id among the wave's 64
  unsigned nb = 0u, X = 0u, orth = 0u, diag = 0u;
  unsigned long long dd = 0ull;
  if (r >= 0) {
    const auto same = [&](int dy, int dx) -> unsigned {
      const int yy = y + dy, xx = x + dx;
      return (yy >= 0 && yy < H && xx >= 0 && xx < W && m[(int64_t)yy * W + xx] == v) ? 1u : 0u;
    };
    const unsigned p2 = same(-1, 0), p3 = same(-1, 1), p4 = same(0, 1), p5 = same(1, 1), p6 = same(1, 0), p7 = same(1, -1),
                   p8 = same(0, -1), p9 = same(-1, -1);
    nb = p2 + p3 + p4 + p5 + p6 + p7 + p8 + p9;
    X = ((p2 ^ 1u) & p3) + ((p3 ^ 1u) & p4) + ((p4 ^ 1u) & p5) + ((p5 ^ 1u) & p6) + ((p6 ^ 1u) & p7) + ((p7 ^ 1u) & p8) +
        ((p8 ^ 1u) & p9) + ((p9 ^ 1u) & p2);
    orth = p4 + p6;  // every pair once: from its left or upper pixel
    diag = (p5 & (p4 ^ 1u) & (p6 ^ 1u)) + (p7 & (p8 ^ 1u) & (p6 ^ 1u));
    if (d2 != nullptr) {
      const int d = d2[img + (int64_t)y * W + x];
      dd = d > 0 ? (unsigned long long)d : 0ull;
    }
  }
  int term[6] = {r >= 0 ? 1 : 0, (int)orth, (int)diag, (r >= 0 && X == 1u && nb <= 2u) ? 1 : 0, (r >= 0 && X >= 3u) ? 1 : 0,
                 (r >= 0 && nb == 0u) ? 1 : 0};
  // the wave's 64 pixels of a row mostly belong to one plant: then one lane adds the wave's sums
  const int first = __ffsll((long long)active) - 1;
  const int r_first = __shfl(r, first);
  if (__ballot(r >= 0 && r != r_first) == 0ull) {
#pragma unroll
    for (int k = 0; k < 6; ++k) term[k] = sk_wave_sum(term[k]);
    unsigned long long sum = dd, top = dd;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(top, o);
      sum += __shfl_xor(sum, o);
      top = other > top ? other : top;
    }
    if ((int)(threadIdx.x & 63) != first) return;
    unsigned long long* o = stats + ((int64_t)b * N + r) * kSkStatCols;
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (term[k] != 0) atomicAdd(o + k, (unsigned long long)term[k]);
    if (sum != 0ull) atomicAdd(o + 6, sum);
    if (top > __hip_atomic_load(o + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(o + 7, top);
    return;
  }
  if (r < 0) return;
  unsigned long long* o = stats + ((int64_t)b * N + r) * kSkStatCols;
#pragma unroll
  for (int k = 0; k < 6; ++k)
    if (term[k] != 0) atomicAdd(o + k, (unsigned long long)term[k]);
  if (dd != 0ull) {
    atomicAdd(o + 6, dd);
    if (dd > __hip_atomic_load(o + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(o + 7, dd);
  }
}

bool sk_size_ok(int B, int H, int W, int N) {
  return H <= kMapMaxSide && W <= kMapMaxSide && B <= kMapMaxBatch && N <= kMapMaxIds;
}

// f(std::integral_constant<int, I>{}) for a per_launch checked before
template <class F>
void for_per_launch(int per, F&& f) {
  if (per == 1) f(std::integral_constant<int, 1>{});
  else if (per == 2) f(std::integral_constant<int, 2>{});
  else if (per == 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_labelmap_skeleton_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || !sk_size_ok(B, H, W, 0)) return -1;
  return sk_plane_bytes(B, H, W) + (int64_t)B * kSkCounters * 4;
}

extern "C" int wm2f_labelmap_skeleton(const void* map, int dtype, int32_t* out, int32_t* status, void* workspace, int B,
                                      int H, int W, int N, int rounds, int per_launch, void* stream) {
  const char* who = "wm2f_labelmap_skeleton";
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N >= 0, "%s: bad size", who);
  if (!sk_size_ok(B, H, W, N)) {
    set_error("%s: sides <= %d, B <= %d, N <= %d (got %d x %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch, kMapMaxIds, H, W, B,
              N);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(rounds >= 1 && rounds <= kSkMaxRounds, "%s: 1 <= rounds <= %d, got %d", who, kSkMaxRounds, rounds);
  WM2F_REQUIRE(per_launch == 0 || per_launch == 1 || per_launch == 2 || per_launch == 4 || per_launch == 8,
               "%s: per_launch must be 0, 1, 2, 4 or 8, got %d", who, per_launch);
  WM2F_REQUIRE(map && out && status && workspace, "%s: null pointer", who);
  WM2F_REQUIRE_MAP_DTYPE(dtype, who);
  WM2F_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0,
               "%s: workspace must be 16-byte aligned, out 4-byte aligned", who);
  const int64_t all_px = (int64_t)B * H * W;
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + (uintptr_t)all_px * 4;
  const uintptr_t m0 = reinterpret_cast<uintptr_t>(map), m1 = m0 + (uintptr_t)all_px * map_elem_bytes(dtype);
  WM2F_REQUIRE(o1 <= m0 || m1 <= o0, "%s: out overlaps map", who);

  hipStream_t s = (hipStream_t)stream;
  const int per = per_launch == 0 ? kSkDefaultPerLaunch : per_launch;
  int32_t* plane = reinterpret_cast<int32_t*>(workspace);
  int32_t* cnt = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(workspace) + sk_plane_bytes(B, H, W));
  const int n_cnt = B * kSkCounters;
  hipLaunchKernelGGL(skel_init_kernel, dim3(ceil_div(n_cnt, kSkThreads)), dim3(kSkThreads), 0, s, cnt, n_cnt);
  const int launches = ceil_div(rounds, per);
  const dim3 grid((unsigned)ceil_div(W, kSkTile), (unsigned)ceil_div(H, kSkTile), (unsigned)B);
  const void* src = map;
  int src_dtype = dtype;
  for (int l = 0; l < launches; ++l) {
    int32_t* dst = ((launches - 1 - l) & 1) ? plane : out;  // the last launch writes out
    const int it0 = l * per, iters = rounds - it0 < per ? rounds - it0 : per;
    const int vec_in = map_vec4_ok(src, src_dtype, W) ? 1 : 0, vec_out = map_vec4_ok(dst, WM2F_I32, W) ? 1 : 0;
    for_map_dtype(src_dtype, [&](auto dt) {
      for_per_launch(per, [&](auto pl) {
        hipLaunchKernelGGL((skel_thin_kernel<decltype(dt)::value, decltype(pl)::value>), grid, dim3(kSkThreads), 0, s, src,
                           dst, cnt, H, W, N, l, it0, iters, vec_in, vec_out);
      });
    });
    src = dst;
    src_dtype = WM2F_I32;
  }
  WM2F_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(skel_status_kernel, dim3((unsigned)B), dim3(kSkThreads), 0, s, cnt, status, rounds, per);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}

extern "C" int wm2f_labelmap_skeleton_stats(const int32_t* skel, const int32_t* d2, const int32_t* ids, const int32_t* n_ids,
                                            int64_t* stats, int B, int H, int W, int N, void* stream) {
  const char* who = "wm2f_labelmap_skeleton_stats";
  WM2F_REQUIRE(B > 0 && H > 0 && W > 0 && N > 0, "%s: bad size", who);
  if (!sk_size_ok(B, H, W, N)) {
    set_error("%s: sides <= %d, B <= %d, N <= %d (got %d x %d, %d, %d)", who, kMapMaxSide, kMapMaxBatch, kMapMaxIds, H, W, B,
              N);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(skel && stats, "%s: null pointer", who);
  WM2F_REQUIRE((ids == nullptr) == (n_ids == nullptr), "%s: ids and n_ids go together", who);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(stats, 0, (size_t)B * N * kSkStatCols * sizeof(int64_t), s) != hipSuccess) {
    set_error("%s: clearing the result failed", who);
    return WM2F_ELAUNCH;
  }
  const dim3 grid((unsigned)ceil_div(W, 64), (unsigned)ceil_div(H, 4), (unsigned)B);
  hipLaunchKernelGGL(skel_stats_kernel, grid, dim3(kSkThreads), 0, s, skel, d2, ids, n_ids,
                     reinterpret_cast<unsigned long long*>(stats), H, W, N);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
