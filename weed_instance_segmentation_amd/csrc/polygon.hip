// Polygon rasterisation with cv2.fillPoly's rules: the cv2 step of the reference's polygon loaders
// (datasets/sorghum_weed/dataset.py:63-85, crop_weed dataset_from_yaml_annotations.py:98-145, mask2former
// inference.py:load_ground_truth).  Integer work only, wave64, no matrix cores.
//
// Each fillPoly call k (1-based rank r = k + 1) paints the union of its outline (8-connected lines, OpenCV's
// LineIterator) and its scan fill (OpenCV's FillEdgeCollection).  Calls overlap in painter's order, so the pixel takes
// the value of the highest-ranked call that covers it: an atomicMax of the rank, whatever the schedule.
//   poly_edges_kernel    one thread per edge: the scan-fill edge record (y0, y1, x at y0, dx; 16.16 fixed point) and
//                        the clipped outline, drawn into the rank map with atomicMax;
//   poly_fill_kernel     one wave per (call, row): the crossings of the call's active edges with the row.  The pairs
//                        (c0, c1), (c2, c3), ... of the sorted crossings fill [c_2j >> 16, c_2j+1 >> 16]; with
//                        a_i = c_i >> 16, pixel x lies in such a span iff #{a_i < x} is odd or x is some a_i.  So the
//                        row needs no sort: one bit per crossing pixel and one toggle bit at a_i + 1 in LDS (any
//                        number of crossings), a prefix XOR along the row, and atomicMax over the covered pixels;
//   poly_resolve_kernel  out = rank ? value[rank - 1] : out.
#include "common.h"

namespace wm2f {
namespace {

constexpr int kThreads = 256;
constexpr int kFillThreads = kWave;  // one wave per (call, row)
constexpr int kMaxWords = WM2F_POLY_MAX_SIDE / 32;
constexpr int64_t kOne = 1 << 16;  // OpenCV's XY_ONE (XY_SHIFT = 16)

// One scan-fill edge record: rows [y0, y1), x at row y0 and the step per row, 16.16 fixed point.  Horizontal edges
// keep y0 = y1 and are never active.
struct Edge {
  int64_t x;
  int64_t dx;
  int32_t y0;
  int32_t y1;
};

// Two's-complement int64 arithmetic (OpenCV's int64 expressions, without signed-overflow UB).
__device__ __forceinline__ int64_t add64(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
__device__ __forceinline__ int64_t mul64(int64_t a, int64_t b) { return (int64_t)((uint64_t)a * (uint64_t)b); }

__device__ __forceinline__ int outcode(int64_t x, int64_t y, int64_t right, int64_t bottom) {
  return (x < 0) + (x > right) * 2 + (y < 0) * 4 + (y > bottom) * 8;
}

// OpenCV's clipLine(Size2l, Point2l&, Point2l&): snap y-codes (endpoint 1, then 2), then x-codes, in float64 with
// truncation toward zero; each snap reads the coordinates as the earlier ones left them.  True iff the clipped
// segment lies in the image.
__device__ bool clip_line(int64_t W, int64_t H, int64_t& x1, int64_t& y1, int64_t& x2, int64_t& y2) {
  const int64_t right = W - 1, bottom = H - 1;
  int c1 = outcode(x1, y1, right, bottom), c2 = outcode(x2, y2, right, bottom);
  if ((c1 & c2) == 0 && (c1 | c2) != 0) {
    int64_t a;
    if (c1 & 12) {
      a = c1 < 8 ? 0 : bottom;
      x1 += (int64_t)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
      y1 = a;
      c1 = (x1 < 0) + (x1 > right) * 2;
    }
    if (c2 & 12) {
      a = c2 < 8 ? 0 : bottom;
      x2 += (int64_t)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
      y2 = a;
      c2 = (x2 < 0) + (x2 > right) * 2;
    }
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
      if (c1) {
        a = c1 == 1 ? 0 : right;
        y1 += (int64_t)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
        x1 = a;
        c1 = 0;
      }
      if (c2) {
        a = c2 == 1 ? 0 : right;
        y2 += (int64_t)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
        x2 = a;
        c2 = 0;
      }
    }
  }
  return (c1 | c2) == 0;
}

__device__ __forceinline__ bool outside(int64_t x, int64_t y, int W, int H) {
  return x < 0 || x >= W || y < 0 || y >= H;
}

// The last index i in [0, n) with offs[i] <= v (offs non-decreasing, offs[0] <= v).
__device__ __forceinline__ int last_le(const int32_t* __restrict__ offs, int n, int v) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offs[mid] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct Tables {
  const int32_t* verts;            // (n_verts, 2) x, y
  const int32_t* contour_offsets;  // (n_contours + 1) into verts
  const int32_t* call_offsets;     // (n_calls + 1) into contours
  int n_verts, n_contours, n_calls;
};

// Edge v runs from the contour's previous vertex (the last one for the contour's first vertex) to vertex v.
__global__ __launch_bounds__(kThreads) void poly_edges_kernel(Tables t, int H, int W, Edge* __restrict__ edges,
                                                              int32_t* __restrict__ rank) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= t.n_verts) return;
  const int c = last_le(t.contour_offsets, t.n_contours, v);
  const int k = last_le(t.call_offsets, t.n_calls, c);
  const int first = t.contour_offsets[c], last = t.contour_offsets[c + 1] - 1;
  const int u = v == first ? last : v - 1;
  const int64_t x0 = t.verts[2 * u], y0 = t.verts[2 * u + 1];
  const int64_t x1 = t.verts[2 * v], y1 = t.verts[2 * v + 1];
  const bool clip = outside(x0, y0, W, H) || outside(x1, y1, W, H);

  // (b) the scan-fill record (CollectPolyEdges, LINE_8, shift 0)
  int64_t p0x = x0 * kOne, p0y = y0, p1x = x1 * kOne, p1y = y1;
  if (clip) {
    int64_t a0 = x0, b0 = y0, a1 = x1, b1 = y1;
    clip_line(W, H, a0, b0, a1, b1);
    if (b0 != b1) {
      p0x = a0 * kOne;
      p0y = b0;
      p1x = a1 * kOne;
      p1y = b1;
    }
  } else {
    p0x += kOne >> 1;
    p1x += kOne >> 1;
  }
  Edge e{0, 0, 0, 0};
  if (y0 != y1) {
    e.dx = (p1x - p0x) / (p1y - p0y);
    if (y0 < y1) {
      e.y0 = (int32_t)y0;
      e.y1 = (int32_t)y1;
      e.x = add64(p0x, mul64(y0 - p0y, e.dx));
    } else {
      e.y0 = (int32_t)y1;
      e.y1 = (int32_t)y0;
      e.x = add64(p1x, mul64(y1 - p1y, e.dx));
    }
  }
  edges[v] = e;

  // (a) the outline: LineIterator(img, p_prev, p_i, 8, leftToRight = true)
  int64_t ax = x0, ay = y0, bx = x1, by = y1;
  if (clip && !clip_line(W, H, ax, ay, bx, by)) return;
  if (bx < ax) {
    int64_t s = ax; ax = bx; bx = s;
    s = ay; ay = by; by = s;
  }
  const int dx = (int)(bx - ax);
  int dy = (int)(by - ay);
  const int sy = dy < 0 ? -1 : 1;
  dy = dy < 0 ? -dy : dy;
  const bool vert = dy > dx;
  const int major = vert ? dy : dx, minor = vert ? dx : dy;
  int err = major - 2 * minor;
  int x = (int)ax, y = (int)ay;
  const int r = k + 1;
  for (int i = 0; i <= major; ++i) {
    if (x >= 0 && x < W && y >= 0 && y < H) atomicMax(rank + (int64_t)y * W + x, r);
    const bool step_minor = err < 0;
    if (vert) {
      y += sy;
      x += step_minor;
    } else {
      x += 1;
      y += step_minor ? sy : 0;
    }
    err += -2 * minor + (step_minor ? 2 * major : 0);
  }
}

// One block (one wave) per (call, row) item in a grid-stride loop.  Item i belongs to the last call k with
// item_offsets[k] <= i and stands for row call_row0[k] + i - item_offsets[k].
__global__ __launch_bounds__(kFillThreads) void poly_fill_kernel(Tables t, const Edge* __restrict__ edges,
                                                                 const int32_t* __restrict__ call_row0,
                                                                 const int32_t* __restrict__ item_offsets, int n_items,
                                                                 int H, int W, int32_t* __restrict__ rank) {
  __shared__ uint32_t s_toggle[kMaxWords];  // bit x: the parity of #{a_i < x} changes at x
  __shared__ uint32_t s_cover[kMaxWords];   // bit x: some a_i == x; then the covered pixels of the row
  const int lane = threadIdx.x;
  const int nw = (W + 31) >> 5;
  for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int k = last_le(item_offsets, t.n_calls, item);
    const int y = call_row0[k] + (item - item_offsets[k]);
    if (y < 0 || y >= H) continue;  // uniform over the block
    for (int w = lane; w < nw; w += kFillThreads) {
      s_toggle[w] = 0;
      s_cover[w] = 0;
    }
    __syncthreads();
    const int e_end = t.contour_offsets[t.call_offsets[k + 1]];
    for (int e = t.contour_offsets[t.call_offsets[k]] + lane; e < e_end; e += kFillThreads) {
      const Edge ed = edges[e];
      if (ed.y0 <= y && y < ed.y1) {
        const int64_t a = add64(ed.x, mul64(y - ed.y0, ed.dx)) >> 16;  // floor, as OpenCV's >> XY_SHIFT
        if (a >= 0 && a < W) atomicOr(s_cover + (a >> 5), 1u << (a & 31));
        const int64_t s = a < 0 ? 0 : a + 1;  // a crossing left of the row toggles the parity at column 0
        if (s < W) atomicXor(s_toggle + (s >> 5), 1u << (s & 31));
      }
    }
    __syncthreads();
    // Prefix XOR of the toggles along the row, 64 words (2048 columns) per step: inside a word by shifts, across
    // words by the parity of the words before (ballot), across steps by a carry.
    uint32_t carry = 0;
    for (int w0 = 0; w0 < nw; w0 += kFillThreads) {
      const int w = w0 + lane;
      const uint32_t tg = w < nw ? s_toggle[w] : 0u;
      uint32_t p = tg;
      p ^= p << 1;
      p ^= p << 2;
      p ^= p << 4;
      p ^= p << 8;
      p ^= p << 16;
      const uint64_t odd = __ballot(__popc(tg) & 1);
      const uint32_t before = ((uint32_t)__popcll(odd & ((1ull << lane) - 1ull)) & 1u) ^ carry;
      carry ^= (uint32_t)__popcll(odd) & 1u;
      if (w < nw) {
        uint32_t cov = (before ? ~p : p) | s_cover[w];
        if (w == nw - 1 && (W & 31)) cov &= (1u << (W & 31)) - 1u;
        s_cover[w] = cov;
      }
    }
    __syncthreads();
    // atomicMax over the covered pixels, one pixel per lane along the row (64-column chunks with nothing covered are
    // skipped by the whole wave)
    int32_t* row = rank + (int64_t)y * W;
    const int r = k + 1;
    for (int x0 = 0; x0 < W; x0 += kFillThreads) {
      const int w = x0 >> 5;
      if ((s_cover[w] | (w + 1 < nw ? s_cover[w + 1] : 0u)) == 0u) continue;
      const int x = x0 + lane;
      if (x < W && ((s_cover[x >> 5] >> (x & 31)) & 1u)) atomicMax(row + x, r);
    }
    __syncthreads();  // the next item clears the bits
  }
}

__global__ __launch_bounds__(kThreads) void poly_resolve_kernel(int64_t n_px, const int32_t* __restrict__ rank,
                                                                const int32_t* __restrict__ values, int n_calls,
                                                                int32_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= n_px) return;
  const int r = rank[p];
  if (r > 0 && r <= n_calls) out[p] = values[r - 1];
}

}  // namespace
}  // namespace wm2f

using namespace wm2f;

extern "C" int64_t wm2f_poly_workspace(int H, int W, int n_verts) {
  if (H <= 0 || W <= 0 || H > WM2F_POLY_MAX_SIDE || W > WM2F_POLY_MAX_SIDE || n_verts < 0) return -1;
  return (int64_t)n_verts * (int64_t)sizeof(Edge) + (int64_t)H * W * (int64_t)sizeof(int32_t);
}

extern "C" int wm2f_poly_fill(int32_t* out, int H, int W, const int32_t* verts, int n_verts,
                              const int32_t* contour_offsets, int n_contours, const int32_t* call_offsets,
                              const int32_t* values, const int32_t* call_row0, const int32_t* item_offsets, int n_calls,
                              int n_items, void* workspace, void* stream) {
  const char* who = "wm2f_poly_fill";
  WM2F_REQUIRE(H > 0 && W > 0, "%s: need positive sizes", who);
  if (H > WM2F_POLY_MAX_SIDE || W > WM2F_POLY_MAX_SIDE) {
    set_error("%s: sides must be <= %d", who, WM2F_POLY_MAX_SIDE);
    return WM2F_EUNSUPPORTED;
  }
  WM2F_REQUIRE(n_verts >= 0 && n_contours >= 0 && n_calls >= 0 && n_items >= 0, "%s: negative count", who);
  if (n_calls == 0) return WM2F_OK;
  WM2F_REQUIRE(out && verts && contour_offsets && call_offsets && values && call_row0 && item_offsets && workspace,
               "%s: null pointer", who);
  WM2F_REQUIRE(n_verts > 0 && n_contours > 0, "%s: %d calls need contours and vertices", who, n_calls);
  hipStream_t s = (hipStream_t)stream;
  Edge* edges = (Edge*)workspace;
  int32_t* rank = (int32_t*)((char*)workspace + (int64_t)n_verts * (int64_t)sizeof(Edge));
  const int64_t n_px = (int64_t)H * W;
  WM2F_REQUIRE(hipMemsetAsync(rank, 0, (size_t)n_px * sizeof(int32_t), s) == hipSuccess, "%s: clearing the rank map "
               "failed", who);
  const Tables t{verts, contour_offsets, call_offsets, n_verts, n_contours, n_calls};
  hipLaunchKernelGGL(poly_edges_kernel, dim3((unsigned)ceil_div(n_verts, kThreads)), dim3(kThreads), 0, s, t, H, W,
                     edges, rank);
  WM2F_CHECK_LAUNCH(who);
  if (n_items > 0) {
    const int grid = n_items < (1 << 18) ? n_items : (1 << 18);
    hipLaunchKernelGGL(poly_fill_kernel, dim3((unsigned)grid), dim3(kFillThreads), 0, s, t, (const Edge*)edges,
                       call_row0, item_offsets, n_items, H, W, rank);
    WM2F_CHECK_LAUNCH(who);
  }
  hipLaunchKernelGGL(poly_resolve_kernel, dim3((unsigned)ceil_div64(n_px, kThreads)), dim3(kThreads), 0, s, n_px,
                     (const int32_t*)rank, values, n_calls, out);
  WM2F_CHECK_LAUNCH(who);
  return WM2F_OK;
}
