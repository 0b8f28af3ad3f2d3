// The labelling that ccl.hip, clean.hip and tiles.hip share: a lock-free union-find, the geometry
// of labelling a pixel map in 32 x 32 tiles, and the unions across tile borders on the global parent array.  Device
// functions and constants only: loads, the neighbour loop inside a tile, counts, flatten passes and launches stay with
// the callers.  What "same set" means is the caller's: the merge step takes the key array and an `active(key)`
// predicate, and joins neighbouring pixels that are active and carry equal keys.
#pragma once
#include "common.h"

namespace wm2f {

// ---- union-find -----------------------------------------------------------------------------------------------------
// parent[x] <= x always holds: a node starts as its own parent and a parent is only ever lowered, by atomicMin.  Hence
//  - a find follows strictly decreasing indices and ends: at most 1023 steps in a tile, at most n - 1 on n nodes;
//  - a root is the smallest index of its set, so the sets and their roots do not depend on the schedule.
// A union links the larger root b under the smaller root a.  If the atomicMin finds that b is a root no more (old != b:
// another thread has just linked b under `old`), parent[b] = min(old, a) keeps b joined to the smaller of the two, and
// the loop goes on to join the other one, `old`, with a: no link is lost.  Every retry continues from an index smaller
// than the root it tried, so a union ends after at most as many rounds as that index has predecessors.
template <int kScope>
__device__ __forceinline__ int find_root(int32_t* parent, int x) {
  int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, kScope);
  while (p != x) {
    x = p;
    p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, kScope);
  }
  return x;
}

template <int kScope>
__device__ __forceinline__ void unite(int32_t* parent, int a, int b) {
  for (;;) {
    a = find_root<kScope>(parent, a);
    b = find_root<kScope>(parent, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(parent + b, a, __ATOMIC_RELAXED, kScope);
    if (old == b) return;
    b = old;
  }
}

// ---- tile geometry --------------------------------------------------------------------------------------------------
// A workgroup of 256 threads owns a 32 x 32 tile; thread t owns column t % 32 of the four rows t / 32 + 8 k.
constexpr int kLabelTile = 32;
constexpr int kLabelTilePx = kLabelTile * kLabelTile;
constexpr int kLabelThreads = 256;
constexpr int kLabelRows = kLabelTilePx / kLabelThreads;     // pixels of the tile per thread
constexpr int kLabelRowStep = kLabelThreads / kLabelTile;    // rows between them

struct TilePixel {
  int lx, ly, li;  // column and row inside the tile, li = ly * 32 + lx
};

// the k-th pixel of this thread, k in [0, kLabelRows)
__device__ __forceinline__ TilePixel tile_pixel(int k) {
  const int lx = threadIdx.x % kLabelTile, ly = threadIdx.x / kLabelTile + k * kLabelRowStep;
  return TilePixel{lx, ly, ly * kLabelTile + lx};
}

// A tile-local index as a linear index of the image whose tile starts at (y0, x0).  Inside a tile the two orders
// agree, so the smallest local index of a set is its smallest image index too.
__device__ __forceinline__ int tile_to_image(int r, int y0, int x0, int W) {
  return (y0 + r / kLabelTile) * W + x0 + r % kLabelTile;
}

// ---- tile borders ---------------------------------------------------------------------------------------------------
// The border pixels of an H x W map: the top row of every tile row but the first (n_rows * W pixels), then the left
// column of every tile column but the first (n_cols * H pixels).  The merge launches take one thread per border pixel.
struct BorderCount {
  int n_rows, n_cols;
  int64_t n_border;
};

__host__ __device__ inline BorderCount border_count(int H, int W) {
  const int n_rows = ceil_div(H, kLabelTile) - 1, n_cols = ceil_div(W, kLabelTile) - 1;
  return BorderCount{n_rows, n_cols, (int64_t)n_rows * W + (int64_t)n_cols * H};
}

struct BorderPixel {
  int y, x;
  bool top;  // on a tile's top row (its neighbours across lie above), else on a tile's left column (to the left)
};

// the t-th border pixel; false when t is past the last one
__device__ __forceinline__ bool border_pixel(int64_t t, int H, int W, BorderPixel& b) {
  const BorderCount n = border_count(H, W);
  if (t >= n.n_border) return false;
  const int64_t n_row_px = (int64_t)n.n_rows * W;
  if (t < n_row_px) {
    b = BorderPixel{(int)(t / W + 1) * kLabelTile, (int)(t % W), true};
  } else {
    const int64_t u = t - n_row_px;
    b = BorderPixel{(int)(u % H), (int)(u / H + 1) * kLabelTile, false};
  }
  return true;
}

// Merge step: the active border pixel p is joined with its neighbours of equal key across the border, on the global
// parent array, after every tile has joined its own pixels (the local phase of the caller: each active pixel united
// with its W and N and, under 8-connectivity, NW and NE neighbours of equal key inside the tile).  Along the border (step: +x on a top row, +y on a left
// column) p has the pixel `across` it and, under 8-connectivity, the diagonal ones back = across - step and
// ahead = across + step; towards a tile corner these reach into the diagonal tile, which is how corners are joined.
// When `across` has p's key, that union stands for the two diagonal ones: back and ahead are neighbours of `across`
// along the border and are joined to it by their own tile or their own border pixel.  Otherwise the diagonals are
// tried.
// One union per run.  Let q = p - step lie in p's tile with p's key (`chain`): the local phase has joined q to p.  If
// back has p's key too, back is the pixel straight across q, so q's thread makes the union (q, back) -- or skips it by
// this same rule, handing it to the pixel before q; that ends at the first pixel of the tile's border segment, whose
// predecessor lies in another tile, so it never skips.  p is thus joined to back without a union of its own: to reach
// `across` (joined to back inside the tile they share; a corner cannot separate them, since chain puts p off the
// segment's first pixel) and to reach back itself.  Only (p, ahead) is never implied.  Under 4-connectivity the
// straight-across union and its skip are all that is left.
template <int kConn, typename Active>
__device__ __forceinline__ void border_unite(const int32_t* key, int32_t* parent, int H, int W, const BorderPixel& b,
                                             Active active) {
  static_assert(kConn == 4 || kConn == 8, "4- or 8-connectivity");
  constexpr int kS = __HIP_MEMORY_SCOPE_AGENT;
  const int p = b.y * W + b.x;
  const int c = key[p];
  if (!active(c)) return;
  const int step = b.top ? 1 : W;
  const int across = b.top ? p - W : p - 1;
  const int pos = b.top ? b.x : b.y, len = b.top ? W : H;
  const bool straight = key[across] == c;
  if (kConn == 4 && !straight) return;
  const bool chain = pos % kLabelTile != 0 && key[p - step] == c;
  const auto back = [&] { return pos > 0 && key[across - step] == c; };  // read only where chain leaves it open
  if (straight) {
    if (!(chain && back())) unite<kS>(parent, p, across);
  } else {
    if (!chain && back()) unite<kS>(parent, p, across - step);
    if (pos + 1 < len && key[across + step] == c) unite<kS>(parent, p, across + step);
  }
}

}  // namespace wm2f
