"""numpy restatement of wm2f_tile_blend, written from the contract in include/wm2f.h and not from the kernel.

`blend` follows the header operation by operation in float32: every product, sum, difference and quotient is one numpy
float32 operation, so it rounds where the header says it rounds, and the views are added in the header's order (f, then r,
then c, ascending).  The GPU tests compare with it bit for bit.

`blend_f64` is a second, independent form for sanity checks with a tolerance: the bilinear resize as two dense float64
interpolation matrices, a flipped view as the reversed resized tile, and the window as normalised separable weights
(the tent of a view over the sum of the tents of one axis, times the same along the other axis, over F).
"""
import numpy as np

F32 = np.float32
FLIP_CODES = {"none": 0, "h": 1, "v": 2, "hv": 3}


def axis_taps(n_src: int, n_dst: int, idx: np.ndarray):
    """grid_logit along one axis: taps i0, i1 and weights l (of i1), h (of i0) for the target coordinates idx."""
    s = F32(n_src) / F32(n_dst)
    a = s * (idx.astype(F32) + F32(0.5)) - F32(0.5)
    a = np.where(a < F32(0), F32(0), a).astype(F32)
    i0 = np.minimum(a.astype(np.int32), n_src - 1)  # a >= 0: the conversion truncates
    i1 = i0 + (i0 < n_src - 1)
    lo = np.minimum(np.maximum(a - i0.astype(F32), F32(0)), F32(1)).astype(F32)
    hi = (F32(1) - lo).astype(F32)
    return i0, i1, lo, hi


def sample(p: np.ndarray, th: int, tw: int, sy: np.ndarray, sx: np.ndarray) -> np.ndarray:
    """p (C, gh, gw) fp32 resized to (th, tw) at rows sy and columns sx -> (C, len(sy), len(sx)) fp32."""
    assert p.dtype == F32
    y0, y1, ly, hy = axis_taps(p.shape[1], th, sy)
    x0, x1, lx, hx = axis_taps(p.shape[2], tw, sx)
    top, bot = p[:, y0], p[:, y1]
    t0 = hx * top[:, :, x0] + lx * top[:, :, x1]
    t1 = hx * bot[:, :, x0] + lx * bot[:, :, x1]
    v = hy[:, None] * t0 + ly[:, None] * t1
    assert v.dtype == F32
    return v


def _cover(origins, side: int, length: int):
    """Per origin the half-open range of image coordinates it covers inside [0, length)."""
    return [(max(0, int(o)), min(length, int(o) + side)) for o in origins]


def counts(ys, xs, F: int, th: int, tw: int, H: int, W: int) -> np.ndarray:
    """n (H, W): the number of covering views of every pixel."""
    rows, cols = np.zeros(H, np.int64), np.zeros(W, np.int64)
    for a, b in _cover(ys, th, H):
        rows[a:b] += 1
    for a, b in _cover(xs, tw, W):
        cols[a:b] += 1
    return F * rows[:, None] * cols[None, :]


def tent(local: np.ndarray, side: int, ramp: int) -> np.ndarray:
    return np.minimum(np.minimum(local + 1, side - local), ramp).astype(np.int32)


def blend(scores, ys, xs, flips, H: int, W: int, th: int, tw: int, ramp_y: int, ramp_x: int):
    """scores (F, R * Cn, C, gh, gw) fp32, ys (R), xs (Cn), flips (F) integers -> seg (H, W) int32, out (C, H, W) fp32."""
    scores = np.asarray(scores)
    assert scores.dtype == F32 and scores.ndim == 5
    F, T, C = scores.shape[:3]
    R, Cn = len(ys), len(xs)
    assert T == R * Cn and len(flips) == F
    n = counts(ys, xs, F, th, tw, H, W)
    acc = np.zeros((C, H, W), F32)
    wsum = np.zeros((H, W), F32)
    for f in range(F):
        for r, (Y0, Y1) in enumerate(_cover(ys, th, H)):
            for c, (X0, X1) in enumerate(_cover(xs, tw, W)):
                if Y0 >= Y1 or X0 >= X1:
                    continue
                y = np.arange(Y0, Y1, dtype=np.int32) - np.int32(ys[r])
                x = np.arange(X0, X1, dtype=np.int32) - np.int32(xs[c])
                w = (tent(y, th, ramp_y)[:, None] * tent(x, tw, ramp_x)[None, :]).astype(F32)  # int32 product, one conversion
                w = np.where(n[Y0:Y1, X0:X1] == 1, F32(1), w).astype(F32)
                sy = th - 1 - y if int(flips[f]) & 2 else y
                sx = tw - 1 - x if int(flips[f]) & 1 else x
                v = sample(scores[f, r * Cn + c], th, tw, sy, sx)
                acc[:, Y0:Y1, X0:X1] = acc[:, Y0:Y1, X0:X1] + w * v
                wsum[Y0:Y1, X0:X1] = wsum[Y0:Y1, X0:X1] + w
    best = acc[0].copy()
    seg = np.zeros((H, W), np.int32)
    for k in range(1, C):
        better = acc[k] > best  # the first maximum wins
        best = np.where(better, acc[k], best)
        seg = np.where(better, np.int32(k), seg)
    seg = np.where(n == 0, np.int32(-1), seg).astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = acc / wsum
    out = np.where(n == 1, acc, out)
    out = np.where(n == 0, F32(0), out).astype(F32)
    return seg, out


# ------------------------------------------------------------------------------------------ the independent form
def resize_matrix(n_src: int, n_dst: int) -> np.ndarray:
    """(n_dst, n_src) float64: bilinear interpolation with align_corners=False as a matrix."""
    A = np.zeros((n_dst, n_src))
    for i in range(n_dst):
        a = max((i + 0.5) * n_src / n_dst - 0.5, 0.0)
        i0 = min(int(np.floor(a)), n_src - 1)
        i1 = min(i0 + 1, n_src - 1)
        A[i, i0] += 1.0 - (a - i0)
        A[i, i1] += a - i0
    return A


def blend_f64(scores, ys, xs, flips, H: int, W: int, th: int, tw: int, ramp_y: int, ramp_x: int):
    """The same blend in float64 with normalised separable weights -> out (C, H, W) float64 (NaN where nothing covers)."""
    scores = np.asarray(scores, np.float64)
    F, T, C, gh, gw = scores.shape
    R, Cn = len(ys), len(xs)
    Ay, Ax = resize_matrix(gh, th), resize_matrix(gw, tw)

    def axis_weights(origins, side, length, ramp):
        w = np.zeros((len(origins), length))
        for i, o in enumerate(origins):
            for P in range(max(0, o), min(length, o + side)):
                w[i, P] = min(P - o + 1, side - (P - o), ramp)
        with np.errstate(invalid="ignore"):
            return w / w.sum(0)

    ny, nx = axis_weights(ys, th, H, ramp_y), axis_weights(xs, tw, W, ramp_x)
    out = np.zeros((C, H, W))
    for f in range(F):
        for r in range(R):
            for c in range(Cn):
                full = np.einsum("yi,kij,xj->kyx", Ay, scores[f, r * Cn + c], Ax)
                if int(flips[f]) & 2:
                    full = full[:, ::-1]
                if int(flips[f]) & 1:
                    full = full[:, :, ::-1]
                Y0, Y1, X0, X1 = max(0, ys[r]), min(H, ys[r] + th), max(0, xs[c]), min(W, xs[c] + tw)
                part = full[:, Y0 - ys[r]:Y1 - ys[r], X0 - xs[c]:X1 - xs[c]]
                out[:, Y0:Y1, X0:X1] += ny[r, Y0:Y1, None] * nx[c, None, X0:X1] * part / F
    covered = counts(ys, xs, F, th, tw, H, W) > 0
    return np.where(covered, out, np.nan)


# ------------------------------------------------------------------------------------------------------ test inputs
def random_scores(F: int, T: int, C: int, gh: int, gw: int, seed: int) -> np.ndarray:
    """Asymmetric random score grids in [0, 1) on a 2^-12 raster, with deliberate exact ties: the last class repeats class
    0 in every view and tile, so its sums equal class 0's bit for bit at every pixel, and wherever class 0 wins the
    first-max rule has to choose it over its copy (across the chunk of eight when C > 8).  With C == 1 there is nothing
    to tie."""
    rng = np.random.default_rng(seed)
    s = (rng.integers(0, 4096, (F, T, C, gh, gw)) / 4096.0).astype(F32)
    if C >= 2:
        s[:, :, C - 1] = s[:, :, 0]
    return s
