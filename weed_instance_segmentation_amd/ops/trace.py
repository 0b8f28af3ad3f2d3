"""Tracing id maps into polygons: the boundary loops of every id in CSR layout."""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import load
from ._core import _id_maps, _launch, _p

CRACK, PIXEL = 0, 1  # coords


def _empty_trace(B, N, device):
    z = lambda n=0: torch.zeros(n, device=device, dtype=torch.int64)
    return torch.zeros(0, 2, device=device, dtype=torch.int32), z(1), z(), z(), z(), z(B * N + 1)


def labelmap_trace(maps: torch.Tensor, N: int, coords: int = PIXEL, simplify: bool = True):
    """The boundary loops of every id of (B, H, W) id maps (fp32 with -1 background, int32 or uint8), ids in [-1, N); id -1
    is not traced.  coords 0 ("crack"): corner-lattice vertices, exact; coords 1 ("pixel"): pixel indices, what
    `cv2.fillPoly` and VIA take.  simplify drops the points on straight runs.  The rules are written out in
    include/wm2f.h.  Returns, all on the device,
    (points (P, 2) int32 x, y; loop_offsets (L + 1) int64; loop_image (L) int64; loop_id (L) int64; twice_area (L) int64;
    slot_offsets (B * N + 1) int64): loop l is points[loop_offsets[l]:loop_offsets[l + 1]], the loops of id k of image b
    are slot_offsets[b * N + k] .. slot_offsets[b * N + k + 1], ordered by leader key; twice_area > 0 marks an outer loop,
    < 0 a hole (the crack value in both coordinate systems).
    Seven launch groups whose kernel count depends on the bit length of the edge count alone, prefix sums and one sort of
    the loops between them, and TWO device-to-host copies: the edge count, then the loop and point counts.  Raises
    ValueError when a map holds a value outside [-1, N)."""
    who = "labelmap_trace"
    maps, dt, B, H, W = _id_maps(maps, who, "tensors", contiguous=False)
    N, coords, simplify = int(N), int(coords), bool(simplify)
    if coords not in (CRACK, PIXEL):
        raise ValueError(f"{who}: coords is 0 (crack) or 1 (pixel), got {coords}")
    if N < 0 or N > _lib.WM2F_RLE_MAX_IDS:
        raise ValueError(f"{who}: N must be in [0, {_lib.WM2F_RLE_MAX_IDS}], got {N}")
    lib = load()
    size = int(lib.wm2f_trace_workspace(B, H, W, N))
    if size < 0:
        raise ValueError(f"{who}: unsupported size {B} x {H} x {W} (4 * B * H * W must stay below 2^31), N = {N}")
    maps = maps.contiguous()  # after the size check: a refused view is never copied
    dev = maps.device
    i32 = lambda n: torch.empty(n, device=dev, dtype=torch.int32)
    ws = torch.empty(size, device=dev, dtype=torch.uint8)
    counts = i32(B + 1)
    _launch("wm2f_trace_count", maps, _p(maps), dt, _p(counts), _p(ws), B, H, W, N, tag="trace_count")
    host = counts.cpu().tolist()  # copy 1: the edge count sizes the work arrays
    E, bad = host[0], host[1:]
    if any(bad):
        b = next(i for i, v in enumerate(bad) if v)
        raise ValueError(f"{who}: image {b} holds {bad[b]} pixels whose value is outside [-1, {N})")
    if E == 0:
        return _empty_trace(B, N, dev)

    edge_ws = torch.empty(int(lib.wm2f_trace_edge_workspace(E)), device=dev, dtype=torch.uint8)
    flag, lead = i32(E), i32(E)
    _launch("wm2f_trace_link", maps, _p(maps), dt, _p(ws), _p(edge_ws), E, B, H, W, N, tag="trace_link")
    _launch("wm2f_trace_rank", maps, _p(edge_ws), E, tag="trace_rank")
    _launch("wm2f_trace_flags", maps, _p(edge_ws), _p(flag), _p(lead), E, H, W, coords, int(simplify), tag="trace_flags")
    lead_prefix = torch.cumsum(lead, 0, dtype=torch.int32)
    n_loops, P = torch.stack([lead_prefix[-1], flag.sum(dtype=torch.int32)]).cpu().tolist()  # copy 2: sizes the result
    if n_loops <= 0 or P <= 0:
        raise _lib.Wm2fError(f"{who}: {E} edges but {n_loops} loops and {P} points")

    loop_key, loop_len = torch.empty(n_loops, device=dev, dtype=torch.int64), i32(n_loops)
    _launch("wm2f_trace_loops", maps, _p(maps), dt, _p(edge_ws), _p(lead_prefix), _p(loop_key), _p(loop_len), E, n_loops,
            B, H, W, N, tag="trace_loops")
    loop_key, order = torch.sort(loop_key)  # (image * N + id, leader): the loop order of the contract
    loop_place = i32(n_loops)
    loop_place[order] = torch.arange(n_loops, device=dev, dtype=torch.int32)
    loop_base = torch.zeros(n_loops + 1, device=dev, dtype=torch.int32)
    torch.cumsum(loop_len[order], 0, dtype=torch.int32, out=loop_base[1:])
    flag_sorted, edge_sorted, term_sorted = i32(E), i32(E), i32(E)
    _launch("wm2f_trace_scatter", maps, _p(edge_ws), _p(flag), _p(lead_prefix), _p(loop_place), _p(loop_base),
            _p(flag_sorted), _p(edge_sorted), _p(term_sorted), E, n_loops, H, W, tag="trace_scatter")
    flag_prefix = torch.zeros(E + 1, device=dev, dtype=torch.int32)
    torch.cumsum(flag_sorted, 0, dtype=torch.int32, out=flag_prefix[1:])
    points = i32(2 * P).view(P, 2)
    _launch("wm2f_trace_emit", maps, _p(edge_ws), _p(flag_sorted), _p(edge_sorted), _p(flag_prefix[1:]), _p(points), E, P,
            H, W, coords, tag="trace_emit")

    base = loop_base.long()
    loop_offsets = flag_prefix[base].long()
    area_prefix = torch.zeros(E + 1, device=dev, dtype=torch.int64)
    torch.cumsum(term_sorted, 0, dtype=torch.int64, out=area_prefix[1:])
    area_at = area_prefix[base]
    slot = loop_key >> 32
    slot_offsets = torch.searchsorted(slot, torch.arange(B * N + 1, device=dev, dtype=torch.int64))
    n = max(N, 1)
    return points, loop_offsets, slot // n, slot % n, area_at[1:] - area_at[:-1], slot_offsets
