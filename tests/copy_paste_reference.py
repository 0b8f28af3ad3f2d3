"""Simple Copy-Paste (contract: include/wm2f.h) restated in numpy, in two independent forms.

`copy_paste_reference` works on id maps, step by step as the contract names them: A (strike what does not land or lands
too little of itself), B (paste, count `before` and `after`), C (repaint destination instances that kept too little).
`copy_paste_stacks` never forms a pasted id map: it works on one boolean mask per instance -- destination masks
`& ~union`, pasted masks appended, empty masks removed -- and is what the GPU path's `mask_labels` are held to.
`map_to_stacks` is the bridge between the two (what `expand_labels` does with a map).
"""
from __future__ import annotations

import numpy as np


def is_id(v) -> np.ndarray:
    v = np.asarray(v)
    return (v >= 0) & (v <= 254)


def shifted(a: np.ndarray, dy: int, dx: int, fill) -> np.ndarray:
    """out[y, x] = a[y - dy, x - dx] where that lies inside the frame, else `fill`; (..., H, W) arrays."""
    H, W = a.shape[-2:]
    out = np.full_like(a, fill)
    ys0, ys1 = max(0, -dy), min(H, H - dy)
    xs0, xs1 = max(0, -dx), min(W, W - dx)
    if ys0 < ys1 and xs0 < xs1:
        out[..., ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx] = a[..., ys0:ys1, xs0:xs1]
    return out


def copy_paste_reference(pixels, maps, source, lut, shift, window=None, num=0, den=1, ignore_index=255):
    """pixels (B, C, H, W) float32, maps (B, H, W) int32, source (B,), lut (B, 256), shift (B, 2), window (B, 2) or None.
    Returns (pixels, maps, lut_final (B, 256) int32, areas (B, 3, 256) int32 = before, after, original).  Pixels move as
    bit patterns (through a uint32 view)."""
    pixels = np.ascontiguousarray(pixels, dtype=np.float32)
    maps = np.ascontiguousarray(maps, dtype=np.int32)
    B, C, H, W = pixels.shape
    bits = pixels.view(np.uint32)
    out_bits, out_maps = bits.copy(), maps.copy()
    lut = np.asarray(lut).astype(np.int64)
    lut_final = np.full((B, 256), -1, dtype=np.int32)
    areas = np.zeros((B, 3, 256), dtype=np.int32)
    num, den = int(num), int(den)
    for b in range(B):
        s = int(source[b])
        h, w = (H, W) if window is None else (int(window[b][0]), int(window[b][1]))
        dy, dx = int(shift[b][0]), int(shift[b][1])
        dest = maps[b]
        take = np.zeros((H, W), dtype=bool)
        new = dest.copy()
        if s >= 0:
            assert s != b
            src_at = shifted(maps[s], dy, dx, -1)  # the source id that would arrive at (y, x)
            inside = np.zeros((H, W), dtype=bool)
            inside[:h, :w] = True
            # A
            for i in range(255):
                if not 0 <= lut[b, i] <= 254:
                    continue
                original = int((maps[s] == i).sum())
                landed = int(((src_at == i) & inside).sum())
                areas[b, 2, i] = original
                if landed > 0 and landed * den >= num * original:
                    lut_final[b, i] = lut[b, i]
            # B
            live = np.zeros(256, dtype=bool)
            live[:255] = lut_final[b, :255] >= 0
            arrives = is_id(src_at)
            take = inside & arrives & live[np.where(arrives, src_at, 0)]
            new[take] = lut_final[b][src_at[take]]
            moved = shifted(bits[s], dy, dx, 0)
            out_bits[b] = np.where(take[None], moved, bits[b])
        for i in range(255):
            areas[b, 0, i] = int((dest == i).sum())
            areas[b, 1, i] = int((new == i).sum())
        # C
        for i in range(255):
            before, after = int(areas[b, 0, i]), int(areas[b, 1, i])
            if after > 0 and after * den < num * before:
                new[new == i] = ignore_index
        out_maps[b] = new
    return out_bits.view(np.float32), out_maps, lut_final, areas


def map_to_stacks(id_map, id_to_class: dict, ignore_index=255):
    """What `expand_labels` makes of one map: ((T, H, W) bool masks of the ascending ids without ignore_index, (T,) classes)."""
    ids = [int(i) for i in np.unique(id_map) if int(i) != ignore_index]
    masks = np.stack([id_map == i for i in ids]) if ids else np.zeros((0,) + id_map.shape, dtype=bool)
    return masks, np.array([int(id_to_class[i]) for i in ids], dtype=np.int64)


def copy_paste_stacks(dest_masks, dest_ids, source_masks, source_ids, new_of: dict, shift, window, num=0, den=1):
    """The second formulation, on mask stacks alone.  `dest_masks` (T, H, W) bool with their ids `dest_ids`,
    `source_masks` (S, H, W) bool with their ids `source_ids`, `new_of` {source id: new id} (the selection).
    Returns the (id, mask) list of the result in ascending id order, empty masks removed."""
    H, W = dest_masks.shape[1:] if len(dest_masks) else source_masks.shape[1:]
    h, w = window
    dy, dx = shift
    frame = np.zeros((H, W), dtype=bool)
    frame[:h, :w] = True
    pasted = []
    for i, m in zip(source_ids, source_masks):
        if int(i) not in new_of:
            continue
        moved = np.zeros((H, W), dtype=bool)
        for y, x in zip(*np.nonzero(m)):
            if 0 <= y + dy < H and 0 <= x + dx < W:
                moved[y + dy, x + dx] = True
        moved &= frame
        if moved.sum() == 0 or moved.sum() * den < num * m.sum():
            continue
        pasted.append((int(new_of[int(i)]), moved))
    union = np.zeros((H, W), dtype=bool)
    for _, m in pasted:
        union |= m
    result = []
    for i, m in zip(dest_ids, dest_masks):
        left = m & ~union
        if left.sum() == 0 or left.sum() * den < num * m.sum():
            continue
        result.append((int(i), left))
    result += pasted
    return sorted(result, key=lambda t: t[0])
