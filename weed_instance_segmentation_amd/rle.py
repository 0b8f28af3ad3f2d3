"""Run-length encodings of id maps, and the COCO results export.

    from weed_instance_segmentation_amd import coco_results, decode_rle, encode_label_maps, save_coco_results
    rles = encode_label_maps(prediction["segmentation"], n=len(prediction["segments_info"]))  # id -> COCO RLE
    save_coco_results("predictions.json", predictions, image_ids)

The pixels are read on the device, twice, whatever the number of segments (csrc/rle.hip: a count launch and a write
launch that leave every segment's TOGGLE positions -- where its membership flips along the scan -- on the device).  This
module is the host half, numpy over those toggle lists without a loop over pixels:
- "coco": column-major alternating run counts starting with a 0-run, `{"size": [H, W], "counts": ...}`, the counts as
  the compressed ASCII string of the COCO API (`rle_to_string` / `rle_from_string`) or as the plain list;
- "hf": the row-major `[start + 1, length, ...]` list of the dependency's `binary_mask_to_rle`.
`decode_rle` paints either form back into a device map (`ops.rle_paint_`).
"""
from __future__ import annotations

import json

import numpy as np
import torch

from . import _lib, ops

_MAX_BATCH = 32  # images per encode / paint call (the kernels' bound)
FORMATS = {"coco": 1, "hf": 0}  # format -> scan order


# ------------------------------------------------------------------------------------------------- the COCO string codec
def rle_to_string(counts) -> str:
    """COCO API's rleToString: counts[i] (minus counts[i - 2] for i > 2) in 5-bit groups, least significant first, bit
    0x20 set on every group but the last, each group + 48 as one ASCII character."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    x = c.copy()
    x[3:] -= c[1:-2]
    groups, alive = [], np.ones(len(x), bool)
    while alive.any():
        g = x & 0x1f
        x = x >> 5  # arithmetic
        more = np.where(g & 0x10, x != -1, x != 0)
        groups.append(np.where(alive, (g | (more.astype(np.int64) << 5)) + 48, 0))
        alive = alive & more
    if not groups:
        return ""
    chars = np.stack(groups, 1).reshape(-1)
    return chars[chars != 0].astype(np.uint8).tobytes().decode("ascii")


def rle_from_string(s) -> list[int]:
    """COCO API's rleFrString, the inverse of `rle_to_string` (str or bytes)."""
    raw = np.frombuffer(s.encode("ascii") if isinstance(s, str) else bytes(s), dtype=np.uint8).astype(np.int64) - 48
    if raw.size == 0:
        return []
    if ((raw < 0) | (raw > 63)).any() or raw[-1] & 0x20:
        raise ValueError("rle_from_string: not a COCO RLE string")
    last = (raw & 0x20) == 0  # the last group of a count
    first = np.concatenate([[True], last[:-1]])
    start = np.nonzero(first)[0]
    k = np.arange(raw.size) - np.repeat(start, np.diff(np.append(start, raw.size)))  # position inside its count
    if int(k.max()) > 12:
        raise ValueError("rle_from_string: a count of more than 13 characters")
    x = np.add.reduceat((raw & 0x1f) << (5 * k), start)
    end = np.nonzero(last)[0]
    x = np.where(raw[end] & 0x10, x | (np.int64(-1) << (5 * (k[end] + 1))), x)  # sign extension
    x[1::2] = np.cumsum(x[1::2])  # counts[i] += counts[i - 2] for i > 2: the odd chain starts at 1 ...
    x[2::2] = np.cumsum(x[2::2])  # ... the even chain at 2; counts[0] stands alone
    return x.tolist()


# ------------------------------------------------------------------------------------------- toggle lists -> encodings
def toggles_to_coco_counts(toggles, n_pixels: int) -> np.ndarray:
    """A segment's toggle list in column-major order -> COCO's alternating run counts, the first a 0-run (0 when the mask
    starts at the first pixel), no trailing 0 when it ends at the last."""
    t = np.asarray(toggles, dtype=np.int64)
    counts = np.diff(np.concatenate([[0], t, [int(n_pixels)]]))
    return counts[:-1] if counts[-1] == 0 and len(counts) > 1 else counts


def toggles_to_hf(toggles) -> np.ndarray:
    """A toggle list in row-major order -> `binary_mask_to_rle`'s [start + 1, length, start + 1, length, ...]."""
    t = np.asarray(toggles, dtype=np.int64)
    out = np.empty_like(t)
    out[0::2] = t[0::2] + 1
    out[1::2] = t[1::2] - t[0::2]
    return out


def encode_toggles(counts, positions, offsets, size, format: str = "coco", compressed: bool = True) -> list[dict]:
    """The host half of `encode_label_maps`: counts (B, N + 1), positions (total) and offsets (B * (N + 1) + 1) as
    `ops.labelmap_toggles` returns them (on the host), size = (H, W) -> per image a dict id -> RLE over the ids with at
    least one pixel, ascending (-1, the background, first)."""
    if format not in FORMATS:
        raise ValueError(f"format must be one of {sorted(FORMATS)}, got {format!r}")
    counts, positions, offsets = np.asarray(counts), np.asarray(positions, dtype=np.int64), np.asarray(offsets)
    H, W = int(size[0]), int(size[1])
    B, N1 = counts.shape
    if format == "hf":  # every list has even length, so the pairs of the whole array are the pairs of the lists
        positions = toggles_to_hf(positions)
    out = []
    for b in range(B):
        image = {}
        for s in np.nonzero(counts[b])[0].tolist():
            o = b * N1 + s
            t = positions[int(offsets[o]):int(offsets[o + 1])]
            if format == "hf":
                image[s - 1] = t.tolist()
            else:
                c = toggles_to_coco_counts(t, H * W)
                image[s - 1] = {"size": [H, W], "counts": rle_to_string(c) if compressed else c.tolist()}
        out.append(image)
    return out


def _as_device_maps(maps, who: str):
    if not torch.cuda.is_available():
        raise _lib.Wm2fError(f"{who} runs on a GPU only (no CPU fallback): no device is visible")
    if isinstance(maps, (list, tuple)):
        maps = torch.stack([torch.as_tensor(m) for m in maps])
    elif isinstance(maps, np.ndarray):
        maps = torch.from_numpy(np.ascontiguousarray(maps))
    if not isinstance(maps, torch.Tensor) or maps.dim() not in (2, 3):
        raise ValueError(f"{who}: expected an (H, W) map, a (B, H, W) stack or a list of maps of one size")
    if maps.dtype not in (torch.float32, torch.int32, torch.uint8):
        raise TypeError(f"{who}: maps fp32 / int32 / uint8, got {maps.dtype}")
    return maps if maps.is_cuda else maps.to(torch.device("cuda", torch.cuda.current_device()))


def encode_label_maps(maps, n: int | None = None, format: str = "coco", compressed: bool = True):
    """Run-length encode every id of one (H, W) id map, a (B, H, W) stack or a list of maps of one size -- fp32 with -1
    background (the post-processor's map), int32 or uint8; a host map is moved to the current GPU.

    The ids are -1 (background) and 0 .. n-1; without `n` it is taken from the maps' maximum (one more
    synchronisation); a value outside [-1, n) raises ValueError.  Returns per image a dict id -> RLE that holds only the
    ids with at least one pixel, in ascending order (one dict for an (H, W) map, else a list of them):
    - format="coco": `{"size": [H, W], "counts": ...}`, column-major, counts as the compressed string, or the list of
      ints with compressed=False;
    - format="hf": the row-major list of `binary_mask_to_rle`."""
    if format not in FORMATS:
        raise ValueError(f"format must be one of {sorted(FORMATS)}, got {format!r}")
    maps = _as_device_maps(maps, "encode_label_maps")
    single = maps.dim() == 2
    stack = maps.unsqueeze(0) if single else maps
    if n is None:
        n = max(0, int(stack.max()) + 1)
    out = []
    for b0 in range(0, stack.shape[0], _MAX_BATCH):
        part = stack[b0:b0 + _MAX_BATCH]
        counts, positions, offsets = ops.labelmap_toggles(part, int(n), FORMATS[format])
        out += encode_toggles(counts, positions.cpu().numpy(), offsets, part.shape[1:], format, compressed)
    return out[0] if single else out


# ------------------------------------------------------------------------------------------------------------ decoding
def rle_to_runs(rle, format: str = "coco") -> np.ndarray:
    """One RLE -> its 1-runs as an (R, 2) int64 array of (start, length) in the format's scan order."""
    if format == "hf":
        l = np.asarray(rle, dtype=np.int64).reshape(-1)
        if l.size % 2:
            raise ValueError("an hf run-length list has an even number of entries")
        runs = np.stack([l[0::2] - 1, l[1::2]], 1)
    else:
        c = rle["counts"]
        c = np.asarray(rle_from_string(c) if isinstance(c, (str, bytes)) else c, dtype=np.int64).reshape(-1)
        ends = np.cumsum(c)
        runs = np.stack([ends[0:-1:2], c[1::2]], 1) if c.size > 1 else np.zeros((0, 2), np.int64)
    return runs[runs[:, 1] != 0]


def _is_image_dict(x) -> bool:
    return isinstance(x, dict) and "counts" not in x


def _runs_of_image(image, values, format):
    if _is_image_dict(image):
        keys = list(image)
        vals = keys if values is None else [values[k] for k in keys] if isinstance(values, dict) else list(values)
        rles = [image[k] for k in keys]
    else:
        rles = list(image)
        vals = list(range(len(rles))) if values is None else list(values)
    if len(vals) != len(rles):
        raise ValueError(f"{len(rles)} RLEs but {len(vals)} values")
    return [(rle_to_runs(r, format), int(v)) for r, v in zip(rles, vals)], [int(v) for v in vals]


def decode_rle(rles, size=None, format: str = "coco", values=None, background: int = -1, as_masks: bool = False,
               device="cuda"):
    """Paint RLEs into an int32 id map on the device (`ops.rle_paint_`).

    `rles` is one image -- a dict id -> RLE as `encode_label_maps` returns it, or a list of RLEs -- and gives an (H, W)
    map; or a list of such dicts, which gives a (B, H, W) stack.  RLE i is painted with `values[i]` (a list in the RLEs'
    order, or for dicts a dict id -> value); by default with its dict key, or its position in the list.  Later RLEs
    paint over earlier ones; uncovered pixels are `background`.  format="coco" takes compressed or plain counts and
    reads the size off the RLEs; format="hf" needs `size` = (H, W).  An RLE that is longer than its image raises
    Wm2fError (it is never clipped).  as_masks=True (one image) returns instead the (T, H, W) uint8 stack
    `map == value` of the painted values (`ops.labelmap_to_masks`; H * W divisible by 4)."""
    if format not in FORMATS:
        raise ValueError(f"format must be one of {sorted(FORMATS)}, got {format!r}")
    batch = isinstance(rles, (list, tuple)) and len(rles) > 0 and all(_is_image_dict(x) for x in rles)
    images = list(rles) if batch else [rles]
    if as_masks and batch:
        raise ValueError("decode_rle: as_masks works on one image")
    if size is None:
        if format == "hf":
            raise ValueError('decode_rle: format="hf" needs size=(H, W)')
        sizes = {tuple(int(v) for v in r["size"]) for im in images for r in (im.values() if _is_image_dict(im) else im)}
        if len(sizes) != 1:
            raise ValueError(f"decode_rle: the RLEs must share one size (pass size= for none), got {sorted(sizes)}")
        size = sizes.pop()
    H, W = int(size[0]), int(size[1])
    out = torch.full((len(images), H, W), int(background), dtype=torch.int32, device=device)
    painted = []
    for b0 in range(0, len(images), _MAX_BATCH):
        rows = []
        for j, image in enumerate(images[b0:b0 + _MAX_BATCH]):
            runs, painted = _runs_of_image(image, values, format)
            for r, v in runs:
                rows.append(np.concatenate([np.full((len(r), 1), j), r, np.full((len(r), 1), v)], 1))
        if not rows:
            continue
        table = np.concatenate(rows).astype(np.int64)
        if table.size and (np.abs(table).max() >= 2 ** 31):
            raise ValueError("decode_rle: a run does not fit int32")
        ops.rle_paint_(out[b0:b0 + _MAX_BATCH], torch.from_numpy(table.astype(np.int32)).to(out.device), FORMATS[format])
    if as_masks:
        return ops.labelmap_to_masks(out[0], torch.tensor(painted, dtype=torch.int32, device=out.device))
    return out if batch else out[0]


# --------------------------------------------------------------------------------------------------- COCO results export
def _category(category_of, label: int):
    if category_of is None:
        return int(label)
    return category_of(label) if callable(category_of) else category_of[label]


def coco_results(results, image_ids, category_of=None) -> list[dict]:
    """The list `post_process_instance_segmentation(..., return_instance_stats=True)` returns -> the COCO results list
    (what `COCO.loadRes` and annotation tools read): per instance that still owns a pixel
    `{"image_id", "category_id", "segmentation": {"size", "counts"}, "bbox": [x, y, w, h], "area", "score"}`.
    `image_ids[i]` names image i; `category_of` maps a label id to the dataset's category id (a dict or a callable; the
    label id itself without one).  One encode call per distinct map size."""
    if len(results) != len(image_ids):
        raise ValueError(f"{len(results)} results but {len(image_ids)} image ids")
    groups: dict = {}
    for i, r in enumerate(results):
        seg = r["segmentation"]
        if not isinstance(seg, torch.Tensor) or seg.dim() != 2:
            raise ValueError("coco_results: every result needs its (H, W) id map as `segmentation`")
        groups.setdefault(tuple(seg.shape), []).append(i)
    out: list = [None] * len(results)
    for rows in groups.values():
        n = max(len(results[i]["segments_info"]) for i in rows)
        encoded = encode_label_maps([results[i]["segmentation"] for i in rows], n=n, format="coco", compressed=True)
        for i, rles in zip(rows, encoded):
            entries = []
            for info in results[i]["segments_info"]:
                if info["id"] not in rles:  # painted over entirely
                    continue
                if "bbox" not in info or "area" not in info:
                    raise ValueError("coco_results: segments_info carries no bbox / area; post-process with "
                                     "return_instance_stats=True")
                entries.append({"image_id": image_ids[i], "category_id": _category(category_of, info["label_id"]),
                                "segmentation": rles[info["id"]], "bbox": [int(v) for v in info["bbox"]],
                                "area": int(info["area"]), "score": float(info["score"])})
            out[i] = entries
    return [e for entries in out for e in entries]


def save_coco_results(path, results, image_ids, category_of=None) -> list[dict]:
    """`coco_results(...)` written to `path` as JSON; returns the list."""
    entries = coco_results(results, image_ids, category_of)
    with open(path, "w") as f:
        json.dump(entries, f)
    return entries
