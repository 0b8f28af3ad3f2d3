"""Segmentation overlays and contours on the GPU: what the reference draws with matplotlib.

    from weed_instance_segmentation_amd import render_segmentation, save_comparison
    picture, legend = render_segmentation(image, result, config=model.config)       # plot_segmentation(ax, image, result, model)
    save_comparison("worst_03.png", image, result, convert_gt_map_to_result(gt_map, id_mapping), config=model.config)

- `render_segmentation` / `render_segmentations` follow models/model_utils.py::plot_segmentation: a fill at alpha 0.4
  and a contour at full colour per segment, `tab20` up to 20 colours and `nipy_spectral` above, a colour per instance
  or per class, the score filter, the legend.
- `render_label_overlay` is the dataset visualisers' picture (datasets/pheno_bench/visualize.py): class colours at
  alpha 0.5 over the whole picture.
One launch of csrc/overlay.hip reads picture and map once, whatever the number of segments, and the picture stays on
the device.  The rendering is at the map's own resolution with exact integer arithmetic (include/wm2f.h); it is not a
reproduction of matplotlib's resampled, anti-aliased figure.  There is no matplotlib import and no CPU route: without a
GPU or the library every renderer raises `Wm2fError`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, _palette, ops

_MAP_DTYPES = (torch.float32, torch.int32, torch.uint8)
_NARROWED = (torch.int64, torch.int16, torch.int8, torch.bool)


def palette(n: int) -> np.ndarray:
    """The (max(n, 1), 3) uint8 colours plot_segmentation picks for n segments (or classes): `tab20` in its own order up
    to 20, above that `nipy_spectral` at np.linspace(0, 1, n) -- entry min(int(x * 256), 255) of its 256-entry table."""
    n = int(n)
    if n <= 20:
        return _palette.tab20()[:max(n, 1)].copy()
    idx = np.minimum((np.linspace(start=0, stop=1, num=n) * 256).astype(np.int64), 255)
    return _palette.nipy_spectral()[idx]


def _label_text(label_id, id2label, config) -> str:
    from_config = getattr(config, "id2label", None)
    if from_config is not None and label_id in from_config:
        return from_config[label_id]
    return (id2label or {}).get(label_id, f"Class {label_id}")


def build_overlay_tables(result: dict, *, id2label: dict | None = None, config=None, instance_mode: bool = True,
                         score_threshold: float = 0.0, alpha: float = 0.4):
    """The kernel's tables for one `{'segmentation', 'segments_info'}` result, as plot_segmentation would colour it.
    Pure host code.  Returns (ids (n) int32 ascending, rgba (n, 4) uint8, order (n) int32, legend [(text, (r, g, b))]).

    Segments with score < `score_threshold` are dropped (a missing score counts as 1.0).  Instance mode: one colour per
    kept segment, legend "<label> <running count per label>".  Class mode: one colour per distinct label_id in sorted
    order, one legend entry per class on first sight.  Label text: `config.id2label`, then `id2label`, then
    'Class <label_id>'.  `order` is the segment's position among the kept ones; an id listed twice keeps its last entry
    (the reference overwrites the earlier fill and draws the later contour on top), both legend entries stay.  Alpha is
    round(alpha * 255); dropped and unlisted segments are not in the tables."""
    kept = [s for s in result["segments_info"] if s.get("score", 1.0) >= score_threshold]
    if instance_mode:
        colours = palette(len(kept))
    else:
        labels = sorted(set(s["label_id"] for s in kept))
        colour_of_label = {lbl: i for i, lbl in enumerate(labels)}
        colours = palette(len(labels))
    a = int(round(float(alpha) * 255))
    if not 0 <= a <= 255:
        raise ValueError(f"alpha must lie in [0, 1], got {alpha}")
    counts, seen, legend, entry = {}, set(), [], {}
    for i, seg in enumerate(kept):
        label_id = seg["label_id"]
        text = _label_text(label_id, id2label, config)
        counts[text] = counts.get(text, 0) + 1
        if instance_mode:
            rgb = tuple(int(v) for v in colours[i % len(colours)])
            legend.append((f"{text} {counts[text]}", rgb))
        else:
            rgb = tuple(int(v) for v in colours[colour_of_label[label_id] % len(colours)])
            if label_id not in seen:
                seen.add(label_id)
                legend.append((text, rgb))
        entry[int(seg["id"])] = (rgb, i)  # a later entry of the same id replaces the earlier one
    ids = np.asarray(sorted(entry), np.int64)
    if len(ids) and (ids.min() < -2 ** 31 or ids.max() >= 2 ** 31):
        raise ValueError("segment ids must fit int32")
    rgba = np.asarray([[*entry[int(k)][0], a] for k in ids], np.uint8).reshape(-1, 4)
    order = np.asarray([entry[int(k)][1] for k in ids], np.int32)
    return ids.astype(np.int32), rgba, order, legend


# ------------------------------------------------------------------------------------------------- device plumbing
def _device():
    if not torch.cuda.is_available():
        raise _lib.Wm2fError("the overlay renderers run on a GPU only (no CPU fallback): no device is visible")
    return torch.device("cuda", torch.cuda.current_device())


def _picture(image, dev) -> torch.Tensor:
    """PIL image, numpy array or torch tensor -> (H, W, 3) uint8 on the device."""
    if not isinstance(image, (np.ndarray, torch.Tensor)):
        image = np.array(image.convert("RGB"))  # PIL (a writable copy)
    t = torch.from_numpy(np.ascontiguousarray(image)) if isinstance(image, np.ndarray) else image
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise TypeError(f"a picture is uint8 (H, W, 3), got {t.dtype} {tuple(t.shape)}")
    return t.to(dev)


def _id_map(seg, dev) -> torch.Tensor:
    """An id map of the post-processors (fp32, int32) or a ground-truth map (uint8, any integer type) -> a device
    tensor of a kernel dtype; wider or narrower integers become int32 after a range check."""
    t = torch.from_numpy(np.ascontiguousarray(seg)) if isinstance(seg, np.ndarray) else torch.as_tensor(seg)
    if t.dim() != 2:
        raise ValueError(f"an id map is (H, W), got {tuple(t.shape)}")
    t = t.to(dev)
    if t.dtype in _NARROWED:
        if t.dtype == torch.int64 and t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
            raise ValueError("an int64 id map must fit int32")
        t = t.to(torch.int32)
    if t.dtype not in _MAP_DTYPES:
        raise TypeError(f"id maps are fp32, uint8 or an integer type, got {t.dtype}")
    return t


def _stack(pictures, maps):
    if len(pictures) != len(maps) or not pictures:
        raise ValueError("as many pictures as maps, and at least one")
    if len({tuple(p.shape) for p in pictures}) != 1 or len({m.dtype for m in maps}) != 1:
        raise ValueError("one call renders pictures of one size and maps of one dtype")
    if tuple(maps[0].shape) != tuple(pictures[0].shape[:2]) or len({tuple(m.shape) for m in maps}) != 1:
        raise ValueError(f"picture {tuple(pictures[0].shape)} and map {tuple(maps[0].shape)} disagree")
    return torch.stack(pictures), torch.stack(maps)


def _pad_tables(tables, dev):
    """[(ids, rgba, order)] per image -> the (B, N) device tensors of ops.labelmap_overlay, or four Nones when N == 0."""
    B, N = len(tables), max(len(t[0]) for t in tables)
    if N == 0:
        return None, None, None, None
    ids, rgba, order = np.zeros((B, N), np.int32), np.zeros((B, N, 4), np.uint8), np.full((B, N), -1, np.int32)
    for b, (i, c, o) in enumerate(tables):
        ids[b, :len(i)], rgba[b, :len(i)], order[b, :len(i)] = i, c, o
    n_ids = np.asarray([len(t[0]) for t in tables], np.int32)
    return tuple(torch.from_numpy(x).to(dev) for x in (ids, n_ids, rgba, order))


# ------------------------------------------------------------------------------------------------------- renderers
def render_segmentations(images, results, *, id2label: dict | None = None, config=None, instance_mode: bool = True,
                         score_threshold: float = 0.0, alpha: float = 0.4, contour_width: int = 2):
    """plot_segmentation for a batch of pictures of one size, in one launch.  Returns the (B, H, W, 3) uint8 device
    tensor and one legend per picture.  See `render_segmentation`."""
    dev = _device()
    w = int(contour_width)
    if not 0 <= w <= 8:
        raise ValueError(f"contour_width goes from 0 to 8, got {contour_width}")
    tables, legends = [], []
    for r in results:
        ids, rgba, order, legend = build_overlay_tables(r, id2label=id2label, config=config, instance_mode=instance_mode,
                                                        score_threshold=score_threshold, alpha=alpha)
        tables.append((ids, rgba, order))
        legends.append(legend)
    pictures, maps = _stack([_picture(i, dev) for i in images], [_id_map(r["segmentation"], dev) for r in results])
    out = ops.labelmap_overlay(pictures, maps, *_pad_tables(tables, dev), default_rgba=(0, 0, 0, 0), inner=(w + 1) // 2,
                               outer=w // 2)
    return out, legends


def render_segmentation(image, result: dict, *, id2label: dict | None = None, config=None, instance_mode: bool = True,
                        score_threshold: float = 0.0, alpha: float = 0.4, contour_width: int = 2):
    """The picture of plot_segmentation(ax, image, result, model, id2label, instance_mode, score_threshold) as a uint8
    (H, W, 3) device tensor, and its legend [(text, (r, g, b)), ...].

    `image`: a PIL image, a numpy array or a torch tensor, uint8 (H, W, 3).  `result`: `{'segmentation',
    'segments_info'}` of a post-processor (fp32 or int32 map) or of `convert_gt_map_to_result` (any integer map; int64
    is narrowed to int32 after a range check).  `config`: anything with an `id2label` (pass `model.config`).
    `contour_width` (0 .. 8) pixels of contour, ceil(w / 2) of them inside the segment and floor(w / 2) outside: the
    default 2 straddles the boundary as the reference's two-point line does; 0 draws fills only."""
    out, legends = render_segmentations([image], [result], id2label=id2label, config=config, instance_mode=instance_mode,
                                        score_threshold=score_threshold, alpha=alpha, contour_width=contour_width)
    return out[0], legends[0]


def render_label_overlay(image, mask, colors: dict, *, default_color=(255, 255, 0), alpha: float = 0.5,
                         names: dict | None = None):
    """The dataset visualisers' picture: `colors[label]` blended at `alpha` over every pixel of the picture, label 0
    included (black unless `colors` says otherwise, so the background darkens as in the reference), labels absent from
    `colors` in `default_color`, no contours.  Returns the uint8 (H, W, 3) device tensor and the legend of the non-zero
    labels present, ascending, as [(names.get(label, 'Class <label>'), (r, g, b))].  Which labels are present comes from
    `ops.labelmap_instance_stats` on the device (labels 0 .. 255 of a uint8 mask, 0 .. 4095 of a wider one)."""
    dev = _device()
    a = int(round(float(alpha) * 255))
    if not 0 <= a <= 255:
        raise ValueError(f"alpha must lie in [0, 1], got {alpha}")
    table = {0: (0, 0, 0), **{int(k): tuple(int(c) for c in v) for k, v in colors.items()}}
    ids = np.asarray(sorted(table), np.int32)
    rgba = np.asarray([[*table[int(k)], a] for k in ids], np.uint8)
    pictures, maps = _stack([_picture(image, dev)], [_id_map(mask, dev)])
    out = ops.labelmap_overlay(pictures, maps, *_pad_tables([(ids, rgba, np.full(len(ids), -1, np.int32))], dev),
                               default_rgba=(*(int(c) for c in default_color), a), inner=0, outer=0)
    area = ops.labelmap_instance_stats(maps, N=256 if maps.dtype == torch.uint8 else 4096)[0, :, 0]
    present = [int(v) for v in torch.nonzero(area > 0).flatten().tolist() if v != 0]
    default = tuple(int(c) for c in default_color)
    legend = [((names or {}).get(lbl, f"Class {lbl}"), table.get(lbl, default)) for lbl in present]
    return out[0], legend


def convert_gt_map_to_result(gt_map, id_mapping: dict) -> dict:
    """models/mask2former/show_worst_predictions.py::convert_gt_map_to_result: a ground-truth id map and its
    {raw id: label_id} mapping as the `{'segmentation', 'segments_info'}` the renderers take.  255 and ids outside the
    mapping are left out (they stay unpainted); every segment has score 1.0.  The map stays where it is."""
    seg = torch.from_numpy(np.ascontiguousarray(gt_map)) if isinstance(gt_map, np.ndarray) else torch.as_tensor(gt_map)
    info = [{"id": int(u), "label_id": id_mapping[int(u)], "score": 1.0}
            for u in torch.unique(seg).tolist() if int(u) != 255 and int(u) in id_mapping]
    return {"segmentation": seg, "segments_info": info}


# ------------------------------------------------------------------------------------------------ host convenience
def _panel(picture: torch.Tensor, legend, title):
    """A rendered picture as a PIL image with its title and legend (upper right) drawn on the host."""
    from PIL import Image, ImageDraw
    img = Image.fromarray(picture.cpu().numpy())
    draw = ImageDraw.Draw(img)
    if title:
        draw.text((5, 4), title, fill=(255, 255, 255), stroke_width=1, stroke_fill=(0, 0, 0))
    if legend:
        line, sw = 13, 9
        width = max(int(draw.textlength(text)) for text, _ in legend) + sw + 14
        x0, y0 = max(0, img.width - width - 4), 4
        draw.rectangle([x0, y0, x0 + width, y0 + line * len(legend) + 5], fill=(245, 245, 245), outline=(90, 90, 90))
        for k, (text, rgb) in enumerate(legend):
            y = y0 + 3 + k * line
            draw.rectangle([x0 + 4, y + 1, x0 + 4 + sw, y + 1 + sw], fill=tuple(rgb), outline=(0, 0, 0))
            draw.text((x0 + sw + 9, y), text, fill=(0, 0, 0))
    return img


def save_comparison(path, image, prediction: dict, ground_truth: dict | None = None, *, id2label: dict | None = None,
                    config=None, instance_mode: bool = True, score_threshold: float = 0.0, alpha: float = 0.4,
                    contour_width: int = 2, titles=("Prediction", "Ground truth")):
    """Writes the rendered prediction to a PNG at `path` -- next to the rendered `ground_truth` result (for instance
    `convert_gt_map_to_result(...)`), side by side, when one is given, as show_worst_predictions.py shows them.  The
    score filter applies to the prediction only.  Legends and titles are drawn on the host with PIL's default font."""
    from PIL import Image
    kw = dict(id2label=id2label, config=config, instance_mode=instance_mode, alpha=alpha, contour_width=contour_width)
    panels = [_panel(*render_segmentation(image, prediction, score_threshold=score_threshold, **kw), titles[0])]
    if ground_truth is not None:
        panels.append(_panel(*render_segmentation(image, ground_truth, **kw), titles[1]))
    sheet = Image.new("RGB", (sum(p.width for p in panels), max(p.height for p in panels)), (255, 255, 255))
    x = 0
    for p in panels:
        sheet.paste(p, (x, 0))
        x += p.width
    sheet.save(path, format="PNG")
    return path
