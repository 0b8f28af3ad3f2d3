"""Writes tests/golden/preprocess_pil.npz: inputs and outputs of the dependency's Mask2FormerImageProcessorPil
(transformers), the contract `weed_instance_segmentation_amd.preprocess` is held to bit for bit.

Run where transformers and Pillow import: `python tests/golden/make_preprocess_golden.py`.  Each case stores its images
(`<case>.img<b>`, uint8 HWC), id maps (`<case>.map<b>`, uint8), the processor keywords and the id -> class dictionaries
as JSON, and the outputs `pixel_values`, `pixel_mask`, `mask_labels<b>`, `class_labels<b>`.
"""
from __future__ import annotations

import json
import os

import numpy as np


def _map(rng, h, w, n_ids, lost_id=None):
    """Blocky instance map: background 0 and ids 1..n_ids as rectangles; `lost_id` is a single pixel."""
    m = np.zeros((h, w), dtype=np.uint8)
    for i in range(1, n_ids + 1):
        y0, x0 = rng.integers(0, max(h - 2, 1)), rng.integers(0, max(w - 2, 1))
        m[y0:y0 + rng.integers(2, max(h // 2, 3)), x0:x0 + rng.integers(2, max(w // 2, 3))] = i
    if lost_id is not None:
        m[h // 2 + 1, w // 2 + 1] = lost_id
    return m


def cases():
    rng = np.random.default_rng(20261015)
    img = lambda h, w: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)  # noqa: E731
    ig = {"ignore_index": 255}
    out = [
        ("upscale_stretch", [img(37, 53)], [_map(rng, 37, 53, 4)], {"size": {"height": 80, "width": 120}, **ig}),
        ("downscale_3x_lost_id", [img(300, 420)], [_map(rng, 300, 420, 6, lost_id=7)],
         {"size": {"height": 96, "width": 128}, "size_divisor": 0, **ig}),
        ("identity", [img(64, 96)], [_map(rng, 64, 96, 3)], {"size": {"height": 64, "width": 96}, **ig}),
        ("one_px_wide", [img(50, 1)], [_map(rng, 50, 1, 2)], {"size": {"height": 40, "width": 24}, "size_divisor": 0,
                                                              **ig}),
        ("shortest_longest", [img(120, 90)], [_map(rng, 120, 90, 5)],
         {"size": {"shortest_edge": 64, "longest_edge": 100}, **ig}),
        ("shortest_longest_raw", [img(30, 200)], [_map(rng, 30, 200, 5)],
         {"size": {"shortest_edge": 64, "longest_edge": 150}, "size_divisor": 0, **ig}),
        ("max_height_width", [img(120, 90)], [_map(rng, 120, 90, 4)], {"size": {"max_height": 70, "max_width": 50},
                                                                      **ig}),
        ("reduce_labels", [img(48, 64)], [_map(rng, 48, 64, 4)], {"size": {"height": 64, "width": 64},
                                                                   "do_reduce_labels": True, **ig}),
        ("mixed_batch", [img(90, 60), img(50, 110), img(64, 64)],
         [_map(rng, 90, 60, 3), _map(rng, 50, 110, 5), _map(rng, 64, 64, 2)],
         {"size": {"shortest_edge": 48, "longest_edge": 96}, **ig}),
        ("empty_instances", [img(40, 40)], [np.full((40, 40), 255, dtype=np.uint8)],
         {"size": {"height": 32, "width": 32}, **ig}),
        ("images_only", [img(33, 47), img(20, 20)], None, {"size": {"shortest_edge": 40, "longest_edge": 64}}),
    ]
    return out


def main():
    import PIL
    import transformers
    from transformers.models.mask2former.image_processing_pil_mask2former import Mask2FormerImageProcessorPil

    proc = Mask2FormerImageProcessorPil()
    z = {"transformers_version": np.array(transformers.__version__), "pillow_version": np.array(PIL.__version__)}
    names = []
    for name, ims, maps, kw in cases():
        names.append(name)
        id2sem = None
        if maps is not None:
            id2sem = [{int(i): int(i) % 3 + 1 for i in np.unique(m)} for m in maps]
            z.update({f"{name}.map{b}": m for b, m in enumerate(maps)})
        r = proc(images=ims, segmentation_maps=maps, instance_id_to_semantic_id=id2sem, return_tensors="pt", **kw)
        z.update({f"{name}.img{b}": im for b, im in enumerate(ims)})
        z[f"{name}.kwargs"] = np.array(json.dumps(kw))
        z[f"{name}.id2sem"] = np.array(json.dumps(id2sem))
        z[f"{name}.pixel_values"] = r["pixel_values"].numpy()
        z[f"{name}.pixel_mask"] = r["pixel_mask"].numpy()
        if maps is not None:
            for b in range(len(ims)):
                z[f"{name}.mask_labels{b}"] = r["mask_labels"][b].numpy()
                z[f"{name}.class_labels{b}"] = r["class_labels"][b].numpy()
    z["cases"] = np.array(json.dumps(names))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "preprocess_pil.npz")
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
