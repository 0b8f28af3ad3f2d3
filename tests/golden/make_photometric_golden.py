"""Writes tests/golden/photometric_pil.npz: small images, colour chains and what Pillow makes of them
(`ImageEnhance.Brightness / Contrast / Color` and a hue shift through `convert("HSV")`, tests/photometric_reference.py:
pil_apply).  DESIGN section 29 holds the GPU path to it byte for byte.

Run where Pillow imports: `python tests/golden/make_photometric_golden.py`.  Each case stores its images (`<case>.img<b>`,
uint8 HWC), the chains as JSON (`<case>.ops`, one list of [kind, value] per image) and Pillow's results (`<case>.out<b>`).
The case `composed_with_geometry` also stores an id map, augmentation rows [flip, h, w, y0, x0, ch, cw], the padded size
and the processor outputs of tests/augment_reference.py:pil_expected on the colour-jittered image, as
make_augment_golden.py does.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

B, C, S, H = "brightness", "contrast", "saturation", "hue"
GEOMETRY = "composed_with_geometry"


def cases():
    """(name, images, chains): chains of one to four steps in different orders, the factors at which a fused blend
    differs, odd widths, a batch with an empty chain and one without contrast."""
    rng = np.random.default_rng(20261019)
    img = lambda h, w: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)  # noqa: E731
    return [
        ("brightness_1p2", [img(40, 57)], [[[B, 1.2]]]),
        ("brightness_0p6_one_pixel", [img(1, 1)], [[[B, 0.6]]]),
        ("contrast_1p6", [img(33, 95)], [[[C, 1.6]]]),
        ("contrast_0p85_row", [img(1, 5)], [[[C, 0.85]]]),
        ("saturation_1p7", [img(5, 7)], [[[S, 1.7]]]),
        ("saturation_0p8", [img(64, 64)], [[[S, 0.8]]]),
        ("hue_minus_0p03", [img(47, 31)], [[[H, -0.03]]]),
        ("hue_zero_still_converts", [img(16, 19)], [[[H, 0.0]]]),
        ("two_steps_hue_then_contrast", [img(29, 96)], [[[H, 0.5], [C, 1.1]]]),
        ("three_steps_without_hue", [img(61, 75)], [[[S, 1.830188512802124], [B, 0.9639175534248352], [C, 0.2928571105003357]]]),
        ("four_steps_bcsh", [img(50, 71)], [[[B, 1.1], [C, 0.8], [S, 1.2], [H, 0.25]]]),
        ("four_steps_hscb", [img(71, 50)], [[[H, -0.5], [S, 0.6], [C, 1.7], [B, 0.85]]]),
        ("batch_mixed", [img(33, 37), img(17, 91), img(45, 23)],
         [[[C, 1.2], [H, 0.1]], [], [[S, 1.6], [B, 0.8]]]),
        (GEOMETRY, [img(75, 80)], [[[S, 1.2], [C, 0.6], [H, -0.2], [B, 1.1]]]),
    ]


def main():
    import PIL
    from augment_reference import blocky_map, pil_expected
    from photometric_reference import pil_apply
    from weed_instance_segmentation_amd.augment import AugmentParams

    z = {"pillow_version": np.array(PIL.__version__)}
    names = []
    for name, ims, chains in cases():
        names.append(name)
        z[f"{name}.ops"] = np.array(json.dumps(chains))
        for b, (im, ops) in enumerate(zip(ims, chains)):
            z[f"{name}.img{b}"], z[f"{name}.out{b}"] = im, pil_apply(im, ops)
        if name == GEOMETRY:
            rows, pad = [[1, 60, 64, 20, 0, 33, 31]], {"height": 48, "width": 48}
            m = blocky_map(np.random.default_rng(7), 75, 80, 4)
            id2sem = [{int(i): int(i) % 3 + 1 for i in np.unique(m)}]
            params = [AugmentParams(r[0], (r[1], r[2]), (r[3], r[4]), (r[5], r[6])) for r in rows]
            pv, pm, ml, cl = pil_expected([z[f"{name}.out0"]], [m], id2sem, params, pad, 255)
            z[f"{name}.map0"], z[f"{name}.params"] = m, np.array(json.dumps(rows))
            z[f"{name}.pad_size"], z[f"{name}.id2sem"] = np.array(json.dumps(pad)), np.array(json.dumps(id2sem))
            z[f"{name}.pixel_values"], z[f"{name}.pixel_mask"] = pv, pm
            z[f"{name}.mask_labels0"], z[f"{name}.class_labels0"] = ml[0], cl[0]
    z["cases"] = np.array(json.dumps(names))
    path = os.path.join(HERE, "photometric_pil.npz")
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
