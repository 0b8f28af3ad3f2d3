"""Writes tests/golden/rotate_pil.npz: small images and id maps, orientations and what Pillow makes of them
(`transpose(FLIP_TOP_BOTTOM)`, `transpose(ROTATE_*)`, `rotate(angle, BILINEAR / NEAREST, fillcolor)`,
tests/rotate_reference.py: pil_orient_image / pil_orient_map).  DESIGN section 30 holds the GPU path to it byte for byte.

Run where Pillow imports: `python tests/golden/make_rotate_golden.py`.  Each case stores its images (`<case>.img<b>`,
uint8 HWC), its id maps (`<case>.map<b>`, uint8 or int32), the orientations as JSON (`<case>.params`, one
[vflip, turns, angle, [r, g, b], map_fill] per image) and Pillow's results (`<case>.out<b>`, `<case>.mout<b>`).  The case
`composed_with_everything` also stores a colour chain, augmentation rows [flip, h, w, y0, x0, ch, cw] that refer to the
turned frame, the padded size and the processor outputs of tests/augment_reference.py:pil_expected on the colour-jittered,
oriented image and the oriented map, as make_photometric_golden.py does.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

COMPOSED = "composed_with_everything"
CHAIN = [["saturation", 1.2], ["contrast", 0.6], ["hue", -0.2], ["brightness", 1.1]]


def cases():
    """(name, sizes, dtype of the maps, params): the eight flip / turn combinations on non-square images with odd widths,
    the angles 1, 13.37, 45, 90 and -7.5, non-zero fills, a batch of three sizes, an int32 map with ids > 255."""
    out = [(f"vflip{v}_turns{k}", [(5 + 2 * k, 9 + 4 * v)], "uint8", [[v, k, 0.0, [0, 0, 0], 0]])
           for v in (0, 1) for k in range(4)]
    out += [
        ("angle_1", [(33, 95)], "uint8", [[0, 0, 1.0, [0, 0, 0], 0]]),
        ("angle_13p37_fills", [(61, 75)], "uint8", [[0, 0, 13.37, [7, 130, 255], 9]]),
        ("angle_45_square", [(64, 64)], "uint8", [[0, 0, 45.0, [255, 0, 1], 200]]),
        ("angle_90_non_square", [(5, 9)], "uint8", [[0, 0, 90.0, [3, 2, 1], 4]]),
        ("angle_minus_7p5_after_flip_and_turn", [(47, 31)], "uint8", [[1, 1, -7.5, [10, 20, 30], 5]]),
        ("batch_of_three", [(33, 37), (17, 91), (45, 23)], "uint8",
         [[0, 3, 30.000001, [1, 2, 3], 1], [0, 0, 0.0, [0, 0, 0], 0], [1, 0, 359.9, [0, 0, 0], 0]]),
        ("int32_ids_above_255", [(40, 57)], "int32", [[1, 2, 89.99, [0, 0, 0], 70001]]),
        (COMPOSED, [(75, 96)], "uint8", [[1, 1, 13.37, [124, 116, 104], 0]]),
    ]
    return out


def main():
    import PIL
    from augment_reference import blocky_map, pil_expected
    from photometric_reference import pil_apply
    from rotate_reference import pil_orient_image, pil_orient_map
    from weed_instance_segmentation_amd.augment import AugmentParams

    rng = np.random.default_rng(20261019)
    z = {"pillow_version": np.array(PIL.__version__)}
    names = []
    for name, sizes, dtype, params in cases():
        names.append(name)
        z[f"{name}.params"] = np.array(json.dumps(params))
        for b, ((H, W), (vf, k, angle, fill, mfill)) in enumerate(zip(sizes, params)):
            im = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            m = blocky_map(rng, H, W, 4) if name == COMPOSED else rng.integers(0, 256 if dtype == "uint8" else 70000,
                                                                               (H, W)).astype(dtype)
            z[f"{name}.img{b}"], z[f"{name}.map{b}"] = im, m
            z[f"{name}.out{b}"] = pil_orient_image(im, vf, k, angle, fill)
            z[f"{name}.mout{b}"] = pil_orient_map(m, vf, k, angle, mfill)
        if name == COMPOSED:
            vf, k, angle, fill, mfill = params[0]
            rows, pad = [[1, 80, 62, 20, 0, 33, 31]], {"height": 48, "width": 48}  # the turned frame is (96, 75)
            m = z[f"{name}.map0"]
            id2sem = [{int(i): int(i) % 3 + 1 for i in np.unique(m)}]
            aug = [AugmentParams(r[0], (r[1], r[2]), (r[3], r[4]), (r[5], r[6])) for r in rows]
            oriented = pil_orient_image(pil_apply(z[f"{name}.img0"], CHAIN), vf, k, angle, fill)
            pv, pm, ml, cl = pil_expected([oriented], [z[f"{name}.mout0"]], id2sem, aug, pad, 255)
            z[f"{name}.chain"], z[f"{name}.rows"] = np.array(json.dumps(CHAIN)), np.array(json.dumps(rows))
            z[f"{name}.pad_size"], z[f"{name}.id2sem"] = np.array(json.dumps(pad)), np.array(json.dumps(id2sem))
            z[f"{name}.pixel_values"], z[f"{name}.pixel_mask"] = pv, pm
            z[f"{name}.mask_labels0"], z[f"{name}.class_labels0"] = ml[0], cl[0]
    z["cases"] = np.array(json.dumps(names))
    path = os.path.join(HERE, "rotate_pil.npz")
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
