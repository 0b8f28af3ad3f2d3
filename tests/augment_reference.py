"""The augmentation contract of DESIGN section 20 restated in numpy (no GPU): mirror the source, apply Pillow's tap
tables of the full resize, cut the window, look up, pad.  tests/test_augment_cpu.py holds it to Pillow itself and to the
dependency's PIL processor; tests/golden/make_augment_golden.py and tests/test_augment_gpu.py use the Pillow route."""
from __future__ import annotations

import numpy as np

from weed_instance_segmentation_amd import preprocess as P


def _apply_bilinear(a: np.ndarray, bounds: np.ndarray, coef: np.ndarray, axis: int) -> np.ndarray:
    """One Pillow 8-bit pass along `axis` of a uint8 array: clip8((2^21 + sum coef * u8) >> 22)."""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    taps = np.arange(coef.shape[1])[None, :]
    valid = taps < bounds[:, 1:2]
    idx = np.where(valid, bounds[:, 0:1] + taps, 0)
    c = np.where(valid, coef, 0).astype(np.int64)
    s = (1 << (P.PRECISION_BITS - 1)) + np.einsum("nk,nk...->n...", c, a[idx])
    return np.moveaxis(np.clip(s >> P.PRECISION_BITS, 0, 255).astype(np.uint8), 0, axis)


def image_window(im: np.ndarray, p) -> np.ndarray:
    """(ch, cw, 3) uint8: steps 1-3 of the contract for an (H, W, 3) image."""
    (h, w), (y0, x0), (ch, cw) = p.size, p.origin, p.window
    H, W = im.shape[:2]
    src = im[:, ::-1] if p.flip else im
    r = _apply_bilinear(_apply_bilinear(src, *P.bilinear_tables(W, w), 1), *P.bilinear_tables(H, h), 0)
    return r[y0:y0 + ch, x0:x0 + cw]


def map_window(m: np.ndarray, p) -> np.ndarray:
    """(ch, cw): steps 1-3 of the contract for an (H, W) id map."""
    (h, w), (y0, x0), (ch, cw) = p.size, p.origin, p.window
    H, W = m.shape
    src = m[:, ::-1] if p.flip else m
    return src[P.nearest_table(H, h)][:, P.nearest_table(W, w)][y0:y0 + ch, x0:x0 + cw]


def pil_image_window(im: np.ndarray, p) -> np.ndarray:
    """The same window from Pillow: transpose, resize, crop."""
    from PIL import Image
    (h, w), (y0, x0), (ch, cw) = p.size, p.origin, p.window
    a = Image.fromarray(im)
    if p.flip:
        a = a.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(a.resize((w, h), Image.BILINEAR).crop((x0, y0, x0 + cw, y0 + ch)))


def pil_map_window(m: np.ndarray, p) -> np.ndarray:
    from PIL import Image
    (h, w), (y0, x0), (ch, cw) = p.size, p.origin, p.window
    a = Image.fromarray(m)
    if p.flip:
        a = a.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(a.resize((w, h), Image.NEAREST).crop((x0, y0, x0 + cw, y0 + ch)))


def assemble(img_windows, map_windows, id2sem, pad_size=None, ignore_index=255, do_reduce_labels=False, lut=None):
    """Steps 4-6: lookup, padding to (Hp, Wp), masks and classes of the ids inside each window.
    Returns (pixel_values, pixel_mask, [mask_labels], [class_labels])."""
    if lut is None:
        lut = P.normalize_table(True, 1 / 255, True, P.IMAGENET_DEFAULT_MEAN, P.IMAGENET_DEFAULT_STD)
    if pad_size is not None:
        Hp, Wp = pad_size["height"], pad_size["width"]
    else:
        Hp, Wp = max(a.shape[0] for a in img_windows), max(a.shape[1] for a in img_windows)
    B = len(img_windows)
    pv = np.zeros((B, 3, Hp, Wp), np.float32)
    pm = np.zeros((B, Hp, Wp), np.int64)
    ml, cl = [], []
    for b, r in enumerate(img_windows):
        ch, cw = r.shape[:2]
        pv[b, :, :ch, :cw] = lut[np.arange(3)[:, None, None], r.transpose(2, 0, 1)]
        pm[b, :ch, :cw] = 1
        if map_windows is None:
            continue
        m = map_windows[b]
        ids = np.unique(m)
        if ignore_index is not None:
            ids = ids[ids != ignore_index]
        if (ch, cw) != (Hp, Wp) and ignore_index is None:
            raise ValueError("padding mask_labels needs ignore_index")
        masks = np.full((len(ids), Hp, Wp), ignore_index if ignore_index is not None else 0, np.float32)
        masks[:, :ch, :cw] = m[None] == ids[:, None, None]
        ml.append(masks)
        d = id2sem[b] if isinstance(id2sem, list) else id2sem
        if d is None:
            cl.append(ids.astype(np.int64))
        elif do_reduce_labels:
            cl.append(np.array([d[int(i) + 1] - 1 for i in ids], np.int64))
        else:
            cl.append(np.array([d[int(i)] for i in ids], np.int64))
    return pv, pm, ml, cl


def restate(images, maps, id2sem, params, pad_size=None, ignore_index=255, do_reduce_labels=False):
    """The whole contract in numpy for a batch; `params` is one AugmentParams per image."""
    if maps is not None and do_reduce_labels:
        maps = [np.where(m == 0, ignore_index, m.astype(np.int64) - 1).astype(np.uint8) for m in maps]
    iw = [image_window(im, p) for im, p in zip(images, params)]
    mw = None if maps is None else [map_window(m, p) for m, p in zip(maps, params)]
    return assemble(iw, mw, id2sem, pad_size, ignore_index, do_reduce_labels)


def pil_expected(images, maps, id2sem, params, pad_size=None, ignore_index=255):
    """The same outputs with the windows taken from Pillow (the golden file's expected values)."""
    iw = [pil_image_window(im, p) for im, p in zip(images, params)]
    mw = None if maps is None else [pil_map_window(m, p) for m, p in zip(maps, params)]
    return assemble(iw, mw, id2sem, pad_size, ignore_index)


def blocky_map(rng, h, w, n_ids) -> np.ndarray:
    """Background 0 and ids 1..n_ids as rectangles."""
    m = np.zeros((h, w), dtype=np.uint8)
    for i in range(1, n_ids + 1):
        y0, x0 = rng.integers(0, max(h - 2, 1)), rng.integers(0, max(w - 2, 1))
        m[y0:y0 + rng.integers(2, max(h // 2, 3)), x0:x0 + rng.integers(2, max(w // 2, 3))] = i
    return m
