"""Instance maps from semantic annotation masks on the GPU: the cv2 part of the reference's dataset
loaders, restated on hand-written HIP (csrc/ccl.hip).

    from weed_instance_segmentation_amd.annotations import PhenoBenchDataset, CropWeedDataset

are drop-ins for datasets/pheno_bench/dataset.py:PhenoBenchDataset and for the CropWeed PNG loader
(datasets/crop_weed/annotation_dependent_implementations/dataset_from_png_annotations.py:CropWeedDataset).

- `connected_components(mask)`: the `cv2.connectedComponents(mask)` contract (8-connectivity).
- `resize_nearest(mask, dsize)`: `cv2.resize(mask, dsize, interpolation=cv2.INTER_NEAREST)`.
- `semantic_to_instance_map` / `color_mask_to_instance_map`: steps 2-4 of the two loaders (nearest resize, one
  `connectedComponents` per class, ids 1, 2, ... in class order with 255 skipped, 255 outside every component), in one
  pass of kernels over the whole map instead of one per class and one full-image paint per component.

Components are numbered the way OpenCV's block-based labelling numbers them: by the first 2 x 2 block of the component in
block-raster order, which is not the raster order of the first pixel (scipy / skimage order).
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

from . import _lib, ops
from ._lib import Wm2fError

__all__ = ["cv2_nearest_table", "connected_components", "resize_nearest", "semantic_to_instance_map",
           "color_mask_to_instance_map", "PhenoBenchDataset", "CropWeedDataset"]


def cv2_nearest_table(src_size: int, dst_size: int) -> np.ndarray:
    """OpenCV's resizeNN source indices along one axis: ifx = 1 / (dst / src) in float64, then
    min(floor(i * ifx), src - 1).  The double rounding is part of the contract (1488 -> 1024 maps column 64 to 92, where
    64 * 1488 // 1024 = 93)."""
    if src_size <= 0 or dst_size <= 0:
        raise ValueError(f"sizes must be positive, got {src_size} -> {dst_size}")
    ifx = 1.0 / (float(dst_size) / float(src_size))
    idx = np.floor(np.arange(dst_size, dtype=np.float64) * ifx).astype(np.int64)
    return np.minimum(idx, src_size - 1).astype(np.int32)


def _require_cuda(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch tensor on the GPU, got {type(t).__name__}")
    if not t.is_cuda:
        raise Wm2fError(f"{name} is on {t.device}: the wm2f kernels run on a GPU only (no CPU fallback)")
    return t


def _tables(src_hw, dsize):
    """(ty, tx, (h, w)) for cv2's dsize = (w, h); None tables when the size does not change."""
    sh, sw = src_hw
    if dsize is None:
        return None, None, (sh, sw)
    w, h = int(dsize[0]), int(dsize[1])
    if w <= 0 or h <= 0:
        raise ValueError(f"dsize must be positive (w, h), got {dsize}")
    if (h, w) == (sh, sw):
        return None, None, (h, w)
    return cv2_nearest_table(sh, h), cv2_nearest_table(sw, w), (h, w)


def connected_components(mask: torch.Tensor, connectivity: int = 8):
    """`cv2.connectedComponents(mask)` on the device: (H, W) uint8 / bool / uint16 / int32 mask, nonzero = foreground.
    Returns (num_labels, labels): labels (H, W) int32 with 0 on the background and components 1 .. num_labels - 1
    numbered as OpenCV numbers them; num_labels counts the background, as cv2's does."""
    if connectivity != 8:
        raise ValueError(f"connectivity={connectivity}: only 8-connectivity is implemented (the reference uses no other)")
    mask = _require_cuda(mask, "mask")
    labels, _, n = ops.label_components(mask, _lib.WM2F_CCL_BINARY, skip_255=False, background=0)
    return n + 1, labels


def resize_nearest(mask: torch.Tensor, dsize) -> torch.Tensor:
    """`cv2.resize(mask, dsize, interpolation=cv2.INTER_NEAREST)` on the device with dsize = (w, h): (H, W) uint8,
    uint16 or int32 maps, (H, W, 3) uint8 colour maps."""
    mask = _require_cuda(mask, "mask")
    ok = (mask.dim() == 2 and mask.dtype in (torch.uint8, torch.uint16, torch.int32)) or (
        mask.dim() == 3 and mask.shape[2] == 3 and mask.dtype == torch.uint8)
    if not ok:
        raise TypeError(f"resize_nearest: expected (H, W) uint8 / uint16 / int32 or (H, W, 3) uint8, got "
                        f"{tuple(mask.shape)} {mask.dtype}")
    w, h = int(dsize[0]), int(dsize[1])
    if w <= 0 or h <= 0:
        raise ValueError(f"dsize must be positive (w, h), got {dsize}")
    sh, sw = int(mask.shape[0]), int(mask.shape[1])
    return ops.resize_nearest_tables(mask, cv2_nearest_table(sh, h), cv2_nearest_table(sw, w))


def semantic_to_instance_map(semantic_mask: torch.Tensor, size=None):
    """PhenoBench's rule (datasets/pheno_bench/dataset.py:85-116) on the device: optional nearest resize to
    size = (w, h) (cv2's dsize order), then one instance per 8-connected component of each nonzero class, classes in
    ascending value order, ids 1, 2, ... with 255 skipped, 255 outside every component.
    `semantic_mask` is (H, W) uint8, uint16 or int32.  Returns (instance_map (h, w) int32 on the device,
    id_to_semantic {id: class value})."""
    m = _require_cuda(semantic_mask, "semantic_mask")
    if m.dim() != 2 or m.dtype not in (torch.uint8, torch.uint16, torch.int32):
        raise TypeError(f"semantic_mask: expected (H, W) uint8 / uint16 / int32, got {tuple(m.shape)} {m.dtype}")
    ty, tx, hw = _tables(m.shape, size)
    out, comp_class, n = ops.label_components(m, _lib.WM2F_CCL_VALUE, hw, ty, tx)
    return out, _id_dict(comp_class.cpu().numpy(), n, None)


def color_mask_to_instance_map(mask_rgb: torch.Tensor, color_map: dict, size=None):
    """The CropWeed PNG rule (dataset_from_png_annotations.py:80-116) on the device: optional nearest resize to
    size = (w, h), then one instance per 8-connected component of the pixels equal to each colour, colours tried in the
    dict's order, ids 1, 2, ... with 255 skipped.  `mask_rgb` is (H, W, 3) uint8 RGB; `color_map` maps a class name to
    {'color': [r, g, b], 'id': semantic id}.  Returns (instance_map (h, w) int32 on the device,
    id_to_semantic {id: color_map[...]['id']})."""
    m = _require_cuda(mask_rgb, "mask_rgb")
    if m.dim() != 3 or m.shape[2] != 3 or m.dtype != torch.uint8:
        raise TypeError(f"mask_rgb: expected (H, W, 3) uint8, got {tuple(m.shape)} {m.dtype}")
    infos = list(color_map.values())
    if not infos or len(infos) > _lib.WM2F_CCL_MAX_COLORS:
        raise ValueError(f"color_map: 1 to {_lib.WM2F_CCL_MAX_COLORS} colours, got {len(infos)}")
    colors = [[int(c) for c in info["color"]] for info in infos]
    ty, tx, hw = _tables(m.shape[:2], size)
    out, comp_class, n = ops.label_components(m, _lib.WM2F_CCL_RGB, hw, ty, tx, colors=colors)
    return out, _id_dict(comp_class.cpu().numpy(), n, [int(info["id"]) for info in infos])


def _id_dict(classes: np.ndarray, n: int, semantic_of_colour):
    ids = np.arange(1, n + 1)
    ids[254:] += 1  # 255 is skipped
    if semantic_of_colour is None:
        return {int(i): int(c) for i, c in zip(ids, classes)}
    return {int(i): semantic_of_colour[int(c) - 1] for i, c in zip(ids, classes)}


def _read_semantic_png(path: str) -> np.ndarray:
    """A semantic PNG as cv2.IMREAD_UNCHANGED gives its values: 16-bit grayscale (PIL mode I;16 or I) or 8-bit L."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode in ("I;16", "I;16B", "I;16L"):
            return np.asarray(im).astype(np.uint16)
        if im.mode == "I":
            a = np.asarray(im)
            if a.size and (int(a.min()) < 0 or int(a.max()) > 65535):
                raise ValueError(f"{path}: 32-bit values outside 0..65535 are not a PNG semantic mask")
            return a.astype(np.uint16)
        if im.mode == "L":
            return np.asarray(im).astype(np.uint8)
        raise ValueError(f"{path}: semantic mask in PIL mode {im.mode!r}; expected a 16-bit (I;16 / I) or 8-bit (L) "
                         "grayscale PNG (palette and colour semantic masks are not read)")


class _AnnotatedPngDataset(torch.utils.data.Dataset):
    """File pairing and item assembly shared by the two loaders; subclasses give the mask file and the instance map."""

    def __init__(self, image_folder_path, annotation_path, processor, label2id: dict, max_input_dim: int = 1024,
                 max_images=None, device="cuda"):
        self.image_folder = image_folder_path
        self.annotation_path = annotation_path
        self.processor = processor
        self.label2id = label2id
        self.max_input_dim = int(max_input_dim)
        self.device = torch.device(device)
        self.image_files = sorted(glob.glob(os.path.join(self.image_folder, "*.png")))
        self.valid_files = []
        for img_path in self.image_files:
            mask_path = os.path.join(self.annotation_path, self._mask_name(os.path.basename(img_path)))
            if os.path.exists(mask_path):
                self.valid_files.append((img_path, mask_path))
                if max_images is not None and len(self.valid_files) >= max_images:
                    break
        print(f'\tLoaded {len(self.valid_files)} valid image/mask pairs from "{self.image_folder}"')

    def __len__(self):
        return len(self.valid_files)

    def __getitem__(self, idx: int) -> dict:
        from PIL import Image
        image_path, mask_path = self.valid_files[idx]
        file_name = os.path.basename(image_path)
        image = Image.open(image_path).convert("RGB")
        mask = self._read_mask(mask_path)
        width, height = image.size
        dsize = None
        if max(width, height) > self.max_input_dim:
            scale_factor = self.max_input_dim / max(width, height)
            new_width, new_height = int(width * scale_factor), int(height * scale_factor)
            image = image.resize(size=(new_width, new_height), resample=Image.BILINEAR)
            dsize = (new_width, new_height)
            width, height = new_width, new_height
        target_size = (height, width)
        instance_map, id_to_semantic = self._instance_map(torch.from_numpy(mask).to(self.device), dsize)
        instance_map = instance_map.cpu().numpy()
        inputs = self.processor(images=[image], segmentation_maps=[instance_map],
                                instance_id_to_semantic_id=id_to_semantic, return_tensors="pt", ignore_index=255)
        return {
            "pixel_values": inputs["pixel_values"][0],
            "mask_labels": inputs["mask_labels"][0],
            "class_labels": inputs["class_labels"][0],
            "target_size": target_size,
            "original_map": instance_map,
            "id_to_semantic": id_to_semantic,
            "file_name": file_name,
        }


class PhenoBenchDataset(_AnnotatedPngDataset):
    """datasets/pheno_bench/dataset.py:PhenoBenchDataset with the instance map built on the GPU.  Images `*.png` in
    `image_folder_path`, the 16-bit semantic mask of the same name in `annotation_path`; `max_input_dim` and
    `max_images` stand for config.MAX_INPUT_DIM and config.MAX_IMAGES."""

    @staticmethod
    def _mask_name(file_name: str) -> str:
        return os.path.splitext(file_name)[0] + ".png"

    @staticmethod
    def _read_mask(path: str) -> np.ndarray:
        return _read_semantic_png(path)

    def _instance_map(self, mask, dsize):
        return semantic_to_instance_map(mask, dsize)


class CropWeedDataset(_AnnotatedPngDataset):
    """The CropWeed PNG loader (dataset_from_png_annotations.py:CropWeedDataset) with the instance map built on the GPU.
    Image `<n>_<anything>.png` pairs with `<n>_annotation.png`, an RGB colour mask (green crop, red weed)."""

    @staticmethod
    def _mask_name(file_name: str) -> str:
        return os.path.splitext(file_name)[0].split("_")[0] + "_annotation.png"

    @staticmethod
    def _read_mask(path: str) -> np.ndarray:
        from PIL import Image
        with Image.open(path) as im:
            return np.array(im.convert("RGB"))

    def color_map(self) -> dict:
        return {
            "crop": {"color": [0, 255, 0], "id": self.label2id.get("crop", 0)},
            "weed": {"color": [255, 0, 0], "id": self.label2id.get("weed", 1)},
        }

    def _instance_map(self, mask, dsize):
        return color_mask_to_instance_map(mask, self.color_map(), dsize)
