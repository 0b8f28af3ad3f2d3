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

The polygon loaders' `cv2.fillPoly` runs on csrc/polygon.hip:

    from weed_instance_segmentation_amd.annotations import SorghumWeedDataset
    from weed_instance_segmentation_amd.annotations import CropWeedYamlDataset as CropWeedDataset
    from weed_instance_segmentation_amd.annotations import load_ground_truth

stand for datasets/sorghum_weed/dataset.py:SorghumWeedDataset, the CWFID YAML loader
(dataset_from_yaml_annotations.py:CropWeedDataset) and models/mask2former/inference.py:load_ground_truth.

- `fill_poly(img, pts, color)`: the `cv2.fillPoly(img, pts, color)` contract on an (H, W) int32 device map.
- `polygons_to_instance_map(polygons, ids, size)`: one fillPoly per polygon, in order, in one launch chain.
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

from . import _lib, ops
from ._lib import Wm2fError

__all__ = ["cv2_nearest_table", "connected_components", "resize_nearest", "semantic_to_instance_map",
           "color_mask_to_instance_map", "PhenoBenchDataset", "CropWeedDataset", "fill_poly",
           "polygons_to_instance_map", "SorghumWeedDataset", "CropWeedYamlDataset", "load_ground_truth"]


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


def semantic_to_instance_map(semantic_mask: torch.Tensor, size=None, split=None):
    """PhenoBench's rule (datasets/pheno_bench/dataset.py:85-116) on the device: optional nearest resize to
    size = (w, h) (cv2's dsize order), then one instance per 8-connected component of each nonzero class, classes in
    ascending value order, ids 1, 2, ... with 255 skipped, 255 outside every component.
    `semantic_mask` is (H, W) uint8, uint16 or int32.  Returns (instance_map (h, w) int32 on the device,
    id_to_semantic {id: class value}).
    `split=SplitOptions(...)` (not in the reference) parts components that are touching plants: the
    parts split off continue the numbering after the last id, 255 skipped, and carry their parent's class."""
    m = _require_cuda(semantic_mask, "semantic_mask")
    if m.dim() != 2 or m.dtype not in (torch.uint8, torch.uint16, torch.int32):
        raise TypeError(f"semantic_mask: expected (H, W) uint8 / uint16 / int32, got {tuple(m.shape)} {m.dtype}")
    ty, tx, hw = _tables(m.shape, size)
    out, comp_class, n = ops.label_components(m, _lib.WM2F_CCL_VALUE, hw, ty, tx)
    return _split_instances(out, _id_dict(comp_class.cpu().numpy(), n, None), n, split)


def color_mask_to_instance_map(mask_rgb: torch.Tensor, color_map: dict, size=None, split=None):
    """The CropWeed PNG rule (dataset_from_png_annotations.py:80-116) on the device: optional nearest resize to
    size = (w, h), then one instance per 8-connected component of the pixels equal to each colour, colours tried in the
    dict's order, ids 1, 2, ... with 255 skipped.  `mask_rgb` is (H, W, 3) uint8 RGB; `color_map` maps a class name to
    {'color': [r, g, b], 'id': semantic id}.  Returns (instance_map (h, w) int32 on the device,
    id_to_semantic {id: color_map[...]['id']}).  `split=SplitOptions(...)`: as for `semantic_to_instance_map`."""
    m = _require_cuda(mask_rgb, "mask_rgb")
    if m.dim() != 3 or m.shape[2] != 3 or m.dtype != torch.uint8:
        raise TypeError(f"mask_rgb: expected (H, W, 3) uint8, got {tuple(m.shape)} {m.dtype}")
    infos = list(color_map.values())
    if not infos or len(infos) > _lib.WM2F_CCL_MAX_COLORS:
        raise ValueError(f"color_map: 1 to {_lib.WM2F_CCL_MAX_COLORS} colours, got {len(infos)}")
    colors = [[int(c) for c in info["color"]] for info in infos]
    ty, tx, hw = _tables(m.shape[:2], size)
    out, comp_class, n = ops.label_components(m, _lib.WM2F_CCL_RGB, hw, ty, tx, colors=colors)
    return _split_instances(out, _id_dict(comp_class.cpu().numpy(), n, [int(info["id"]) for info in infos]), n, split)


def _id_dict(classes: np.ndarray, n: int, semantic_of_colour):
    ids = np.arange(1, n + 1)
    ids[254:] += 1  # 255 is skipped
    if semantic_of_colour is None:
        return {int(i): int(c) for i, c in zip(ids, classes)}
    return {int(i): semantic_of_colour[int(c) - 1] for i, c in zip(ids, classes)}


def _loader_id(k):
    """The loader's id of the k-th instance, k from 0: 1, 2, ... with 255 skipped (a number or an array)."""
    return k + 1 + (k >= 254)


def _split_instances(out: torch.Tensor, id_to_semantic: dict, n: int, split):
    """`split=` of the two PNG loaders: the loader's map (ids 1 .. with 255 skipped, 255 background) is renumbered
    0 .. n-1 with -1 background, split, and numbered back; the dictionary gets the parts split off."""
    if split is None:
        return out, id_to_semantic
    from .instances import SplitOptions, split_rows
    if not isinstance(split, SplitOptions):
        raise TypeError(f"split must be a SplitOptions or None, got {type(split).__name__}")
    if n == 0:
        return out, id_to_semantic
    compact = torch.where(out == 255, -1, out - 1 - (out > 255).to(out.dtype))
    parted, info, status = split_rows(compact.unsqueeze(0), n, split)
    parted = parted[0]
    out = torch.where(parted < 0, 255, _loader_id(parted)).to(torch.int32)
    host = torch.cat([status[0, :1], info[0, :, 0]]).cpu().numpy()
    n_out, parents = min(int(host[0]), split.id_space(n)), host[1:]
    ids = dict(id_to_semantic)
    for j in range(n, n_out):
        ids[int(_loader_id(j))] = id_to_semantic[int(_loader_id(int(parents[j])))]
    return out, ids


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
    """File pairing and item assembly shared by the two loaders; subclasses give the mask file and the instance map.
    `split_touching=SplitOptions(...)` (not in the reference; default off) parts connected components that are touching
    plants, see `semantic_to_instance_map`."""

    def __init__(self, image_folder_path, annotation_path, processor, label2id: dict, max_input_dim: int = 1024,
                 max_images=None, device="cuda", augment=None, generator=None, compact: bool = False, split_touching=None):
        self.image_folder = image_folder_path
        self.split_touching = split_touching  # a SplitOptions: components that are touching plants are parted (section 37)
        self.annotation_path = annotation_path
        self.processor = processor
        self.label2id = label2id
        self.max_input_dim = int(max_input_dim)
        self.device = torch.device(device)
        self.augment, self.generator = augment, generator  # a TrainAugmentation and its CPU torch.Generator, or None
        self.compact = bool(compact)  # items carry the processed id map instead of the mask stack
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
        return _assemble_item(self.processor, image, instance_map.cpu().numpy(), id_to_semantic, target_size, file_name,
                              self.augment, self.generator, self.compact)


def _assemble_item(processor, image, instance_map: np.ndarray, id_to_semantic: dict, target_size, file_name,
                   augment=None, generator=None, compact: bool = False) -> dict:
    """The item every reference loader returns: the processor's outputs for one image and its (H, W) int32 instance map
    (255 = ignore), with the map itself, the id dict, the target size and the file name.
    With `augment` (a TrainAugmentation) the parameters are drawn here for the loaded image from
    `generator`, `target_size` becomes the drawn window and the item also carries the parameters under "augment";
    `original_map` and `id_to_semantic` still describe the file.
    With `compact` the item carries `instance_map`, the processed (Hp, Wp) int32 id map on the device, and neither
    `mask_labels` nor `class_labels`: `collate_fn` and `expand_labels` take it as any compact sample, and `copy_paste`
    works on such batches.  `id_to_semantic` names its ids: the processing leaves ids as they are."""
    call, extra = {}, {}
    if augment is not None:
        params = augment.sample(instance_map.shape[0], instance_map.shape[1], generator)
        call = {"augment": params, "pad_size": augment.pad_size}
        extra = {"augment": params}
        target_size = params.window
    if compact:  # the stack the processor also builds is dropped below: keep it at a byte per pixel
        call["mask_dtype"] = torch.uint8
    inputs =processor(images=[image], segmentation_maps=[instance_map], instance_id_to_semantic_id=id_to_semantic,
                       return_tensors="pt", ignore_index=255, return_instance_maps=compact, **call)
    labels = ({"instance_map": inputs["instance_maps"][0]} if compact else
              {"mask_labels": inputs["mask_labels"][0], "class_labels": inputs["class_labels"][0]})
    return {
        **extra,
        "pixel_values": inputs["pixel_values"][0],
        **labels,
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
        return semantic_to_instance_map(mask, dsize, split=self.split_touching)


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
        return color_mask_to_instance_map(mask, self.color_map(), dsize, split=self.split_touching)


# ------------------------------------------------------------------------------------------- polygons
def _contour(pts, name: str) -> np.ndarray:
    a = np.asarray(pts)
    if a.ndim == 3 and a.shape[1] == 1:  # cv2's (N, 1, 2) contour layout
        a = a[:, 0, :]
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{name}: expected an (N, 2) array of x, y points, got shape {a.shape}")
    if a.shape[0] == 0:
        raise ValueError(f"{name}: a contour needs at least one point (cv2.fillPoly fails on an empty one)")
    if a.dtype.kind not in "iu":
        raise ValueError(f"{name}: expected integer points, got {a.dtype}")
    if int(np.abs(a.astype(np.int64)).max()) > _lib.WM2F_POLY_MAX_COORD:
        raise ValueError(f"{name}: coordinates must lie within +-{_lib.WM2F_POLY_MAX_COORD}")
    return a.astype(np.int64)


def _check_map(img, name: str) -> torch.Tensor:
    img = _require_cuda(img, name)
    if img.dim() != 2 or img.dtype != torch.int32 or not img.is_contiguous():
        raise TypeError(f"{name}: expected a contiguous (H, W) int32 map, got {tuple(img.shape)} {img.dtype}")
    if img.shape[0] <= 0 or img.shape[1] <= 0:
        raise ValueError(f"{name}: empty map {tuple(img.shape)}")
    return img


def _fill_calls(img: torch.Tensor, calls, values) -> torch.Tensor:
    """One fillPoly per entry of `calls` (a list of contour lists), in order, with the matching value."""
    verts, n_contours = [], []
    for k, contours in enumerate(calls):
        for j, pts in enumerate(contours):
            a = np.asarray(pts)
            if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] == 0 or a.dtype.kind not in "iu":
                a = _contour(pts, f"polygon {k}, contour {j}")  # the (N, 1, 2) layout, or raises with the reason
            verts.append(a)
        n_contours.append(len(contours))
    if not verts:
        v, c_off = np.zeros((0, 2), dtype=np.int64), np.zeros(1, dtype=np.int64)
    else:
        v = np.concatenate(verts).astype(np.int64, copy=False)
        if int(np.abs(v).max()) > _lib.WM2F_POLY_MAX_COORD:
            raise ValueError(f"coordinates must lie within +-{_lib.WM2F_POLY_MAX_COORD}")
        c_off = np.concatenate([[0], np.cumsum([len(a) for a in verts])])
    k_off = np.concatenate([[0], np.cumsum(n_contours, dtype=np.int64)])
    return ops.fill_polygons(img, v, c_off, k_off, np.asarray(values, dtype=np.int64))


def fill_poly(img: torch.Tensor, pts, color: int) -> torch.Tensor:
    """`cv2.fillPoly(img, pts, color)` with the reference's arguments (LINE_8, shift 0, no offset) on an (H, W) int32
    device map, in place; returns `img`.  `pts` is a list of (N, 2) integer x, y arrays; its contours share one edge
    table, so overlaps follow the even-odd rule (holes), as in cv2.  The outline is painted too, and points outside the
    map are clipped as OpenCV clips them."""
    img = _check_map(img, "img")
    if isinstance(pts, np.ndarray) and pts.ndim == 2:
        raise ValueError("pts: expected a list of (N, 2) contours, as cv2.fillPoly takes; got one (N, 2) array")
    return _fill_calls(img, [list(pts)], [int(color)])


def polygons_to_instance_map(polygons, ids, size, background: int = 255, device="cuda") -> torch.Tensor:
    """The instance map of the polygon loaders: an (H, W) int32 map of `background` with size = (H, W), then
    `cv2.fillPoly(map, [polygons[i]], ids[i])` for every i in order (later polygons overwrite earlier ones), as one
    chain of kernels.  Returns the map on the device."""
    h, w = int(size[0]), int(size[1])
    if h <= 0 or w <= 0:
        raise ValueError(f"size must be positive (H, W), got {size}")
    if len(polygons) != len(ids):
        raise ValueError(f"{len(polygons)} polygons but {len(ids)} ids")
    out = torch.full((h, w), int(background), dtype=torch.int32, device=device)
    _check_map(out, "map")
    return _fill_calls(out, [[p] for p in polygons], [int(i) for i in ids])


def rle_to_instance_map(rles, ids, size=None, background: int = 255, device="cuda") -> torch.Tensor:
    """`polygons_to_instance_map` for annotations stored as COCO RLE (crowd regions, exported datasets): an (H, W) int32
    map of `background`, then RLE i (compressed or plain counts) painted with ids[i] in order, later ones over earlier
    ones -- the caller numbers the ids as for polygons (1, 2, ..., skipping 255 where the loader does).  `size` = (H, W)
    must agree with the RLEs' own; without it theirs is taken.  Returns the map on the device."""
    from .rle import decode_rle
    rles = list(rles)
    if len(rles) != len(ids):
        raise ValueError(f"{len(rles)} RLEs but {len(ids)} ids")
    if size is not None:
        h, w = int(size[0]), int(size[1])
        if h <= 0 or w <= 0:
            raise ValueError(f"size must be positive (H, W), got {size}")
        for k, r in enumerate(rles):
            if tuple(int(v) for v in r["size"]) != (h, w):
                raise ValueError(f"RLE {k} has size {list(r['size'])}, the map {[h, w]}")
        if not rles:
            return torch.full((h, w), int(background), dtype=torch.int32, device=device)
    return decode_rle(rles, size=size, format="coco", values=[int(i) for i in ids], background=background, device=device)


# ---- host-side annotation parsing (the reference loaders' rules; no GPU involved)
def _via_polygons(entry: dict, label2id: dict, scale_x: float, scale_y: float, skip_255: bool):
    """The polygons of one VIA-JSON entry (Sorghum, inference.py's ground truth): 'polygon' shapes whose 'classname'
    is in label2id, in order, ids 1, 2, ... (255 skipped when skip_255), points scaled by int(v * scale) per axis.
    Returns (polygons, ids, id_to_semantic)."""
    polygons, ids, id_to_semantic = [], [], {}
    current = 1
    for region in entry.get("regions", []):
        shape_attr = region["shape_attributes"]
        region_attr = region["region_attributes"]
        if shape_attr["name"] != "polygon":
            continue
        class_name = region_attr.get("classname", None)
        if class_name not in label2id:
            continue
        if skip_255 and current == 255:
            current += 1
        xs = [int(x * scale_x) for x in shape_attr["all_points_x"]]
        ys = [int(y * scale_y) for y in shape_attr["all_points_y"]]
        polygons.append(np.array(list(zip(xs, ys)), dtype=np.int64).reshape(-1, 2))
        ids.append(current)
        id_to_semantic[current] = label2id[class_name]
        current += 1
    return polygons, ids, id_to_semantic


def _cwfid_polygons(annotation: dict, label2id: dict, scale: float):
    """The polygons of one CWFID YAML file: regions whose 'type' is in label2id, ids 1, 2, ... with 255 skipped.  A
    float pair becomes a one-point list; other scalars, length mismatches and fewer than 3 points skip the region
    (the id is not consumed).  Returns (polygons, ids, id_to_semantic)."""
    polygons, ids, id_to_semantic = [], [], {}
    current = 1
    regions = annotation.get("annotation", []) or []
    for region in regions:
        type_name = region.get("type")
        if type_name not in label2id:
            continue
        if current == 255:
            current += 1
        points = region.get("points", {})
        xs, ys = points.get("x", []), points.get("y", [])
        if not isinstance(xs, list) or not isinstance(ys, list):
            if isinstance(xs, float) and isinstance(ys, float):
                xs, ys = [xs], [ys]
            else:
                print("skipping region with invalid points format (not lists)")
                print(f"xs: {xs}\n ys: {ys}")
                continue
        if len(xs) != len(ys) or len(xs) < 3:
            continue
        polygons.append(np.array([[int(x * scale), int(y * scale)] for x, y in zip(xs, ys)], dtype=np.int64))
        ids.append(current)
        id_to_semantic[current] = label2id[type_name]
        current += 1
    return polygons, ids, id_to_semantic


def _open_scaled(image_path: str, max_input_dim: int):
    """The image as the reference loaders read it: RGB, resized with PIL BILINEAR to int(side * s), s = max_input_dim /
    max(w, h), when larger than max_input_dim.  Returns (image, scale_factor)."""
    from PIL import Image
    image = Image.open(image_path).convert("RGB")
    width, height = image.size
    scale_factor = 1.0
    if max(width, height) > max_input_dim:
        scale_factor = max_input_dim / max(width, height)
        image = image.resize(size=(int(width * scale_factor), int(height * scale_factor)), resample=Image.BILINEAR)
    return image, scale_factor


class SorghumWeedDataset(torch.utils.data.Dataset):
    """datasets/sorghum_weed/dataset.py:SorghumWeedDataset with the instance map painted on the GPU.  `annotation_path`
    is a VIA JSON file; entries are kept when their image exists in `image_folder_path` and they have regions.
    `max_input_dim` and `max_images` stand for config.MAX_INPUT_DIM and config.MAX_IMAGES."""

    def __init__(self, image_folder_path, annotation_path, processor, label2id: dict, max_input_dim: int = 1024,
                 max_images=None, device="cuda", augment=None, generator=None, compact: bool = False):
        import json
        self.image_folder = image_folder_path
        self.processor = processor
        self.label2id = label2id
        self.max_input_dim = int(max_input_dim)
        self.device = torch.device(device)
        self.augment, self.generator = augment, generator  # a TrainAugmentation and its CPU torch.Generator, or None
        self.compact = bool(compact)  # items carry the processed id map instead of the mask stack
        with open(annotation_path, "r") as f:
            self.data = list(json.load(f).values())
        self.valid_entries = []
        for entry in self.data:
            if os.path.exists(os.path.join(self.image_folder, entry["filename"])) and len(entry.get("regions", [])) > 0:
                self.valid_entries.append(entry)
                if max_images is not None and len(self.valid_entries) >= max_images:
                    break
        print(f'\t\tLoaded {len(self.valid_entries)} valid images from "{annotation_path}"')

    def __len__(self):
        return len(self.valid_entries)

    def __getitem__(self, idx: int) -> dict:
        entry = self.valid_entries[idx]
        image, scale = _open_scaled(os.path.join(self.image_folder, entry["filename"]), self.max_input_dim)
        width, height = image.size
        polygons, ids, id_to_semantic = _via_polygons(entry, self.label2id, scale, scale, skip_255=True)
        instance_map = polygons_to_instance_map(polygons, ids, (height, width), 255, self.device).cpu().numpy()
        return _assemble_item(self.processor, image, instance_map, id_to_semantic, (height, width), entry["filename"],
                              self.augment, self.generator, self.compact)


class CropWeedYamlDataset(torch.utils.data.Dataset):
    """The CWFID YAML loader (dataset_from_yaml_annotations.py:CropWeedDataset) with the instance map painted on the
    GPU.  `annotation_path` is a folder of `*.yaml` files (sorted); each names its image with the 'filename' key."""

    def __init__(self, image_folder_path, annotation_path, processor, label2id: dict, max_input_dim: int = 1024,
                 max_images=None, device="cuda", augment=None, generator=None, compact: bool = False):
        import yaml
        self.image_folder = image_folder_path
        self.annotation_path = annotation_path
        self.processor = processor
        self.label2id = label2id
        self.max_input_dim = int(max_input_dim)
        self.device = torch.device(device)
        self.augment, self.generator = augment, generator  # a TrainAugmentation and its CPU torch.Generator, or None
        self.compact = bool(compact)  # items carry the processed id map instead of the mask stack
        yaml_files = sorted(glob.glob(os.path.join(self.annotation_path, "*.yaml")))
        self.valid_files = []
        print(f'Scanning {len(yaml_files)} annotation files in "{self.annotation_path}"...')
        for yaml_path in yaml_files:
            try:
                with open(yaml_path, "r") as f:
                    data = yaml.safe_load(f)
                if not data:
                    continue
                img_filename = data.get("filename")
                if not img_filename:
                    continue
                img_path = os.path.join(self.image_folder, img_filename)
                if os.path.exists(img_path):
                    self.valid_files.append((img_path, yaml_path))
                    if max_images is not None and len(self.valid_files) >= max_images:
                        break
            except Exception as e:
                print(f'Warning: Error reading "{yaml_path}":\n\t {e}')
        print(f'\tLoaded {len(self.valid_files)} valid image/yaml pairs from "{self.image_folder}"')

    def __len__(self):
        return len(self.valid_files)

    def __getitem__(self, idx: int) -> dict:
        import yaml
        image_path, yaml_path = self.valid_files[idx]
        image, scale = _open_scaled(image_path, self.max_input_dim)
        with open(yaml_path, "r") as f:
            annotation = yaml.safe_load(f)
        width, height = image.size
        polygons, ids, id_to_semantic = _cwfid_polygons(annotation, self.label2id, scale)
        instance_map = polygons_to_instance_map(polygons, ids, (height, width), 255, self.device).cpu().numpy()
        return _assemble_item(self.processor, image, instance_map, id_to_semantic, (height, width),
                              os.path.basename(image_path), self.augment, self.generator, self.compact)


def load_ground_truth(image_name: str, target_size: tuple, annotation_file: str, img_dir: str, label2id: dict,
                      device="cuda"):
    """models/mask2former/inference.py:load_ground_truth with the map painted on the GPU.  target_size = (W, H); points
    scale by target / original size per axis (1:1 when the image is missing); zero background, ids 1, 2, ... (no 255
    skip).  Returns {'segmentation': (H, W) int32 CPU tensor, 'segments_info': [{'id', 'label_id', 'score'}]}, or None
    where the reference prints a message and returns None."""
    import json
    if not os.path.exists(annotation_file):
        print(f"Annotation file not found: {annotation_file}")
        return None
    try:
        with open(annotation_file, "r") as f:
            data = json.load(f)
    except Exception as e:
        print(f"Error loading JSON: {e}")
        return None
    entry = next((item for item in data.values() if item["filename"] == image_name), None)
    if not entry:
        print(f'No annotation found for "{image_name}"')
        return None
    image_path = os.path.join(img_dir, image_name)
    if os.path.exists(image_path):
        from PIL import Image
        with Image.open(image_path) as orig_img:
            orig_w, orig_h = orig_img.size
    else:
        print("Warning: Original image file not found. Assuming 1:1 scale.")
        orig_w, orig_h = target_size
    target_w, target_h = target_size
    polygons, ids, id_to_semantic = _via_polygons(entry, label2id, target_w / orig_w, target_h / orig_h,
                                                  skip_255=False)
    segmentation = polygons_to_instance_map(polygons, ids, (target_h, target_w), 0, device).cpu()
    segments_info = [{"id": i, "label_id": id_to_semantic[i], "score": 1.0} for i in ids]
    return {"segmentation": segmentation, "segments_info": segments_info}
