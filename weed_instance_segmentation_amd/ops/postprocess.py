"""Instance, semantic and panoptic post-processing on the 384 x 384 grid."""
from __future__ import annotations

import torch

from ._core import _launch, _p, _req


_GRID = (384, 384)  # the dependency's hard-coded intermediate size (image_processing_mask2former.py:680-682)


def instance_scores(mask_logits: torch.Tensor, qidx: torch.Tensor):
    """(sum of sigmoid over set pixels, number of set pixels) of each selected query's mask on the 384 x 384 grid."""
    mask_logits, qidx = _req(mask_logits, "mask_logits"), _req(qidx, "qidx", torch.int32)
    B, Q, h, w = mask_logits.shape
    K = qidx.shape[1]
    s = torch.empty(B, K, device=mask_logits.device, dtype=torch.float32)
    c = torch.empty_like(s)
    _launch("wm2f_instance_scores", mask_logits, _p(mask_logits), _p(qidx), _p(s), _p(c), B, Q, K, h, w, _GRID[0], _GRID[1])
    return s, c


def instance_any(mask_logits, qidx, cand, size):
    mask_logits, qidx, cand = _req(mask_logits, "mask_logits"), _req(qidx, "qidx", torch.int32), _req(cand, "cand", torch.uint8)
    B, Q, h, w = mask_logits.shape
    K = qidx.shape[1]
    out = torch.empty(B, K, device=mask_logits.device, dtype=torch.int32)
    _launch("wm2f_instance_any", mask_logits, _p(mask_logits), _p(qidx), _p(cand), _p(out), B, Q, K, h, w, _GRID[0], _GRID[1],
            int(size[0]), int(size[1]))
    return out


def instance_segmentation(mask_logits, kept_q, n_kept, size):
    mask_logits = _req(mask_logits, "mask_logits")
    kept_q, n_kept = _req(kept_q, "kept_q", torch.int32), _req(n_kept, "n_kept", torch.int32)
    B, Q, h, w = mask_logits.shape
    K = kept_q.shape[1]
    seg = torch.empty(B, int(size[0]), int(size[1]), device=mask_logits.device, dtype=torch.float32)
    _launch("wm2f_instance_segmentation", mask_logits, _p(mask_logits), _p(kept_q), _p(n_kept), _p(seg), B, Q, K, h, w, _GRID[0],
            _GRID[1], int(size[0]), int(size[1]))
    return seg


def instance_maps(image_logits, kept_q, n, size):
    image_logits, kept_q = _req(image_logits, "image_logits"), _req(kept_q, "kept_q", torch.int32)
    Q, h, w = image_logits.shape
    maps = torch.empty(n, int(size[0]), int(size[1]), device=image_logits.device, dtype=torch.float32)
    _launch("wm2f_instance_maps", image_logits, _p(image_logits), _p(kept_q), int(n), _p(maps), h, w, _GRID[0], _GRID[1],
            int(size[0]), int(size[1]))
    return maps


# ------------------------------------------------------ semantic and panoptic post-processing
def semantic_scores(mask_logits: torch.Tensor, class_probs: torch.Tensor) -> torch.Tensor:
    """einsum("bqc,bqhw->bchw", class_probs, sigmoid(bilinear_384(mask_logits))): (B, C, 384, 384) fp32."""
    mask_logits, class_probs = _req(mask_logits, "mask_logits"), _req(class_probs, "class_probs")
    B, Q, h, w = mask_logits.shape
    C = class_probs.shape[-1]
    if class_probs.shape != (B, Q, C):
        raise ValueError(f"semantic_scores: class_probs {tuple(class_probs.shape)} does not match logits {tuple(mask_logits.shape)}")
    S = torch.empty(B, C, _GRID[0], _GRID[1], device=mask_logits.device, dtype=torch.float32)
    _launch("wm2f_semantic_scores", S, _p(mask_logits), _p(class_probs), _p(S), B, Q, C, h, w, _GRID[0], _GRID[1],
            tag="semantic_scores")
    return S


def semantic_resize_argmax(scores: torch.Tensor, rows: torch.Tensor, size, want_scores: bool = False):
    """Bilinear resize of scores[rows] (B, C, gh, gw) to `size`, first-max argmax over C: ((n, H, W) int64,
    (n, C, H, W) fp32 resized scores or None)."""
    scores, rows = _req(scores, "scores"), _req(rows, "rows", torch.int32)
    _, C, gh, gw = scores.shape
    n, H, W = rows.numel(), int(size[0]), int(size[1])
    seg = torch.empty(n, H, W, device=scores.device, dtype=torch.int64)
    out = torch.empty(n, C, H, W, device=scores.device, dtype=torch.float32) if want_scores else None
    _launch("wm2f_semantic_resize_argmax", seg, _p(scores), _p(rows), n, _p(seg), _p(out), C, gh, gw, H, W,
            tag="semantic_resize_argmax")
    return seg, out


def panoptic_probs(mask_logits: torch.Tensor, kept_q: torch.Tensor, n_kept: torch.Tensor) -> torch.Tensor:
    """sigmoid(bilinear_384(mask_logits[b, kept_q[b, k]])) for k < n_kept[b]: (B, K, 384, 384) fp32 (slots past
    n_kept[b] are left unwritten)."""
    mask_logits = _req(mask_logits, "mask_logits")
    kept_q, n_kept = _req(kept_q, "kept_q", torch.int32), _req(n_kept, "n_kept", torch.int32)
    B, Q, h, w = mask_logits.shape
    K = kept_q.shape[1]
    G = torch.empty(B, K, _GRID[0], _GRID[1], device=mask_logits.device, dtype=torch.float32)
    _launch("wm2f_panoptic_probs", G, _p(mask_logits), _p(kept_q), _p(n_kept), _p(G), B, Q, K, h, w, _GRID[0], _GRID[1],
            tag="panoptic_probs")
    return G


def panoptic_segments(probs: torch.Tensor, rows: torch.Tensor, n_kept: torch.Tensor, scores: torch.Tensor, counts: torch.Tensor,
                      size, mask_threshold: float) -> torch.Tensor:
    """Argmax over the kept queries of bilinear(probs[b, k]) * scores[b, k] at `size` for the images `rows`:
    (n, H, W) int32 query indices.  Adds into counts (B, K, 2) int32 the pixels at or above mask_threshold and the
    pixels each query owns."""
    probs, rows = _req(probs, "probs"), _req(rows, "rows", torch.int32)
    n_kept, scores = _req(n_kept, "n_kept", torch.int32), _req(scores, "scores")
    counts = _req(counts, "counts", torch.int32)
    B, K, gh, gw = probs.shape
    if scores.shape != (B, K) or counts.shape != (B, K, 2) or n_kept.shape != (B,):
        raise ValueError("panoptic_segments: scores (B, K), counts (B, K, 2) and n_kept (B,) must match probs (B, K, h, w)")
    n, H, W = rows.numel(), int(size[0]), int(size[1])
    seg = torch.empty(n, H, W, device=probs.device, dtype=torch.int32)
    _launch("wm2f_panoptic_segments", seg, _p(probs), _p(rows), _p(n_kept), _p(scores), _p(seg), _p(counts), n, K, gh, gw, H, W,
            float(mask_threshold), tag="panoptic_segments")
    return seg


def panoptic_relabel_(seg: torch.Tensor, rows: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """seg[j] = table[rows[j]][seg[j]] in place (seg (n, H, W) int32 query indices, table (B, K) int32 segment ids)."""
    seg, rows, table = _req(seg, "seg", torch.int32), _req(rows, "rows", torch.int32), _req(table, "table", torch.int32)
    n = rows.numel()
    if seg.shape[0] != n:
        raise ValueError("panoptic_relabel_: one map per row")
    _launch("wm2f_panoptic_relabel", seg, _p(seg), _p(rows), _p(table), n, int(table.shape[1]), seg[0].numel(),
            tag="panoptic_relabel")
    return seg
