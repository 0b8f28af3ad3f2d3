"""K4: the matcher's cost matrices and the batched linear sum assignment."""
from __future__ import annotations

import torch

from .._lib import host_i32, load
from ._core import _f32, _launch, _p, _ptr_table, _req


def matcher_cost(mask_logits, class_logits, tgt_masks, tgt_counts, tgt_classes, points, w_class, w_mask, w_dice):
    """K4 -- all cost matrices of a step in one go (HF:444-472), no sync.

    mask_logits (NL,B,Q,h,w) or a list of NL (B,Q,h,w) tensors (not stacked); class_logits (NL,B,Q,C1); tgt_masks (sum T, Ht, Wt) fp32 or uint8;
    tgt_counts: python list of T_i; tgt_classes (sum T,) int64; points (NL,B,P,2).
    Returns cost (NL,B,Q,Tmax) fp32 on the device; columns >= T_i are zero."""
    class_logits, points = _req(_f32(class_logits), "class_logits"), _req(_f32(points), "points")
    levels = None
    if isinstance(mask_logits, (list, tuple)):  # one (B,Q,h,w) tensor per level, used where it is
        levels = [_req(_f32(m), "mask level") for m in mask_logits]
        mask_logits = levels[0]
        NL, (B, Q, h, w) = len(levels), mask_logits.shape
        if any(m.shape != mask_logits.shape for m in levels):
            raise ValueError("matcher_cost: level tensors of different shapes")
    else:
        mask_logits = _req(_f32(mask_logits), "mask_logits")
        NL, B, Q, h, w = mask_logits.shape
    C1 = class_logits.shape[-1]
    P = points.shape[2]
    if tgt_masks.dtype == torch.bool:
        tgt_masks = tgt_masks.view(torch.uint8)
    tdt = 1 if tgt_masks.dtype == torch.uint8 else 0
    tgt_masks = _req(tgt_masks, "tgt_masks", torch.uint8 if tdt else torch.float32)
    tgt_classes = _req(tgt_classes, "tgt_classes", torch.int64)
    offs = [0]
    for t in tgt_counts:
        offs.append(offs[-1] + int(t))
    Tsum, Tmax = offs[-1], max([int(t) for t in tgt_counts] + [1])
    if tgt_masks.shape[0] != Tsum or tgt_classes.shape[0] != Tsum or len(tgt_counts) != B:
        raise ValueError("matcher_cost: target counts disagree with the target tensors")
    Ht, Wt = tgt_masks.shape[-2:]
    cost = torch.zeros(NL, B, Q, Tmax, device=mask_logits.device, dtype=torch.float32)
    ws = torch.empty(max(int(load().wm2f_matcher_workspace(NL, B, Q, P, Tsum)), 4), device=mask_logits.device, dtype=torch.uint8)
    if levels is not None:
        _launch("wm2f_matcher_cost_levels", mask_logits, _ptr_table(levels), _p(class_logits), _p(tgt_masks), tdt, host_i32(offs),
                _p(tgt_classes), _p(points), _p(cost), _p(ws), NL, B, Q, C1, h, w, Ht, Wt, P, Tmax, float(w_class), float(w_mask),
                float(w_dice), tag="matcher_cost")
    else:
        _launch("wm2f_matcher_cost", mask_logits, _p(mask_logits), _p(class_logits), _p(tgt_masks), tdt, host_i32(offs),
                _p(tgt_classes), _p(points), _p(cost), _p(ws), NL, B, Q, C1, h, w, Ht, Wt, P, Tmax, float(w_class), float(w_mask),
                float(w_dice), tag="matcher_cost")
    return cost


def lsa_batched(cost: torch.Tensor, counts: torch.Tensor, t_cap: int):
    """Linear sum assignment of every (level, image) cost matrix on the device (HF:474 without the host round trip).
    cost (NL, B, Q, Tmax) fp32; counts (B) int32 on the device = targets per image.  Returns rows, cols (NL, B, t_cap) int32:
    the min(Q, T_b) matched (query, target) pairs per problem sorted by query, bit-identical to scipy's
    linear_sum_assignment(cost[l, b, :, :T_b]); entries beyond min(Q, T_b) are unspecified."""
    cost = _req(cost, "cost")
    counts = _req(counts, "counts", torch.int32)
    NL, B, Q, Tmax = cost.shape
    rows = torch.empty(NL, B, t_cap, device=cost.device, dtype=torch.int32)
    cols = torch.empty_like(rows)
    _launch("wm2f_lsa_batched", cost, _p(cost), _p(counts), _p(rows), _p(cols), NL * B, B, Q, Tmax, int(t_cap), tag="lsa_batched")
    return rows, cols
