"""The loss kernels: point sampling, top-point selection and the per-mask BCE / dice rows."""
from __future__ import annotations

import torch

from .. import _lib
from ._core import _amp_bwd, _amp_fwd, _launch, _p, _ptr_table, _req


class _PointSample(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, feat, pts, map_index):
        tdt = 1 if feat.dtype in (torch.uint8, torch.bool) else 0
        if feat.dtype == torch.bool:
            feat = feat.view(torch.uint8)
        feat = _req(feat, "feat", torch.uint8 if tdt else torch.float32)
        pts = _req(pts, "pts")
        N, H, W = feat.shape
        M, P = pts.shape[:2]
        if pts.dim() != 3 or pts.shape[2] != 2:
            raise ValueError(f"point_sample: pts {tuple(pts.shape)}")
        if map_index is None:
            if M != N:
                raise ValueError(f"point_sample: {M} point rows for {N} maps and no map_index")
        else:
            map_index = _req(map_index, "map_index", torch.int32)
            if map_index.shape != (M,):
                raise ValueError(f"point_sample: map_index {tuple(map_index.shape)} != ({M},)")
        out = torch.empty(M, P, device=feat.device, dtype=torch.float32)
        _launch("wm2f_point_sample_fwd", feat, _p(feat), tdt, _p(pts), _p(map_index), _p(out), M, H, W, P)
        ctx.save_for_backward(pts, map_index)
        ctx.shape = (N, H, W)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, grad_out):
        pts, map_index = ctx.saved_tensors
        N, H, W = ctx.shape
        grad_out = _req(grad_out, "grad_out")
        g = torch.zeros(N, H, W, device=pts.device, dtype=torch.float32)
        _launch("wm2f_point_sample_bwd", pts, _p(grad_out), _p(pts), _p(map_index), _p(g), pts.shape[0], H, W, pts.shape[1])
        return g, None, None


def point_sample(feat: torch.Tensor, pts: torch.Tensor, map_index: torch.Tensor | None = None) -> torch.Tensor:
    """sample_point (HF:245-274) for single-channel maps: feat (N,H,W), pts (M,P,2) in [0,1] (x,y) -> (M,P).
    Row m samples feat[map_index[m]] (int32) -- or feat[m] when map_index is None."""
    return _PointSample.apply(feat, pts, map_index)


class _PointSampleLevels(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, pts, index, neg_abs, unique, *maps):
        maps = [_req(m, "level map") for m in maps]
        pts, index = _req(pts, "pts"), _req(index, "index", torch.int32)
        NL, M, P = pts.shape[:3]
        N, H, W = maps[0].shape
        if len(maps) != NL or index.shape != (NL, M) or any(m.shape != (N, H, W) for m in maps):
            raise ValueError("point_sample_levels: one (N,H,W) map per level, pts (NL,M,P,2), index (NL,M)")
        out = torch.empty(NL, M, P, device=pts.device, dtype=torch.float32)
        _launch("wm2f_point_sample_levels_fwd", pts, _ptr_table(maps), NL, _p(pts), _p(index), _p(out), M, H, W, P,
                1 if neg_abs else 0, tag="point_sample_levels_fwd")
        ctx.save_for_backward(pts, index)
        ctx.shape = (NL, N, H, W)
        ctx.unique = bool(unique) and W <= 16384
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, grad_out):
        pts, index = ctx.saved_tensors
        NL, N, H, W = ctx.shape
        grad_out = _req(grad_out, "grad_out")
        grads = [torch.zeros(N, H, W, device=pts.device, dtype=torch.float32) for _ in range(NL)]
        _launch("wm2f_point_sample_levels_bwd_unique" if ctx.unique else "wm2f_point_sample_levels_bwd", pts, _p(grad_out), _p(pts),
                _p(index), _ptr_table(grads), NL, pts.shape[1], H, W, pts.shape[2], tag="point_sample_levels_bwd",
                what="wm2f_point_sample_levels_bwd")
        return (None, None, None, None, *grads)


def select_top_points(score: torch.Tensor, pts: torch.Tensor, k: int, out_points: int | None = None) -> torch.Tensor:
    """The points of the k largest scores of each row (HF:688-704: `gather(coords, topk(uncertainty, k)[1])`), without the sort
    a stock top-k of thousands is: score (R, n) fp32, pts (R, n, 2) -> (R, out_points or k, 2) whose first k entries are the
    selected points in INDEX order (the losses sum over points: only the set matters; equal scores at the threshold: lowest
    indices first; NaN ranks highest).  Entries k.. are left for the caller (the random points of HF:700-703).  No autograd."""
    score, pts = _req(score, "score"), _req(pts, "pts")
    R, n = score.shape
    if pts.shape != (R, n, 2) or not 0 < k <= n:
        raise ValueError(f"select_top_points: score {tuple(score.shape)} pts {tuple(pts.shape)} k {k}")
    P = int(out_points) if out_points is not None else int(k)
    out = torch.empty(R, P, 2, device=score.device, dtype=torch.float32)
    rc = _launch("wm2f_select_top_points", score, _p(score), _p(pts), _p(out), R, n, int(k), P, tag="select_top_points", raw=True)
    if rc == _lib.WM2F_EUNSUPPORTED:  # more candidates per row than LDS holds: the stock sort
        idx = torch.sort(torch.topk(score, k=k, dim=1)[1], dim=1)[0]  # index order, as the kernel writes them
        out[:, :k] = torch.gather(pts, 1, idx[..., None].expand(-1, -1, 2))
    return out


def point_sample_levels(maps, pts: torch.Tensor, index: torch.Tensor, neg_abs: bool = False, unique_index: bool = False) -> torch.Tensor:
    """sample_point (HF:245-274) on one (N,H,W) map tensor PER LEVEL without stacking them: pts (NL,M,P,2) in [0,1]
    (x,y), index (NL,M) int32 = which map of its level row m samples -> (NL,M,P).  neg_abs: -|value| (HF:688-690).
    unique_index: the caller guarantees that no map is indexed twice within a level (the matched rows of a one-to-one
    assignment) -- the backward then accumulates each map in LDS bands and stores it, without global atomics."""
    return _PointSampleLevels.apply(pts, index, bool(neg_abs), bool(unique_index), *maps)


class _MaskLossRows(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, logits, labels):
        logits, labels = _req(logits, "logits"), _req(labels, "labels")
        R, P = logits.shape
        sums = torch.empty(R, 4, device=logits.device, dtype=torch.float32)
        bce, dice = torch.empty(R, device=logits.device), torch.empty(R, device=logits.device)
        _launch("wm2f_mask_loss_rows_fwd", logits, _p(logits), _p(labels), _p(sums), _p(bce), _p(dice), R, P,
                tag="mask_loss_rows_fwd")
        ctx.save_for_backward(logits, labels, sums)
        return bce, dice

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_bce, g_dice):
        logits, labels, sums = ctx.saved_tensors
        R, P = logits.shape
        g_bce, g_dice = _req(g_bce, "g_bce"), _req(g_dice, "g_dice")
        grad = torch.empty_like(logits)
        _launch("wm2f_mask_loss_rows_bwd", logits, _p(logits), _p(labels), _p(sums), _p(g_bce), _p(g_dice), _p(grad), R, P,
                tag="mask_loss_rows_bwd")
        return grad, None


def mask_loss_rows(logits: torch.Tensor, labels: torch.Tensor):
    """Per matched mask (row): (mean BCE-with-logits over its points HF:308-324, dice HF:278-305), differentiable in logits."""
    return _MaskLossRows.apply(logits, labels)
