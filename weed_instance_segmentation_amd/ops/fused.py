"""Fused inference passes over NCHW maps and token matrices (no autograd)."""
from __future__ import annotations

from typing import Sequence

import torch

from ._core import _launch, _p, _req


def bias_act_(x: torch.Tensor, bias: torch.Tensor, residual: torch.Tensor | None = None, relu: bool = True):
    """In place: x <- act(x + bias[c] (+ residual)) for an NCHW tensor (inference, no autograd)."""
    if not x.is_contiguous():
        raise ValueError("bias_act_: x must be NCHW-contiguous")
    _req(x, "x"), _req(bias, "bias")
    N, C, H, W = x.shape
    if residual is not None:
        residual = _req(residual, "residual")
        if residual.shape != x.shape:
            raise ValueError("bias_act_: residual shape")
    _launch("wm2f_bias_act", x, _p(x), _p(bias), _p(residual), _p(x), N, C, H * W, 1 if relu else 0)
    return x


def add_broadcast(a: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    """a (B, ...) + p (1, ...) -- the same trailing shape, broadcast over the batch (a level's positional embedding added to its
    tokens, HF `with_pos_embed`).  Inference only (no autograd); fp32, element count of a row a multiple of 4."""
    a, p = _req(a, "a"), _req(p, "p")
    if p.shape[0] != 1 or p.shape[1:] != a.shape[1:] or (a.numel() // a.shape[0]) % 4:
        raise ValueError(f"add_broadcast: a {tuple(a.shape)} p {tuple(p.shape)}")
    out = torch.empty_like(a)
    _launch("wm2f_add_broadcast", a, _p(a), _p(p), _p(out), int(a.shape[0]), int(a.numel() // a.shape[0]))
    return out


def tokens_to_nchw(tokens: torch.Tensor, start: int, h: int, w: int) -> torch.Tensor:
    """tokens (B, S, C) rows [start, start + h*w) -> (B, C, h, w), tiled transpose (inference only, no autograd)."""
    tokens = _req(tokens, "tokens")
    B, S, C = tokens.shape
    out = torch.empty(B, C, h, w, device=tokens.device, dtype=torch.float32)
    _launch("wm2f_tokens_to_nchw", tokens, _p(tokens), _p(out), B, S, C, int(start), h * w)
    return out


def group_norm_tokens_(x: torch.Tensor, bias: torch.Tensor | None, groups: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                       tokens: torch.Tensor, start: int) -> torch.Tensor:
    """tokens[:, start:start+H*W, :] <- GroupNorm(x + bias) in token layout, for x (B, C, H, W) and tokens (B, S, C)
    (inference, no autograd): one level's input projection of the pixel decoder, HF:1341-1357."""
    if not x.is_contiguous() or not tokens.is_contiguous():
        raise ValueError("group_norm_tokens_: x and tokens must be contiguous")
    _req(x, "x"), _req(tokens, "tokens")
    gamma, beta = _req(gamma, "gamma"), _req(beta, "beta")
    if bias is not None:
        bias = _req(bias, "bias")
    B, C, H, W = x.shape
    if tokens.dim() != 3 or tokens.shape[0] != B or tokens.shape[2] != C:
        raise ValueError("group_norm_tokens_: tokens must be (B, S, C)")
    ws = torch.empty(2 * B * groups, device=x.device, dtype=torch.float64)
    _launch("wm2f_group_norm_tokens", x, _p(x), _p(bias), _p(gamma), _p(beta), _p(tokens), _p(ws), B, C, int(groups), H * W,
            int(tokens.shape[1]), int(start), float(eps))
    return tokens


def group_norm_tokens_from_stats_(x: torch.Tensor, stats: torch.Tensor, bias: torch.Tensor | None, groups: int, gamma: torch.Tensor,
                                  beta: torch.Tensor, eps: float, tokens: torch.Tensor, start: int) -> torch.Tensor:
    """group_norm_tokens_ from a filled statistics workspace `stats` (B, groups, 2) fp64 = (sum, sum of squares) of x + bias
    per image and group (a convolution epilogue wrote it: conv1x1_gn): no statistics pass."""
    if not x.is_contiguous() or not tokens.is_contiguous():
        raise ValueError("group_norm_tokens_from_stats_: x and tokens must be contiguous")
    _req(x, "x"), _req(tokens, "tokens")
    gamma, beta, stats = _req(gamma, "gamma"), _req(beta, "beta"), _req(stats, "stats", torch.float64)
    if bias is not None:
        bias = _req(bias, "bias")
    B, C, H, W = x.shape
    if tokens.dim() != 3 or tokens.shape[0] != B or tokens.shape[2] != C:
        raise ValueError("group_norm_tokens_from_stats_: tokens must be (B, S, C)")
    if stats.numel() != 2 * B * int(groups):
        raise ValueError("group_norm_tokens_from_stats_: stats must be (B, groups, 2)")
    _launch("wm2f_group_norm_tokens_apply", x, _p(x), _p(bias), _p(gamma), _p(beta), _p(tokens), _p(stats), B, C, int(groups),
            H * W, int(tokens.shape[1]), int(start), float(eps))
    return tokens


def group_norm_act_from_stats_(x: torch.Tensor, stats: torch.Tensor, groups: int, gamma: torch.Tensor, beta: torch.Tensor,
                               eps: float, up: torch.Tensor | None = None, relu: bool = False) -> torch.Tensor:
    """group_norm_act_ from a filled statistics workspace `stats` (B, groups, 2) fp64 = (sum, sum of squares) of x per image
    and group (a convolution epilogue wrote it: conv1x1_gn, conv3x3_stats): no statistics pass."""
    if not x.is_contiguous():
        raise ValueError("group_norm_act_from_stats_: x must be NCHW-contiguous")
    _req(x, "x")
    gamma, beta, stats = _req(gamma, "gamma"), _req(beta, "beta"), _req(stats, "stats", torch.float64)
    B, C, H, W = x.shape
    if stats.numel() != 2 * B * int(groups):
        raise ValueError("group_norm_act_from_stats_: stats must be (B, groups, 2)")
    Hs = Ws = 0
    if up is not None:
        up = _req(up, "up")
        if up.dim() != 4 or up.shape[:2] != x.shape[:2]:
            raise ValueError("group_norm_act_from_stats_: up must be (B, C, Hs, Ws)")
        Hs, Ws = int(up.shape[2]), int(up.shape[3])
    _launch("wm2f_group_norm_act_apply", x, _p(x), _p(gamma), _p(beta), _p(up), _p(x), _p(stats), B, C, int(groups), H, W, Hs,
            Ws, float(eps), 1 if relu else 0)
    return x


def resize_bilinear(x: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    """F.interpolate(x, size=size, mode="bilinear", align_corners=False) for an NCHW fp32 map (inference, no autograd)."""
    if not x.is_contiguous():
        raise ValueError("resize_bilinear: x must be NCHW-contiguous")
    _req(x, "x")
    N, C, H, W = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    y = torch.empty(N, C, Ho, Wo, device=x.device, dtype=torch.float32)
    _launch("wm2f_resize_bilinear", x, _p(x), _p(y), N * C, H, W, Ho, Wo)
    return y


def resize_pyramid(x: torch.Tensor):
    """(half, quarter, eighth)-size bilinear resizes of an NCHW fp32 map in ONE pass (H, W divisible by 8): bit for bit
    `resize_bilinear(x, (H/2, W/2))`, `(H/4, W/4)`, `(H/8, W/8)`.  Inference, no autograd."""
    if not x.is_contiguous():
        raise ValueError("resize_pyramid: x must be NCHW-contiguous")
    _req(x, "x")
    N, C, H, W = x.shape
    if H % 8 or W % 8:
        raise ValueError("resize_pyramid: H and W must be divisible by 8")
    ys = [torch.empty(N, C, H >> k, W >> k, device=x.device, dtype=torch.float32) for k in (1, 2, 3)]
    _launch("wm2f_resize_pyramid", x, _p(x), _p(ys[0]), _p(ys[1]), _p(ys[2]), N * C, H, W, tag="resize_pyramid")
    return ys


def bias_relu_maxpool(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """MaxPool2d(3, 2, 1)(ReLU(x + bias[c])) of an NCHW map in one pass (inference, no autograd): the ResNet stem tail."""
    if not x.is_contiguous():
        raise ValueError("bias_relu_maxpool: x must be NCHW-contiguous")
    _req(x, "x"), _req(bias, "bias")
    N, C, H, W = x.shape
    y = torch.empty(N, C, H // 2, W // 2, device=x.device, dtype=torch.float32)
    _launch("wm2f_bias_relu_maxpool", x, _p(x), _p(bias), _p(y), N, C, H, W)
    return y


def group_norm_act_(x: torch.Tensor, groups: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                    up: torch.Tensor | None = None, relu: bool = False) -> torch.Tensor:
    """In place: x <- act(GroupNorm(x) (+ bilinear upsample of `up` to x's size, align_corners=False)) for an NCHW map
    (inference, no autograd) -- the GroupNorm tails of the FPN step, HF:1395-1405."""
    if not x.is_contiguous():
        raise ValueError("group_norm_act_: x must be NCHW-contiguous")
    _req(x, "x")
    gamma, beta = _req(gamma, "gamma"), _req(beta, "beta")
    B, C, H, W = x.shape
    Hs = Ws = 0
    if up is not None:
        up = _req(up, "up")
        if up.dim() != 4 or up.shape[:2] != x.shape[:2]:
            raise ValueError("group_norm_act_: up must be (B, C, Hs, Ws)")
        Hs, Ws = int(up.shape[2]), int(up.shape[3])
    ws = torch.empty(2 * B * groups, device=x.device, dtype=torch.float64)
    _launch("wm2f_group_norm_act", x, _p(x), _p(gamma), _p(beta), _p(up), _p(x), _p(ws), B, C, int(groups), H, W, Hs, Ws,
            float(eps), 1 if relu else 0)
    return x
