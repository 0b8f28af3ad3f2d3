"""K1: multi-scale deformable attention (forward, backward, the rows / packed / lanes inference forms)."""
from __future__ import annotations

from typing import Sequence

import torch

from .. import _lib
from .. import ops as _flags  # the package itself: K1_BWD_DETERMINISTIC is assigned on it and read when a backward runs
from .._lib import WM2F_BF16, WM2F_F32, load
from ._core import _amp_bwd, _amp_fwd, _f32, _launch, _levels, _p, _req


class _MSDeformAttn(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, value, loc, attn_w, level_hw):
        value, loc, attn_w = _req(value, "value"), _req(loc, "loc"), _req(attn_w, "attn_w")
        B, S, H, D = value.shape
        _, Q, _, L, P, _ = loc.shape
        if loc.shape != (B, Q, H, L, P, 2) or attn_w.shape != (B, Q, H, L, P):
            raise ValueError(f"msdeform: shapes disagree: value {tuple(value.shape)} loc {tuple(loc.shape)} "
                             f"attn_w {tuple(attn_w.shape)}")
        out = torch.empty(B, Q, H * D, device=value.device, dtype=value.dtype)
        _launch("wm2f_msdeform_fwd", value, _p(value), _p(loc), _p(attn_w), _p(out), _levels(level_hw), B, S, Q, H, D, L, P,
                WM2F_F32, tag="msdeform_fwd")
        ctx.save_for_backward(value, loc, attn_w)
        ctx.level_hw = tuple(tuple(int(x) for x in hw) for hw in level_hw)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, grad_out):
        value, loc, attn_w = ctx.saved_tensors
        g_value, g_loc, g_w = ms_deform_attn_bwd(value, ctx.level_hw, loc, attn_w, grad_out)
        return g_value, g_loc, g_w, None


def k1_bwd_deterministic(deterministic: bool | None = None) -> bool:
    """Which K1 backward runs: the caller's choice, else the package flag ops.K1_BWD_DETERMINISTIC as it stands at this call,
    else torch's deterministic-algorithms switch."""
    if deterministic is None:
        deterministic = _flags.K1_BWD_DETERMINISTIC
    return torch.are_deterministic_algorithms_enabled() if deterministic is None else bool(deterministic)


def ms_deform_attn_bwd(value, level_hw, loc, attn_w, grad_out, deterministic: bool | None = None):
    """K1 backward (the autograd of HF:798-837): (grad_value, grad_loc, grad_attn_w).  `deterministic`: the fixed-point
    form of the grad_value scatter (wm2f_msdeform_bwd_det, run-to-run identical); default: module flag
    K1_BWD_DETERMINISTIC, else torch's deterministic-algorithms switch.  Shapes the fixed-point form does not cover
    raise under that switch (as torch's own ops without a deterministic form do) unless it is in warn-only mode."""
    value, loc, attn_w = _req(value, "value"), _req(loc, "loc"), _req(attn_w, "attn_w")
    grad_out = _req(grad_out, "grad_out")
    B, S, H, D = value.shape
    _, Q, _, L, P, _ = loc.shape
    g_loc = torch.empty_like(loc)
    g_w = torch.empty_like(attn_w)
    lv = _levels(level_hw)
    if k1_bwd_deterministic(deterministic):
        g_value = torch.empty_like(value)
        ws = torch.empty(max(16, int(load().wm2f_msdeform_bwd_det_workspace(lv, B, S, H, D, L))), device=value.device, dtype=torch.uint8)
        rc = _launch("wm2f_msdeform_bwd_det", value, _p(value), _p(loc), _p(attn_w), _p(grad_out), _p(g_value), _p(g_loc),
                     _p(g_w), _p(ws), lv, B, S, Q, H, D, L, P, WM2F_F32, tag="msdeform_bwd_det", raw=True)
        if rc != _lib.WM2F_EUNSUPPORTED:
            return g_value, g_loc, g_w
        if not torch.is_deterministic_algorithms_warn_only_enabled():
            raise RuntimeError("ms_deform_attn backward: no deterministic form for this shape (" + (load().wm2f_last_error() or b"?").decode() + ")")
    g_value = torch.zeros_like(value)
    _launch("wm2f_msdeform_bwd", value, _p(value), _p(loc), _p(attn_w), _p(grad_out), _p(g_value), _p(g_loc), _p(g_w), lv, B, S,
            Q, H, D, L, P, WM2F_F32, tag="msdeform_bwd")
    return g_value, g_loc, g_w


def ms_deform_attn(value: torch.Tensor, level_hw: Sequence[Sequence[int]], loc: torch.Tensor,
                   attn_w: torch.Tensor) -> torch.Tensor:
    """K1 -- multi_scale_deformable_attention (HF:798-837).
    value (B,S,heads,D), loc (B,Q,heads,L,P,2), attn_w (B,Q,heads,L,P) -> (B,Q,heads*D)."""
    return _MSDeformAttn.apply(value, loc, attn_w, level_hw)


def k1_rows_applies(value: torch.Tensor, rows: torch.Tensor, level_hw, heads: int, n_points: int = 4) -> bool:
    """Host-side copy of the shape test of wm2f_msdeform_rows_fwd / _bwd (K1 for training on the merged projection's rows):
    the streaming kernel's shapes (3 levels 1 : 2 : 4 coarse first, 4 points, head_dim 32, queries == tokens), an even head
    count, rows fp32 or bf16, and no deterministic-algorithms request (the fixed-point grad_value form takes loc / attn_w)."""
    if not (value.is_cuda and rows.is_cuda and value.dim() == 4 and rows.dim() == 3) or heads % 2:
        return False
    B, S, H, D = value.shape
    if H != heads or rows.shape != (B, S, heads * 3 * n_points * 3) or rows.dtype not in (torch.float32, torch.bfloat16):
        return False
    if value.dtype not in (torch.float32, rows.dtype):
        return False
    return (not k1_bwd_deterministic()) and k1_lanes_applies(level_hw, S, D, n_points, B, heads)


class _MSDeformAttnRows(torch.autograd.Function):
    """K1 with the prologue of HF:983-1002 inside, differentiable: (value, rows = [offsets | logits]) -> out, with the backward
    kernels writing the ROW gradient directly (wm2f_msdeform_rows_fwd / _bwd).  rows / out / their gradients share one dtype
    (fp32, or bf16 under bf16 autocast); value is cast to fp32 once (the kernels' windows are fp32) and kept for the backward."""

    @staticmethod
    def forward(ctx, value, rows, level_hw, heads):
        B, S, H, D = value.shape
        v32 = _req(value if value.dtype == torch.float32 else value.float(), "value")
        rows = _req(rows, "rows", rows.dtype)
        lp = rows.dtype == torch.bfloat16
        out = torch.empty(B, S, H * D, device=value.device, dtype=rows.dtype)
        _launch("wm2f_msdeform_rows_fwd", v32, _p(v32), _p(rows), _p(out), _levels(level_hw), B, S, S, H, D, 3, 4,
                WM2F_BF16 if lp else WM2F_F32, tag="msdeform_rows_fwd")
        ctx.save_for_backward(v32, rows)
        ctx.level_hw = tuple(tuple(int(x) for x in hw) for hw in level_hw)
        ctx.value_dtype = value.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        v32, rows = ctx.saved_tensors
        B, S, H, D = v32.shape
        lp = rows.dtype == torch.bfloat16
        grad_out = _req(grad_out if grad_out.dtype == rows.dtype else grad_out.to(rows.dtype), "grad_out", rows.dtype)
        g_value = torch.empty_like(v32)  # (cleared by the backward's first kernel)
        g_rows = torch.empty_like(rows)
        _launch("wm2f_msdeform_rows_bwd", v32, _p(v32), _p(rows), _p(grad_out), _p(g_value), _p(g_rows), _levels(ctx.level_hw), B,
                S, S, H, D, 3, 4, WM2F_BF16 if lp else WM2F_F32, tag="msdeform_rows_bwd")
        return (g_value if ctx.value_dtype == torch.float32 else g_value.to(ctx.value_dtype)), g_rows, None, None


def ms_deform_attn_rows(value: torch.Tensor, level_hw, rows: torch.Tensor, heads: int) -> torch.Tensor:
    """K1 on the merged projection's rows, with autograd (training): value (B,S,heads,32) fp32 / bf16, rows (B,S,heads*36) =
    [offsets (heads,3,4,2) | logits (heads,12)] fp32 / bf16 -> (B,S,heads*32) in the rows' dtype.  Reference points are the
    tokens' pixel centres (HF:1127-1156 with valid ratios of 1).  Check k1_rows_applies first."""
    if not k1_rows_applies(value, rows, level_hw, heads):
        raise ValueError("ms_deform_attn_rows: shapes / dtypes outside wm2f_msdeform_rows_fwd (see k1_rows_applies)")
    return _MSDeformAttnRows.apply(value, rows, level_hw, heads)


def ms_deform_attn_fused(value: torch.Tensor, level_hw, offsets: torch.Tensor, logits: torch.Tensor,
                         ref: torch.Tensor) -> torch.Tensor:
    """K1 with the softmax / location prologue of HF:983-1002 fused (inference path, no autograd).
    offsets (B,Q,heads,L,P,2) raw, logits (B,Q,heads,L*P) raw, ref (Q,L,2)."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (value, offsets, logits)):
        raise RuntimeError("ms_deform_attn_fused has no backward; use ms_deform_attn when training")
    value, offsets, logits, ref = (_req(_f32(value), "value"), _req(_f32(offsets), "offsets"), _req(_f32(logits), "logits"),
                                   _req(_f32(ref), "ref"))
    B, S, H, D = value.shape
    _, Q, _, L, P, _ = offsets.shape
    if logits.shape != (B, Q, H, L * P) or ref.shape != (Q, L, 2):
        raise ValueError("ms_deform_attn_fused: shapes disagree")
    out = torch.empty(B, Q, H * D, device=value.device, dtype=value.dtype)
    _launch("wm2f_msdeform_fused_fwd", value, _p(value), _p(offsets), _p(logits), _p(ref), _p(out), _levels(level_hw), B, S, Q, H,
            D, L, P, WM2F_F32, tag="msdeform_fused_fwd")
    return out


def ms_deform_attn_fused_packed(value, level_hw, packed, ref, heads: int, L: int, P: int, margin: int = 4):
    """Inference K1 fed by ONE merged projection: packed (B,Q,heads*L*P*3) = [offsets | logits] per token.
    Falls back to the two-array fused kernel (after splitting) where the LDS-window kernel does not apply."""
    if torch.is_grad_enabled() and (value.requires_grad or packed.requires_grad):
        raise RuntimeError("ms_deform_attn_fused_packed has no backward; use ms_deform_attn when training")
    value, packed, ref = _req(_f32(value), "value"), _req(_f32(packed), "packed"), _f32(ref)
    B, S, H, D = value.shape
    Q = packed.shape[1]
    if H != heads or packed.shape != (B, Q, heads * L * P * 3):
        raise ValueError(f"ms_deform_attn_fused_packed: value {tuple(value.shape)} packed {tuple(packed.shape)}")
    out = torch.empty(B, Q, H * D, device=value.device, dtype=value.dtype)
    rc = _launch("wm2f_msdeform_fused_packed_fwd", value, _p(value), _p(packed), _p(out), _levels(level_hw), B, S, Q, H, D, L, P,
                 WM2F_F32, int(margin), tag="msdeform_fused_fwd", raw=True)
    if rc == _lib.WM2F_EUNSUPPORTED:  # shape outside the LDS-window kernels -> direct-gather HIP kernel
        n_off = heads * L * P * 2
        off = packed[..., :n_off].reshape(B, Q, heads, L, P, 2).contiguous()
        logits = packed[..., n_off:].reshape(B, Q, heads, L * P).contiguous()
        return ms_deform_attn_fused(value, level_hw, off, logits, ref)
    return out


def k1_lanes_applies(level_hw, n_tokens: int, head_dim: int, n_points: int, batch: int = 1, heads: int = 8) -> bool:
    """Host-side copy of the shape test of wm2f_msdeform_fused_lanes_fwd (the streaming kernel): 3 levels with sides
    exactly 1 : 2 : 4 coarse first, 4 points, head_dim 32, queries == tokens, 32-bit offsets."""
    if len(level_hw) != 3 or n_points != 4 or head_dim != 32:
        return False
    (h0, w0), (h1, w1), (h2, w2) = [(int(a), int(b)) for a, b in level_hw]
    if (h1, w1) != (2 * h0, 2 * w0) or (h2, w2) != (4 * h0, 4 * w0) or h0 < 1 or w0 < 1 or 21 * h0 * w0 != n_tokens:
        return False
    row = heads * 3 * 4 * 3 * 4
    return batch * n_tokens < (1 << 24) and batch * n_tokens * row < 0x7fffffff and batch * n_tokens * heads * 128 < 0x7fffffff


def k1_lane_order(heads: int) -> torch.Tensor:
    """Row permutation that turns the [sampling_offsets ; attention_weights] projection (heads*24 offset rows, then heads*12
    logit rows; L = 3, P = 4) into the kernel's record order (include/wm2f.h, wm2f_msdeform_fused_lanes_fwd): 36 numbers per
    head in 16-byte pieces -- [x0 y0 x1 y1] of lanes (= point slots) 0..3, [x2 y2 w0 w1] of lanes 0..3, w2 of lanes 0..3."""
    L, P = 3, 4
    n_off = heads * L * P * 2
    h = torch.arange(heads)[:, None]
    j = torch.arange(P)[None, :]
    off = lambda l, xy: ((h * L + l) * P + j) * 2 + xy       # (heads, P) row index of offsets[h, l, j, xy]
    lg = lambda l: n_off + h * (L * P) + l * P + j             # (heads, P) row index of logits[h, l * P + j]
    a = torch.stack([off(0, 0), off(0, 1), off(1, 0), off(1, 1)], -1).reshape(heads, 16)
    b = torch.stack([off(2, 0), off(2, 1), lg(0), lg(1)], -1).reshape(heads, 16)
    return torch.cat([a, b, lg(2)], 1).reshape(-1)


def k1_lane_rows(offsets: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
    """(B, S, heads, 3, 4, 2) offsets and (B, S, heads, 12) logits -> (B, S, heads * 36) rows in the kernel's record order
    (what the merged projection with its rows permuted by `k1_lane_order` writes); tests and tools build operands with it."""
    B, S, H = offsets.shape[:3]
    packed = torch.cat([offsets.reshape(B, S, -1), logits.reshape(B, S, -1)], -1)
    return packed[..., k1_lane_order(H).to(packed.device)].contiguous()


def ms_deform_attn_fused_lanes(value, level_hw, lanes, heads: int, head_major: bool = False, value_head_major: bool = False,
                               slab_order: bool = False):
    """Inference K1 fed by ONE merged projection whose rows are in lane-major order (include/wm2f.h,
    wm2f_msdeform_fused_lanes_fwd): lanes (B,Q,heads*36), or head-major (heads,B,Q,36) -- what token_linear(out_group=36)
    writes and the kernel reads in fewer cache lines.  Streaming kernel only -- check `k1_lanes_applies` first; a shape it
    does not take RAISES (no silent re-route: the caller owns the row order of its projection)."""
    if torch.is_grad_enabled() and (value.requires_grad or lanes.requires_grad):
        raise RuntimeError("ms_deform_attn_fused_lanes has no backward; use ms_deform_attn when training")
    value, lanes = _req(_f32(value), "value"), _req(_f32(lanes), "lanes")
    if value_head_major:  # (heads, B, S, D): what token_linear(out_group=D) writes
        H, B, S, D = value.shape
    else:
        B, S, H, D = value.shape
    Q = lanes.shape[2] if head_major else lanes.shape[1]
    if H != heads or tuple(lanes.shape) != ((heads, B, Q, 36) if head_major else (B, Q, heads * 36)):
        raise ValueError(f"ms_deform_attn_fused_lanes: value {tuple(value.shape)} lanes {tuple(lanes.shape)} head_major={head_major}")
    out = torch.empty(B, Q, H * D, device=value.device, dtype=value.dtype)
    _launch("wm2f_msdeform_fused_lanes_fwd", value, _p(value), _p(lanes), _p(out), _levels(level_hw), B, S, Q, H, D, 3, 4,
            WM2F_F32, (1 if head_major else 0) | (2 if value_head_major else 0) | (4 if slab_order else 0),
            tag="msdeform_fused_fwd")
    return out


def ms_deform_attn_variant(value, level_hw, a, b, ref=None, fused=False, variant=0, margin=4) -> torch.Tensor:
    """K1 with the kernel variant exposed (no autograd): variant 0 auto, 1 direct gather, 2 LDS windows.
    fused=False: a = loc, b = attn_w.  fused=True: a = raw offsets, b = raw logits, ref (Q,L,2)."""
    value, a, b = _req(value, "value"), _req(a, "a"), _req(b, "b")
    if fused:
        ref = _req(ref, "ref")
    B, S, H, D = value.shape
    _, Q, _, L, P, _ = a.shape
    out = torch.empty(B, Q, H * D, device=value.device, dtype=value.dtype)
    _launch("wm2f_msdeform_fwd_v", value, _p(value), _p(a), _p(b), _p(ref if fused else None), _p(out), _levels(level_hw), B, S,
            Q, H, D, L, P, WM2F_F32, 1 if fused else 0, int(variant), int(margin), tag=f"msdeform_v{variant}")
    return out
