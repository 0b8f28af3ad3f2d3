"""K3: the mask einsums, fp32 and bf16, their backward kernels and the attention-mask epilogues."""
from __future__ import annotations

from typing import Sequence

import torch

from .._lib import WM2F_F32, load
from ._core import _launch, _p, _f32, _req, _amp_fwd, _amp_bwd


class _MaskEinsum(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, emb, pix, tag=None):
        emb, pix = _req(emb, "emb"), _req(pix, "pix")
        B, Q, C = emb.shape
        if pix.dim() != 4 or pix.shape[0] != B or pix.shape[1] != C:
            raise ValueError(f"mask_einsum: emb {tuple(emb.shape)} vs pix {tuple(pix.shape)}")
        Hh, Ww = pix.shape[2:]
        out = torch.empty(B, Q, Hh, Ww, device=emb.device, dtype=emb.dtype)
        _launch("wm2f_mask_einsum_fwd", emb, _p(emb), _p(pix), _p(out), B, Q, C, Hh * Ww, WM2F_F32,
                tag="mask_einsum_fwd" + (f"_{tag}" if tag else ""))
        ctx.save_for_backward(emb, pix)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, grad_out):
        emb, pix = ctx.saved_tensors
        g_emb, g_pix = mask_einsum_bwd(emb, pix, grad_out, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return g_emb, g_pix, None


def mask_einsum_bwd_applies(Q: int, C: int, HW: int) -> bool:
    """Shapes the hand-written K3 backward covers (wm2f.h); others take two batched library GEMMs."""
    return C % 64 == 0 and Q % 4 == 0 and HW % 4 == 0 and (C + 16) * HW * 4 < 2 ** 31 and (Q + 16) * HW * 4 < 2 ** 31


def mask_einsum_bwd(emb, pix, grad_out, want_emb=True, want_pix=True):
    """K3 backward: g_emb (B,Q,C) = grad x pix^T, g_pix (B,C,H,W) = emb^T x grad (wm2f_mask_einsum_bwd; deterministic)."""
    B, Q, C = emb.shape
    HW = int(pix.shape[2]) * int(pix.shape[3])
    if not mask_einsum_bwd_applies(Q, C, HW):
        go = grad_out.reshape(B, Q, -1)
        g_emb = torch.bmm(go, pix.reshape(B, C, -1).transpose(1, 2)) if want_emb else None
        g_pix = torch.bmm(emb.transpose(1, 2), go).view_as(pix) if want_pix else None
        return g_emb, g_pix
    emb, pix, go = _req(emb, "emb"), _req(pix, "pix"), _req(grad_out.contiguous(), "grad_out")
    g_emb = torch.empty_like(emb) if want_emb else None
    g_pix = torch.empty_like(pix) if want_pix else None
    if not (want_emb or want_pix):
        return None, None
    ws = torch.empty(int(load().wm2f_mask_einsum_bwd_workspace(B, Q, C, HW)), device=emb.device, dtype=torch.uint8)
    _launch("wm2f_mask_einsum_bwd", emb, _p(emb), _p(pix), _p(go), _p(g_emb) if want_emb else None,
            _p(g_pix) if want_pix else None, _p(ws), B, Q, C, HW, WM2F_F32, tag="mask_einsum_bwd")
    return g_emb, g_pix


def mask_einsum(emb: torch.Tensor, pix: torch.Tensor, tag: str | None = None) -> torch.Tensor:
    """K3 -- einsum('bqc,bchw->bqhw') (HF:2046) on the fp32 matrix cores.  `tag` only names the launch for the kernel timer."""
    return _MaskEinsum.apply(emb, pix, tag)


def nchw_to_pixel_major_bf16(pix: torch.Tensor) -> torch.Tensor:
    """(B, C, H, W) bf16 -> (B, H*W, C) bf16 (tiled transpose; no autograd: used as saved data of mask_einsum_bf16)."""
    pix = _req(pix.detach(), "pix", torch.bfloat16)
    B, C, Hh, Ww = pix.shape
    out = torch.empty(B, Hh * Ww, C, device=pix.device, dtype=torch.bfloat16)
    _launch("wm2f_nchw_to_pixel_major_bf16", pix, _p(pix), _p(out), B, C, Hh * Ww)
    return out


class _MaskEinsumBf16(torch.autograd.Function):
    """bf16 operands, fp32 logits.  `pix_t` is the pixel-major copy of `pix` (made once per forward)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, emb, pix, pix_t):
        emb = _req(emb if emb.dtype == torch.bfloat16 else emb.to(torch.bfloat16), "emb", torch.bfloat16)
        pix_t = _req(pix_t, "pix_t", torch.bfloat16)
        B, Q, C = emb.shape
        Hh, Ww = pix.shape[2:]
        if pix_t.shape != (B, Hh * Ww, C):
            raise ValueError(f"mask_einsum_bf16: pix_t {tuple(pix_t.shape)} vs emb {tuple(emb.shape)}, pix {tuple(pix.shape)}")
        out = torch.empty(B, Q, Hh, Ww, device=emb.device, dtype=torch.float32)
        for q0 in range(0, Q, 112):  # the kernel holds at most 7 query tiles
            q1 = min(Q, q0 + 112)
            e = emb[:, q0:q1].contiguous() if (q0, q1) != (0, Q) else emb
            o = out[:, q0:q1] if (q0, q1) != (0, Q) else out
            oc = o if o.is_contiguous() else torch.empty(B, q1 - q0, Hh, Ww, device=emb.device, dtype=torch.float32)
            _launch("wm2f_mask_einsum_bf16_fwd", emb, _p(e), _p(pix_t), _p(oc), B, q1 - q0, C, Hh * Ww,
                    tag="mask_einsum_bf16_fwd")
            if oc is not o:
                o.copy_(oc)
        # `pix` (the NCHW tensor) is the backward's right operand: contiguous along the pixel contraction.  It is an input
        # of the forward and alive anyway; pix_t is kept only for shapes the backward kernels do not cover.
        ctx.save_for_backward(emb, pix_t, pix)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, grad_out):
        emb, pix_t, pix = ctx.saved_tensors
        g_emb, g_pix = mask_einsum_bf16_bwd(emb, pix, grad_out, ctx.needs_input_grad[0], ctx.needs_input_grad[1], pix_t)
        return g_emb, g_pix, None


def mask_einsum_bf16_bwd_applies(Q: int, C: int, HW: int) -> bool:
    """Shapes the hand-written bf16 K3 backward covers (wm2f.h); others take two batched library GEMMs."""
    return C % 64 == 0 and Q % 4 == 0 and Q <= 112 and HW % 8 == 0 and (C + 16) * HW * 2 < 2 ** 31 and (Q + 16) * HW * 4 < 2 ** 31


def mask_einsum_bf16_bwd(emb, pix, grad_out, want_emb=True, want_pix=True, pix_t=None):
    """K3 backward under bf16 autocast: emb (B,Q,C) bf16, pix (B,C,H,W) bf16, grad_out (B,Q,H,W) fp32 -> g_emb, g_pix bf16
    (wm2f_mask_einsum_bf16_bwd: grad rounded to bf16 in registers, fp32 accumulation, deterministic)."""
    B, Q, C = emb.shape
    HW = int(pix.shape[2]) * int(pix.shape[3])
    if not (want_emb or want_pix):
        return None, None
    if not mask_einsum_bf16_bwd_applies(Q, C, HW) or pix.dtype != torch.bfloat16 or not pix.is_contiguous():
        go = grad_out.reshape(B, Q, -1).to(torch.bfloat16)
        if pix_t is None:
            pix_t = pix.reshape(B, C, HW).transpose(1, 2).to(torch.bfloat16)
        g_emb = torch.bmm(go, pix_t) if want_emb else None
        g_pix = torch.bmm(emb.transpose(1, 2), go).view(pix.shape).to(pix.dtype) if want_pix else None
        return g_emb, g_pix
    emb = _req(emb, "emb", torch.bfloat16)
    pix = _req(pix, "pix", torch.bfloat16)
    go = _req(grad_out.contiguous(), "grad_out")
    g_emb = torch.empty_like(emb) if want_emb else None
    g_pix = torch.empty_like(pix) if want_pix else None
    ws = torch.empty(int(load().wm2f_mask_einsum_bf16_bwd_workspace(B, Q, C, HW)), device=emb.device, dtype=torch.uint8)
    _launch("wm2f_mask_einsum_bf16_bwd", emb, _p(emb), _p(pix), _p(go), _p(g_emb) if want_emb else None,
            _p(g_pix) if want_pix else None, _p(ws), B, Q, C, HW, tag="mask_einsum_bf16_bwd")
    return g_emb, g_pix


def mask_einsum_bf16(emb: torch.Tensor, pix: torch.Tensor, pix_t: torch.Tensor) -> torch.Tensor:
    """K3 under bf16 autocast: emb (B,Q,C), pix (B,C,H,W) bf16 (for shape and gradient), pix_t = nchw_to_pixel_major_bf16(pix)
    -> fp32 logits (B,Q,H,W)."""
    return _MaskEinsumBf16.apply(emb, pix, pix_t)


def mask_einsum_attn_mask(emb: torch.Tensor, pix_level: torch.Tensor, tag: str | None = None):
    """K3 with the thresholding epilogue fused (HF:2046, :2051-2053, :1912-1914): emb (B,Q,C), pix_level (B,C,h,w) = the
    mask features at the LEVEL's resolution -> (mask (B,Q,h*w) uint8 1 = blocked, row_open (B,Q) int32).  No logits are
    written; no autograd (the dependency detaches the mask, HF:2054)."""
    emb, pix_level = _req(_f32(emb.detach()), "emb"), _req(_f32(pix_level.detach()), "pix_level")
    B, Q, C = emb.shape
    if pix_level.dim() != 4 or pix_level.shape[0] != B or pix_level.shape[1] != C:
        raise ValueError(f"mask_einsum_attn_mask: emb {tuple(emb.shape)} vs pix {tuple(pix_level.shape)}")
    HW = int(pix_level.shape[2]) * int(pix_level.shape[3])
    mask = torch.empty(B, Q, HW, device=emb.device, dtype=torch.uint8)
    row_open = torch.empty(B, Q, device=emb.device, dtype=torch.int32)
    _launch("wm2f_mask_einsum_attn_mask_fwd", emb, _p(emb), _p(pix_level), _p(mask), _p(row_open), B, Q, C, HW, WM2F_F32,
            tag="mask_einsum_attn_mask" + (f"_{tag}" if tag else ""))
    return mask, row_open


def attn_mask_build(logits: torch.Tensor, size: Sequence[int]):
    """HF:2048-2054 + HF:1912-1914: (mask (B,Q,Hn*Wn) uint8 1=blocked, row_open (B,Q) int32).  No grad."""
    logits = _req(_f32(logits.detach()), "logits")
    B, Q, H, W = logits.shape
    Hn, Wn = int(size[0]), int(size[1])
    mask = torch.empty(B, Q, Hn * Wn, device=logits.device, dtype=torch.uint8)
    row_open = torch.empty(B, Q, device=logits.device, dtype=torch.int32)
    _launch("wm2f_attn_mask_build", logits, _p(logits), _p(mask), _p(row_open), B, Q, H, W, Hn, Wn, tag="attn_mask_build")
    return mask, row_open
