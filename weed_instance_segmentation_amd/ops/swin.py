"""Swin shifted-window attention: the inference launch and the trainable pair."""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import WM2F_BF16, WM2F_F32, load
from ._core import _launch, _p, _req


SWIN_WINDOW_SIZES = (4, 7, 12)
SWIN_HEAD_DIMS = (16, 32)


def swin_window_attention_applies(window_size: int, head_dim: int, dtype: torch.dtype, device) -> bool:
    """Shapes wm2f_swin_window_attn_fwd is built for: a GPU, fp32 or bf16 tokens, window 4 / 7 / 12, head_dim 16 / 32."""
    return (torch.device(device).type == "cuda" and dtype in (torch.float32, torch.bfloat16)
            and int(window_size) in SWIN_WINDOW_SIZES and int(head_dim) in SWIN_HEAD_DIMS)


def _swin_window_attention_args(fn: str, q, k, v, bias_table, dims, heads, window_size, shift, k_pad, v_pad):
    """The argument checks both Swin window-attention ops share; returns contiguous tensors and plain ints."""
    if q.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{fn}: q: expected float32 or bfloat16, got {q.dtype}")
    dt = q.dtype
    q, k, v = _req(q, "q", dt), _req(k, "k", dt), _req(v, "v", dt)
    bias_table = _req(bias_table, "bias_table")
    H, W = int(dims[0]), int(dims[1])
    ws, shift, heads = int(window_size), int(shift), int(heads)
    if q.dim() != 3 or heads <= 0 or q.shape[2] % heads:
        raise ValueError(f"{fn}: q {tuple(q.shape)} heads {heads}")
    B, N, E = q.shape
    D = E // heads
    if N != H * W or H <= 0 or W <= 0 or k.shape != q.shape or v.shape != q.shape:
        raise ValueError(f"{fn}: q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)} dims {(H, W)}")
    if ws <= 0 or not 0 <= shift < ws:
        raise ValueError(f"{fn}: shift {shift} outside [0, window {ws})")
    if bias_table.shape != ((2 * ws - 1) ** 2, heads):
        raise ValueError(f"{fn}: bias_table {tuple(bias_table.shape)} != {((2 * ws - 1) ** 2, heads)}")
    if not swin_window_attention_applies(ws, D, dt, q.device):
        raise ValueError(f"{fn}: window {ws} / head_dim {D} not built "
                         f"(windows {SWIN_WINDOW_SIZES}, head dims {SWIN_HEAD_DIMS})")
    pads = []
    for name, t in (("k_pad", k_pad), ("v_pad", v_pad)):
        if t is not None:
            t = _req(t, name, dt)
            if t.shape != (E,):
                raise ValueError(f"{fn}: {name} {tuple(t.shape)} != {(E,)}")
        pads.append(t)
    return q, k, v, bias_table, pads[0], pads[1], (H, W), heads, ws, shift


def _aligned16(t):
    """A view into a flat parameter bucket may start anywhere: the kernels read 16-byte pieces."""
    return t.clone() if t is not None and t.data_ptr() % 16 else t


def swin_window_attention(q, k, v, bias_table, dims, heads: int, window_size: int, shift: int, k_pad=None, v_pad=None):
    """Shifted-window attention of one Swin layer in ONE launch (inference only, no autograd): pad, roll, window partition,
    softmax(q k^T / sqrt(D) + relative-position bias + shift mask) v, window reverse, roll back and crop.
    q, k, v (B, H*W, heads*D) in image order, fp32 or bf16; bias_table ((2 ws - 1)^2, heads) fp32, the parameter itself;
    dims = (H, W); k_pad / v_pad (heads*D): key / value row of a padding token (the k / v Linear's bias), None = zeros.
    Returns (B, H*W, heads*D) in image order, dtype of q.  Contract: include/wm2f.h.
    Training goes through swin_window_attention_train."""
    ts = {"q": q, "k": k, "v": v, "bias_table": bias_table, "k_pad": k_pad, "v_pad": v_pad}
    for name, t in ts.items():
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError(f"swin_window_attention: {name}: expected a tensor")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts.values()):
        raise _lib.Wm2fError("swin_window_attention has no backward: call it under no_grad or on tensors that do not "
                             "require grad (training calls swin_window_attention_train)")
    q, k, v, bias_table, k_pad, v_pad, (H, W), heads, ws, shift = _swin_window_attention_args(
        "swin_window_attention", q, k, v, bias_table, dims, heads, window_size, shift, k_pad, v_pad)
    k_pad, v_pad = _aligned16(k_pad), _aligned16(v_pad)
    B, _, E = q.shape
    out = torch.empty_like(q)
    _launch("wm2f_swin_window_attn_fwd", q, _p(q), _p(k), _p(v), _p(k_pad), _p(v_pad), _p(bias_table), _p(out), B, H, W, heads,
            E // heads, ws, shift, WM2F_BF16 if q.dtype == torch.bfloat16 else WM2F_F32, tag=f"swin_window_attn_ws{ws}")
    return out


class _SwinWindowAttn(torch.autograd.Function):
    """wm2f_swin_window_attn_train_fwd / wm2f_swin_window_attn_bwd.  Saves the inputs and the rows' log-sum-exp; the table
    and the padding rows are read from the caller's tensors at both calls (no cache)."""

    @staticmethod
    def forward(ctx, q, k, v, bias_table, k_pad, v_pad, dims, heads, ws, shift):
        k_pad, v_pad = _aligned16(k_pad), _aligned16(v_pad)
        B, N, E = q.shape
        out = torch.empty_like(q)
        lse = torch.empty(B, heads, N, device=q.device, dtype=torch.float32)
        _launch("wm2f_swin_window_attn_train_fwd", q, _p(q), _p(k), _p(v), _p(k_pad), _p(v_pad), _p(bias_table), _p(out), _p(lse),
                B, dims[0], dims[1], heads, E // heads, ws, shift, WM2F_BF16 if q.dtype == torch.bfloat16 else WM2F_F32,
                tag=f"swin_window_attn_train_ws{ws}")
        ctx.save_for_backward(q, k, v, bias_table, k_pad, v_pad, lse)
        ctx.geom = (dims, heads, ws, shift)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, bias_table, k_pad, v_pad, lse = ctx.saved_tensors
        (H, W), heads, ws, shift = ctx.geom
        grad_out = _req(grad_out, "grad_out", q.dtype)
        B, _, E = q.shape
        D = E // heads
        need = ctx.needs_input_grad
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        f32 = lambda want, *shape: torch.empty(*shape, device=q.device, dtype=torch.float32) if want else None
        gt = f32(need[3], *bias_table.shape)
        gkp, gvp = f32(need[4] and k_pad is not None, E), f32(need[5] and v_pad is not None, E)
        space = None
        if gt is not None or gkp is not None or gvp is not None:
            space = torch.empty(int(load().wm2f_swin_window_attn_bwd_workspace(B, H, W, heads, D, ws)), device=q.device,
                                dtype=torch.uint8)
        _launch("wm2f_swin_window_attn_bwd", q, _p(q), _p(k), _p(v), _p(k_pad), _p(v_pad), _p(bias_table), _p(lse), _p(grad_out),
                _p(gq), _p(gk), _p(gv), _p(gkp), _p(gvp), _p(gt), _p(space), B, H, W, heads, D, ws, shift,
                WM2F_BF16 if q.dtype == torch.bfloat16 else WM2F_F32, tag=f"swin_window_attn_bwd_ws{ws}")
        cast = lambda gr, like: None if gr is None else gr.to(like.dtype)
        return gq, gk, gv, gt, cast(gkp, k_pad), cast(gvp, v_pad), None, None, None, None


def swin_window_attention_train(q, k, v, bias_table, dims, heads: int, window_size: int, shift: int, k_pad=None, v_pad=None):
    """swin_window_attention with a backward: the same contract, arguments and checks, differentiable in q, k, v,
    bias_table, k_pad and v_pad (include/wm2f.h: wm2f_swin_window_attn_train_fwd / _bwd).  grad q / k / v come back in
    q's dtype, the others in the dtype of the tensor passed in; an input that does not require grad costs no reduction.
    The table's and the padding rows' gradients are summed in a fixed order: two calls give the same bits."""
    for name, t in {"q": q, "k": k, "v": v, "bias_table": bias_table, "k_pad": k_pad, "v_pad": v_pad}.items():
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError(f"swin_window_attention_train: {name}: expected a tensor")
    args = _swin_window_attention_args("swin_window_attention_train", q, k, v, bias_table, dims, heads, window_size, shift,
                                       k_pad, v_pad)
    with torch.autocast("cuda", enabled=False):
        return _SwinWindowAttn.apply(*args)
