"""The split-bf16 GEMMs and convolutions, and the token Linears' weight gradient."""
from __future__ import annotations

import torch

from .. import ops as _flags  # the package itself: SPLIT_PRECISION is assigned on it and read when a split kernel is called
from .._lib import Wm2fError, load
from ..derived import derived
from ._core import _launch, _p, _req
from .fused import bias_act_, bias_relu_maxpool


_LEVEL_PIECES = {None: 3, "highest": 3, "high": 2, "medium": 1}


def _split_pieces():
    """(pieces, tag suffix) of the package flag ops.SPLIT_PRECISION as it stands at this call: the `pieces` argument of the
    wm2f_*_split_*_p entry points and what the launch tags carry below "highest" ("_p2", "_p1")."""
    level = _flags.SPLIT_PRECISION
    if not (level is None or isinstance(level, str)) or level not in _LEVEL_PIECES:
        raise ValueError(f"ops.SPLIT_PRECISION = {level!r}: 'highest', 'high', 'medium' or None")
    pieces = _LEVEL_PIECES[level]
    return pieces, ("" if pieces == 3 else f"_p{pieces}")


def token_linear_applies(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """Shapes token_linear is built for: fp32 on a GPU, N in {256, 288, 512, 768, 1024}, K a multiple of 32, x / out below
    2 GiB (the fp32-MFMA kernel, split=False, additionally needs N in {256, 288} and K a multiple of 64)."""
    N, K = weight.shape
    M = x.numel() // max(K, 1)
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and N in (256, 288, 512, 768, 1024)
            and K % 32 == 0 and x.shape[-1] == K and M * K * 4 < (1 << 31) and M * N * 4 < (1 << 31)
            and N * K * 6 < (1 << 31))


def split_weight(weight: torch.Tensor) -> torch.Tensor:
    """The three bf16 pieces of an fp32 weight (N, K) in wm2f_token_linear_split_fwd's fragment order (N * K * 6 bytes,
    returned as a uint8 tensor).  Callers that reuse a weight cache this per weight version (split_weight_cached)."""
    weight = _req(weight, "weight")
    N, K = weight.shape
    ws = torch.empty(N * K * 6, device=weight.device, dtype=torch.uint8)
    _launch("wm2f_token_linear_split_weight", weight, _p(weight), _p(ws), N, K)
    return ws


def _check_split(w_split: torch.Tensor, nbytes: int, x: torch.Tensor, message: str) -> None:
    """A caller's split weight: `nbytes` bytes of uint8 on x's device, or ValueError(message)."""
    if w_split.dtype != torch.uint8 or w_split.numel() != nbytes or w_split.device != x.device:
        raise ValueError(message)


ROWS_NATURAL, ROWS_FFN = 0, 1  # WM2F_ROWS_* of include/wm2f.h


def ffn_row_order(n_rows: int) -> torch.Tensor:
    """The row map of ROWS_FFN for a weight of n_rows rows (a multiple of 32), from the library: entry n is the weight row
    that split_weight_rows(weight, ROWS_FFN) puts at row position n (include/wm2f.h, wm2f_token_ffn_row)."""
    lib = load()
    return torch.tensor([lib.wm2f_token_ffn_row(n) for n in range(n_rows)], dtype=torch.long)


def split_weight_rows(weight: torch.Tensor, row_order: int = ROWS_FFN) -> torch.Tensor:
    """split_weight with the rows of the weight (N, K) in another order, done by the kernel on the original weight
    (wm2f_token_linear_split_weight_rows): ROWS_NATURAL gives split_weight's bytes, ROWS_FFN (N % 32 == 0) the order
    token_ffn reads fc1's weight in, the bytes of split_weight(weight[ffn_row_order(N)])."""
    weight = _req(weight, "weight")
    N, K = weight.shape
    ws = torch.empty(N * K * 6, device=weight.device, dtype=torch.uint8)
    _launch("wm2f_token_linear_split_weight_rows", weight, _p(weight), _p(ws), N, K, int(row_order))
    return ws


def split_weight_cached(owner, name: str, weight: torch.Tensor, base: torch.Tensor | None = None,
                        tap_major: bool = False) -> torch.Tensor:
    """split_weight(weight), cached for `owner` under `name` by derived() and redone when the weight changes (`base` when
    weight is a fresh view of it each call).  A 1x1 convolution kernel (N, K, 1, 1) is split as (N, K).
    tap_major=True: weight is a convolution kernel, split in the K order its kernel reads: (N, Cin, 3, 3) as conv3x3 does
    (split_weight_3x3), (64, Cin, 7, 7) as stem_conv_pool does (split_weight_stem)."""
    if not tap_major:
        make = lambda: split_weight(weight.view(weight.shape[0], -1) if weight.dim() == 4 else weight)
    else:
        make = lambda: (split_weight_stem if tuple(weight.shape[2:]) == (7, 7) else split_weight_3x3)(weight)
    return derived(owner, name, (weight if base is None else base,), make)


def split_weight_rows_cached(owner, name: str, weight: torch.Tensor, row_order: int = ROWS_FFN) -> torch.Tensor:
    """split_weight_rows(weight, row_order), cached as split_weight_cached caches split_weight, under a `name` of its own
    (the plain split of the same weight lives under another)."""
    return derived(owner, name, (weight,), lambda: split_weight_rows(weight, row_order))


def split_weight_3x3(weight: torch.Tensor) -> torch.Tensor:
    """The split of a 3x3 kernel (N, Cin, 3, 3) for wm2f_conv3x3_split_fwd: split_weight of its tap-major reorder
    (N, 3, 3, Cin) seen as (N, 9 Cin), so that column (3 dy + dx) Cin + c is tap (dy, dx) of channel c."""
    N = int(weight.shape[0])
    return split_weight(weight.permute(0, 2, 3, 1).reshape(N, -1).contiguous())


def token_linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, relu: bool = False, residual: torch.Tensor | None = None,
                 ln: tuple | None = None, pos: torch.Tensor | None = None, out_group: int = 0, split: bool = True,
                 w_split: torch.Tensor | None = None):
    """Linear over tokens with its epilogue fused (inference, no autograd): x (..., K) @ weight (N, K)^T + bias, then
    optional ReLU, optional LayerNorm(value + residual) with ln = (gamma, beta, eps), and with `pos` (rows_per_image, N)
    additionally out + pos broadcast over the batch.  Returns out, or (out, out + pos).
    out_group = G > 0: the result comes back feature-group major, (N // G, *x.shape[:-1], G) -- with G = 36 K1's operand rows
    head-major (ms_deform_attn_fused_lanes(..., head_major=True)).
    split=True (default): the split-bf16 kernel (wm2f_token_linear_split_fwd, fp32 accuracy on the bf16 matrix cores), with
    `w_split` = split_weight(weight) if the caller keeps one; split=False: the fp32-MFMA kernel (wm2f_token_linear_fwd)."""
    x, weight, bias = _req(x, "x"), _req(weight, "weight"), _req(bias, "bias")
    N, K = weight.shape
    if x.shape[-1] != K or bias.shape != (N,):
        raise ValueError(f"token_linear: x {tuple(x.shape)} weight {tuple(weight.shape)} bias {tuple(bias.shape)}")
    M = x.numel() // K
    if out_group and (out_group % 4 or N % out_group or ln is not None):
        raise ValueError("token_linear: out_group must divide N, be a multiple of 4 and exclude the LayerNorm epilogue")
    out = (torch.empty(N // out_group, *x.shape[:-1], out_group, device=x.device, dtype=torch.float32) if out_group
           else torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32))
    gamma = beta = None
    eps = 0.0
    if ln is not None:
        gamma, beta, eps = _req(ln[0], "gamma"), _req(ln[1], "beta"), float(ln[2])
    if residual is not None:
        residual = _req(residual, "residual")
        if residual.numel() != M * N:
            raise ValueError("token_linear: residual shape")
    out_pos, pos_rows = None, 0
    if pos is not None:
        pos = _req(pos, "pos")
        pos_rows = pos.numel() // N
        if M % pos_rows:
            raise ValueError("token_linear: pos rows do not divide the token count")
        out_pos = torch.empty_like(out)
    tag = f"token_linear_K{K}_N{N}" + ("_ln" if ln is not None else "")
    if split:
        if w_split is None:
            w_split = split_weight(weight)
        else:
            _check_split(w_split, N * K * 6, x, "token_linear: w_split is not split_weight(weight)")
        pieces, lvl = _split_pieces()
        _launch("wm2f_token_linear_split_fwd_p", x, _p(x), _p(w_split), _p(bias), _p(residual), _p(gamma), _p(beta), _p(pos),
                _p(out), _p(out_pos), M, K, N, 1 if relu else 0, pos_rows, eps, int(out_group), pieces,
                tag=tag + "_split" + lvl)
    else:
        _launch("wm2f_token_linear_fwd", x, _p(x), _p(weight), _p(bias), _p(residual), _p(gamma), _p(beta), _p(pos), _p(out),
                _p(out_pos), M, K, N, 1 if relu else 0, pos_rows, eps, int(out_group), tag=tag)
    return (out, out_pos) if pos is not None else out


def token_ffn_applies(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor) -> bool:
    """Shapes token_ffn is built for: fp32 on a GPU, w1 (F, 256) and w2 (256, F) with F in {256, 512, 768, 1024},
    x (..., 256) below 2 GiB."""
    if w1.dim() != 2 or w2.dim() != 2:
        return False
    F_, K = w1.shape
    N = w2.shape[0]
    M = x.numel() // max(K, 1)
    return (x.is_cuda and x.dtype == torch.float32 and w1.dtype == torch.float32 and w2.dtype == torch.float32
            and K == 256 and N == 256 and w2.shape[1] == F_ and F_ in (256, 512, 768, 1024) and x.shape[-1] == K
            and M * 256 * 4 < (1 << 31))


def token_ffn(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, residual: torch.Tensor,
              ln: tuple, pos: torch.Tensor | None = None, w1_split: torch.Tensor | None = None,
              w2_split: torch.Tensor | None = None):
    """The feed-forward pair of an encoder layer in one kernel (inference, no autograd; wm2f_token_ffn_split_fwd, DESIGN
    §13.3): LayerNorm(relu(x @ w1^T + b1) @ w2^T + b2 + residual) with ln = (gamma, beta, eps), and with `pos`
    (rows_per_image, 256) additionally out + pos broadcast over the batch.  Returns out, or (out, out + pos) -- the bits of
        token_linear(token_linear(x, w1, b1, relu=True), w2, b2, residual=residual, ln=ln, pos=pos)
    without the (M, F) intermediate, at every ops.SPLIT_PRECISION.  w1_split = split_weight_rows(w1, ROWS_FFN) and
    w2_split = split_weight(w2) if the caller keeps them.  The shapes of token_ffn_applies."""
    x, w1, b1, w2, b2 = _req(x, "x"), _req(w1, "w1"), _req(b1, "b1"), _req(w2, "w2"), _req(b2, "b2")
    F_, K = w1.shape
    N = w2.shape[0]
    if x.shape[-1] != K or b1.shape != (F_,) or w2.shape != (N, F_) or b2.shape != (N,):
        raise ValueError(f"token_ffn: x {tuple(x.shape)} w1 {tuple(w1.shape)} b1 {tuple(b1.shape)} w2 {tuple(w2.shape)} "
                         f"b2 {tuple(b2.shape)}")
    if residual is None or ln is None:
        raise ValueError("token_ffn: the residual and the LayerNorm are part of the kernel")
    M = x.numel() // K
    residual = _req(residual, "residual")
    if residual.numel() != M * N:
        raise ValueError("token_ffn: residual shape")
    gamma, beta, eps = _req(ln[0], "gamma"), _req(ln[1], "beta"), float(ln[2])
    out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
    out_pos, pos_rows = None, 0
    if pos is not None:
        pos = _req(pos, "pos")
        pos_rows = pos.numel() // N
        if M % pos_rows:
            raise ValueError("token_ffn: pos rows do not divide the token count")
        out_pos = torch.empty_like(out)
    for ws, what in ((w1_split, "w1_split is not split_weight_rows(w1, ROWS_FFN)"), (w2_split, "w2_split is not split_weight(w2)")):
        if ws is not None:
            _check_split(ws, F_ * K * 6, x, "token_ffn: " + what)
    if w1_split is None:
        w1_split = split_weight_rows(w1, ROWS_FFN)
    if w2_split is None:
        w2_split = split_weight(w2)
    pieces, lvl = _split_pieces()
    _launch("wm2f_token_ffn_split_fwd_p", x, _p(x), _p(w1_split), _p(b1), _p(w2_split), _p(b2), _p(residual), _p(gamma), _p(beta),
            _p(pos), _p(out), _p(out_pos), M, K, F_, N, pos_rows, eps, pieces, tag=f"token_ffn_K{K}_F{F_}_split" + lvl)
    return (out, out_pos) if pos is not None else out


_SWIN_LINEAR_LIMIT = 1 << 31  # bytes of x, of an output and of the residual in one call (32-bit buffer offsets)


def swin_linear_applies(x: torch.Tensor, weight: torch.Tensor, n_out: int = 1) -> bool:
    """Shapes swin_linear is built for: fp32 on a GPU, weight (N, K) with K a multiple of 32 and N of 16 (n_out = 3: N / 3 a
    multiple of 16), x (..., K) with at least one row, the split weight below 2 GiB.  Any M: rows are cut into calls."""
    if not isinstance(weight, torch.Tensor) or weight.dim() != 2 or x.dim() < 1 or n_out not in (1, 3):
        return False
    N, K = int(weight.shape[0]), int(weight.shape[1])
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and K > 0 and K % 32 == 0
            and N > 0 and N % 16 == 0 and x.shape[-1] == K and x.numel() >= K and N * K * 6 < (1 << 31)
            and (n_out == 1 or (N % 3 == 0 and (N // 3) % 16 == 0)))


def _aligned16(t):
    """A view into a flat parameter bucket, or a row range of a larger tensor, may start anywhere: the kernel reads 16-byte
    pieces, so such a tensor is copied."""
    return t.clone() if t is not None and t.data_ptr() % 16 else t


def swin_linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, *, gelu: bool = False,
                residual: torch.Tensor | None = None, n_out: int = 1, w_split: torch.Tensor | None = None, config: int = -1):
    """A Linear of the Swin backbone with its epilogue fused (inference, no autograd; wm2f_swin_linear_split_fwd_p, DESIGN
    §45): x (..., K) @ weight (N, K)^T + bias (None: no bias), then one of: nothing; gelu=True, the exact GELU; residual
    (..., N), added.  fp32 accuracy on the bf16 matrix cores at ops.SPLIT_PRECISION "highest", the lower levels as the other
    split kernels.  n_out = 3 (bias epilogue only) returns the three N / 3-wide column blocks as three contiguous tensors:
    the merged q | k | v projection.  `w_split` = split_weight(weight) if the caller keeps one.  config >= 0 forces an entry
    of the kernel's tile table (tests, tuning; the same bits), -1 lets the host choose.  Rows are cut into several calls
    when x, an output or the residual reaches 2 GiB.  A strided or 16-byte-unaligned tensor is copied first (as _req does
    for strides).  The shapes of swin_linear_applies."""
    ts = {"x": x, "weight": weight, "bias": bias, "residual": residual}
    for name, t in ts.items():
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError(f"swin_linear: {name}: expected a tensor")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts.values()):
        raise Wm2fError("swin_linear has no backward: call it under no_grad or on tensors that do not require grad")
    x, weight = _aligned16(_req(x, "x")), _req(weight, "weight")
    if weight.dim() != 2 or x.dim() < 1:
        raise ValueError(f"swin_linear: x {tuple(x.shape)} weight {tuple(weight.shape)}")
    N, K = int(weight.shape[0]), int(weight.shape[1])
    if gelu and residual is not None:
        raise ValueError("swin_linear: one epilogue: gelu or residual")
    if n_out not in (1, 3) or (n_out == 3 and (gelu or residual is not None)):
        raise ValueError("swin_linear: n_out is 1, or 3 with the bias epilogue")
    if not swin_linear_applies(x, weight, n_out):
        raise ValueError(f"swin_linear: x {tuple(x.shape)} weight {tuple(weight.shape)} n_out {n_out} outside swin_linear_applies")
    M = x.numel() // K
    if bias is not None:
        bias = _aligned16(_req(bias, "bias"))
        if bias.shape != (N,):
            raise ValueError(f"swin_linear: bias {tuple(bias.shape)} for {N} features")
    if residual is not None:
        residual = _aligned16(_req(residual, "residual"))
        if residual.numel() != M * N:
            raise ValueError("swin_linear: residual shape")
    if w_split is None:
        w_split = split_weight(weight)
    else:
        _check_split(w_split, N * K * 6, x, "swin_linear: w_split is not split_weight(weight)")
    n3 = N // n_out
    outs = [torch.empty(*x.shape[:-1], n3, device=x.device, dtype=torch.float32) for _ in range(n_out)]
    pieces, lvl = _split_pieces()
    epilogue = 1 if gelu else (2 if residual is not None else 0)
    tag = f"swin_linear_K{K}_N{N}" + ("_gelu" if gelu else "") + ("_res" if residual is not None else "") + \
        ("_qkv" if n_out == 3 else "") + lvl
    rows = max(1, (_SWIN_LINEAR_LIMIT - 1) // (4 * max(K, N)))  # whole rows per call; a row is a multiple of 64 bytes
    x2, r2, o2 = x.view(M, K), None if residual is None else residual.view(M, N), [o.view(M, n3) for o in outs]
    for m0 in range(0, M, rows):
        m1 = min(M, m0 + rows)
        oc = [o[m0:m1] for o in o2] + [None] * (3 - n_out)
        _launch("wm2f_swin_linear_split_fwd_p", x, _p(x2[m0:m1]), _p(w_split), _p(bias), _p(None if r2 is None else r2[m0:m1]),
                _p(oc[0]), _p(oc[1]), _p(oc[2]), m1 - m0, K, N, epilogue, int(n_out), int(config), pieces, tag=tag)
    return outs[0] if n_out == 1 else tuple(outs)


def conv1x1_applies(x: torch.Tensor, weight: torch.Tensor, stride: int = 1) -> bool:
    """Shapes wm2f_conv1x1_split_fwd is built for: fp32 NCHW on a GPU, weight (N, K, 1, 1) or (N, K) with K % 32 == 0 and
    N % 64 == 0, stride 1 or 2, one image of x / out below 2 GiB, the split weight below 2 GiB."""
    if x.dim() != 4 or weight.dim() not in (2, 4) or (weight.dim() == 4 and weight.shape[2:] != (1, 1)):
        return False
    N, K = int(weight.shape[0]), int(weight.shape[1])
    _, C, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and C == K and K % 32 == 0
            and N % 64 == 0 and stride in (1, 2) and K * H * W * 4 < (1 << 31) and N * Ho * Wo * 4 < (1 << 31)
            and N * K * 6 < (1 << 31))


def conv1x1(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, residual: torch.Tensor | None = None,
            relu: bool = False, stride: int = 1, split: bool = True, w_split: torch.Tensor | None = None,
            config: int = -1) -> torch.Tensor:
    """1x1 convolution without padding, epilogue fused (inference, no autograd): act(conv(x, weight, stride) + bias
    (+ residual)), x (B, K, H, W) fp32.  The residual epilogue needs bias and relu.
    split=True: wm2f_conv1x1_split_fwd (fp32 accuracy on the bf16 matrix cores), with `w_split` = split_weight of the
    weight seen as (N, K) if the caller keeps one; shapes outside conv1x1_applies take the split=False path.  config >= 0
    forces an entry of the kernel's tile table (tests, tuning; the same bits), -1 lets the kernel choose.
    split=False: F.conv2d, then bias_act_ (or the same in torch ops when Ho * Wo is not a multiple of 4)."""
    if residual is not None and (bias is None or not relu):
        raise ValueError("conv1x1: the residual epilogue is bias + residual + ReLU")
    if relu and bias is None:
        raise ValueError("conv1x1: the ReLU epilogues carry a bias")
    N, K = int(weight.shape[0]), int(weight.shape[1])
    if not split or not conv1x1_applies(x, weight, stride):
        w4 = weight if weight.dim() == 4 else weight.view(N, K, 1, 1)
        y = torch.nn.functional.conv2d(x, w4, None, stride)
        if bias is None:
            return y
        if (y.shape[-1] * y.shape[-2]) % 4 == 0:
            return bias_act_(y, bias, residual, relu)
        y = y + bias[None, :, None, None]
        if residual is not None:
            y = y + residual
        return torch.relu(y) if relu else y
    x = _req(x, "x")
    w2 = _req(weight.reshape(N, K), "weight")
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if bias is not None:
        bias = _req(bias, "bias")
        if bias.shape != (N,):
            raise ValueError(f"conv1x1: bias {tuple(bias.shape)} for {N} channels")
    if residual is not None:
        residual = _req(residual, "residual")
        if residual.shape != (B, N, Ho, Wo):
            raise ValueError(f"conv1x1: residual {tuple(residual.shape)}, output ({B}, {N}, {Ho}, {Wo})")
    if w_split is None:
        w_split = split_weight(w2)
    else:
        _check_split(w_split, N * K * 6, x, "conv1x1: w_split is not split_weight(weight)")
    out = torch.empty(B, N, Ho, Wo, device=x.device, dtype=torch.float32)
    pieces, lvl = _split_pieces()
    _launch("wm2f_conv1x1_split_fwd_p", x, _p(x), _p(w_split), _p(bias), _p(residual), _p(out), B, K, N, H, W, int(stride),
            1 if relu else 0, int(config), pieces, tag=f"conv1x1_K{K}_N{N}_P{Ho * Wo}{lvl}")
    return out


def conv1x1_dual_applies(x1: torch.Tensor, w1: torch.Tensor, x2: torch.Tensor, w2: torch.Tensor, stride2: int = 1) -> bool:
    """Shapes wm2f_conv1x1_split_dual_fwd_p is built for: each (x, weight) pair inside conv1x1_applies (x1 at stride 1, x2 at
    stride2), the same device, batch and N, and x2 sampled at stride2 landing on x1's map."""
    if stride2 not in (1, 2) or not (conv1x1_applies(x1, w1, 1) and conv1x1_applies(x2, w2, stride2)):
        return False
    _, _, Ho, Wo = x1.shape
    _, _, H2, W2 = x2.shape
    return (x1.device == x2.device and x1.shape[0] == x2.shape[0] and int(w1.shape[0]) == int(w2.shape[0])
            and (H2 - 1) // stride2 + 1 == Ho and (W2 - 1) // stride2 + 1 == Wo)


def conv1x1_dual(x1: torch.Tensor, w1: torch.Tensor, x2: torch.Tensor, w2: torch.Tensor, bias: torch.Tensor, stride2: int = 1,
                 w1_split: torch.Tensor | None = None, w2_split: torch.Tensor | None = None, config: int = -1,
                 split: bool = True) -> torch.Tensor:
    """relu(conv1x1(x1, w1) + conv1x1(x2, w2, stride2) + bias) as ONE GEMM over the concatenated K (inference, no autograd;
    wm2f_conv1x1_split_dual_fwd_p): a bottleneck's conv3 on x1 (B, K1, Ho, Wo) plus its projection shortcut on
    x2 (B, K2, H2, W2), whose full-width output never reaches memory.  w1_split / w2_split = split_weight of each weight seen
    as (N, K) if the caller keeps them -- two separate splits, read through two pointers.  config as conv1x1's.
    split=False, and shapes outside conv1x1_dual_applies: the two-call route,
        conv1x1(x1, w1, bias, residual=conv1x1(x2, w2, stride=stride2), relu=True)
    on the same `split`."""
    if bias is None:
        raise ValueError("conv1x1_dual: the epilogue is + bias + ReLU")
    if not split or not conv1x1_dual_applies(x1, w1, x2, w2, stride2):
        sc = conv1x1(x2, w2, None, stride=stride2, split=split, w_split=w2_split if split else None)
        if not x1.is_cuda:  # the same in torch ops (bias_act_ is a GPU kernel)
            w4 = w1 if w1.dim() == 4 else w1.view(*w1.shape, 1, 1)
            return torch.relu(torch.nn.functional.conv2d(x1, w4) + bias[None, :, None, None] + sc)
        return conv1x1(x1, w1, bias, sc, True, 1, split=split, w_split=w1_split if split else None)
    x1, x2, bias = _req(x1, "x1"), _req(x2, "x2"), _req(bias, "bias")
    N, K1, K2 = int(w1.shape[0]), int(w1.shape[1]), int(w2.shape[1])
    B, _, Ho, Wo = x1.shape
    _, _, H2, W2 = x2.shape
    if bias.shape != (N,):
        raise ValueError(f"conv1x1_dual: bias {tuple(bias.shape)} for {N} channels")
    splits = []
    for w, ws, K, name in ((w1, w1_split, K1, "w1"), (w2, w2_split, K2, "w2")):
        if ws is None:
            ws = split_weight(_req(w.reshape(N, K), name))
        else:
            _check_split(ws, N * K * 6, x1, f"conv1x1_dual: {name}_split is not split_weight({name})")
        splits.append(ws)
    out = torch.empty(B, N, Ho, Wo, device=x1.device, dtype=torch.float32)
    pieces, lvl = _split_pieces()
    _launch("wm2f_conv1x1_split_dual_fwd_p", x1, _p(x1), _p(splits[0]), _p(x2), _p(splits[1]), _p(bias), _p(out), B, K1, K2, N,
            Ho, Wo, H2, W2, int(stride2), int(config), pieces, tag=f"conv1x1_K{K1}+{K2}_N{N}_P{Ho * Wo}{lvl}")
    return out


def conv_group_stats_applies(channels: int, groups: int) -> bool:
    """Group sizes for which the split convolutions' epilogue produces the GroupNorm statistics of its output
    (conv1x1_gn, conv3x3_stats): groups of 4, 8 or 16 channels, each inside one 16-channel row tile of the kernel.  Any
    other size keeps the separate statistics pass (group_norm_act_, group_norm_tokens_)."""
    return groups > 0 and channels % groups == 0 and channels // groups in (4, 8, 16)


def conv1x1_gn(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, stride: int = 1,
               w_split: torch.Tensor | None = None, config: int = -1, stats_groups: int = 0, norm: tuple | None = None):
    """conv1x1 on the split kernel (raw or + bias; the shapes of conv1x1_applies) with GroupNorm folded in on one side:
    stats_groups = G > 0: returns (out, stats), stats (B, G, 2) fp64 = (sum, sum of squares) of out per image and group, from
        the kernel's epilogue -- the filled workspace group_norm_act_from_stats_ / group_norm_tokens_from_stats_ read.
        Needs conv_group_stats_applies(N, G).
    norm = (stats, groups, gamma, beta, eps, relu): x is read as act(GroupNorm(x)) from the filled workspace `stats` of x --
        bit for bit conv1x1 of group_norm_act_from_stats_(x, ...), without that pass over x.  Needs bias and stride 1.
        Returns out.
    `out` is bit for bit conv1x1's.  Inference, no autograd; exactly one of the two options."""
    if (stats_groups > 0) == (norm is not None):
        raise ValueError("conv1x1_gn: exactly one of stats_groups and norm")
    if not conv1x1_applies(x, weight, stride):
        raise ValueError("conv1x1_gn: shapes outside conv1x1_applies take conv1x1 and the separate GroupNorm passes")
    N, K = int(weight.shape[0]), int(weight.shape[1])
    x = _req(x, "x")
    w2 = _req(weight.reshape(N, K), "weight")
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if bias is not None:
        bias = _req(bias, "bias")
        if bias.shape != (N,):
            raise ValueError(f"conv1x1_gn: bias {tuple(bias.shape)} for {N} channels")
    if w_split is None:
        w_split = split_weight(w2)
    else:
        _check_split(w_split, N * K * 6, x, "conv1x1_gn: w_split is not split_weight(weight)")
    stats = nstats = ngamma = nbeta = None
    nG, neps, nrelu = 0, 0.0, False
    if norm is not None:
        nstats, nG, ngamma, nbeta, neps, nrelu = norm
        nstats, ngamma, nbeta = _req(nstats, "norm stats", torch.float64), _req(ngamma, "gamma"), _req(nbeta, "beta")
        if nstats.numel() != 2 * B * int(nG) or ngamma.shape != (K,) or nbeta.shape != (K,):
            raise ValueError("conv1x1_gn: norm = (stats (B, G, 2) fp64, G, gamma (K), beta (K), eps, relu)")
    else:
        stats = torch.empty(B, int(stats_groups), 2, device=x.device, dtype=torch.float64)
    out = torch.empty(B, N, Ho, Wo, device=x.device, dtype=torch.float32)
    pieces, lvl = _split_pieces()
    _launch("wm2f_conv1x1_split_gn_fwd_p", x, _p(x), _p(w_split), _p(bias), _p(out), _p(stats), int(stats_groups), _p(nstats),
            _p(ngamma), _p(nbeta), int(nG), float(neps), 1 if nrelu else 0, B, K, N, H, W, int(stride), int(config), pieces,
            tag=f"conv1x1_K{K}_N{N}_P{Ho * Wo}{lvl}")
    return out if norm is not None else (out, stats)


def _conv3x3_route(route: int | None) -> int:
    """The `route` argument of the wm2f_conv3x3_split_*_r entry points: an explicit 0 (direct kernel) or 1 (staged kernel,
    refused where it is not built), else the host's rule (-1) while ops.CONV3X3_STAGED is True and the direct kernel while
    it is False."""
    if route is None:
        return -1 if _flags.CONV3X3_STAGED else 0
    if route not in (-1, 0, 1):
        raise ValueError(f"conv3x3: route = {route!r}: None, -1 (the host's rule), 0 (direct) or 1 (staged)")
    return int(route)


def conv3x3_stats(x: torch.Tensor, weight: torch.Tensor, groups: int, stride: int = 1, w_split: torch.Tensor | None = None,
                  config: int = -1):
    """conv3x3 on the split kernel without bias (the shapes of conv3x3_applies), plus the GroupNorm statistics of its output
    from the epilogue: returns (out, stats), stats (B, groups, 2) fp64 as conv1x1_gn's.  `out` is bit for bit conv3x3's.
    Needs conv_group_stats_applies(N, groups).  The route of the launch follows ops.CONV3X3_STAGED (conv3x3_stats_route
    forces one).  Inference, no autograd."""
    return conv3x3_stats_route(x, weight, groups, None, stride, w_split, config)


def conv3x3_stats_route(x: torch.Tensor, weight: torch.Tensor, groups: int, route: int | None, stride: int = 1,
                        w_split: torch.Tensor | None = None, config: int = -1):
    """conv3x3_stats with the `route` argument of conv3x3_route: 0 the direct kernel, 1 the staged kernel (refused where it is
    not built), None as ops.CONV3X3_STAGED says.  `out` has the same bits on both routes; the statistics are the same fp32
    partials where the map width is a multiple of 32, and within the same bound elsewhere."""
    if not conv3x3_applies(x, weight, stride):
        raise ValueError("conv3x3_stats: shapes outside conv3x3_applies take conv3x3 and the separate GroupNorm passes")
    x = _req(x, "x")
    N, Cin = int(weight.shape[0]), int(weight.shape[1])
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if w_split is None:
        w_split = split_weight_3x3(_req(weight, "weight"))
    else:
        _check_split(w_split, N * 9 * Cin * 6, x, "conv3x3_stats: w_split is not split_weight_3x3(weight)")
    out = torch.empty(B, N, Ho, Wo, device=x.device, dtype=torch.float32)
    stats = torch.empty(B, int(groups), 2, device=x.device, dtype=torch.float64)
    pieces, lvl = _split_pieces()
    _launch("wm2f_conv3x3_split_stats_fwd_r", x, _p(x), _p(w_split), _p(out), _p(stats), int(groups), B, Cin, N, H, W,
            int(stride), int(config), pieces, _conv3x3_route(route), tag=f"conv3x3_C{Cin}_N{N}_P{Ho * Wo}{lvl}")
    return out, stats


def conv3x3_applies(x: torch.Tensor, weight: torch.Tensor, stride: int = 1) -> bool:
    """Shapes wm2f_conv3x3_split_fwd is built for: fp32 NCHW on a GPU, weight (N, Cin, 3, 3) with Cin % 32 == 0 and
    N % 64 == 0, stride 1 or 2 (padding 1, dilation 1, one group), one image of x / out below 2 GiB, the split weight
    below 2 GiB."""
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        return False
    N, C = int(weight.shape[0]), int(weight.shape[1])
    _, K, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and C == K and K % 32 == 0
            and N % 64 == 0 and stride in (1, 2) and K * H * W * 4 < (1 << 31) and N * Ho * Wo * 4 < (1 << 31)
            and N * 9 * K * 6 < (1 << 31))


def conv3x3(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, relu: bool = False, stride: int = 1,
            split: bool = True, w_split: torch.Tensor | None = None, config: int = -1) -> torch.Tensor:
    """3x3 convolution with padding 1, epilogue fused (inference, no autograd): act(conv(x, weight, stride) + bias),
    x (B, Cin, H, W) fp32, weight (N, Cin, 3, 3).  The ReLU epilogue needs a bias.
    split=True: wm2f_conv3x3_split_fwd (fp32 accuracy on the bf16 matrix cores), with `w_split` = split_weight_3x3(weight)
    if the caller keeps one; shapes outside conv3x3_applies take the split=False path.  config >= 0 forces an entry of the
    kernel's tile table (tests, tuning; the same bits), -1 lets the kernel choose.  The route of the launch
    (direct or staged kernel, the same bits: DESIGN §15) follows ops.CONV3X3_STAGED; conv3x3_route forces one.
    split=False: F.conv2d, then bias_act_ (or the same in torch ops when Ho * Wo is not a multiple of 4)."""
    return _conv3x3(x, weight, bias, relu, stride, split, w_split, config, None)


def conv3x3_route(x: torch.Tensor, weight: torch.Tensor, route: int | None, bias: torch.Tensor | None = None, relu: bool = False,
                  stride: int = 1, w_split: torch.Tensor | None = None, config: int = -1) -> torch.Tensor:
    """conv3x3 on the split kernel with the route of the launch: 0 the direct kernel, 1 the staged kernel (the
    x tile split once per channel block in LDS; stride 1 and the WN = 1 entries, refused with Wm2fError elsewhere), the
    same bits; None follows ops.CONV3X3_STAGED (True: the host's rule, False: direct)."""
    return _conv3x3(x, weight, bias, relu, stride, True, w_split, config, route)


def _conv3x3(x, weight, bias, relu, stride, split, w_split, config, route):
    if relu and bias is None:
        raise ValueError("conv3x3: the ReLU epilogue carries a bias")
    if not split or not conv3x3_applies(x, weight, stride):
        y = torch.nn.functional.conv2d(x, weight, None, stride, 1)
        if bias is None:
            return y
        if (y.shape[-1] * y.shape[-2]) % 4 == 0:
            return bias_act_(y, bias, None, relu)
        y = y + bias[None, :, None, None]
        return torch.relu(y) if relu else y
    x = _req(x, "x")
    N, Cin = int(weight.shape[0]), int(weight.shape[1])
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if bias is not None:
        bias = _req(bias, "bias")
        if bias.shape != (N,):
            raise ValueError(f"conv3x3: bias {tuple(bias.shape)} for {N} channels")
    if w_split is None:
        w_split = split_weight_3x3(_req(weight, "weight"))
    else:
        _check_split(w_split, N * 9 * Cin * 6, x, "conv3x3: w_split is not split_weight_3x3(weight)")
    out = torch.empty(B, N, Ho, Wo, device=x.device, dtype=torch.float32)
    pieces, lvl = _split_pieces()
    _launch("wm2f_conv3x3_split_fwd_r", x, _p(x), _p(w_split), _p(bias), _p(out), B, Cin, N, H, W, int(stride),
            1 if relu else 0, int(config), pieces, _conv3x3_route(route), tag=f"conv3x3_C{Cin}_N{N}_P{Ho * Wo}{lvl}")
    return out


STEM_K = 160  # K of the stem's split weight: five k-steps of 32


def stem_weight_columns(cin: int) -> torch.Tensor:
    """The K order wm2f_stem7x7_pool_fwd reads (csrc/stem_split.hip): for each of the 160 columns of its weight matrix the
    index of the tap it holds in the flat (c, ky, kx) order of a (Cin, 7, 7) kernel, or -1 for a column of padding.
    Column 8 G + i, i < 7, is tap (G // 7, G % 7, i) for the first min(7 Cin, 20) kernel rows G -- a lane's 8 consecutive
    columns are one kernel row, 7 consecutive floats of one input row; with Cin = 3 the 21st kernel row (2, 6) rides in
    the eighth columns, column 8 G + 7 holding its tap kx = G for G < 7."""
    if cin not in (1, 2, 3):
        raise ValueError(f"stem_weight_columns: Cin = {cin} (1, 2 and 3 are built)")
    cols = torch.full((STEM_K,), -1, dtype=torch.long)
    rows = 7 * cin
    for G in range(min(rows, STEM_K // 8)):
        cols[8 * G:8 * G + 7] = torch.arange(7 * G, 7 * G + 7)
    if rows > STEM_K // 8:
        cols[7:8 * 7:8] = torch.arange(7 * 20, 7 * 21)
    return cols


def stem_weight_matrix(weight: torch.Tensor) -> torch.Tensor:
    """The stem's (64, Cin, 7, 7) kernel as the (64, 160) matrix of stem_weight_columns, zero in the padding columns."""
    N, cin = int(weight.shape[0]), int(weight.shape[1])
    cols = stem_weight_columns(cin).to(weight.device)
    flat = torch.cat([weight.reshape(N, -1), weight.new_zeros(N, 1)], 1)
    return flat[:, torch.where(cols < 0, torch.full_like(cols, 49 * cin), cols)].contiguous()


def split_weight_stem(weight: torch.Tensor) -> torch.Tensor:
    """The split of the stem's kernel (64, Cin, 7, 7) for wm2f_stem7x7_pool_fwd: split_weight of stem_weight_matrix."""
    return split_weight(stem_weight_matrix(_req(weight, "weight")))


def stem_conv_pool_applies(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """Shapes wm2f_stem7x7_pool_fwd is built for: fp32 NCHW on a GPU, weight (64, Cin, 7, 7) with Cin in {1, 2, 3}, one
    image of x / out below 2 GiB (any map size)."""
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[2:]) != (7, 7):
        return False
    N, C = int(weight.shape[0]), int(weight.shape[1])
    _, K, H, W = x.shape
    Hp, Wp = ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and C == K and C in (1, 2, 3)
            and N == 64 and H >= 1 and W >= 1 and K * H * W * 4 < (1 << 31) and N * Hp * Wp * 4 < (1 << 31))


def stem_conv_pool(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, w_split: torch.Tensor | None = None,
                   split: bool = True, grid: int = 0) -> torch.Tensor:
    """The ResNet stem (inference, no autograd): MaxPool2d(3, 2, 1)(ReLU(conv2d(x, weight, stride 2, padding 3) + bias)),
    x (B, Cin, H, W) fp32, weight (N, Cin, 7, 7) with BatchNorm folded in by the caller.
    split=True: wm2f_stem7x7_pool_fwd, one kernel at fp32 accuracy on the bf16 matrix cores (the raw convolution never
    reaches memory), with `w_split` = split_weight_stem(weight) if the caller keeps one; shapes outside
    stem_conv_pool_applies take the split=False path.  grid > 0 forces that many workgroups (tests; the same bits), 0 lets
    the kernel choose.
    split=False: F.conv2d, then bias_relu_maxpool (or the same in torch ops where its map conditions fail)."""
    if not split or not stem_conv_pool_applies(x, weight):
        y = torch.nn.functional.conv2d(x, weight, None, 2, 3)
        if y.is_cuda and y.dtype == torch.float32 and y.shape[-2] % 2 == 0 and y.shape[-1] % 8 == 0:
            return bias_relu_maxpool(y, bias)
        return torch.nn.functional.max_pool2d(torch.relu_(y.add_(bias[None, :, None, None])), 3, 2, 1)
    x, bias = _req(x, "x"), _req(bias, "bias")
    N, Cin = int(weight.shape[0]), int(weight.shape[1])
    B, _, H, W = x.shape
    if bias.shape != (N,):
        raise ValueError(f"stem_conv_pool: bias {tuple(bias.shape)} for {N} channels")
    if w_split is None:
        w_split = split_weight_stem(weight)
    else:
        _check_split(w_split, N * STEM_K * 6, x, "stem_conv_pool: w_split is not split_weight_stem(weight)")
    out = torch.empty(B, N, ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1, device=x.device, dtype=torch.float32)
    pieces, lvl = _split_pieces()
    _launch("wm2f_stem7x7_pool_fwd_p", x, _p(x), _p(w_split), _p(bias), _p(out), B, Cin, N, H, W, int(grid), pieces,
            tag="stem7x7_pool" + lvl)
    return out


def token_wgrad_applies(dy: torch.Tensor, x: torch.Tensor) -> bool:
    """Shapes wm2f_token_wgrad_bf16 / _f32 are built for: both operands bf16 or both fp32 on a GPU, feature counts multiples
    of 8, operands below 2 GiB."""
    N, K = dy.shape[-1], x.shape[-1]
    M = x.numel() // max(K, 1)
    es = x.element_size()
    return (dy.is_cuda and x.is_cuda and dy.dtype == x.dtype and x.dtype in (torch.bfloat16, torch.float32) and N % 8 == 0
            and K % 8 == 0 and dy.numel() == M * N and M * N * es < 0x7fffffff and M * K * es < 0x7fffffff)


def token_wgrad(dy: torch.Tensor, x: torch.Tensor, want_bias: bool = True):
    """Weight (and bias) gradient of a Linear over tokens: dy (..., N), x (..., K), both bf16 or both fp32 -> dw (N, K) fp32 =
    dy^T x and db (N) fp32 = column sums of dy (None without `want_bias`).  fp32 accumulation, deterministic (include/wm2f.h)."""
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"token_wgrad: {x.dtype}")
    dy, x = _req(dy, "dy", x.dtype), _req(x, "x", x.dtype)
    N, K = dy.shape[-1], x.shape[-1]
    M = x.numel() // K
    if dy.numel() != M * N:
        raise ValueError(f"token_wgrad: dy {tuple(dy.shape)} x {tuple(x.shape)}")
    dw = torch.empty(N, K, device=x.device, dtype=torch.float32)
    db = torch.empty(N, device=x.device, dtype=torch.float32) if want_bias else None
    bf = x.dtype == torch.bfloat16
    ws = torch.empty(max(16, int(load().wm2f_token_wgrad_workspace(M, N, K))), device=x.device, dtype=torch.uint8)
    _launch("wm2f_token_wgrad_bf16" if bf else "wm2f_token_wgrad_f32", x, _p(dy), _p(x), _p(dw), _p(db), _p(ws), M, N, K,
            tag=f"token_wgrad_{'bf16' if bf else 'f32'}_N{N}_K{K}", what="wm2f_token_wgrad")
    return dw, db


class _TokenLinear(torch.autograd.Function):
    """nn.Linear over tokens with the weight gradient on wm2f_token_wgrad_*: forward and input gradient are the library's GEMMs
    (in bf16 under bf16 autocast, as autocast runs F.linear; in fp32 otherwise), dW / db come back in fp32 -- the parameters'
    dtype -- from ONE pass over dy and x."""

    @staticmethod
    def forward(ctx, x, weight, bias, bf16):
        cdt = torch.bfloat16 if bf16 else torch.float32
        xc, wc = x.to(cdt), weight.to(cdt)
        ctx.save_for_backward(xc, wc)
        ctx.x_dtype, ctx.has_bias, ctx.cdt = x.dtype, bias is not None, cdt
        return torch.nn.functional.linear(xc, wc, None if bias is None else bias.to(cdt))

    @staticmethod
    def backward(ctx, grad_out):
        xc, wc = ctx.saved_tensors
        g = grad_out.to(ctx.cdt).contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.matmul(g, wc).to(ctx.x_dtype)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gw, gb = token_wgrad(g, xc.contiguous(), want_bias=ctx.has_bias)
        return gx, gw, gb, None


def linear_tokens(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None) -> torch.Tensor:
    """F.linear for the token matrices of the pixel decoder's encoder layers.  In training on a GPU (fp32, or under bf16
    autocast) the weight-gradient product -- a 256 x 256 output with a contraction over every token of the batch, which a
    library GEMM runs on 16 of 256 CUs -- goes to wm2f_token_wgrad_*.  Everything else is plain F.linear."""
    amp = torch.is_autocast_enabled("cuda")
    bf16 = amp and torch.get_autocast_dtype("cuda") == torch.bfloat16
    if (torch.is_grad_enabled() and x.is_cuda and weight.requires_grad and weight.dtype == torch.float32
            and (bf16 or (not amp and x.dtype == torch.float32))
            and weight.shape[0] % 8 == 0 and weight.shape[1] % 8 == 0
            and x.numel() // weight.shape[1] * max(weight.shape) * (2 if bf16 else 4) < 0x7fffffff):
        with torch.autocast("cuda", enabled=False):
            return _TokenLinear.apply(x, weight, bias, bf16)
    return torch.nn.functional.linear(x, weight, bias)
