"""What the split-bf16 GEMM tests share (csrc/token_gemm_split.hip, conv1x1_split.hip, conv3x3_split.hip):
seeded input generators, fp64 references of the three ops with their epilogues, the error measure, the fp32 comparator and
the accuracy rule.  A plain module: it imports without a GPU, and every function works on the device its tensors are on.

The accuracy rule.  With e = max |out - ref| / (sum_k |x_k w_k| + |b| + |r|) of the kernel under test and e32 the same
measure of an fp32 computation of the same data, a case passes when  e <= 2 e32 + 2^-23.  The factor 2 is the project's
rule (§13); 2^-23 is §13's bound on the three products the kernels leave out, which keeps the rule meaningful where the
fp32 comparator happens to be exact (bf16-exact operands, small integers)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

FLT_MAX = 3.4028234663852886e38
RULE_FLOOR = 2.0 ** -23
FAMILIES = ("ints", "randn", "wide", "cancel", "postrelu", "bf16", "fltmax", "bnfold")
VALUE_FAMILIES = FAMILIES[2:]  # (c) to (h) of the value-range tests
NT = (256, 256, 256, 128, 64)  # channels of a workgroup tile, per entry of the convolutions' configuration table
RAW, BIAS, RELU, RES = "raw", "bias", "relu", "res"
SCALINGS = ((30, -7), (-30, 12), (45, 45), (-20, -20))  # (a, b) of the power-of-two equivariance cases


# ---------------------------------------------------------------------------------------------------------------- inputs
def operands(family: str, M: int, K: int, N: int, seed: int, taps: int = 1):
    """x (M, K), w (N, taps, K), bias (N,): fp32 CPU tensors from a seeded CPU generator.  K is the contraction (channel)
    axis of both operands; `taps` = 9 gives a 3x3 kernel's weight with the channel axis last.
      ints      exact small integers in [-3, 3], bias in [-5, 5]: every partial sum is an integer below 2^24
      randn     unit-scale x, w of variance 1 / (taps K), bias 0.1 randn (the existing tests' data)
      wide      randn 2^randint(-20, 20) per element, on both operands
      cancel    odd columns of x = even columns (1 + 2^-12), odd columns of w = - even columns
      postrelu  x = 50 relu(randn)
      bf16      both operands exactly representable in bf16
      fltmax    three columns of x are FLT_MAX, -FLT_MAX and 3.3961e38 (just below the tie between the largest finite
                bf16 and 2^128); the matching columns of w are scaled by 2^-30
      bnfold    row n of w and entry n of the bias multiplied by 2^s_n, s_n in [-12, 12] (a folded BatchNorm)"""
    g = torch.Generator().manual_seed(seed)
    if family == "ints":
        x = torch.randint(-3, 4, (M, K), generator=g).float()
        w = torch.randint(-3, 4, (N, taps, K), generator=g).float()
        b = torch.randint(-5, 6, (N,), generator=g).float()
        return x, w, b
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, taps, K, generator=g) * (1.0 / math.sqrt(taps * K))
    b = torch.randn(N, generator=g) * 0.1
    if family == "randn":
        pass
    elif family == "wide":
        x = x * torch.exp2(torch.randint(-20, 21, (M, K), generator=g).float())
        w = w * torch.exp2(torch.randint(-20, 21, (N, taps, K), generator=g).float())
    elif family == "cancel":
        x[:, 1::2] = x[:, 0::2] * (1.0 + 2.0 ** -12)
        w[:, :, 1::2] = -w[:, :, 0::2]
    elif family == "postrelu":
        x = 50.0 * x.relu()
    elif family == "bf16":
        x, w = x.bfloat16().float(), w.bfloat16().float()
    elif family == "fltmax":
        cols = (1, K // 2, K - 1)
        for c, v in zip(cols, (FLT_MAX, -FLT_MAX, 3.3961e38)):
            x[:, c] = v
            w[:, :, c] *= 2.0 ** -30
    elif family == "bnfold":
        s = torch.exp2(torch.randint(-12, 13, (N,), generator=g).float())
        w = w * s[:, None, None]
        b = b * s
    else:
        raise ValueError(family)
    return x, w, b


def extra(shape, seed: int, ints: bool = False):
    """A residual, a LayerNorm parameter or a `pos` table of the given shape (CPU, seeded)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-5, 6, shape, generator=g).float() if ints else torch.randn(shape, generator=g)


def floor_at_2_pow_minus_10(t: torch.Tensor) -> torch.Tensor:
    """Magnitudes below 2^-10 raised to 2^-10 (signs kept, zeros become +2^-10): data whose scaled copies stay clear of
    underflow in every piece and product of the power-of-two equivariance cases."""
    s = torch.where(t < 0, -1.0, 1.0).to(t.dtype)
    return s * t.abs().clamp_min(2.0 ** -10)


def equivariance_operands(M: int, K: int, N: int, seed: int, taps: int = 1):
    """x, w, bias of the power-of-two equivariance cases: the randn family with every magnitude at least 2^-10, so that
    2^a x and 2^b w with (a, b) in SCALINGS stay inside [2^-70, 2^70] and no piece, product or partial sum of either run
    underflows or overflows: the split, the RNE conversions and the fp32 sums then commute with the scaling, bit for bit."""
    x, w, b = operands("randn", M, K, N, seed, taps)
    return floor_at_2_pow_minus_10(x), floor_at_2_pow_minus_10(w), floor_at_2_pow_minus_10(b)


def channel_exponents(N: int, seed: int) -> torch.Tensor:
    """2^s_n, s_n in [-12, 12], per output channel (CPU, seeded)."""
    g = torch.Generator().manual_seed(seed)
    return torch.exp2(torch.randint(-12, 13, (N,), generator=g).float())


def tiny_operands(x_exp: int, M: int, K: int, N: int, seed: int, taps: int = 1):
    """The randn family with x at scale 2^x_exp, w at scale 2^40 and the bias at the outputs' scale: x around and below
    the floor (2^-110, §13) under which its third piece falls below bf16's subnormal step."""
    x, w, b = operands("randn", M, K, N, seed, taps)
    return x * 2.0 ** x_exp, w * 2.0 ** 40, b * 2.0 ** (x_exp + 40)


def as_image(x: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    """Rows (B H W, K) as an NCHW image (B, K, H, W): the contraction axis becomes the channels."""
    return x.view(B, H, W, x.shape[1]).permute(0, 3, 1, 2).contiguous()


def as_w1x1(w: torch.Tensor) -> torch.Tensor:
    return w[:, 0].contiguous()  # (N, K)


def as_w3x3(w: torch.Tensor) -> torch.Tensor:
    """(N, 9, Cin) as OIHW (N, Cin, 3, 3): tap t = 3 dy + dx."""
    N, _, C = w.shape
    return w.view(N, 3, 3, C).permute(0, 3, 1, 2).contiguous()


def out_hw(H: int, W: int, stride: int):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


# ------------------------------------------------------------------------------------------------------ fp64 references
def token_ref(x, w, b, relu=False, residual=None, ln=None, pos=None):
    """fp64 reference of ops.token_linear: (out, mag, out + pos or None).  mag = sum_k |x_k w_k| + |b| (+ |residual|),
    the error measure's denominator (of the value the LayerNorm normalises, when there is one)."""
    xd, wd = x.double(), w.double()
    y = torch.addmm(b.double(), xd, wd.t())
    mag = xd.abs() @ wd.abs().t() + b.double().abs()
    if relu:
        y = y.relu()
    if residual is not None:
        y = y + residual.double()
        mag = mag + residual.double().abs()
    if ln is not None:
        y = F.layer_norm(y, (w.shape[0],), ln[0].double(), ln[1].double(), ln[2])
    yp = None
    if pos is not None:
        yp = y + pos.double().repeat(x.shape[0] // pos.shape[0], 1)
    return y, mag, yp


def group_major(out: torch.Tensor, G: int) -> torch.Tensor:
    """Row-major (M, N) as ops.token_linear(..., out_group=G) returns it: (N / G, M, G)."""
    M, N = out.shape
    return out.view(M, N // G, G).permute(1, 0, 2)


def conv1x1_ref(x, w, b=None, residual=None, relu=False, stride=1):
    """fp64 reference of ops.conv1x1, x (B, K, H, W), w (N, K): (out (B, N, Ho, Wo), mag)."""
    B, _, H, W = x.shape
    Ho, Wo = out_hw(H, W, stride)
    xs = x[:, :, ::stride, ::stride].double().flatten(2)
    wd = w.double().flatten(1)
    y = torch.matmul(wd, xs)
    mag = torch.matmul(wd.abs(), xs.abs())
    if b is not None:
        y = y + b.double()[None, :, None]
        mag = mag + b.double().abs()[None, :, None]
    if residual is not None:
        y = y + residual.double().flatten(2)
        mag = mag + residual.double().abs().flatten(2)
    if relu:
        y = y.relu()
    return y.view(B, -1, Ho, Wo), mag.view(B, -1, Ho, Wo)


def conv3x3_ref(x, w, b=None, relu=False, stride=1):
    """fp64 reference of ops.conv3x3 (padding 1), x (B, Cin, H, W), w (N, Cin, 3, 3): (out, mag), by F.unfold + matmul."""
    B, _, H, W = x.shape
    Ho, Wo = out_hw(H, W, stride)
    cols = F.unfold(x.double(), 3, padding=1, stride=stride)  # (B, Cin 9, P), c-major like w.flatten(1)
    wd = w.double().flatten(1)
    y = torch.matmul(wd, cols)
    mag = torch.matmul(wd.abs(), cols.abs())
    if b is not None:
        y = y + b.double()[None, :, None]
        mag = mag + b.double().abs()[None, :, None]
    if relu:
        y = y.relu()
    return y.view(B, -1, Ho, Wo), mag.view(B, -1, Ho, Wo)


# ------------------------------------------------------------------------------------------------- measure, comparator
def rel_err(out: torch.Tensor, ref: torch.Tensor, mag: torch.Tensor) -> float:
    """max |out - ref| / mag; a non-finite output counts as an infinite error."""
    d = (out.double() - ref).abs() / mag.clamp_min(1e-300)
    d = torch.where(torch.isfinite(out), d, torch.full_like(d, float("inf")))
    return d.max().item()


def rule(e: float, e32: float) -> bool:
    return e <= 2.0 * e32 + RULE_FLOOR


def token_fp32(ops, x, w, b, relu=False, residual=None, ln=None):
    """The fp32 comparator of a token Linear: the fp32-MFMA kernel (split=False) where it is built (N in {256, 288},
    K % 64 == 0), otherwise the same chain in stock fp32 torch ops."""
    N, K = w.shape
    if ops is not None and x.is_cuda and N in (256, 288) and K % 64 == 0:
        return ops.token_linear(x, w, b, relu=relu, residual=residual, ln=ln, split=False)
    y = torch.addmm(b, x, w.t())
    if relu:
        y = y.relu()
    if residual is not None:
        y = y + residual
    if ln is not None:
        y = F.layer_norm(y, (N,), ln[0], ln[1], ln[2])
    return y


def conv1x1_fp32(ops, x, w, b=None, residual=None, relu=False, stride=1):
    """The fp32 comparator of a 1x1 convolution: ops.conv1x1(..., split=False), the library convolution + epilogue."""
    N, K = w.shape
    if ops is not None and x.is_cuda:
        return ops.conv1x1(x, w.view(N, K, 1, 1), b, None if residual is None else residual.clone(), relu, stride, split=False)
    y = F.conv2d(x, w.view(N, K, 1, 1), b, stride)
    if residual is not None:
        y = y + residual
    return y.relu() if relu else y


def conv3x3_fp32(x, w, b=None, relu=False, stride=1):
    """The fp32 comparator of a 3x3 convolution: the same convolution as an fp32 im2col GEMM in stock torch ops.  (The
    split=False route is the library's convolution, Winograd at stride 1, whose larger error would make the rule looser;
    §15 does not use it as the bar.)"""
    B, _, H, W = x.shape
    Ho, Wo = out_hw(H, W, stride)
    y = torch.matmul(w.flatten(1), F.unfold(x, 3, padding=1, stride=stride))
    if b is not None:
        y = y + b[None, :, None]
    if relu:
        y = y.relu()
    return y.view(B, -1, Ho, Wo)
