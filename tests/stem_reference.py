"""What the ResNet stem tests share (csrc/stem_split.hip): the fp64 reference of
MaxPool2d(3, 2, 1)(ReLU(conv7x7 / 2 + bias)) with the normaliser of the accuracy rule, the fp32 comparator, seeded inputs
and the maps.  A plain module: it imports without a GPU, and every function works on the device its tensors are on.

The measure and the rule are those of tests/split_gemm_cases.py, unchanged: e = max |out - ref| / mag, a case passes when
e <= 2 e32 + 2^-23.  For a pooled value |max a_i - max r_i| <= max |a_i - r_i|, so the window maximum of the per-pixel
normaliser sum_k |x_k w_k| + |b| is the sound normaliser of a pooled output."""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

STRIP_P = 15  # pooled columns of a wave's strip (kStripP of csrc/stem_split.hip)
RING = 8      # input rows of a wave's ring (a conv row reads 7, the next row's 2 new ones replace the oldest)
# one full strip plus one pooled column (Wp = 16), one ring of pooled rows plus one (Hp = 9): Hi = 4 Hp - 1, Wi = 4 Wp - 1
TILE_MAP = (4 * (RING + 1) - 1, 4 * (STRIP_P + 1) - 1)
MAPS = [(1, 1), (2, 3), (5, 4), (7, 9), (16, 16), (33, 31), (66, 130), TILE_MAP]
CINS = (1, 3)
BATCHES = (1, 3)
N = 64


def out_hw(H: int, W: int):
    """(Hp, Wp) of an H x W image: the 7x7 / 2 convolution with padding 3, then the 3x3 / 2 pool with padding 1."""
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1


def stem_ref(x, w, b):
    """fp64 reference: (out, mag), out = max_pool2d(relu(conv2d(x, w, stride 2, padding 3) + b), 3, 2, 1) on doubles and
    mag = max_pool2d(conv2d(|x|, |w|) + |b|, 3, 2, 1)."""
    xd, wd, bd = x.double(), w.double(), b.double()
    y = F.conv2d(xd, wd, None, 2, 3) + bd[None, :, None, None]
    mag = F.conv2d(xd.abs(), wd.abs(), None, 2, 3) + bd.abs()[None, :, None, None]
    return F.max_pool2d(y.relu(), 3, 2, 1), F.max_pool2d(mag, 3, 2, 1)


def stem_fp32(x, w, b):
    """The fp32 comparator: the same chain with the convolution as an fp32 im2col GEMM in stock torch ops."""
    B, _, H, W = x.shape
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.matmul(w.flatten(1), F.unfold(x, 7, padding=3, stride=2)) + b[None, :, None]
    return F.max_pool2d(y.relu().view(B, -1, Hc, Wc), 3, 2, 1)


@functools.lru_cache(maxsize=None)
def case(family: str, B: int, cin: int, H: int, W: int):
    """x (B, Cin, H, W), w (64, Cin, 7, 7), bias (64,): fp32 CPU tensors from a seeded CPU generator, with the fp64
    reference (out, mag) computed once on the CPU.  Callers must not write to what they get.
      ints    exact small integers in [-3, 3], bias in [-5, 5]: every partial sum is an integer below 2^24
      randn   unit-scale x, w of variance 1 / (49 Cin), bias 0.1 randn
      wide    randn 2^randint(-20, 20) per element, on both operands
      fltmax  x is +-FLT_MAX at random, w is randn 2^-30"""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + 3 * cin + B)
    if family == "ints":
        x = torch.randint(-3, 4, (B, cin, H, W), generator=g).float()
        w = torch.randint(-3, 4, (N, cin, 7, 7), generator=g).float()
        b = torch.randint(-5, 6, (N,), generator=g).float()
    else:
        x = torch.randn(B, cin, H, W, generator=g)
        w = torch.randn(N, cin, 7, 7, generator=g) * (1.0 / math.sqrt(49 * cin))
        b = torch.randn(N, generator=g) * 0.1
        if family == "wide":
            x = x * torch.exp2(torch.randint(-20, 21, x.shape, generator=g).float())
            w = w * torch.exp2(torch.randint(-20, 21, w.shape, generator=g).float())
        elif family == "fltmax":
            x = torch.where(x > 0, torch.finfo(torch.float32).max, -torch.finfo(torch.float32).max)
            w = torch.randn(N, cin, 7, 7, generator=g) * 2.0 ** -30
        elif family != "randn":
            raise ValueError(family)
    ref, mag = stem_ref(x, w, b)
    return x, w, b, ref, mag


def nonfinite_mask(B: int, H: int, W: int, bad):
    """Where an output must be non-finite: (B, Hp, Wp) bool, true where the pool o conv receptive field holds one of the
    pixels `bad` = [(b, y, x), ...] -- an indicator convolution (ones, 7x7 / 2, padding 3) and the pool of it."""
    hit = torch.zeros(B, 1, H, W, dtype=torch.float64)
    for bi, y, xx in bad:
        hit[bi, 0, y, xx] = 1.0
    conv = F.conv2d(hit, torch.ones(1, 1, 7, 7, dtype=torch.float64), None, 2, 3)
    return F.max_pool2d(conv, 3, 2, 1)[:, 0] > 0
