"""What the inference-precision tests share (csrc/token_gemm_split.hip, conv1x1_split.hip, conv3x3_split.hip,
stem_split.hip at P = 3, 2, 1 pieces): the piece split restated in torch, the sum of the kept products in float64, the h
piece of an operand, and the accuracy rule per level.  A plain module: it imports without a GPU, and every function works
on the device its tensors are on.

The levels.  With both operands written as bf16 pieces a = h + m + l (h from a clamped to the largest finite bf16),
    highest   3 pieces, the six products m.m, l.h, h.l, m.h, h.m, h.h           e <= 2 e32 + 2^-23   (§13)
    high      2 pieces, the three products m.h, h.m, h.h                        e <= 2 e32 + 2^-14
    medium    1 piece, the product h.h                                          e <= 2 e32 + 2^-6
e and e32 are the measure of tests/split_gemm_cases.py.  The floors are derived, not fitted: at two pieces the dropped
h.l, l.h and m.m are each at most 2^-16 (1 + 2^-7) sum |x w| (|m| <= 2^-8 |a|, |a - h - m| <= 2^-16 |a|), and three of them
stay below 2^-14; at one piece |a - h| <= 2^-8 |a| (with the clamp) on both operands gives 2^-7 + 2^-16 < 2^-6."""
from __future__ import annotations

import torch

BF16_MAX = 3.3895313892515355e38  # largest finite bf16, 0x7F7F
LEVELS = ("highest", "high", "medium")
PIECES = {"highest": 3, "high": 2, "medium": 1}
FLOORS = {"highest": 2.0 ** -23, "high": 2.0 ** -14, "medium": 2.0 ** -6}
# (W piece, x piece) of the kept products, in the order the kernels chain them; 0 = h, 1 = m, 2 = l
PRODUCTS = {3: ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0)), 2: ((1, 0), (0, 1), (0, 0)), 1: ((0, 0),)}


def h_piece(a: torch.Tensor) -> torch.Tensor:
    """The first piece as fp32: the round-to-nearest-even bf16 of `a` clamped to the largest finite bf16."""
    return a.clamp(-BF16_MAX, BF16_MAX).bfloat16().float()


def split_pieces(a: torch.Tensor, P: int):
    """The P-piece split of an fp32 tensor, each piece as fp32 (its values are bf16 values): h, then the RNE bf16 of what
    the pieces before leave.  The differences are exact in fp32."""
    if P not in (1, 2, 3):
        raise ValueError(P)
    pieces = [h_piece(a)]
    rest = a
    for _ in range(P - 1):
        rest = rest - pieces[-1]
        pieces.append(rest.bfloat16().float())
    return pieces


def kept_sum(x: torch.Tensor, w: torch.Tensor, P: int) -> torch.Tensor:
    """float64 sum over k of the products a P-piece kernel keeps, x (M, K) against w (N, K): (M, N)."""
    xp = [p.double() for p in split_pieces(x, P)]
    wp = [p.double() for p in split_pieces(w, P)]
    out = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float64, device=x.device)
    for wi, xi in PRODUCTS[P]:
        out = out + xp[xi] @ wp[wi].t()
    return out


def rule(e: float, e32: float, level: str) -> bool:
    return e <= 2.0 * e32 + FLOORS[level]
