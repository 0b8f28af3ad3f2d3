"""Preconditions of the split-bf16 shape and value-range tests (tests/split_gemm_cases.py), checked on
the host: every input family stays inside §13's derived bound under the numpy restatement of the split, the near-FLT_MAX
family leaves the accuracy rule something to say, the equivariance data stays clear of underflow and overflow, and the
convolutions' configuration rule finds a tile for every N it admits."""
import numpy as np
import pytest
import torch

import split_gemm_cases as S
from test_token_gemm_split_cpu import BF16_MAX, bf16_rne, split3
from weed_instance_segmentation_amd import _lib

M, K, N = 64, 96, 48


def _six_products(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    xh, xm, xl = (p.astype(np.float64) for p in split3(x))
    wh, wm, wl = (p.astype(np.float64) for p in split3(w))
    return xh @ wh.T + xh @ wm.T + xm @ wh.T + xh @ wl.T + xl @ wh.T + xm @ wm.T


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("taps", [1, 9])
def test_every_family_is_within_the_derived_bound_on_the_host(family, taps):
    """|six products - exact| <= 2^-23 sum_k |x_k w_k|: the three products left out are each at most 2^-24 |x w| (§13).
    The randn families measure about 2^-28; mixed exponents (wide) measure 3.75e-8, between 2^-25 and 2^-23."""
    x, w, _ = S.operands(family, M, taps * K, N, seed=5, taps=1)
    x, w = x.numpy(), w[:, 0].numpy()
    exact = x.astype(np.float64) @ w.astype(np.float64).T
    mag = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    err = np.abs(_six_products(x, w) - exact)
    assert np.all(err <= 2.0 ** -23 * mag), (err / np.maximum(mag, 1e-300)).max()
    assert mag.min() > 0


def test_ints_family_is_exact_in_fp32():
    x, w, b = S.operands("ints", M, 2048, N, seed=1)
    assert x.abs().max() <= 3 and w.abs().max() <= 3 and b.abs().max() <= 5
    assert torch.equal(x, x.round()) and torch.equal(w, w.round())
    assert 9 * 2048 + 5 + 5 < 2 ** 24  # every partial sum, with the bias and an integer residual, is an fp32 integer
    ref, _, _ = S.token_ref(x, w[:, 0], b)
    assert torch.equal(ref.float().double(), ref)


def test_family_shapes_and_structure():
    x, w, _ = S.operands("cancel", M, K, N, seed=2, taps=9)
    assert x.shape == (M, K) and w.shape == (N, 9, K)
    assert torch.equal(x[:, 1::2], x[:, 0::2] * (1.0 + 2.0 ** -12)) and torch.equal(w[:, :, 1::2], -w[:, :, 0::2])
    x, w, _ = S.operands("bf16", M, K, N, seed=2)
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(w.bfloat16().float(), w)
    x, _, _ = S.operands("postrelu", M, K, N, seed=2)
    assert x.min() == 0 and x.max() > 50
    x, w, _ = S.operands("wide", M, K, N, seed=2)
    assert x.abs().max() / x.abs().min() > 2.0 ** 30 and w.abs().max() / w.abs().min() > 2.0 ** 30
    xa, _, _ = S.operands("randn", M, K, N, seed=2)
    xb, _, _ = S.operands("randn", M, K, N, seed=2)
    assert torch.equal(xa, xb)  # seeded
    w3 = S.as_w3x3(S.operands("randn", M, 32, 64, seed=2, taps=9)[1])
    assert w3.shape == (64, 32, 3, 3)
    img = S.as_image(torch.arange(2 * 3 * 5 * 4.0).view(30, 4), 2, 3, 5)
    assert img.shape == (2, 4, 3, 5) and img[1, 2, 1, 3] == ((1 * 3 + 1) * 5 + 3) * 4 + 2


@pytest.mark.parametrize("taps", [1, 9])
def test_near_flt_max_family_leaves_the_rule_meaningful(taps):
    x, w, b = S.operands("fltmax", 531, K, 256, seed=3, taps=taps)
    assert torch.isfinite(x).all() and torch.isfinite(w).all() and torch.isfinite(b).all()
    assert (x == S.FLT_MAX).any() and (x == -S.FLT_MAX).any() and (x == np.float32(3.3961e38)).any()
    w2 = w.flatten(1)  # the 3x3 case at its worst: one pixel seeing the same x under all nine taps
    x9 = x.repeat(1, taps)
    mag = x9.double().abs() @ w2.double().abs().t()
    assert mag.max() < 2.0 ** 120
    assert torch.isfinite(x9 @ w2.t()).all()  # an fp32 matmul of the same data
    # what the clamp is for: the RNE bf16 of FLT_MAX is inf, that of 3.3961e38 the largest finite bf16
    r = bf16_rne(np.array([S.FLT_MAX, 3.3961e38], np.float32))
    assert np.isinf(r[0]) and r[1] == BF16_MAX
    h, m, lo = split3(x.numpy())
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(m)) and np.all(np.isfinite(lo))


@pytest.mark.parametrize("taps", [1, 9])
def test_equivariance_operands_stay_between_2_pow_minus_70_and_2_pow_70(taps):
    x, w, b = S.equivariance_operands(531, 96, 256, seed=4, taps=taps)
    assert x.abs().min() >= 2.0 ** -10 and w.abs().min() >= 2.0 ** -10 and b.abs().min() >= 2.0 ** -10
    for a, bb in S.SCALINGS:
        for t, e in ((x, a), (w, bb)):
            s = t * 2.0 ** e
            assert s.abs().min() >= 2.0 ** -70 and s.abs().max() <= 2.0 ** 70, (a, bb)
        # the scaled bias and outputs: finite and normal in fp32
        mag = (x.repeat(1, taps).double().abs() @ w.flatten(1).double().abs().t() + b.double().abs()) * 2.0 ** (a + bb)
        assert mag.max() < 2.0 ** 120 and (b.abs() * 2.0 ** (a + bb)).min() > 2.0 ** -120
    s = S.channel_exponents(256, seed=4)
    assert s.min() >= 2.0 ** -12 and s.max() <= 2.0 ** 12 and torch.equal(torch.log2(s), torch.log2(s).round())


def test_tiny_operands_scales():
    x, w, b = S.tiny_operands(-112, 64, 96, 64, seed=6)
    assert torch.isfinite(w).all() and (x != 0).all() and x.abs().max() < 2.0 ** -108 and w.abs().max() < 2.0 ** 44
    assert (b != 0).all()
    # below the 2^-110 floor the host split loses at most 2^-134 per element (§13)
    h, m, lo = split3(x.numpy())
    rec = h.astype(np.float64) + m.astype(np.float64) + lo.astype(np.float64)
    loss = np.abs(rec - x.numpy().astype(np.float64))
    assert loss.max() <= 2.0 ** -134 and loss.max() > 0
    x, _, _ = S.tiny_operands(-100, 64, 96, 64, seed=6)
    h, m, lo = split3(x.numpy())
    big = np.abs(x.numpy()) >= 2.0 ** -110
    rec = h.astype(np.float64) + m.astype(np.float64) + lo.astype(np.float64)
    assert np.array_equal(rec[big], x.numpy().astype(np.float64)[big])


@pytest.mark.parametrize("name", ["wm2f_conv1x1_split_config", "wm2f_conv3x3_split_config"])
def test_configuration_lattice(name):
    fn = getattr(_lib.load(), name)
    for n_cu in (64, 256, 304):
        for B in (1, 3, 8):
            for P in (1, 15, 16, 17, 63, 65, 850, 4096, 65536):
                for Nc in range(64, 2049, 64):
                    ci = fn(Nc, P, B, n_cu)
                    assert 0 <= ci < len(S.NT) and Nc % S.NT[ci] == 0, (Nc, P, B, n_cu, ci)
                    if Nc % 128:  # 64, 192, 320, 448, ...: only the last entry fits
                        assert ci == len(S.NT) - 1
                for Nc in (16, 32, 48, 96, 100, 160, 255, 1000, 2000, 2040):
                    assert fn(Nc, P, B, n_cu) == -1, (Nc, P, B, n_cu)
