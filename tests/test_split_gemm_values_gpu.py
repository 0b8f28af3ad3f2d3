"""The split-bf16 GEMM kernels (csrc/token_gemm_split.hip, conv1x1_split.hip, conv3x3_split.hip) away
from unit-scale randn: mixed exponents, cancellation, post-ReLU and bf16-exact operands, operands at FLT_MAX (the clamp of
the first piece), folded-BatchNorm-like rows, power-of-two equivariance bit for bit, and x around the 2^-110 floor of the
split.  One small shape per kernel; the inputs, references and the accuracy rule are those of tests/split_gemm_cases.py."""
import pytest
import torch

import split_gemm_cases as S

pytestmark = pytest.mark.gpu

M_TOK, N_TOK = 531, 256          # 34 token tiles, the last with three live rows
C1 = dict(K=96, N=64, H=9, W=11, B=2)
C3 = dict(C=32, N=64, H=9, W=11, B=2)
KERNELS = ["token96", "token256", "conv1x1", "conv3x3"]
EPIS = {"token96": (S.BIAS, S.RELU), "token256": (S.BIAS, S.RELU), "conv1x1": (S.RAW, S.BIAS, S.RELU, S.RES),
        "conv3x3": (S.RAW, S.BIAS, S.RELU)}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


def _cuda(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def _shape(kernel):
    """(rows of x, K, N, taps) of a kernel's case."""
    if kernel.startswith("token"):
        return M_TOK, int(kernel[5:]), N_TOK, 1
    if kernel == "conv1x1":
        return C1["B"] * C1["H"] * C1["W"], C1["K"], C1["N"], 1
    return C3["B"] * C3["H"] * C3["W"], C3["C"], C3["N"], 9


def _place(kernel, x, w, b):
    """Generator output as the kernel's operands on the GPU."""
    if kernel.startswith("token"):
        return _cuda(x, S.as_w1x1(w), b)
    if kernel == "conv1x1":
        return _cuda(S.as_image(x, C1["B"], C1["H"], C1["W"]), S.as_w1x1(w), b)
    return _cuda(S.as_image(x, C3["B"], C3["H"], C3["W"]), S.as_w3x3(w), b)


def _residual(kernel, seed, stride=1):
    if kernel != "conv1x1":
        return None
    Ho, Wo = S.out_hw(C1["H"], C1["W"], stride)
    return S.extra((C1["B"], C1["N"], Ho, Wo), seed).cuda()


def _run(ops, kernel, x, w, b, r, epi, stride=1):
    """(out, ref, mag, fp32 comparator's out) of one epilogue."""
    relu = epi in (S.RELU, S.RES)
    bb = None if epi == S.RAW else b
    if kernel.startswith("token"):
        out = ops.token_linear(x, w, b, relu=relu)
        ref, mag, _ = S.token_ref(x, w, b, relu)
        return out, ref, mag, S.token_fp32(ops, x, w, b, relu)
    if kernel == "conv1x1":
        rr = r if epi == S.RES else None
        out = ops.conv1x1(x, w, bb, rr, relu, stride)
        ref, mag = S.conv1x1_ref(x, w, bb, rr, relu, stride)
        return out, ref, mag, S.conv1x1_fp32(ops, x, w, bb, rr, relu, stride)
    out = ops.conv3x3(x, w, bb, relu, stride)
    ref, mag = S.conv3x3_ref(x, w, bb, relu, stride)
    return out, ref, mag, S.conv3x3_fp32(x, w, bb, relu, stride)


def _op(ops, kernel, x, w, b, r, epi, stride=1):
    return _run(ops, kernel, x, w, b, r, epi, stride)[0]


@pytest.mark.parametrize("family", S.VALUE_FAMILIES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_value_families_under_the_accuracy_rule(ops, kernel, family):
    M, K, N, taps = _shape(kernel)
    x, w, b = _place(kernel, *S.operands(family, M, K, N, seed=11, taps=taps))
    r = _residual(kernel, 12)
    if r is not None and family == "fltmax":
        r = r * 2.0 ** 90  # a residual at the outputs' scale
    for epi in EPIS[kernel]:
        for stride in ((1,) if kernel.startswith("token") else (1, 2)):
            rs = _residual(kernel, 12, stride) if stride == 2 else r
            out, ref, mag, out32 = _run(ops, kernel, x, w, b, rs, epi, stride)
            e, e32 = S.rel_err(out, ref, mag), S.rel_err(out32, ref, mag)
            print(f"{kernel} {family} {epi} /{stride}: e {e:.3e} e32 {e32:.3e}")
            if family == "fltmax":
                assert torch.isfinite(out).all(), (epi, stride)
                assert torch.isfinite(out32).all(), (epi, stride)  # the rule is not vacuous
            assert S.rule(e, e32), (epi, stride, e, e32)


@pytest.mark.parametrize("a,b2", S.SCALINGS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_power_of_two_equivariance(ops, kernel, a, b2):
    """op(2^a x, 2^b w, 2^(a+b) bias, 2^(a+b) residual) == 2^(a+b) op(x, w, bias, residual), bit for bit."""
    M, K, N, taps = _shape(kernel)
    x, w, b = _place(kernel, *S.equivariance_operands(M, K, N, seed=21, taps=taps))
    r = _residual(kernel, 22)
    r = None if r is None else S.floor_at_2_pow_minus_10(r)
    sa, sb, so = 2.0 ** a, 2.0 ** b2, 2.0 ** (a + b2)
    for epi in EPIS[kernel]:
        base = _op(ops, kernel, x, w, b, r, epi)
        got = _op(ops, kernel, x * sa, w * sb, b * so, None if r is None else r * so, epi)
        assert torch.isfinite(got).all() and (got != 0).any()
        assert torch.equal(got, base * so), (epi, (got - base * so).abs().max().item())


@pytest.mark.parametrize("kernel", KERNELS)
def test_per_channel_power_of_two_equivariance(ops, kernel):
    """Row n of w and entry n of the bias (and the residual's channel n) scaled by 2^s_n: output channel n scales by 2^s_n."""
    M, K, N, taps = _shape(kernel)
    x, w, b = _place(kernel, *S.equivariance_operands(M, K, N, seed=31, taps=taps))
    r = _residual(kernel, 32)
    s = S.channel_exponents(N, seed=33).cuda()
    ws = w * s.view(-1, *([1] * (w.dim() - 1)))
    so = s if kernel.startswith("token") else s.view(1, -1, 1, 1)
    for epi in EPIS[kernel]:
        base = _op(ops, kernel, x, w, b, r, epi)
        got = _op(ops, kernel, x, ws, b * s, None if r is None else r * so, epi)
        assert torch.equal(got, base * so), epi


def _floor_case(ops, kernel, x_exp):
    M, K, N, taps = _shape(kernel)
    x, w, b = _place(kernel, *S.tiny_operands(x_exp, M, K, N, seed=41, taps=taps))
    epi = S.BIAS
    out, ref, mag, out32 = _run(ops, kernel, x, w, b, None, epi)
    e32 = S.rel_err(out32, ref, mag)
    # sum_k |w_k| per output: the error measure's denominator of an all-ones x (for 3x3, the taps inside the map)
    wsum = _run(ops, kernel, torch.ones_like(x), w, torch.zeros_like(b), None, epi)[2]
    return out, ref, mag, e32, wsum


@pytest.mark.parametrize("kernel", KERNELS)
def test_x_at_2_pow_minus_100_is_above_the_floor(ops, kernel):
    out, ref, mag, e32, _ = _floor_case(ops, kernel, -100)
    e = S.rel_err(out, ref, mag)
    print(f"{kernel} x at 2^-100: e {e:.3e} e32 {e32:.3e}")
    assert S.rule(e, e32), (e, e32)


@pytest.mark.parametrize("kernel", KERNELS)
def test_x_at_2_pow_minus_112_loses_at_most_the_subnormal_step(ops, kernel):
    """Below 2^-110 the third piece of x falls under bf16's subnormal step 2^-133: each element loses at most 2^-134 (§13),
    so an output at most 2^-134 sum_k |w_k| on top of the rule; the bound carries a factor 2."""
    out, ref, mag, e32, wsum = _floor_case(ops, kernel, -112)
    err = (out.double() - ref).abs()
    bound = (2.0 * e32 + S.RULE_FLOOR) * mag + 2.0 ** -133 * wsum
    worst = (err / bound).max().item()
    print(f"{kernel} x at 2^-112: max err / bound {worst:.3e}, e32 {e32:.3e}, "
          f"max err / (2^-134 sum|w|) {(err / (2.0 ** -134 * wsum)).max().item():.3e}, plain e {S.rel_err(out, ref, mag):.3e}")
    assert torch.isfinite(out).all()
    assert (err <= bound).all(), worst
