"""The selectable inference precision of the split-bf16 kernels on the GPU: ops.token_linear, conv1x1,
conv1x1_gn, conv3x3, conv3x3_stats and stem_conv_pool at "high" (two pieces, three products) and "medium" (one piece, one
product), at the smallest shapes at which each loader and epilogue can go wrong.

The rule per level is that of tests/split_precision_reference.py: e <= 2 e32 + floor, floor = 2^-14 / 2^-6, e and e32 the
measure and the fp32 comparator of tests/split_gemm_cases.py.  Small integers are held to the fp64 reference bit for bit;
bf16-exact random operands cannot be (an fp32 sum of K exact products rounds, at "highest" as well), so for them the test
is the level-independence: the same bits at all three levels.

The LayerNorm epilogue is measured on the normalised output in the forms of test_split_gemm_shapes_gpu.py, e <= 2 e32 + c1
and e <= c2 max|ref| sqrt(K), with c1 = 1e-6 and c2 = 3e-6 scaled by floor / 2^-23.

pos_rows = 17 needs a token count it divides, which 531 is not: the tiled-pos case runs at M = 51.

End to end, d = max |out - out_highest| / max |out_highest| per output tensor; the figures of the first run are in DESIGN §35."""
import functools
import math
import re

import pytest
import torch
import torch.nn.functional as F

import split_gemm_cases as S
import split_precision_reference as R
import stem_reference as ST

pytestmark = pytest.mark.gpu

LOW = ("high", "medium")
EXACT = ("ints", "bf16")
ACCURACY = ("randn", "wide", "cancel", "fltmax", "bnfold")
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def pkg(ops):
    import weed_instance_segmentation_amd as _pkg
    return _pkg


def _at(pkg, level, fn):
    with pkg.inference_precision(level):
        return fn()


def _all_levels(pkg, fn):
    return {level: _at(pkg, level, fn) for level in R.LEVELS}


def _cuda(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def _h_plus_m(h: torch.Tensor) -> torch.Tensor:
    """h + m with h the given bf16 values and m one bit, 2^(e - 10 - j) with e the exponent of h and j in 0 .. 5, of either
    sign: |m| <= 2^-10 |h|, the sum is exact in fp32, its split is (h, m, 0)."""
    g = torch.Generator(device=h.device).manual_seed(int(h.numel()))
    _, ex = torch.frexp(h)  # h = mant 2^ex, mant in [0.5, 1)
    j = torch.randint(0, 6, h.shape, generator=g, device=h.device)
    sign = torch.randint(0, 2, h.shape, generator=g, device=h.device).float() * 2 - 1
    one_bit = ((ex.to(torch.int32) - 11 - j.to(torch.int32) + 127) << 23).view(torch.float32)  # 2^(ex - 11 - j), exactly
    m = torch.where(h == 0, torch.zeros_like(h), sign * one_bit)
    x = h + m
    p = R.split_pieces(x, 3)
    assert torch.equal(p[0], h) and torch.equal(p[1], m) and not p[2].any()
    return x


def _bf16(t):
    return t.bfloat16().float()


def _errors_ordered(outs, ref, mag, what):
    e = {level: S.rel_err(outs[level], ref, mag) for level in R.LEVELS}
    print(f"{what}: e highest {e['highest']:.3e} high {e['high']:.3e} medium {e['medium']:.3e}")
    assert not torch.equal(outs["highest"], outs["high"]) and not torch.equal(outs["high"], outs["medium"]), what
    assert not torch.equal(outs["highest"], outs["medium"]), what
    assert e["medium"] > e["high"] > e["highest"], (what, e)


def _sentinel_survives(call, *bufs):
    """A refused call returns non-zero and launches nothing: the buffers keep their sentinel."""
    for t in bufs:
        t.fill_(-7.0)
    rc = call()
    torch.cuda.synchronize()
    return rc != 0 and all(bool((t == -7.0).all()) for t in bufs)


# ================================================================================================================ token
TOKEN_KN = [(32, 256), (96, 288), (288, 1024)]
TOKEN_M = (1, 17, 531)
LN_KN = [(32, 256), (96, 288)]


@functools.lru_cache(maxsize=None)
def _tok(family, M, K, N):
    """x (M, K), w (N, K), bias on the GPU, shared and never written."""
    x, w, b = S.operands(family, M, K, N, seed=M + 3 * K + N)
    return _cuda(x, S.as_w1x1(w), b)


@functools.lru_cache(maxsize=None)
def _tok_ref(family, M, K, N, relu):
    x, w, b = _tok(family, M, K, N)
    ref, mag, _ = S.token_ref(x, w, b, relu)
    return ref, mag, (None if family == "ints" else S.rel_err(S.token_fp32(_OPS[0], x, w, b, relu), ref, mag))


_OPS = [None]  # the ops module for the cached comparators


@functools.lru_cache(maxsize=None)
def _ln(family, M, N, res, rows):
    ints = family == "ints"
    seed = M + N + rows
    gamma, beta = S.extra((N,), seed + 1), S.extra((N,), seed + 2)
    r = S.extra((M, N), seed + 3, ints) if res else None
    pe = S.extra((rows, N), seed + 4, ints) if rows else None
    gamma, beta, r, pe = _cuda(gamma, beta, r, pe)
    return (gamma, beta, 1e-5), r, pe


@pytest.mark.parametrize("K,N", TOKEN_KN)
@pytest.mark.parametrize("level", LOW)
def test_token_bias_relu_and_out_group(ops, pkg, level, K, N):
    _OPS[0] = ops
    for M in TOKEN_M:
        for family in EXACT + ACCURACY:
            x, w, b = _tok(family, M, K, N)
            ws = ops.split_weight(w)
            for relu in (False, True):
                what = f"token {level} M={M} K={K} N={N} relu={relu} {family}"
                run = lambda: ops.token_linear(x, w, b, relu=relu, w_split=ws)
                out = _at(pkg, level, run)
                ref, mag, e32 = _tok_ref(family, M, K, N, relu)
                if family in EXACT:
                    outs = _all_levels(pkg, run)
                    assert torch.equal(outs["high"], outs["highest"]) and torch.equal(outs["medium"], outs["highest"]), what
                    if family == "ints":
                        assert torch.equal(out, ref.float()), what
                    else:  # the bits of "highest": its rule
                        assert S.rule(S.rel_err(out, ref, mag), e32), what
                else:
                    e = S.rel_err(out, ref, mag)
                    print(f"{what}: e {e:.3e} e32 {e32:.3e}")
                    assert R.rule(e, e32, level), (what, e, e32)
                    assert torch.isfinite(out).all(), what
                for G in sorted({N} | ({36} if N % 36 == 0 else set())):
                    got = _at(pkg, level, lambda: ops.token_linear(x, w, b, relu=relu, out_group=G, w_split=ws))
                    assert got.shape == (N // G, M, G) and torch.equal(got, S.group_major(out, G)), (what, G)


@pytest.mark.parametrize("K,N", LN_KN)
@pytest.mark.parametrize("level", LOW)
def test_token_layernorm_and_pos(ops, pkg, level, K, N):
    scale = R.FLOORS[level] / R.FLOORS["highest"]
    for M in (1, 17, 51, 531):
        for family in ("ints", "randn"):
            x, w, b = _tok(family, M, K, N)
            ws = ops.split_weight(w)
            for res in (False, True):
                for rows in sorted({M} | ({17} if M % 17 == 0 else set())):
                    what = f"token+ln {level} M={M} K={K} N={N} res={res} rows={rows} {family}"
                    lnp, r, pe = _ln(family, M, N, res, rows)
                    run = lambda: ops.token_linear(x, w, b, residual=r, ln=lnp, pos=pe, w_split=ws)
                    out, outp = _at(pkg, level, run)
                    ref, _, _ = S.token_ref(x, w, b, residual=r, ln=lnp)
                    out32 = S.token_fp32(ops, x, w, b, residual=r, ln=lnp)
                    e, e32 = (out.double() - ref).abs().max().item(), (out32.double() - ref).abs().max().item()
                    print(f"{what}: e {e:.3e} e32 {e32:.3e}")
                    assert torch.isfinite(out).all(), what
                    assert e <= 2 * e32 + 1e-6 * scale, (what, e, e32)
                    assert e <= 3e-6 * scale * ref.abs().max().item() * math.sqrt(K), (what, e)
                    assert torch.equal(outp, out + pe.repeat(M // rows, 1)), what  # one fp32 add of token t's row t % rows
                    assert torch.equal(_at(pkg, level, lambda: ops.token_linear(x, w, b, residual=r, ln=lnp, w_split=ws)), out)
                    if family == "ints":  # the normalised value is exact at every level, so the epilogue sees the same bits
                        assert torch.equal(out, _at(pkg, "highest", run)[0]), what


@pytest.mark.parametrize("K,N", TOKEN_KN)
def test_token_medium_is_highest_on_the_h_pieces(ops, pkg, K, N):
    for M in TOKEN_M:
        for family in ("randn", "wide"):
            x, w, b = _tok(family, M, K, N)
            xh, wh = R.h_piece(x), R.h_piece(w)
            variants = [dict(relu=False), dict(relu=True), dict(out_group=N)]
            if N <= 288:
                lnp, r, pe = _ln("randn", M, N, True, M)
                variants += [dict(residual=r, ln=lnp), dict(residual=r, ln=lnp, pos=pe)]
            for kw in variants:
                got = _at(pkg, "medium", lambda: ops.token_linear(x, w, b, **kw))
                want = _at(pkg, "highest", lambda: ops.token_linear(xh, wh, b, **kw))
                got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
                assert all(torch.equal(g, t) for g, t in zip(got, want)), (M, K, N, family, sorted(kw))


@pytest.mark.parametrize("K,N", TOKEN_KN)
def test_token_high_is_neither_highest_nor_medium(ops, pkg, K, N):
    _OPS[0] = ops
    M = 531
    x, w, b = _tok("randn", M, K, N)
    ref, mag, _ = _tok_ref("randn", M, K, N, False)
    _errors_ordered(_all_levels(pkg, lambda: ops.token_linear(x, w, b)), ref, mag, f"token K={K} N={N}")
    for x2, w2 in ((_h_plus_m(_bf16(x)), _bf16(w)), (_bf16(x), _h_plus_m(_bf16(w)))):
        outs = _all_levels(pkg, lambda: ops.token_linear(x2, w2, b, relu=True))
        assert torch.equal(outs["high"], outs["highest"]) and not torch.equal(outs["medium"], outs["highest"])


@pytest.mark.parametrize("K,N", TOKEN_KN)
@pytest.mark.parametrize("level", LOW)
def test_token_determinism_and_nan(ops, pkg, level, K, N):
    M = 531
    x, w, b = _tok("randn", M, K, N)
    ws = ops.split_weight(w)
    cuts = ((5, 6), (7, 300), (494, 531))  # none on a 16-token tile border
    with pkg.inference_precision(level):
        full = ops.token_linear(x, w, b, relu=True, w_split=ws)
        assert torch.equal(ops.token_linear(x, w, b, relu=True, w_split=ws), full)
        assert torch.equal(ops.token_linear(x, w, b, relu=True), full)  # an uncached split is the same split
        for r0, r1 in cuts:
            assert torch.equal(ops.token_linear(x[r0:r1], w, b, relu=True, w_split=ws), full[r0:r1]), (r0, r1)
        kw = {}
        if N <= 288:
            lnp, r, _ = _ln("randn", M, N, True, M)
            kw = dict(ln=lnp)
            full = ops.token_linear(x, w, b, residual=r, ln=lnp, w_split=ws)
            for r0, r1 in cuts:
                assert torch.equal(ops.token_linear(x[r0:r1], w, b, residual=r[r0:r1], ln=lnp, w_split=ws), full[r0:r1]), (r0, r1)
        for row, col, bad in ((0, 0, NAN), (17, K - 1, NAN), (M - 1, K // 2, float("inf"))):
            xn = x.clone()
            xn[row, col] = bad
            fin = torch.isfinite(ops.token_linear(xn, w, b, w_split=ws, **kw))
            want = torch.ones_like(fin)
            want[row] = False
            assert torch.equal(fin, want), (row, col, bad)


# ============================================================================================================== conv1x1
C1_KN = [(32, 64), (96, 256)]
C1_MAPS = [(1, 1), (9, 11), (37, 41)]
C1_EPIS = (S.RAW, S.BIAS, S.RELU, S.RES)


@functools.lru_cache(maxsize=None)
def _c1(family, B, K, N, H, W, stride):
    seed = K + 7 * N + 31 * H + W + stride + B
    x, w, b = S.operands(family, B * H * W, K, N, seed)
    Ho, Wo = S.out_hw(H, W, stride)
    r = S.extra((B, N, Ho, Wo), seed + 1, family == "ints")
    return _cuda(S.as_image(x, B, H, W), S.as_w1x1(w), b, r)


def _c1_args(epi, b, r):
    return (None if epi == S.RAW else b), (r if epi == S.RES else None), epi in (S.RELU, S.RES)


@functools.lru_cache(maxsize=None)
def _c1_ref(family, B, K, N, H, W, stride, epi):
    x, w, b, r = _c1(family, B, K, N, H, W, stride)
    bb, rr, relu = _c1_args(epi, b, r)
    ref, mag = S.conv1x1_ref(x, w, bb, rr, relu, stride)
    return ref, mag, (None if family == "ints" else S.rel_err(S.conv1x1_fp32(_OPS[0], x, w, bb, rr, relu, stride), ref, mag))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K,N", C1_KN)
@pytest.mark.parametrize("level", LOW)
def test_conv1x1_epilogues(ops, pkg, level, K, N, B):
    _OPS[0] = ops
    for H, W in C1_MAPS:
        for stride in (1, 2):
            for family in EXACT + ACCURACY:
                x, w, b, r = _c1(family, B, K, N, H, W, stride)
                ws = ops.split_weight(w)
                for epi in C1_EPIS:
                    bb, rr, relu = _c1_args(epi, b, r)
                    what = f"conv1x1 {level} K={K} N={N} {H}x{W}/{stride} B={B} {epi} {family}"
                    run = lambda: ops.conv1x1(x, w, bb, rr, relu, stride, w_split=ws)
                    out = _at(pkg, level, run)
                    assert out.shape == (B, N, *S.out_hw(H, W, stride))
                    ref, mag, e32 = _c1_ref(family, B, K, N, H, W, stride, epi)
                    if family in EXACT:
                        outs = _all_levels(pkg, run)
                        assert torch.equal(outs["high"], outs["highest"]) and torch.equal(outs["medium"], outs["highest"]), what
                        if family == "ints":
                            assert torch.equal(out, ref.float()), what
                        else:  # the bits of "highest": its rule
                            assert S.rule(S.rel_err(out, ref, mag), e32), what
                    else:
                        e = S.rel_err(out, ref, mag)
                        print(f"{what}: e {e:.3e} e32 {e32:.3e}")
                        assert R.rule(e, e32, level), (what, e, e32)
                        assert torch.isfinite(out).all(), what


@pytest.mark.parametrize("K,N", C1_KN)
def test_conv1x1_medium_is_highest_on_the_h_pieces(ops, pkg, K, N):
    for H, W in C1_MAPS:
        for stride in (1, 2):
            for family in ("randn", "wide"):
                x, w, b, r = _c1(family, 3, K, N, H, W, stride)
                xh, wh = R.h_piece(x), R.h_piece(w)
                for epi in C1_EPIS:
                    bb, rr, relu = _c1_args(epi, b, r)
                    got = _at(pkg, "medium", lambda: ops.conv1x1(x, w, bb, rr, relu, stride))
                    want = _at(pkg, "highest", lambda: ops.conv1x1(xh, wh, bb, rr, relu, stride))
                    assert torch.equal(got, want), (K, N, H, W, stride, family, epi)


@pytest.mark.parametrize("K,N", C1_KN)
def test_conv1x1_high_is_neither_highest_nor_medium(ops, pkg, K, N):
    _OPS[0] = ops
    B, H, W, stride = 3, 37, 41, 1
    x, w, b, r = _c1("randn", B, K, N, H, W, stride)
    ref, mag, _ = _c1_ref("randn", B, K, N, H, W, stride, S.BIAS)
    _errors_ordered(_all_levels(pkg, lambda: ops.conv1x1(x, w, b)), ref, mag, f"conv1x1 K={K} N={N}")
    for x2, w2 in ((_h_plus_m(_bf16(x)), _bf16(w)), (_bf16(x), _h_plus_m(_bf16(w)))):
        outs = _all_levels(pkg, lambda: ops.conv1x1(x2, w2, b, r, True))
        assert torch.equal(outs["high"], outs["highest"]) and not torch.equal(outs["medium"], outs["highest"])


@pytest.mark.parametrize("K,N", C1_KN)
@pytest.mark.parametrize("level", LOW)
def test_conv1x1_determinism_configurations_sampling_and_nan(ops, pkg, level, K, N):
    from weed_instance_segmentation_amd import _lib
    lib, B, pieces = _lib.load(), 3, R.PIECES[level]
    with pkg.inference_precision(level):
        for (H, W), stride in (((1, 1), 1), ((9, 11), 2), ((37, 41), 2), ((37, 41), 1)):
            x, w, b, r = _c1("randn", B, K, N, H, W, stride)
            ws = ops.split_weight(w)
            fits = 0
            for epi in (S.RAW, S.RES):
                bb, rr, relu = _c1_args(epi, b, r)
                auto = ops.conv1x1(x, w, bb, rr, relu, stride, w_split=ws)
                assert torch.equal(ops.conv1x1(x, w, bb, rr, relu, stride, w_split=ws), auto)
                for i in range(B):
                    ri = None if rr is None else rr[i:i + 1].contiguous()
                    assert torch.equal(ops.conv1x1(x[i:i + 1].contiguous(), w, bb, ri, relu, stride, w_split=ws), auto[i:i + 1])
                for ci, nt in enumerate(S.NT):
                    if N % nt == 0:
                        fits += 1
                        assert torch.equal(ops.conv1x1(x, w, bb, rr, relu, stride, w_split=ws, config=ci), auto), (epi, ci)
                    else:  # refused through the C ABI
                        out = torch.empty_like(auto)
                        assert _sentinel_survives(lambda: lib.wm2f_conv1x1_split_fwd_p(
                            ops._p(x), ops._p(ws), ops._p(bb), ops._p(rr), ops._p(out), B, K, N, H, W, stride, 1 if relu else 0,
                            ci, pieces, ops._stream(x)), out), (epi, ci)
                        with pytest.raises(_lib.Wm2fError):
                            ops.conv1x1(x, w, bb, rr, relu, stride, w_split=ws, config=ci)
            assert fits >= 2  # the 64-channel tile divides every N
            clean = ops.conv1x1(x, w, b, r, True, stride, w_split=ws)
            if stride == 2:  # the pixels the stride skips are never read
                xn = x.clone()
                xn[:, :, 1::2, :] = NAN
                xn[:, :, :, 1::2] = NAN
                assert torch.equal(ops.conv1x1(xn, w, b, r, True, 2, w_split=ws), clean)
            Ho, Wo = S.out_hw(H, W, stride)
            ho, wo = Ho // 2, Wo - 1
            xn = x.clone()
            xn[B - 1, K // 2, stride * ho, stride * wo] = NAN
            fin = torch.isfinite(ops.conv1x1(xn, w, b, r, True, stride, w_split=ws))
            want = torch.ones_like(fin)
            want[B - 1, :, ho, wo] = False
            assert torch.equal(fin, want), (H, W, stride)


# ============================================================================================================== conv3x3
C3_CN = [(32, 64), (96, 192)]
C3_MAPS = [(1, 1), (2, 3), (17, 1), (33, 31)]
C3_EPIS = (S.RAW, S.BIAS, S.RELU)


@functools.lru_cache(maxsize=None)
def _c3(family, B, C, N, H, W):
    x, w, b = S.operands(family, B * H * W, C, N, C + 7 * N + 31 * H + W + B, taps=9)
    return _cuda(S.as_image(x, B, H, W), S.as_w3x3(w), b)


@functools.lru_cache(maxsize=None)
def _c3_ref(family, B, C, N, H, W, stride, epi):
    x, w, b = _c3(family, B, C, N, H, W)
    bb, relu = (None if epi == S.RAW else b), epi == S.RELU
    ref, mag = S.conv3x3_ref(x, w, bb, relu, stride)
    return ref, mag, (None if family == "ints" else S.rel_err(S.conv3x3_fp32(x, w, bb, relu, stride), ref, mag))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C,N", C3_CN)
@pytest.mark.parametrize("level", LOW)
def test_conv3x3_epilogues(ops, pkg, level, C, N, B):
    for H, W in C3_MAPS:
        for stride in (1, 2):
            for family in EXACT + ACCURACY:
                x, w, b = _c3(family, B, C, N, H, W)
                ws = ops.split_weight_3x3(w)
                for epi in C3_EPIS:
                    bb, relu = (None if epi == S.RAW else b), epi == S.RELU
                    what = f"conv3x3 {level} C={C} N={N} {H}x{W}/{stride} B={B} {epi} {family}"
                    run = lambda: ops.conv3x3(x, w, bb, relu, stride, w_split=ws)
                    out = _at(pkg, level, run)
                    assert out.shape == (B, N, *S.out_hw(H, W, stride))
                    ref, mag, e32 = _c3_ref(family, B, C, N, H, W, stride, epi)
                    if family in EXACT:
                        outs = _all_levels(pkg, run)
                        assert torch.equal(outs["high"], outs["highest"]) and torch.equal(outs["medium"], outs["highest"]), what
                        if family == "ints":
                            assert torch.equal(out, ref.float()), what
                        else:  # the bits of "highest": its rule
                            assert S.rule(S.rel_err(out, ref, mag), e32), what
                    else:
                        e = S.rel_err(out, ref, mag)
                        print(f"{what}: e {e:.3e} e32 {e32:.3e}")
                        assert R.rule(e, e32, level), (what, e, e32)
                        assert torch.isfinite(out).all(), what


@pytest.mark.parametrize("C,N", C3_CN)
def test_conv3x3_medium_is_highest_on_the_h_pieces(ops, pkg, C, N):
    for H, W in C3_MAPS:
        for stride in (1, 2):
            for family in ("randn", "wide"):
                x, w, b = _c3(family, 3, C, N, H, W)
                xh, wh = R.h_piece(x), R.h_piece(w)
                for epi in C3_EPIS:
                    bb, relu = (None if epi == S.RAW else b), epi == S.RELU
                    got = _at(pkg, "medium", lambda: ops.conv3x3(x, w, bb, relu, stride))
                    want = _at(pkg, "highest", lambda: ops.conv3x3(xh, wh, bb, relu, stride))
                    assert torch.equal(got, want), (C, N, H, W, stride, family, epi)


@pytest.mark.parametrize("C,N", C3_CN)
def test_conv3x3_high_is_neither_highest_nor_medium(ops, pkg, C, N):
    B, H, W = 3, 33, 31
    x, w, b = _c3("randn", B, C, N, H, W)
    ref, mag, _ = _c3_ref("randn", B, C, N, H, W, 1, S.BIAS)
    _errors_ordered(_all_levels(pkg, lambda: ops.conv3x3(x, w, b)), ref, mag, f"conv3x3 C={C} N={N}")
    for x2, w2 in ((_h_plus_m(_bf16(x)), _bf16(w)), (_bf16(x), _h_plus_m(_bf16(w)))):
        outs = _all_levels(pkg, lambda: ops.conv3x3(x2, w2, b, True, 2))
        assert torch.equal(outs["high"], outs["highest"]) and not torch.equal(outs["medium"], outs["highest"])


@pytest.mark.parametrize("C,N", C3_CN)
@pytest.mark.parametrize("level", LOW)
def test_conv3x3_determinism_configurations_and_nan(ops, pkg, level, C, N):
    from weed_instance_segmentation_amd import _lib
    lib, B, pieces = _lib.load(), 3, R.PIECES[level]
    with pkg.inference_precision(level):
        for (H, W), stride in (((1, 1), 1), ((2, 3), 2), ((17, 1), 2), ((33, 31), 2), ((33, 31), 1)):
            x, w, b = _c3("randn", B, C, N, H, W)
            ws = ops.split_weight_3x3(w)
            for epi in (S.RAW, S.RELU):
                bb, relu = (None if epi == S.RAW else b), epi == S.RELU
                auto = ops.conv3x3(x, w, bb, relu, stride, w_split=ws)
                assert torch.equal(ops.conv3x3(x, w, bb, relu, stride, w_split=ws), auto)
                for i in range(B):
                    assert torch.equal(ops.conv3x3(x[i:i + 1].contiguous(), w, bb, relu, stride, w_split=ws), auto[i:i + 1])
                for ci, nt in enumerate(S.NT):
                    if N % nt == 0:
                        assert torch.equal(ops.conv3x3(x, w, bb, relu, stride, w_split=ws, config=ci), auto), (epi, ci)
                    else:
                        out = torch.empty_like(auto)
                        assert _sentinel_survives(lambda: lib.wm2f_conv3x3_split_fwd_p(
                            ops._p(x), ops._p(ws), ops._p(bb), ops._p(out), B, C, N, H, W, stride, 1 if relu else 0, ci, pieces,
                            ops._stream(x)), out), (epi, ci)
                        with pytest.raises(_lib.Wm2fError):
                            ops.conv3x3(x, w, bb, relu, stride, w_split=ws, config=ci)
            # a NaN gives non-finite outputs at exactly the outputs whose window holds it
            bi, y, xx = B - 1, H // 2, W - 1
            xn = x.clone()
            xn[bi, C // 2, y, xx] = NAN
            hit = torch.zeros(B, 1, H, W, device="cuda", dtype=torch.float64)
            hit[bi, 0, y, xx] = 1.0
            want = F.conv2d(hit, torch.ones(1, 1, 3, 3, device="cuda", dtype=torch.float64), None, stride, 1) > 0
            fin = torch.isfinite(ops.conv3x3(xn, w, b, True, stride, w_split=ws))
            assert torch.equal(fin, ~want.expand_as(fin)), (H, W, stride)


# ================================================================================================================= stem
STEM_CASES = [(H, W, cin, B) for (H, W) in ST.MAPS for cin in ST.CINS for B in ST.BATCHES]


@pytest.mark.parametrize("level", LOW)
def test_stem_exactness_accuracy_and_determinism(ops, pkg, level):
    for H, W, cin, B in STEM_CASES:
        x, w, b, ref, _ = ST.case("ints", B, cin, H, W)
        xd, wd, bd = _cuda(x, w, b)
        outs = _all_levels(pkg, lambda: ops.stem_conv_pool(xd, wd, bd))
        assert torch.equal(outs[level].cpu().double(), ref), (H, W, cin, B)
        assert torch.equal(outs["high"], outs["highest"]) and torch.equal(outs["medium"], outs["highest"])
        for family in ("randn", "wide", "fltmax"):
            x, w, b, ref, mag = ST.case(family, B, cin, H, W)
            xd, wd, bd = _cuda(x, w, b)
            ws = ops.split_weight_stem(wd)
            out = _at(pkg, level, lambda: ops.stem_conv_pool(xd, wd, bd, w_split=ws))
            e, e32 = S.rel_err(out.cpu(), ref, mag), S.rel_err(ST.stem_fp32(xd, wd, bd).cpu(), ref, mag)
            print(f"stem {level} {family} {H}x{W} Cin={cin} B={B}: e {e:.3e} e32 {e32:.3e}")
            assert R.rule(e, e32, level), (family, H, W, cin, B, e, e32)
            assert torch.isfinite(out).all()
            if family == "randn":
                xb, wb = _bf16(xd), _bf16(wd)  # bf16-exact operands: the same bits at every level
                o = _all_levels(pkg, lambda: ops.stem_conv_pool(xb, wb, bd))
                assert torch.equal(o["high"], o["highest"]) and torch.equal(o["medium"], o["highest"])
                with pkg.inference_precision(level):
                    assert torch.equal(ops.stem_conv_pool(xd, wd, bd, w_split=ws), out)
                    assert torch.equal(ops.stem_conv_pool(xd, wd, bd), out)
                    for i in range(B):
                        assert torch.equal(ops.stem_conv_pool(xd[i:i + 1].contiguous(), wd, bd, w_split=ws), out[i:i + 1]), i
                    for grid in (1, 2):
                        assert torch.equal(ops.stem_conv_pool(xd, wd, bd, w_split=ws, grid=grid), out), grid


def test_stem_medium_is_highest_on_the_h_pieces(ops, pkg):
    for H, W, cin, B in STEM_CASES:
        for family in ("randn", "wide"):
            x, w, b, _, _ = ST.case(family, B, cin, H, W)
            xd, wd, bd = _cuda(x, w, b)
            got = _at(pkg, "medium", lambda: ops.stem_conv_pool(xd, wd, bd))
            want = _at(pkg, "highest", lambda: ops.stem_conv_pool(R.h_piece(xd), R.h_piece(wd), bd))
            assert torch.equal(got, want), (H, W, cin, B, family)


def test_stem_high_is_neither_highest_nor_medium(ops, pkg):
    for cin in ST.CINS:
        H, W = ST.MAPS[-2]
        x, w, b, ref, mag = ST.case("randn", 3, cin, H, W)
        xd, wd, bd = _cuda(x, w, b)
        outs = {k: v.cpu() for k, v in _all_levels(pkg, lambda: ops.stem_conv_pool(xd, wd, bd)).items()}
        _errors_ordered(outs, ref, mag, f"stem Cin={cin}")
        for x2, w2 in ((_h_plus_m(_bf16(xd)), _bf16(wd)), (_bf16(xd), _h_plus_m(_bf16(wd)))):
            o = _all_levels(pkg, lambda: ops.stem_conv_pool(x2, w2, bd))
            assert torch.equal(o["high"], o["highest"]) and not torch.equal(o["medium"], o["highest"])


@pytest.mark.parametrize("level", LOW)
def test_stem_nonfinite_exactly_in_the_receptive_field(ops, pkg, level):
    for H, W, cin, B in STEM_CASES:
        x, w, b, _, _ = ST.case("randn", B, cin, H, W)
        xd, wd, bd = _cuda(x, w, b)
        ws = ops.split_weight_stem(wd)
        for k, (y, xx) in enumerate(((0, 0), (H - 1, W - 1), (H // 2, W // 2))):
            bi, c = k % B, k % cin
            bad = xd.clone()
            bad[bi, c, y, xx] = (NAN, float("inf"), -float("inf"))[k % 3]
            want = ST.nonfinite_mask(B, H, W, [(bi, y, xx)])
            fin = torch.isfinite(_at(pkg, level, lambda: ops.stem_conv_pool(bad, wd, bd, w_split=ws))).cpu()
            assert torch.equal(fin, ~want[:, None].expand_as(fin)), (H, W, cin, B, y, xx)


# ===================================================================================== statistics, normalised operand
GN_MAPS = [(1, 1), (9, 11), (33, 31)]
CPGS = (4, 8, 16)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _ternary(shape, g):
    return torch.randint(-1, 2, shape, generator=g, device="cuda").float()


def _ref_stats(out, G):
    v = out.double().reshape(out.shape[0], G, -1)
    return torch.stack((v.sum(-1), (v * v).sum(-1)), -1)


@pytest.mark.parametrize("level", LOW)
def test_statistics_epilogues(ops, pkg, level):
    """The stored output is the plain entry point's at the same level; ternary operands (K = 32: every fp32 partial of a
    workgroup is an exact integer) give statistics equal to fp64 sums of the stored output."""
    K, N, B = 32, 64, 3
    with pkg.inference_precision(level):
        for i, (H, W) in enumerate(GN_MAPS):
            for family in ("ternary", "randn"):
                g = _gen(100 + i)
                if family == "ternary":
                    x, w1, w3 = _ternary((B, K, H, W), g), _ternary((N, K, 1, 1), g), _ternary((N, K, 3, 3), g)
                    bias = _ternary((N,), g)
                    w3[:, :, 0::2, 0::2] = 0.0  # five of the nine taps: |v| <= 160, 512 squares stay below 2^24
                else:
                    x = torch.randn(B, K, H, W, generator=g, device="cuda")
                    w1 = torch.randn(N, K, 1, 1, generator=g, device="cuda") / math.sqrt(K)
                    w3 = torch.randn(N, K, 3, 3, generator=g, device="cuda") / math.sqrt(9 * K)
                    bias = torch.randn(N, generator=g, device="cuda")
                for stride in (1, 2):
                    for b in (None, bias):
                        want = ops.conv1x1(x, w1, b, stride=stride)
                        for cpg in CPGS:
                            out, stats = ops.conv1x1_gn(x, w1, b, stride=stride, stats_groups=N // cpg)
                            assert torch.equal(out, want), (H, W, family, stride, cpg)
                            if family == "ternary":
                                assert torch.equal(stats, _ref_stats(out, N // cpg)), (H, W, stride, cpg)
                    want = ops.conv3x3(x, w3, stride=stride)
                    for cpg in CPGS:
                        out, stats = ops.conv3x3_stats(x, w3, N // cpg, stride=stride)
                        assert torch.equal(out, want), (H, W, family, stride, cpg)
                        if family == "ternary":
                            assert torch.equal(stats, _ref_stats(out, N // cpg)), (H, W, stride, cpg)


@pytest.mark.parametrize("relu", [False, True], ids=["affine", "relu"])
@pytest.mark.parametrize("level", LOW)
def test_normalised_operand(ops, pkg, level, relu):
    """The fused call against the apply pass on a copy followed by ops.conv1x1 at the same level, bit for bit."""
    N, eps, B = 64, 1e-5, 3
    with pkg.inference_precision(level):
        for K in (32, 96):
            for cpg in CPGS if K == 32 else (4, 8):
                G = K // cpg
                for i, (H, W) in enumerate(GN_MAPS):
                    g = _gen(3000 * K + 100 * G + 10 * i)
                    x = torch.randn(B, K, H, W, generator=g, device="cuda") * 3.0 + 0.5
                    w = torch.randn(N, K, 1, 1, generator=g, device="cuda") / math.sqrt(K)
                    b = torch.randn(N, generator=g, device="cuda")
                    gamma, beta = torch.randn(K, generator=g, device="cuda"), torch.randn(K, generator=g, device="cuda")
                    stats = _ref_stats(x, G)
                    two = ops.group_norm_act_from_stats_(x.clone(), stats, G, gamma, beta, eps, relu=relu)
                    want = ops.conv1x1(two, w, b)
                    got = ops.conv1x1_gn(x, w, b, norm=(stats, G, gamma, beta, eps, relu))
                    assert torch.equal(got, want), (K, G, H, W, relu)
    # and the levels differ on this route too
    outs = _all_levels(pkg, lambda: ops.conv1x1_gn(x, w, b, norm=(stats, G, gamma, beta, eps, relu)))
    assert not torch.equal(outs["highest"], outs["high"]) and not torch.equal(outs["high"], outs["medium"])


# ====================================================================================================== bad `pieces` values
def test_bad_pieces_values_are_refused_before_any_launch(ops):
    """pieces = 0 and 4 through the C ABI: an error, nothing launched, the outputs keep their sentinel."""
    from weed_instance_segmentation_amd import _lib
    lib = _lib.load()
    g = _gen(5)
    p, s = ops._p, ops._stream(torch.zeros(1, device="cuda"))
    M, K, N, H, W = 48, 32, 256, 6, 8
    xt, wt, bt = torch.randn(M, K, generator=g, device="cuda"), torch.randn(N, K, generator=g, device="cuda"), torch.randn(N, device="cuda")
    wst, ot = ops.split_weight(wt), torch.empty(M, N, device="cuda")
    xc = torch.randn(1, K, H, W, generator=g, device="cuda")
    w3 = torch.randn(N, K, 3, 3, generator=g, device="cuda")
    ws3, oc = ops.split_weight_3x3(w3), torch.empty(1, N, H, W, device="cuda")
    st = torch.empty(1, N // 8, 2, device="cuda", dtype=torch.float64)
    xs, wsm = torch.randn(1, 3, 16, 16, generator=g, device="cuda"), torch.randn(64, 3, 7, 7, generator=g, device="cuda")
    wss, bs, os_ = ops.split_weight_stem(wsm), torch.randn(64, device="cuda"), torch.empty(1, 64, 4, 4, device="cuda")
    N0 = ops._p(None)
    calls = {
        "wm2f_token_linear_split_fwd_p": (lambda q: lib.wm2f_token_linear_split_fwd_p(
            p(xt), p(wst), p(bt), N0, N0, N0, N0, p(ot), N0, M, K, N, 0, 0, 0.0, 0, q, s), (ot,)),
        "wm2f_conv1x1_split_fwd_p": (lambda q: lib.wm2f_conv1x1_split_fwd_p(
            p(xc), p(wst), p(bt), N0, p(oc), 1, K, N, H, W, 1, 0, -1, q, s), (oc,)),
        "wm2f_conv1x1_split_gn_fwd_p": (lambda q: lib.wm2f_conv1x1_split_gn_fwd_p(
            p(xc), p(wst), p(bt), p(oc), p(st), N // 8, N0, N0, N0, 0, 0.0, 0, 1, K, N, H, W, 1, -1, q, s), (oc, st)),
        "wm2f_conv3x3_split_fwd_p": (lambda q: lib.wm2f_conv3x3_split_fwd_p(
            p(xc), p(ws3), p(bt), p(oc), 1, K, N, H, W, 1, 0, -1, q, s), (oc,)),
        "wm2f_conv3x3_split_stats_fwd_p": (lambda q: lib.wm2f_conv3x3_split_stats_fwd_p(
            p(xc), p(ws3), p(oc), p(st), N // 8, 1, K, N, H, W, 1, -1, q, s), (oc, st)),
        "wm2f_stem7x7_pool_fwd_p": (lambda q: lib.wm2f_stem7x7_pool_fwd_p(
            p(xs), p(wss), p(bs), p(os_), 1, 3, 64, 16, 16, 0, q, s), (os_,)),
    }
    for name, (call, bufs) in calls.items():
        for q in (0, 4, -1):
            assert _sentinel_survives(lambda: call(q), *bufs), (name, q)
            assert lib.wm2f_last_error() and b"pieces" in lib.wm2f_last_error(), name
        for q in (1, 2, 3):  # and the same arguments are accepted at the built values
            assert call(q) == 0, (name, q, lib.wm2f_last_error())
    torch.cuda.synchronize()


# =========================================================================================================== end to end
SPLIT_TAG = re.compile(r"^(token_linear_.*_split|conv1x1_K|conv3x3_C|stem7x7_pool)")
LEVEL_TAG = re.compile(r"_p[12]$")


@pytest.fixture(scope="module")
def modules(ops):
    """The pixel decoder at the benchmark's widths on 32^2 .. 4^2 maps (built as test_conv_groupnorm_fused_gpu.py builds
    it) and the ResNet stem with one bottleneck stage, with non-trivial norms."""
    from weed_instance_segmentation_amd import Mask2FormerConfig
    from weed_instance_segmentation_amd.backbone_resnet import Stage, _Embedder
    from weed_instance_segmentation_amd.modeling import Mask2FormerPixelDecoder
    torch.manual_seed(0)
    cfg = Mask2FormerConfig(num_labels=3, encoder_layers=2)
    dec = Mask2FormerPixelDecoder(cfg, [256, 512, 1024, 2048]).cuda().eval()
    stem, stage = _Embedder(3, 64).cuda().eval(), Stage(64, 256, 1, 2, False).cuda().eval()
    with torch.no_grad():
        for m in [*dec.modules(), *stem.modules(), *stage.modules()]:
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.normal_(1.0, 0.3)
                m.bias.normal_(0.0, 0.3)
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.normal_(1.0, 0.3)
                m.bias.normal_(0.0, 0.3)
                m.running_mean.normal_(0.0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
    g = _gen(11)
    feats = [torch.randn(2, c, s, s, generator=g, device="cuda") for c, s in ((256, 32), (512, 16), (1024, 8), (2048, 4))]
    image = torch.randn(2, 3, 64, 64, generator=g, device="cuda")

    def run():
        with torch.no_grad():
            mask, outs = dec(feats)
            res = stage(stem(image))
        return [t.float() for t in (mask, *outs, res)]

    return run


def test_end_to_end_routing(ops, pkg, modules):
    """Inside inference_precision("high") every split launch carries the level and none another; afterwards none does."""
    def tags():
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        try:
            modules()
            torch.cuda.synchronize()
        finally:
            ops.set_kernel_timer(None)
        return [t for t in timer.records if SPLIT_TAG.match(t)], {t: len(v) for t, v in timer.records.items()}

    with pkg.inference_precision("high"):
        inside, counts_in = tags()
    after, counts_after = tags()
    assert inside and all(t.endswith("_p2") for t in inside), inside
    assert after and not any(LEVEL_TAG.search(t) for t in after), after
    assert sorted(t[:-3] for t in inside) == sorted(after)  # the same sites
    assert {t[:-3]: n for t, n in counts_in.items() if t in inside} == {t: n for t, n in counts_after.items() if t in after}
    assert {k for t in after for k in ("token", "conv1x1", "conv3x3", "stem") if t.startswith(k)} == {"token", "conv1x1", "conv3x3", "stem"}
    with pkg.inference_precision("medium"):
        inside, _ = tags()
    assert inside and all(t.endswith("_p1") for t in inside), inside


def test_end_to_end_accuracy(ops, pkg, modules, monkeypatch):
    """d_medium <= 2 d_amp (medium rounds GEMM operands only, autocast rounds activations too) and
    d_high <= 2^-6 d_amp + 2 d_off (2^-8, the ratio of the floors, times 4 for the norms; d_off, the library fp32 route, is
    the fp32 noise out_highest itself sits in)."""
    ref = _at(pkg, "highest", modules)
    high, medium = _at(pkg, "high", modules), _at(pkg, "medium", modules)
    with torch.autocast("cuda", torch.bfloat16):
        amp = modules()

    real_token, real_stem = ops.token_linear, ops.stem_conv_pool

    def token_off(x, weight, bias, relu=False, residual=None, ln=None, pos=None, out_group=0, split=True, w_split=None):
        N, K = weight.shape
        if N in (256, 288) and K % 64 == 0:
            return real_token(x, weight, bias, relu, residual, ln, pos, out_group, split=False)
        assert residual is None and ln is None and pos is None and not out_group  # fc1
        y = F.linear(x, weight, bias)
        return y.relu() if relu else y

    with monkeypatch.context() as mp:
        for flag in ("CONV1X1_SPLIT", "CONV3X3_SPLIT", "CONV_GN_FUSED"):
            mp.setattr(ops, flag, False)
        mp.setattr(ops, "token_linear", token_off)
        mp.setattr(ops, "stem_conv_pool", lambda x, w, b, w_split=None, split=True, grid=0: real_stem(x, w, b, split=False))
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        try:
            off = modules()
            torch.cuda.synchronize()
        finally:
            ops.set_kernel_timer(None)
        assert not any(SPLIT_TAG.match(t) for t in timer.records), list(timer.records)  # no split kernel on this route

    def d(out):
        return [((a - r).abs().max() / r.abs().max()).item() for a, r in zip(out, ref)]

    names = ["mask_features", "multi_scale[0]", "multi_scale[1]", "multi_scale[2]", "resnet stage"]
    rows = list(zip(names, d(high), d(medium), d(amp), d(off)))
    for name, dh, dm, da, do in rows:
        print(f"end to end {name}: d_high {dh:.3e} d_medium {dm:.3e} d_amp {da:.3e} d_off {do:.3e}")
    for name, dh, dm, da, do in rows:
        assert all(math.isfinite(v) for v in (dh, dm, da, do)), name
        assert dm <= 2.0 * da, (name, dm, da)
        assert dh <= 2.0 ** -6 * da + 2.0 * do, (name, dh, da, do)
