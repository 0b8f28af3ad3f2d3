"""The split-bf16 GEMM kernels (csrc/token_gemm_split.hip, conv1x1_split.hip, conv3x3_split.hip) at
the shapes their dispatch admits and the model-shape tests do not launch: one and an odd number of k-steps through the
two-slot LDS ring, N that only the last tile entry divides, fewer token tiles than CUs, ragged token and pixel tails, maps
of one pixel, `pos_rows` that is no multiple of 16, `out_group` with ReLU and with the sliced N.

Every case runs exact small integers (torch.equal with the fp64 reference: addressing and the ring, bit for bit) and randn
under the accuracy rule of tests/split_gemm_cases.py, and a second call gives the same bits.  The LayerNorm epilogue is
not exact on integers either (mean, variance, rsqrt), so its cases hold both families to the forms of
test_token_gemm_split_gpu.py: e <= 2 e32 + 1e-6 and e <= 3e-6 max|ref| sqrt(K) on the normalised output.

K = 2048 through the token kernel, which sums its six MFMAs straight into the accumulator where the convolutions sum each
k-step from zero, passes the rule (measured e 2.9e-7 against e32 3.7e-7 of the fp32-MFMA kernel at M = 272 C + 3)."""
import math

import pytest
import torch

import split_gemm_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def n_cu(ops):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cuda(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


# ---------------------------------------------------------------------------------------------------------------- token
# token counts by the CU count C (one persistent workgroup per CU, 8 waves, two 16-token tiles per wave and turn)
M_FORMS = {
    "1": lambda C: 1,                      # one tile, one live row
    "17": lambda C: 17,                    # fewer tiles than CUs
    "16C-11": lambda C: 16 * C - 11,       # one tile per CU, a ragged last tile
    "16(C+1)": lambda C: 16 * (C + 1),     # one tile more than CUs
    "48C+8": lambda C: 48 * C + 8,         # three tiles per CU: five of eight waves idle
    "272C+3": lambda C: 272 * C + 3,       # seventeen per CU: odd shares, a turn with one live column tile
}
# one k-step; three (Swin-T's K = 96) with the 18-row-tile slice; five with two slices; three with three slices; nine
# with four; 64 k-steps, the largest K the route admits
TOKEN_KN = [(32, 256), (96, 288), (160, 512), (96, 768), (288, 1024), (2048, 256)]
FAMILIES = ("ints", "randn")


def _token_case(family, M, K, N, seed):
    x, w, b = S.operands(family, M, K, N, seed)
    return _cuda(x, S.as_w1x1(w), b)


def _check_linear(ops, family, out, x, w, b, relu, what):
    ref, mag, _ = S.token_ref(x, w, b, relu)
    if family == "ints":
        assert torch.equal(out, ref.float()), what
        return
    e = S.rel_err(out, ref, mag)
    e32 = S.rel_err(S.token_fp32(ops, x, w, b, relu), ref, mag)
    print(f"{what}: e {e:.3e} e32 {e32:.3e}")
    assert S.rule(e, e32), (what, e, e32)


@pytest.mark.parametrize("K,N", TOKEN_KN)
@pytest.mark.parametrize("m_form", list(M_FORMS))
def test_token_bias_and_relu(ops, n_cu, m_form, K, N):
    M = M_FORMS[m_form](n_cu)
    for family in FAMILIES:
        x, w, b = _token_case(family, M, K, N, seed=M + 3 * K + N)
        ws = ops.split_weight(w)
        for relu in (False, True):
            out = ops.token_linear(x, w, b, relu=relu, w_split=ws)
            assert out.shape == (M, N)
            _check_linear(ops, family, out, x, w, b, relu, f"token M={M} K={K} N={N} relu={relu} {family}")
            assert torch.equal(ops.token_linear(x, w, b, relu=relu, w_split=ws), out)


OUT_GROUPS = [(K, N, G) for K, N in TOKEN_KN for G in sorted({4, 32, 64, N} | ({36} if N == 288 else set())) if N % G == 0]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("K,N,G", OUT_GROUPS)
def test_token_out_group_is_the_row_major_result_permuted(ops, n_cu, K, N, G, relu):
    for M in (17, 16 * n_cu - 11):
        for family in FAMILIES:
            x, w, b = _token_case(family, M, K, N, seed=M + K + N + G)
            ws = ops.split_weight(w)
            base = ops.token_linear(x, w, b, relu=relu, w_split=ws)
            _check_linear(ops, family, base, x, w, b, relu, f"token M={M} K={K} N={N} relu={relu} {family}")
            got = ops.token_linear(x, w, b, relu=relu, out_group=G, w_split=ws)
            assert got.shape == (N // G, M, G)
            assert torch.equal(got, S.group_major(base, G))
            assert torch.equal(ops.token_linear(x, w, b, relu=relu, out_group=G, w_split=ws), got)


def _ln_case(family, M, N, seed, res, pos_rows=0):
    ints = family == "ints"
    gamma, beta = S.extra((N,), seed + 1), S.extra((N,), seed + 2)
    r = S.extra((M, N), seed + 3, ints) if res else None
    pe = S.extra((pos_rows, N), seed + 4, ints) if pos_rows else None
    gamma, beta, r, pe = _cuda(gamma, beta, r, pe)
    return (gamma, beta, 1e-5), r, pe


def _check_layernorm(ops, out, x, w, b, r, lnp, what):
    """The LayerNorm epilogue in the forms of test_token_gemm_split_gpu.py: absolute errors of the normalised output."""
    K = w.shape[1]
    ref, _, _ = S.token_ref(x, w, b, residual=r, ln=lnp)
    out32 = S.token_fp32(ops, x, w, b, residual=r, ln=lnp)
    e, e32 = (out.double() - ref).abs().max().item(), (out32.double() - ref).abs().max().item()
    print(f"{what}: e {e:.3e} e32 {e32:.3e}")
    assert torch.isfinite(out).all(), what
    assert e <= 2 * e32 + 1e-6, (what, e, e32)
    assert e <= 3e-6 * ref.abs().max().item() * math.sqrt(K), (what, e)
    return ref


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("K,N", [(32, 256), (96, 288), (2048, 256)])
@pytest.mark.parametrize("m_form", list(M_FORMS))
def test_token_layernorm(ops, n_cu, m_form, K, N, res):
    M = M_FORMS[m_form](n_cu)
    for family in FAMILIES:
        x, w, b = _token_case(family, M, K, N, seed=M + 5 * K + N)
        lnp, r, _ = _ln_case(family, M, N, M + K, res)
        ws = ops.split_weight(w)
        out = ops.token_linear(x, w, b, residual=r, ln=lnp, w_split=ws)
        _check_layernorm(ops, out, x, w, b, r, lnp, f"token+ln M={M} K={K} N={N} res={res} {family}")
        assert torch.equal(ops.token_linear(x, w, b, residual=r, ln=lnp, w_split=ws), out)


# (M, pos_rows): a row per token; 850 rows (25 x 34, no multiple of 16) under two and three
# images; 17 rows under three; one row under every token
POS_CASES = [("16C-11", "M"), (1700, 850), (2550, 850), (51, 17), ("16C-11", 1), (17, 1)]


@pytest.mark.parametrize("K,N", [(32, 256), (96, 288)])
@pytest.mark.parametrize("M,rows", POS_CASES)
def test_token_pos_rows(ops, n_cu, M, rows, K, N):
    M = M_FORMS[M](n_cu) if isinstance(M, str) else M
    rows = M if rows == "M" else rows
    for family in FAMILIES:
        x, w, b = _token_case(family, M, K, N, seed=M + K + rows)
        lnp, r, pe = _ln_case(family, M, N, M + rows, True, rows)
        ws = ops.split_weight(w)
        out, outp = ops.token_linear(x, w, b, residual=r, ln=lnp, pos=pe, w_split=ws)
        ref = _check_layernorm(ops, out, x, w, b, r, lnp, f"token+ln+pos M={M} rows={rows} K={K} N={N} {family}")
        tiled = pe.repeat(M // rows, 1)
        assert torch.equal(outp, out + tiled)  # one fp32 add of token t's row t % rows
        refp = ref + tiled.double()
        assert (outp.double() - refp).abs().max().item() <= 3e-6 * refp.abs().max().item() * math.sqrt(K)
        assert torch.equal(ops.token_linear(x, w, b, residual=r, ln=lnp, w_split=ws), out)  # the same bits without pos
        again = ops.token_linear(x, w, b, residual=r, ln=lnp, pos=pe, w_split=ws)
        assert torch.equal(again[0], out) and torch.equal(again[1], outp)


@pytest.mark.parametrize("K,N", TOKEN_KN)
def test_token_row_slices_reproduce_the_full_result(ops, n_cu, K, N):
    M = 48 * n_cu + 8
    x, w, b = _token_case("randn", M, K, N, seed=K + N)
    ws = ops.split_weight(w)
    cuts = ((5, 6), (7, 1003), (M - 37, M), (16 * n_cu - 3, 32 * n_cu + 5))  # none on a 16-token tile border
    full = ops.token_linear(x, w, b, relu=True, w_split=ws)
    for r0, r1 in cuts:
        assert torch.equal(ops.token_linear(x[r0:r1], w, b, relu=True, w_split=ws), full[r0:r1]), (r0, r1)
    if N <= 288:
        lnp, r, _ = _ln_case("randn", M, N, K, True)
        full = ops.token_linear(x, w, b, residual=r, ln=lnp, w_split=ws)
        for r0, r1 in cuts:
            assert torch.equal(ops.token_linear(x[r0:r1], w, b, residual=r[r0:r1], ln=lnp, w_split=ws), full[r0:r1]), (r0, r1)


# ------------------------------------------------------------------------------------------------------- convolutions
# one k-step; three; five with N that only the 64-channel tile divides; six, likewise; twelve; twenty-four
C1_KN = [(32, 64), (96, 256), (160, 192), (192, 320), (384, 256), (768, 448)]
C1_MAPS = [(1, 1, 1), (1, 1, 2), (2, 3, 2), (1, 17, 1), (17, 1, 2), (5, 13, 1), (5, 7, 2), (4, 6, 2), (16, 16, 1), (37, 41, 2)]
C3_CN = [(32, 64), (96, 192), (160, 320), (192, 256)]
C3_MAPS = [(1, 1), (1, 17), (17, 1), (2, 2), (3, 3), (4, 6), (33, 31)]
C1_EPIS = (S.RAW, S.BIAS, S.RELU, S.RES)
C3_EPIS = (S.RAW, S.BIAS, S.RELU)


def _c1_case(family, B, K, N, H, W, stride, seed):
    x, w, b = S.operands(family, B * H * W, K, N, seed)
    Ho, Wo = S.out_hw(H, W, stride)
    r = S.extra((B, N, Ho, Wo), seed + 1, family == "ints")
    return _cuda(S.as_image(x, B, H, W), S.as_w1x1(w), b, r)


def _c1_args(epi, b, r):
    return (None if epi == S.RAW else b), (r if epi == S.RES else None), epi in (S.RELU, S.RES)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W,stride", C1_MAPS)
@pytest.mark.parametrize("K,N", C1_KN)
def test_conv1x1_epilogues(ops, K, N, H, W, stride, B):
    Ho, Wo = S.out_hw(H, W, stride)
    for family in FAMILIES:
        x, w, b, r = _c1_case(family, B, K, N, H, W, stride, seed=K + 7 * N + 31 * H + W + stride + B)
        ws = ops.split_weight(w)
        for epi in C1_EPIS:
            bb, rr, relu = _c1_args(epi, b, r)
            out = ops.conv1x1(x, w, bb, rr, relu, stride, w_split=ws)
            assert out.shape == (B, N, Ho, Wo)
            ref, mag = S.conv1x1_ref(x, w, bb, rr, relu, stride)
            what = f"conv1x1 K={K} N={N} {H}x{W}/{stride} B={B} {epi} {family}"
            if family == "ints":
                assert torch.equal(out, ref.float()), what
            else:
                e = S.rel_err(out, ref, mag)
                e32 = S.rel_err(S.conv1x1_fp32(ops, x, w, bb, rr, relu, stride), ref, mag)
                print(f"{what}: e {e:.3e} e32 {e32:.3e}")
                assert S.rule(e, e32), (what, e, e32)
            assert torch.equal(ops.conv1x1(x, w, bb, rr, relu, stride, w_split=ws), out)


def _sentinel_survives(call, out):
    """A refused call returns non-zero and launches nothing: the output buffer keeps its sentinel."""
    out.fill_(-7.0)
    rc = call()
    torch.cuda.synchronize()
    return rc != 0 and bool((out == -7.0).all())


@pytest.mark.parametrize("H,W,stride", [(1, 1, 1), (5, 7, 2), (37, 41, 2), (16, 16, 1)])
@pytest.mark.parametrize("K,N", C1_KN)
def test_conv1x1_forced_configurations(ops, K, N, H, W, stride):
    from weed_instance_segmentation_amd import _lib
    B = 3
    x, w, b, r = _c1_case("randn", B, K, N, H, W, stride, seed=K + N + H)
    ws = ops.split_weight(w)
    lib = _lib.load()
    fits = 0
    for epi in (S.RAW, S.RES):
        bb, rr, relu = _c1_args(epi, b, r)
        auto = ops.conv1x1(x, w, bb, rr, relu, stride, w_split=ws)
        for ci, nt in enumerate(S.NT):
            if N % nt == 0:
                fits += 1
                assert torch.equal(ops.conv1x1(x, w, bb, rr, relu, stride, w_split=ws, config=ci), auto), (epi, ci)
            else:  # refused through the C ABI
                out = torch.empty_like(auto)
                assert _sentinel_survives(lambda: lib.wm2f_conv1x1_split_fwd(
                    ops._p(x), ops._p(ws), ops._p(bb), ops._p(rr), ops._p(out), B, K, N, H, W, stride, 1 if relu else 0, ci,
                    ops._stream(x)), out), (epi, ci)
                with pytest.raises(_lib.Wm2fError):
                    ops.conv1x1(x, w, bb, rr, relu, stride, w_split=ws, config=ci)
    assert fits >= 2  # the 64-channel tile divides every N


@pytest.mark.parametrize("H,W", [(2, 3), (17, 1), (5, 7), (4, 6), (37, 41)])
@pytest.mark.parametrize("K,N", [(32, 64), (96, 256), (160, 192)])
def test_conv1x1_stride_2_never_reads_an_unsampled_pixel(ops, K, N, H, W):
    x, w, b, r = _c1_case("randn", 3, K, N, H, W, 2, seed=K + H + W)
    clean = ops.conv1x1(x, w, b, r, True, 2)
    x[:, :, 1::2, :] = float("nan")
    x[:, :, :, 1::2] = float("nan")
    assert torch.isnan(x).any()
    assert torch.equal(ops.conv1x1(x, w, b, r, True, 2), clean)


def _c3_case(family, B, C, N, H, W, seed):
    x, w, b = S.operands(family, B * H * W, C, N, seed, taps=9)
    return _cuda(S.as_image(x, B, H, W), S.as_w3x3(w), b)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("H,W", C3_MAPS)
@pytest.mark.parametrize("C,N", C3_CN)
def test_conv3x3_epilogues(ops, C, N, H, W, stride, B):
    Ho, Wo = S.out_hw(H, W, stride)
    for family in FAMILIES:
        x, w, b = _c3_case(family, B, C, N, H, W, seed=C + 7 * N + 31 * H + W + stride + B)
        ws = ops.split_weight_3x3(w)
        for epi in C3_EPIS:
            bb, relu = (None if epi == S.RAW else b), epi == S.RELU
            out = ops.conv3x3(x, w, bb, relu, stride, w_split=ws)
            assert out.shape == (B, N, Ho, Wo)
            ref, mag = S.conv3x3_ref(x, w, bb, relu, stride)
            what = f"conv3x3 C={C} N={N} {H}x{W}/{stride} B={B} {epi} {family}"
            if family == "ints":
                assert torch.equal(out, ref.float()), what
            else:
                e = S.rel_err(out, ref, mag)
                e32 = S.rel_err(S.conv3x3_fp32(x, w, bb, relu, stride), ref, mag)
                print(f"{what}: e {e:.3e} e32 {e32:.3e}")
                assert S.rule(e, e32), (what, e, e32)
            assert torch.equal(ops.conv3x3(x, w, bb, relu, stride, w_split=ws), out)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("H,W", [(1, 1), (4, 6), (33, 31)])
@pytest.mark.parametrize("C,N", C3_CN)
def test_conv3x3_forced_configurations(ops, C, N, H, W, stride):
    from weed_instance_segmentation_amd import _lib
    B = 3
    x, w, b = _c3_case("randn", B, C, N, H, W, seed=C + N + H)
    ws = ops.split_weight_3x3(w)
    lib = _lib.load()
    for epi in (S.RAW, S.RELU):
        bb, relu = (None if epi == S.RAW else b), epi == S.RELU
        auto = ops.conv3x3(x, w, bb, relu, stride, w_split=ws)
        for ci, nt in enumerate(S.NT):
            if N % nt == 0:
                assert torch.equal(ops.conv3x3(x, w, bb, relu, stride, w_split=ws, config=ci), auto), (epi, ci)
            else:
                out = torch.empty_like(auto)
                assert _sentinel_survives(lambda: lib.wm2f_conv3x3_split_fwd(
                    ops._p(x), ops._p(ws), ops._p(bb), ops._p(out), B, C, N, H, W, stride, 1 if relu else 0, ci,
                    ops._stream(x)), out), (epi, ci)
                with pytest.raises(_lib.Wm2fError):
                    ops.conv3x3(x, w, bb, relu, stride, w_split=ws, config=ci)
