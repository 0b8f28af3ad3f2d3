"""wm2f_token_linear_split_fwd (split-bf16 token GEMM, csrc/token_gemm_split.hip) at the model's shapes:
accuracy against fp64 next to the fp32-MFMA kernel (wm2f_token_linear_fwd) on the same data, bit-identity on repeated and
sub-batch inputs, non-finite propagation."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

M_ENC = 8 * 21504  # encoder tokens of the benchmark: B = 8 at 1024^2 (32^2 + 64^2 + 128^2 per image)
S_IMG = 21504


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


def _case(M, K, N, seed, ln=False, res=False, pos=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, K, generator=g, device="cuda")
    w = torch.randn(N, K, generator=g, device="cuda") * (1.0 / math.sqrt(K))
    b = torch.randn(N, generator=g, device="cuda") * 0.1
    r = torch.randn(M, N, generator=g, device="cuda") if res else None
    lnp = (torch.randn(N, generator=g, device="cuda"), torch.randn(N, generator=g, device="cuda"), 1e-5) if ln else None
    pe = torch.randn(S_IMG if M % S_IMG == 0 else M, N, generator=g, device="cuda") if pos else None
    return x, w, b, r, lnp, pe


def _linear_err(out, x, w, b, relu):
    """max |out - ref| / sum_k |x_k w_k| over the outputs, ref in fp64 on the GPU."""
    xd, wd = x.double(), w.double()
    ref = torch.addmm(b.double(), xd, wd.t())
    if relu:
        ref = ref.relu()
    mag = xd.abs() @ wd.abs().t()
    return ((out.double() - ref).abs() / mag.clamp_min(1e-300)).max().item(), ref


def _fp32_kernel(ops, x, w, b, relu):
    """The fp32-MFMA kernel on the same data (N > 288: 256-wide slices of W)."""
    N = w.shape[0]
    if N <= 288:
        return ops.token_linear(x, w, b, relu=relu, split=False)
    return torch.cat([ops.token_linear(x, w[i:i + 256].contiguous(), b[i:i + 256].contiguous(), relu=relu, split=False)
                      for i in range(0, N, 256)], dim=-1)


# the five encoder call sites: value_proj, merged offsets | logits, fc1 (bias + ReLU), plus project_kv's token counts
@pytest.mark.parametrize("M,K,N,relu", [(M_ENC, 256, 256, False), (M_ENC, 256, 288, False), (M_ENC, 256, 1024, True),
                                        (8 * 1024, 256, 256, False), (8 * 4096, 256, 256, False), (8 * 16384, 256, 256, False)])
def test_split_linear_accuracy_determinism_and_sub_batches(ops, M, K, N, relu):
    x, w, b, _, _, _ = _case(M, K, N, seed=M + K + N)
    ws = ops.split_weight(w)
    out = ops.token_linear(x, w, b, relu=relu, w_split=ws)
    err, ref = _linear_err(out, x, w, b, relu)
    err32, _ = _linear_err(_fp32_kernel(ops, x, w, b, relu), x, w, b, relu)
    assert err <= 2 * err32, (err, err32)
    scale = ref.abs().max().item()
    assert (out.double() - ref).abs().max().item() <= 3e-6 * scale * math.sqrt(K)
    del ref
    assert torch.equal(ops.token_linear(x, w, b, relu=relu, w_split=ws), out)
    assert torch.equal(ops.token_linear(x, w, b, relu=relu), out)  # an uncached split is the same split
    for r0, r1 in ((0, 1), (1000, 5003), (M - 37, M)):
        assert torch.equal(ops.token_linear(x[r0:r1], w, b, relu=relu, w_split=ws), out[r0:r1])
    if N == 288:  # K1's head-major rows: the same bits at other addresses
        got = ops.token_linear(x, w, b, out_group=36, w_split=ws)
        assert torch.equal(got, out.view(M, 8, 36).permute(1, 0, 2))
    if N == 256 and M == M_ENC:  # head-major value
        got = ops.token_linear(x, w, b, out_group=32, w_split=ws)
        assert torch.equal(got, out.view(M, 8, 32).permute(1, 0, 2))


# output_proj + residual + self_attn_layer_norm; fc2 + residual + final_layer_norm + the next layer's hidden + pos
@pytest.mark.parametrize("K,pos", [(256, False), (1024, True)])
def test_split_linear_layernorm_epilogue(ops, K, pos):
    M, N = M_ENC, 256
    x, w, b, r, lnp, pe = _case(M, K, N, seed=K, ln=True, res=True, pos=pos)
    ws = ops.split_weight(w)
    got = ops.token_linear(x, w, b, residual=r, ln=lnp, pos=pe, w_split=ws)
    got32 = ops.token_linear(x, w, b, residual=r, ln=lnp, pos=pe, split=False)
    out, outp = got if pos else (got, None)
    out32 = got32[0] if pos else got32
    ref = torch.nn.functional.layer_norm(torch.addmm(b.double(), x.double(), w.double().t()) + r.double(), (N,),
                                         lnp[0].double(), lnp[1].double(), 1e-5)
    e, e32 = (out.double() - ref).abs().max().item(), (out32.double() - ref).abs().max().item()
    assert e <= 2 * e32 + 1e-6, (e, e32)
    assert e <= 3e-6 * ref.abs().max().item() * math.sqrt(K)
    if pos:
        refp = ref + pe.double().repeat(M // pe.shape[0], 1)
        assert (outp.double() - refp).abs().max().item() <= 3e-6 * refp.abs().max().item() * math.sqrt(K)
    del ref
    again = ops.token_linear(x, w, b, residual=r, ln=lnp, pos=pe, w_split=ws)
    assert torch.equal(again[0] if pos else again, out)
    # one image of the batch alone: the same rows, bit for bit (pos rows are per image)
    i0, i1 = 3 * S_IMG, 4 * S_IMG
    sub = ops.token_linear(x[i0:i1], w, b, residual=r[i0:i1], ln=lnp, pos=pe, w_split=ws)
    assert torch.equal(sub[0] if pos else sub, out[i0:i1])
    if pos:
        assert torch.equal(sub[1], outp[i0:i1])


@pytest.mark.parametrize("K,N,ln", [(256, 256, False), (256, 1024, False), (1024, 256, True)])
def test_split_linear_nonfinite_inputs(ops, K, N, ln):
    M = 4096 + 37
    x, w, b, r, lnp, _ = _case(M, K, N, seed=11 * K + N, ln=ln, res=ln)
    bad = torch.tensor([0, 17, 1000, 4095, M - 1], device="cuda")
    x[bad[0], 3] = float("nan")
    x[bad[1], K - 1] = float("inf")
    x[bad[2], 40] = -float("inf")
    x[bad[3], 0] = float("nan")
    x[bad[4], 100] = float("inf")
    out = ops.token_linear(x, w, b, residual=r, ln=lnp)
    ref = torch.addmm(b.double(), x.double(), w.double().t())
    fin = torch.isfinite(out)
    assert torch.equal(fin, torch.isfinite(ref) if not ln else torch.isfinite(ref).all(1, keepdim=True).expand_as(ref))
    rows = torch.zeros(M, dtype=torch.bool, device="cuda")
    rows[bad] = True
    assert not fin[rows].any() and fin[~rows].all()
