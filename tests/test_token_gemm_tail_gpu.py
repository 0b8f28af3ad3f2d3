"""The token kernel's last turn (csrc/token_gemm_split.hip, DESIGN.md §13 "A one-tile turn costs one tile").

A wave walks its share of 16-token column tiles two per turn.  When one tile is left the kernel skips the second tile's
split and its six-MFMA chains (a wave-uniform branch), so the turn costs one tile.  The MFMA sequence of a live tile is
what it was, and a skipped tile's accumulators stay zero and are never stored.

Token counts, by the CU count C (one persistent workgroup per CU while there are tiles, 8 waves each), chosen so that the
last turn of a wave has 0, 1 and 2 live tiles:
  16            one tile: one workgroup, wave 0 has 1, waves 1-7 have 0
  16*8          8 tiles: 8 workgroups of one tile each (C >= 8), or all waves of few workgroups with 1
  16*(8*2+1)    17 tiles: one each for 17 workgroups (or shares of 2 and 3 where C < 17)
  16*(2C)       two tiles per CU: waves 0, 1 have 1, the others 0
  16*(8C)       eight per CU: every wave has 1
  16*(10C+3)-5  ten or eleven per CU: shares of 2 and 1 (and 2, 2, 2, 1 ...), a ragged last tile
The first forms are also project_kv's regime, one tile per working wave, which ran two.

Each case runs the three epilogue families -- bias (+ ReLU) row-major, feature-group-major, residual + LayerNorm -- on
exact small integers (torch.equal with the fp64 reference) and on randn under the rule of tests/split_gemm_cases.py.  The
LayerNorm epilogue is built for N <= 288 only, so (288, 1024) runs the other two; it is not exact on integers (mean,
variance, rsqrt), so both families are held to the forms test_split_gemm_shapes_gpu.py holds it to.

Prefix invariance: the first M rows of a run at M + 48 (another tile distribution: other waves take the one-tile turn)
equal the run at M bit for bit, for every epilogue."""
import functools
import math

import pytest
import torch

import split_gemm_cases as S

pytestmark = pytest.mark.gpu

M_FORMS = {
    "16": lambda C: 16,
    "16*8": lambda C: 16 * 8,
    "16*17": lambda C: 16 * (8 * 2 + 1),
    "16*2C": lambda C: 16 * (2 * C),
    "16*8C": lambda C: 16 * (8 * C),
    "16*(10C+3)-5": lambda C: 16 * (10 * C + 3) - 5,
}
TOKEN_KN = [(32, 256), (96, 288), (288, 1024)]
FAMILIES = ("ints", "randn")
EXTRA_ROWS = 16 * 3
OUT_GROUP = 32  # divides 256, 288 and 1024


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def n_cu(ops):
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=2)
def _case(family, M, K, N):
    """Inputs of M + EXTRA_ROWS tokens on the device (the run at M takes the first M rows), computed once per case."""
    Mx = M + EXTRA_ROWS
    seed = M + 3 * K + N
    x, w, b = S.operands(family, Mx, K, N, seed)
    ints = family == "ints"
    gamma, beta, r = S.extra((N,), seed + 1), S.extra((N,), seed + 2), S.extra((Mx, N), seed + 3, ints)
    return tuple(t.cuda() for t in (x, S.as_w1x1(w), b, gamma, beta, r))


def _runs(ops, x, w, b, gamma, beta, r, ws):
    """Every epilogue family the shape is built for: {name: output}."""
    N = w.shape[0]
    outs = {
        "bias": ops.token_linear(x, w, b, w_split=ws),
        "relu": ops.token_linear(x, w, b, relu=True, w_split=ws),
        "group": ops.token_linear(x, w, b, relu=True, out_group=OUT_GROUP, w_split=ws),
    }
    if N <= 288:
        outs["ln"] = ops.token_linear(x, w, b, residual=r, ln=(gamma, beta, 1e-5), w_split=ws)
    return outs


@pytest.mark.parametrize("K,N", TOKEN_KN)
@pytest.mark.parametrize("m_form", list(M_FORMS))
def test_last_turn_with_0_1_2_live_tiles(ops, n_cu, m_form, K, N):
    M = M_FORMS[m_form](n_cu)
    for family in FAMILIES:
        xx, w, b, gamma, beta, rr = _case(family, M, K, N)
        x, r = xx[:M], rr[:M]
        ws = ops.split_weight(w)
        outs = _runs(ops, x, w, b, gamma, beta, r, ws)
        for relu in (False, True):
            out = outs["relu" if relu else "bias"]
            assert out.shape == (M, N)
            ref, mag, _ = S.token_ref(x, w, b, relu)
            what = f"token tail M={M} K={K} N={N} relu={relu} {family}"
            if family == "ints":
                assert torch.equal(out, ref.float()), what
            else:
                e = S.rel_err(out, ref, mag)
                e32 = S.rel_err(S.token_fp32(ops, x, w, b, relu), ref, mag)
                print(f"{what}: e {e:.3e} e32 {e32:.3e}")
                assert S.rule(e, e32), (what, e, e32)
        # feature-group major: the row-major bits, permuted (so exact on integers and under the rule on randn as well)
        assert outs["group"].shape == (N // OUT_GROUP, M, OUT_GROUP)
        assert torch.equal(outs["group"], S.group_major(outs["relu"], OUT_GROUP)), (M, K, N, family)
        if "ln" in outs:
            lnp = (gamma, beta, 1e-5)
            out = outs["ln"]
            ref, _, _ = S.token_ref(x, w, b, residual=r, ln=lnp)
            out32 = S.token_fp32(ops, x, w, b, residual=r, ln=lnp)
            e, e32 = (out.double() - ref).abs().max().item(), (out32.double() - ref).abs().max().item()
            print(f"token tail + ln M={M} K={K} N={N} {family}: e {e:.3e} e32 {e32:.3e}")
            assert torch.isfinite(out).all()
            assert e <= 2 * e32 + 1e-6, (M, K, N, family, e, e32)
            assert e <= 3e-6 * ref.abs().max().item() * math.sqrt(K), (M, K, N, family, e)


@pytest.mark.parametrize("K,N", TOKEN_KN)
@pytest.mark.parametrize("m_form", list(M_FORMS))
def test_prefix_of_a_longer_run_is_the_run(ops, n_cu, m_form, K, N):
    M = M_FORMS[m_form](n_cu)
    xx, w, b, gamma, beta, rr = _case("randn", M, K, N)
    ws = ops.split_weight(w)
    short = _runs(ops, xx[:M], w, b, gamma, beta, rr[:M], ws)
    long = _runs(ops, xx, w, b, gamma, beta, rr, ws)
    for name, out in short.items():
        head = long[name][:, :M] if name == "group" else long[name][:M]
        assert torch.equal(head, out), (name, M, K, N)
