"""Parity of the HIP kernels (through the C ABI) against the CPU oracle and the golden vectors.
Needs a real MI355X:  python -m pytest tests -m gpu

Tolerances: fp32 results within 1e-3 relative of the oracle (BASELINE.json north_star); in practice
the kernels sit at 1e-5..1e-6, and the tests hold them to that.  Index outputs are bit-exact."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import m2f_oracle as O

pytestmark = pytest.mark.gpu

T = lambda a: torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


def dev(t):
    return t.cuda()


# ----------------------------------------------------------------------------------------- K1
@pytest.mark.parametrize("tag", ["toy", "rect", "d8"])
def test_k1_golden(ops, tag):
    g = load_golden(f"k1_msdeform_{tag}.npz")
    out = ops.ms_deform_attn(dev(T(g["value"])), g["level_hw"].tolist(), dev(T(g["loc"])), dev(T(g["w"])))
    torch.testing.assert_close(out.cpu(), T(g["out"]), rtol=1e-5, atol=2e-6)


def _rand_k1(B, shapes, H, D, seed, spread=1.2):
    g = torch.Generator().manual_seed(seed)
    S = sum(h * w for h, w in shapes)
    L, P = len(shapes), 4
    value = torch.randn(B, S, H, D, generator=g)
    loc = torch.rand(B, S, H, L, P, 2, generator=g) * spread - (spread - 1) / 2
    w = torch.softmax(torch.randn(B, S, H, L * P, generator=g), -1).view(B, S, H, L, P)
    return value, loc, w


@pytest.mark.parametrize("shapes,B,H,D", [([(8, 8), (16, 16), (32, 32)], 2, 8, 32),
                                          ([(5, 7), (10, 14), (20, 28)], 3, 8, 32),
                                          ([(4, 4), (8, 8)], 1, 4, 16),
                                          ([(6, 6)], 2, 2, 64)])
def test_k1_random_vs_oracle(ops, shapes, B, H, D):
    value, loc, w = _rand_k1(B, shapes, H, D, 1)
    ref = O.msdeform_attn_core(value, shapes, loc, w)
    out = ops.ms_deform_attn(dev(value), shapes, dev(loc), dev(w))
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-5, atol=5e-6)


def test_k1_fused_prologue(ops):
    shapes = [(8, 8), (16, 16), (32, 32)]
    B, H, D, L, P = 2, 8, 32, 3, 4
    g = torch.Generator().manual_seed(2)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(B, S, H, D, generator=g)
    off = torch.randn(B, S, H, L, P, 2, generator=g) * 3
    logits = torch.randn(B, S, H, L * P, generator=g) * 2
    ref_pts = O.reference_points(shapes, 1)[0].contiguous()  # (S, L, 2)
    norm = torch.tensor([[ww, hh] for hh, ww in shapes], dtype=torch.long)
    loc = ref_pts[None, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    aw = torch.softmax(logits, -1).view(B, S, H, L, P)
    ref = O.msdeform_attn_core(value, shapes, loc, aw)
    out = ops.ms_deform_attn_fused(dev(value), shapes, dev(off), dev(logits), dev(ref_pts))
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("variant,margin", [(1, 4), (2, 4), (2, 0), (4, 4), (0, 7)])
@pytest.mark.parametrize("tag", ["toy", "rect"])
def test_k1_variants_golden(ops, tag, variant, margin):
    """The three kernels the library runs -- direct gather (1), LDS windows (2), streaming quads (4; what `auto` picks
    here) -- give the same answer; the window margin never changes it (the golden locations are spread far outside any
    margin, so the slow path is exercised)."""
    g = load_golden(f"k1_msdeform_{tag}.npz")
    out = ops.ms_deform_attn_variant(dev(T(g["value"])), g["level_hw"].tolist(), dev(T(g["loc"])), dev(T(g["w"])),
                                     variant=variant, margin=margin)
    torch.testing.assert_close(out.cpu(), T(g["out"]), rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("shapes,B", [([(8, 8), (16, 16), (32, 32)], 2), ([(5, 7), (10, 14), (20, 28)], 3),
                                      ([(7, 9), (13, 17), (25, 33)], 1), ([(12, 20), (24, 40)], 2),
                                      ([(32, 32), (64, 64), (128, 128)], 1)])
@pytest.mark.parametrize("fused", [False, True])
def test_k1_tiled_local_offsets(ops, shapes, B, fused):
    """Offsets of a few pixels around the reference points (the module's regime): fast LDS path,
    odd level sizes included (tiles with ragged query counts)."""
    H, D, L, P = 8, 32, len(shapes), 4
    g = torch.Generator().manual_seed(11)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(B, S, H, D, generator=g)
    off = torch.randn(B, S, H, L, P, 2, generator=g) * 2.5
    off[0, 3, 0, 0, 0] = torch.tensor([40.0, -35.0])  # far outlier -> slow path
    logits = torch.randn(B, S, H, L * P, generator=g)
    ref_pts = O.reference_points(shapes, 1)[0].contiguous()
    norm = torch.tensor([[ww, hh] for hh, ww in shapes], dtype=torch.long)
    loc = ref_pts[None, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    aw = torch.softmax(logits, -1).view(B, S, H, L, P)
    ref = O.msdeform_attn_core(value, shapes, loc, aw)
    for margin, variant in ((4, 2), (2, 2)):
        if fused:
            out = ops.ms_deform_attn_variant(dev(value), shapes, dev(off), dev(logits), dev(ref_pts), fused=True,
                                             variant=variant, margin=margin)
        else:
            out = ops.ms_deform_attn_variant(dev(value), shapes, dev(loc), dev(aw), variant=variant, margin=margin)
        torch.testing.assert_close(out.cpu(), ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("shapes,B", [([(8, 8), (16, 16), (32, 32)], 2), ([(5, 7), (10, 14), (20, 28)], 3),
                                      ([(1, 1), (2, 2), (4, 4)], 2), ([(3, 9), (6, 18), (12, 36)], 1),
                                      ([(9, 5), (18, 10), (36, 20)], 2), ([(32, 32), (64, 64), (128, 128)], 1),
                                      ([(32, 32), (64, 64), (128, 128)], 6)])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("spread", ["local", "wide"])
@pytest.mark.parametrize("variant", [4])
def test_k1_quad_kernel(ops, shapes, B, fused, spread, variant):
    """The streaming quad kernel (variant 4: persistent workgroups + loader waves; what `auto` picks for the encoder's
    1:2:4 pyramids) through the two-array entry points: ragged edge tiles, several tiles per workgroup, offsets inside
    the window margin (fast path) and far outside it (every point on the slow path)."""
    H, D, L, P = 8, 32, 3, 4
    g = torch.Generator().manual_seed(21)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(B, S, H, D, generator=g)
    off = torch.randn(B, S, H, L, P, 2, generator=g) * (2.0 if spread == "local" else 30.0)
    off[0, S // 2, 1, 2, 3] = torch.tensor([-60.0, 45.0])
    off[0, 0, 0, 0, 0] = torch.tensor([4.999, -4.999])  # the window's last column / first row
    logits = torch.randn(B, S, H, L * P, generator=g) * 2
    ref_pts = O.reference_points(shapes, 1)[0].contiguous()
    norm = torch.tensor([[ww, hh] for hh, ww in shapes], dtype=torch.long)
    loc = ref_pts[None, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    aw = torch.softmax(logits, -1).view(B, S, H, L, P)
    ref = O.msdeform_attn_core(value, shapes, loc, aw)
    if fused:
        out = ops.ms_deform_attn_variant(dev(value), shapes, dev(off), dev(logits), dev(ref_pts), fused=True, variant=variant)
    else:
        out = ops.ms_deform_attn_variant(dev(value), shapes, dev(loc), dev(aw), variant=variant)
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-4, atol=2e-5)  # fp32: 12-term sums of O(1) values


def test_k1_quad_kernel_refuses_other_pyramids(ops):
    """A forced kernel choice that does not apply raises; so do the superseded kernels and A/B variants, which exist in
    the profiling build only (include/wm2f_prof.h)."""
    from weed_instance_segmentation_amd._lib import Wm2fError
    shapes = [(12, 20), (24, 40)]
    value, loc, w = _rand_k1(1, shapes, 8, 32, 2)
    with pytest.raises(Wm2fError):
        ops.ms_deform_attn_variant(dev(value), shapes, dev(loc), dev(w), variant=4)
    shapes = [(4, 4), (8, 8), (16, 16)]
    value, loc, w = _rand_k1(1, shapes, 8, 32, 3)
    for variant in (3, 5, 6, 7, 8, 62, 44, 74):
        with pytest.raises(Wm2fError):
            ops.ms_deform_attn_variant(dev(value), shapes, dev(loc), dev(w), variant=variant)


@pytest.mark.parametrize("shapes,D", [([(8, 8), (16, 16), (32, 32)], 32), ([(5, 7), (10, 14), (20, 28)], 32),
                                      ([(4, 4), (8, 8), (16, 16)], 16)])
def test_k1_fused_packed(ops, shapes, D):
    """One merged [offsets | logits] row per token (the module's inference path), incl. the fallback (D=16)."""
    B, H, L, P = 2, 8, 3, 4
    g = torch.Generator().manual_seed(12)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(B, S, H, D, generator=g)
    packed = torch.randn(B, S, H * L * P * 3, generator=g) * 2
    off = packed[..., :H * L * P * 2].reshape(B, S, H, L, P, 2)
    logits = packed[..., H * L * P * 2:].reshape(B, S, H, L * P)
    ref_pts = O.reference_points(shapes, 1)[0].contiguous()
    norm = torch.tensor([[ww, hh] for hh, ww in shapes], dtype=torch.long)
    loc = ref_pts[None, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    ref = O.msdeform_attn_core(value, shapes, loc, torch.softmax(logits, -1).view(B, S, H, L, P))
    out = ops.ms_deform_attn_fused_packed(dev(value), shapes, dev(packed), dev(ref_pts), H, L, P)
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("shapes,B,spread", [([(8, 8), (16, 16), (32, 32)], 2, 2.0), ([(5, 7), (10, 14), (20, 28)], 3, 2.0),
                                             ([(2, 3), (4, 6), (8, 12)], 1, 2.0), ([(9, 11), (18, 22), (36, 44)], 2, 9.0),
                                             # more (image, head, tile) units than workgroups: the persistent walk takes steps
                                             ([(16, 16), (32, 32), (64, 64)], 3, 2.0), ([(12, 20), (24, 40), (48, 80)], 5, 2.0),
                                             ([(13, 21), (26, 42), (52, 84)], 4, 6.0)])
def test_k1_fused_lanes(ops, shapes, B, spread):
    """The lane-major row order (wm2f_msdeform_fused_lanes_fwd): the same numbers as the [offsets | logits] rows, permuted
    as include/wm2f.h says, give the same result as the oracle -- ragged tiles, and offsets far beyond the window margin
    (spread 9: the slow path reads the lane-major rows too)."""
    H, L, P, D = 8, 3, 4, 32
    g = torch.Generator().manual_seed(13)
    S = sum(h * w for h, w in shapes)
    assert ops.k1_lanes_applies(shapes, S, D, P, B, H)
    value = torch.randn(B, S, H, D, generator=g)
    off = torch.randn(B, S, H, L, P, 2, generator=g) * spread
    logits = torch.randn(B, S, H, L * P, generator=g) * 2
    lanes = ops.k1_lane_rows(off, logits).view(B, S, H, 36)  # the record order of include/wm2f.h
    assert torch.equal(lanes[0, 5, 2, 4 * 1 + 2:4 * 1 + 4], off[0, 5, 2, 1, 1]) and lanes[0, 5, 2, 32 + 3] == logits[0, 5, 2, 2 * 4 + 3]
    ref_pts = O.reference_points(shapes, 1)[0].contiguous()
    norm = torch.tensor([[ww, hh] for hh, ww in shapes], dtype=torch.long)
    loc = ref_pts[None, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    ref = O.msdeform_attn_core(value, shapes, loc, torch.softmax(logits, -1).view(B, S, H, L, P))
    out = ops.ms_deform_attn_fused_lanes(dev(value), shapes, dev(lanes.reshape(B, S, H * 36)), H)
    # |out| reaches ~4 here (12 weighted samples of N(0,1) values); the fused prologue's exp / reciprocal differ from the
    # oracle's softmax by an fp32 ulp or two of that: 5e-5 absolute = 1.2e-5 of the range (3 of 6.4 M elements pass 2e-5)
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-4, atol=5e-5)
    # the other fused form on the same numbers: identical arithmetic, so identical bits
    packed = torch.cat([off.reshape(B, S, -1), logits.reshape(B, S, -1)], -1)
    out2 = ops.ms_deform_attn_fused_packed(dev(value), shapes, dev(packed), dev(ref_pts), H, L, P)
    assert torch.equal(out, out2)
    # the same rows stored head-major, (heads, B, S, 36): same loads per lane from other addresses, so identical bits
    out3 = ops.ms_deform_attn_fused_lanes(dev(value), shapes, dev(lanes.permute(2, 0, 1, 3).contiguous()), H, head_major=True)
    assert torch.equal(out, out3)
    # value stored head-major, (heads, B, S, 32): the loaders read the same pixels through other strides
    out4 = ops.ms_deform_attn_fused_lanes(dev(value.permute(2, 0, 1, 3).contiguous()), shapes, dev(lanes.reshape(B, S, H * 36)), H, value_head_major=True)
    assert torch.equal(out, out4)
    # slab order (heads outermost: an XCD's workgroups walk one (image, head) slab together): another work order, same bits
    out5 = ops.ms_deform_attn_fused_lanes(dev(value), shapes, dev(lanes.permute(2, 0, 1, 3).contiguous()), H,
                                          head_major=True, slab_order=True)
    assert torch.equal(out, out5)
    out6 = ops.ms_deform_attn_fused_lanes(dev(value), shapes, dev(lanes.reshape(B, S, H * 36)), H, slab_order=True)
    assert torch.equal(out, out6)
    assert not ops.k1_lanes_applies([(5, 7), (10, 14), (20, 27)], 5 * 7 + 10 * 14 + 20 * 27, D, P, B, H)
    with pytest.raises(Exception):  # a shape outside the streaming kernel is refused, not re-routed
        ops.ms_deform_attn_fused_lanes(dev(value[:, :20 * 5]), [(2, 2), (4, 4), (8, 10)], dev(lanes.reshape(B, S, H * 36)[:, :100]), H)


def test_k1_backward(ops):
    shapes = [(4, 6), (8, 12), (16, 24)]
    value, loc, w = _rand_k1(2, shapes, 8, 32, 3, spread=1.1)
    go = torch.randn(2, value.shape[1], 8 * 32, generator=torch.Generator().manual_seed(4))
    v0, l0, w0 = value.clone().requires_grad_(), loc.clone().requires_grad_(), w.clone().requires_grad_()
    O.msdeform_attn_core(v0, shapes, l0, w0).backward(go)
    v1, l1, w1 = dev(value).requires_grad_(), dev(loc).requires_grad_(), dev(w).requires_grad_()
    ops.ms_deform_attn(v1, shapes, l1, w1).backward(dev(go))
    torch.testing.assert_close(v1.grad.cpu(), v0.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(w1.grad.cpu(), w0.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(l1.grad.cpu(), l0.grad, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("shapes,B", [([(8, 8), (16, 16), (32, 32)], 2), ([(5, 7), (10, 14), (20, 28)], 1),
                                      ([(12, 20), (24, 40)], 2)])
def test_k1_backward_local_offsets(ops, shapes, B):
    """LDS-window backward in its fast regime (offsets of a few pixels) plus one far outlier."""
    H, D, L, P = 8, 32, len(shapes), 4
    g = torch.Generator().manual_seed(13)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(B, S, H, D, generator=g)
    off = torch.randn(B, S, H, L, P, 2, generator=g) * 2.0
    off[0, 5, 1, 0, 2] = torch.tensor([-30.0, 25.0])
    ref_pts = O.reference_points(shapes, 1)[0].contiguous()
    norm = torch.tensor([[ww, hh] for hh, ww in shapes], dtype=torch.long)
    loc = (ref_pts[None, :, None, :, None, :] + off / norm[None, None, None, :, None, :]).contiguous()
    w = torch.softmax(torch.randn(B, S, H, L * P, generator=g), -1).view(B, S, H, L, P).contiguous()
    go = torch.randn(B, S, H * D, generator=g)
    v0, l0, w0 = value.clone().requires_grad_(), loc.clone().requires_grad_(), w.clone().requires_grad_()
    O.msdeform_attn_core(v0, shapes, l0, w0).backward(go)
    v1, l1, w1 = dev(value).requires_grad_(), dev(loc).requires_grad_(), dev(w).requires_grad_()
    ops.ms_deform_attn(v1, shapes, l1, w1).backward(dev(go))
    torch.testing.assert_close(v1.grad.cpu(), v0.grad, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(w1.grad.cpu(), w0.grad, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(l1.grad.cpu(), l0.grad, rtol=1e-3, atol=2e-4)


def _rows_case(shapes, B, spread, seed=21):
    H, L, P, D = 8, 3, 4, 32
    g = torch.Generator().manual_seed(seed)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(B, S, H, D, generator=g)
    off = torch.randn(B, S, H, L, P, 2, generator=g) * spread
    off[0, 5, 1, 0, 2] = torch.tensor([-30.0, 25.0])  # far beyond the window margin: the kernels' slow paths
    off[0, 7, 3, 2, 1] = torch.tensor([1000.0, -1000.0])  # outside every image: no contribution, zero gradient
    logits = torch.randn(B, S, H, L * P, generator=g) * 2
    go = torch.randn(B, S, H * D, generator=g)
    return value, off, logits, go


def _rows_oracle(value, rows, shapes, go, H=8, L=3, P=4):
    """The composition of HF:983-1002 + :798-837 on the oracle, with autograd: gradients w.r.t. value and the rows."""
    B, S = rows.shape[:2]
    v0, r0 = value.clone().requires_grad_(), rows.clone().requires_grad_()
    n_off = H * L * P * 2
    off = r0[..., :n_off].view(B, S, H, L, P, 2)
    ref_pts = O.reference_points(shapes, 1)[0].contiguous()
    norm = torch.tensor([[ww, hh] for hh, ww in shapes], dtype=value.dtype)
    loc = ref_pts[None, :, None, :, None, :].to(value.dtype) + off / norm[None, None, None, :, None, :]
    aw = torch.softmax(r0[..., n_off:].view(B, S, H, L * P), -1).view(B, S, H, L, P)
    out = O.msdeform_attn_core(v0, shapes, loc, aw)
    out.backward(go)
    return out.detach(), v0.grad, r0.grad


@pytest.mark.parametrize("shapes,B,spread", [([(8, 8), (16, 16), (32, 32)], 2, 2.0), ([(5, 7), (10, 14), (20, 28)], 3, 2.0),
                                             ([(2, 3), (4, 6), (8, 12)], 1, 1.0), ([(12, 20), (24, 40), (48, 80)], 2, 3.0)])
def test_k1_rows_training_op_fp32(ops, shapes, B, spread):
    """wm2f_msdeform_rows_fwd / _bwd: K1 on the merged projection's [offsets | logits] rows with the prologue inside, forward
    and backward, against the oracle's autograd of the same composition in float64."""
    H = 8
    value, off, logits, go = _rows_case(shapes, B, spread)
    S = value.shape[1]
    rows = torch.cat([off.reshape(B, S, -1), logits.reshape(B, S, -1)], -1).contiguous()
    out0, gv0, gr0 = _rows_oracle(value.double(), rows.double(), shapes, go.double())
    v1, r1 = dev(value).requires_grad_(), dev(rows).requires_grad_()
    assert ops.k1_rows_applies(v1, r1, shapes, H)
    out = ops.ms_deform_attn_rows(v1, shapes, r1, H)
    out.backward(dev(go))
    torch.testing.assert_close(out.detach().cpu().double(), out0, rtol=1e-4, atol=5e-5)
    torch.testing.assert_close(v1.grad.cpu().double(), gv0, rtol=1e-4, atol=3e-5)
    n_off = H * 3 * 4 * 2
    # offsets: the gradient is piecewise constant in the fractional position; logits: through the softmax
    # (a sampling pixel within an fp32 ulp of an integer lands in the neighbouring cell in float64: that point's offset gradient is
    # the other side of the kink -- a handful of the 10^5..10^6 points, not a tolerance)
    def close_but(a, b_, rtol, atol, max_bad):
        bad = (a - b_).abs() > atol + rtol * b_.abs()
        assert int(bad.sum()) <= max_bad, (int(bad.sum()), float((a - b_).abs().max()))
    close_but(r1.grad[..., :n_off].cpu().double(), gr0[..., :n_off], 1e-3, 2e-4, 4)
    torch.testing.assert_close(r1.grad[..., n_off:].cpu().double(), gr0[..., n_off:], rtol=1e-3, atol=1e-4)
    assert float(r1.grad.view(B, S, -1)[0, 7, 3 * 24 + (2 * 4 + 1) * 2]) == 0.0  # the point outside every image
    # the same numbers through the unfused composition on the device (ops.ms_deform_attn + torch's prologue): same kernels
    # underneath, so the two agree far inside the oracle tolerance
    v2, r2 = dev(value).requires_grad_(), dev(rows).requires_grad_()
    ref_pts = dev(O.reference_points(shapes, 1)[0].contiguous())
    norm = dev(torch.tensor([[ww, hh] for hh, ww in shapes], dtype=torch.float32))
    loc = ref_pts[None, :, None, :, None, :] + r2[..., :n_off].view(B, S, H, 3, 4, 2) / norm[None, None, None, :, None, :]
    aw = torch.softmax(r2[..., n_off:].view(B, S, H, 12), -1).view(B, S, H, 3, 4)
    out2 = ops.ms_deform_attn(v2, shapes, loc, aw)
    out2.backward(dev(go))
    # (the composition rounds offsets / (W, H) and multiplies back: sampling pixels differ by an ulp or two of the coordinate)
    torch.testing.assert_close(out.detach(), out2.detach(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(v1.grad, v2.grad, rtol=1e-4, atol=1e-4)
    close_but(r1.grad.cpu(), r2.grad.cpu(), 1e-3, 3e-4, 8)


@pytest.mark.parametrize("shapes,B", [([(8, 8), (16, 16), (32, 32)], 2), ([(5, 7), (10, 14), (20, 28)], 3)])
def test_k1_rows_training_op_bf16(ops, shapes, B):
    """The bf16 form (rows, out, grad_out, grad_rows bf16; value cast to fp32 once): on bf16-representable inputs it is the fp32
    form's arithmetic with ONE rounding of each output to bf16."""
    H = 8
    value, off, logits, go = _rows_case(shapes, B, 2.0, seed=22)
    S = value.shape[1]
    bf = lambda t: t.to(torch.bfloat16)
    rows = bf(torch.cat([off.reshape(B, S, -1), logits.reshape(B, S, -1)], -1)).contiguous()
    value, go = bf(value), bf(go)
    v1, r1 = dev(value.float()).requires_grad_(), dev(rows.float()).requires_grad_()
    out1 = ops.ms_deform_attn_rows(v1, shapes, r1, H)
    out1.backward(dev(go.float()))
    v2, r2 = dev(value).requires_grad_(), dev(rows).requires_grad_()
    assert ops.k1_rows_applies(v2, r2, shapes, H)
    out2 = ops.ms_deform_attn_rows(v2, shapes, r2, H)
    assert out2.dtype == torch.bfloat16
    out2.backward(dev(go))
    assert v2.grad.dtype == torch.bfloat16 and r2.grad.dtype == torch.bfloat16
    assert torch.equal(out2.detach(), out1.detach().to(torch.bfloat16))  # same arithmetic, one rounding
    # grad_value: the fp32 sums differ only by the order of the atomics; then one rounding
    torch.testing.assert_close(v2.grad.float(), v1.grad, rtol=1e-2, atol=1e-2 * float(v1.grad.abs().max()) / 16)
    # row gradients: the fp32 form's numbers to within one bf16 rounding (two template instantiations of one source: the compiler
    # may contract their multiply-adds differently, an fp32 ulp that now and then crosses a bf16 rounding boundary)
    torch.testing.assert_close(r2.grad.float(), r1.grad, rtol=2.0 ** -7, atol=1e-6 * float(r1.grad.abs().max()))
    assert float((r2.grad != r1.grad.to(torch.bfloat16)).float().mean()) < 1e-3
    # under torch.autocast the module route hands bf16 rows to the same op
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out3 = ops.ms_deform_attn_rows(dev(value), shapes, dev(rows), H)
    assert torch.equal(out3, out2.detach())


@pytest.mark.parametrize("shapes,B,scale", [([(8, 8), (16, 16), (32, 32)], 2, 1.0), ([(5, 7), (10, 14), (20, 28)], 1, 1e-6),
                                            ([(12, 20), (24, 40)], 2, 3e4)])
def test_k1_backward_deterministic_form(ops, shapes, B, scale):
    """wm2f_msdeform_bwd_det: the grad_value scatter as integer adds in one fixed-point unit per (image, head).  Against
    the oracle's autograd like the float-atomic form (gradient magnitudes from 1e-6 to 3e4: the unit follows the
    largest |grad_out|), bit-identical from run to run and under a different stream of other work, with one image's
    gradients a million times smaller than the other's, and through torch's deterministic-algorithms switch."""
    H, D, L, P = 8, 32, len(shapes), 4
    g = torch.Generator().manual_seed(17)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(B, S, H, D, generator=g)
    off = torch.randn(B, S, H, L, P, 2, generator=g) * 2.5
    off[0, 5, 1, 0, 2] = torch.tensor([-30.0, 25.0])  # out of every window: the straight-to-memory adds
    off[0, 9, 2, L - 1, 1] = torch.tensor([14.0, -9.0])
    ref_pts = O.reference_points(shapes, 1)[0].contiguous()
    norm = torch.tensor([[ww, hh] for hh, ww in shapes], dtype=torch.long)
    loc = (ref_pts[None, :, None, :, None, :] + off / norm[None, None, None, :, None, :]).contiguous()
    w = torch.softmax(torch.randn(B, S, H, L * P, generator=g), -1).view(B, S, H, L, P).contiguous()
    go = torch.randn(B, S, H * D, generator=g) * scale
    if B > 1:
        go[1] *= 1e-6
    v0, l0, w0 = value.clone().requires_grad_(), loc.clone().requires_grad_(), w.clone().requires_grad_()
    O.msdeform_attn_core(v0, shapes, l0, w0).backward(go)
    gv, gl, gw = ops.ms_deform_attn_bwd(dev(value), shapes, dev(loc), dev(w), dev(go), deterministic=True)
    for b in range(B):
        ref = v0.grad[b]
        torch.testing.assert_close(gv[b].cpu(), ref, rtol=1e-4, atol=2e-5 * float(go[b].abs().max()))
    torch.testing.assert_close(gw.cpu(), w0.grad, rtol=1e-4, atol=2e-5 * scale)
    torch.testing.assert_close(gl.cpu(), l0.grad, rtol=1e-3, atol=2e-4 * scale)
    for _ in range(3):
        junk = torch.randn(1 << 20, device=gv.device).sin_()  # other work in flight
        gv2, gl2, gw2 = ops.ms_deform_attn_bwd(dev(value), shapes, dev(loc), dev(w), dev(go), deterministic=True)
        assert torch.equal(gv2, gv) and torch.equal(gl2, gl) and torch.equal(gw2, gw)
        del junk
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        v1, l1, w1 = dev(value).requires_grad_(), dev(loc).requires_grad_(), dev(w).requires_grad_()
        ops.ms_deform_attn(v1, shapes, l1, w1).backward(dev(go))
        assert torch.equal(v1.grad, gv)
        with pytest.raises(RuntimeError):  # no fixed-point form for head_dim 16: refused under the switch, not silently float atomics
            ops.ms_deform_attn_bwd(dev(value[..., :16].contiguous()), shapes, dev(loc), dev(w), dev(go[..., :H * 16].contiguous()))
    finally:
        torch.use_deterministic_algorithms(prev)


def test_k1_backward_deterministic_warn_only_takes_the_other_kernel(ops):
    """A shape without a fixed-point form (head_dim 16) under the deterministic switch in warn-only mode: the library answers
    "unsupported", and the float-atomic backward runs behind the same call.  Against the oracle's autograd, at the
    tolerances of test_k1_backward."""
    shapes, B, H, D = [(2, 2), (4, 4)], 1, 2, 16
    value, loc, w = _rand_k1(B, shapes, H, D, 5, spread=1.1)
    go = torch.randn(B, value.shape[1], H * D, generator=torch.Generator().manual_seed(6))
    v0, l0, w0 = value.clone().requires_grad_(), loc.clone().requires_grad_(), w.clone().requires_grad_()
    O.msdeform_attn_core(v0, shapes, l0, w0).backward(go)
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        gv, gl, gw = ops.ms_deform_attn_bwd(dev(value), shapes, dev(loc), dev(w), dev(go))
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)
    torch.testing.assert_close(gv.cpu(), v0.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(gw.cpu(), w0.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(gl.cpu(), l0.grad, rtol=1e-3, atol=1e-4)


def test_k1_rows_applies_follows_the_package_flag(ops):
    """The rows kernels have no deterministic form: ops.K1_BWD_DETERMINISTIC = True, assigned on the package, turns
    k1_rows_applies off at the smallest shape those kernels accept.  No launch."""
    shapes, B, H = [(1, 1), (2, 2), (4, 4)], 1, 2
    value = torch.zeros(B, 21, H, 32, device="cuda")
    rows = torch.zeros(B, 21, H * 36, device="cuda")
    assert ops.k1_rows_applies(value, rows, shapes, H) is True
    prev = ops.K1_BWD_DETERMINISTIC
    ops.K1_BWD_DETERMINISTIC = True
    try:
        assert ops.k1_rows_applies(value, rows, shapes, H) is False
    finally:
        ops.K1_BWD_DETERMINISTIC = prev


# ----------------------------------------------------------------------------------------- K3
def test_k3_golden(ops):
    g = load_golden("k3_mask_predictor.npz")
    out = ops.mask_einsum(dev(T(g["mask_embeddings"])), dev(T(g["pix"])))
    torch.testing.assert_close(out.cpu(), T(g["logits"]), rtol=1e-4, atol=1e-4)
    for i in range(5):
        m, ro = ops.attn_mask_build(dev(T(g["logits"])), g[f"size_{i}"])
        exp = T(g[f"attn_mask_{i}"])
        mism = (m.cpu().bool() != exp).float().mean().item()
        assert mism <= 1e-5, f"size {g[f'size_{i}']}: {mism}"
        assert torch.equal(ro.cpu().bool(), ~exp.all(-1))


@pytest.mark.parametrize("B,Q,C,H,W", [(2, 100, 256, 64, 64), (1, 200, 256, 32, 48), (2, 10, 64, 16, 24),
                                       (1, 37, 128, 20, 36), (1, 100, 256, 3, 12), (2, 20, 64, 8, 8), (1, 68, 256, 16, 16),
                                       (1, 99, 256, 8, 16), (1, 224, 256, 8, 8),
                                       # 1..4 rows over a multiple of 16 with small C (regression: wrong main-tile rows)
                                       (2, 100, 64, 32, 48), (1, 200, 64, 24, 32), (2, 84, 64, 24, 32), (2, 100, 128, 32, 48),
                                       (1, 200, 128, 24, 32), (2, 68, 32, 16, 20)])
def test_k3_random(ops, B, Q, C, H, W):
    g = torch.Generator().manual_seed(5)
    emb = torch.randn(B, Q, C, generator=g)
    pix = torch.randn(B, C, H, W, generator=g)
    ref = torch.einsum("bqc,bchw->bqhw", emb.double(), pix.double())
    out = ops.mask_einsum(dev(emb), dev(pix)).cpu()
    scale = ref.abs().max().item()
    assert (out.double() - ref).abs().max().item() <= 2e-6 * scale * math.sqrt(C)
    # exact-integer data pins the fragment layout (a swapped row/col map cannot pass)
    emb_i = torch.randint(-3, 4, (B, Q, C), generator=g).float()
    pix_i = torch.randint(-3, 4, (B, C, H, W), generator=g).float()
    assert torch.equal(ops.mask_einsum(dev(emb_i), dev(pix_i)).cpu(), torch.einsum("bqc,bchw->bqhw", emb_i, pix_i))


@pytest.mark.parametrize("B,Q,C,H,W", [(8, 100, 256, 32, 32), (8, 100, 256, 64, 64), (2, 100, 256, 128, 128), (1, 100, 256, 32, 32),
                                       (2, 200, 256, 16, 24), (1, 37, 64, 5, 16), (3, 16, 32, 8, 8), (1, 5, 16, 2, 2),
                                       (2, 100, 64, 32, 48), (1, 113, 128, 20, 36), (8, 100, 256, 8, 8)])
def test_k3_fused_attention_mask_epilogue(ops, B, Q, C, H, W):
    """wm2f_mask_einsum_attn_mask_fwd (HF:2046 + :2051-2053 + :1912-1914 in one launch, no logits written), over the
    shapes that exercise every work split (1 / 2 / 4 / 6+4 / 7 row tiles per wave, 4- and 8-wave workgroups, ragged
    strips and query tails).  Exact integer operands give exact logits, so every bit is decided: blocked <=> logit < 0
    (a zero logit has sigmoid 0.5, which is not < 0.5).  Then real-valued operands against the two-launch route
    (einsum, then threshold): equal wherever the logit is clear of the threshold."""
    g = torch.Generator().manual_seed(B * 1000 + Q + H)
    emb_i = torch.randint(-3, 4, (B, Q, C), generator=g).float()
    pix_i = torch.randint(-3, 4, (B, C, H, W), generator=g).float()
    emb_i[0, min(3, Q - 1)] = 5.0
    pix_i[0] = pix_i[0].abs() * -1.0 - 1.0 if B > 1 else pix_i[0]  # image 0 (when there are several): query 3 blocked everywhere
    logits = torch.einsum("bqc,bchw->bqhw", emb_i, pix_i).flatten(2)
    m, ro = ops.mask_einsum_attn_mask(dev(emb_i), dev(pix_i))
    assert m.shape == (B, Q, H * W) and m.dtype == torch.uint8 and ro.shape == (B, Q) and ro.dtype == torch.int32
    assert torch.equal(m.cpu().bool(), logits < 0)
    assert torch.equal(ro.cpu().bool(), ~(logits < 0).all(-1))
    if B > 1:
        assert not bool(ro[0, min(3, Q - 1)])  # a fully blocked row was present
    emb = torch.randn(B, Q, C, generator=g)
    pix = torch.randn(B, C, H, W, generator=g)
    lg = ops.mask_einsum(dev(emb), dev(pix))
    m2, ro2 = ops.attn_mask_build(lg, (H, W))
    m1, ro1 = ops.mask_einsum_attn_mask(dev(emb), dev(pix))
    clear = (lg.flatten(2).abs() > 1e-5 * lg.abs().max()).cpu()
    assert torch.equal(m1.cpu()[clear], m2.cpu()[clear])  # (the remainder rows take another summation order)
    assert (m1 != m2).float().mean().item() < 1e-4
    assert torch.equal(ro1.cpu().bool(), (m1 == 0).any(-1).cpu())


def test_k3_fused_attention_mask_epilogue_golden(ops):
    """The level-resolution route on the dependency's own vectors (k3_mask_predictor.npz): the mask features resized to
    the target size (wm2f_resize_bilinear), then the fused einsum + threshold, against the masks the dependency made by
    resizing its full-resolution logits (HF:2046-2054).  Resize and einsum commute in real arithmetic; in fp32 the two
    orders differ by rounding, so bits may differ only where the dependency's resized logit is within 1e-4 of its range
    of the threshold."""
    g = load_golden("k3_mask_predictor.npz")
    emb, pix, logits = dev(T(g["mask_embeddings"])), dev(T(g["pix"])), T(g["logits"])
    n = 0
    for i in range(5):
        size = tuple(int(v) for v in g[f"size_{i}"])
        if size[1] % 4:
            continue  # the route needs widths divisible by 4 (the model falls back to the two-launch route otherwise)
        n += 1
        m, ro = ops.mask_einsum_attn_mask(emb, ops.resize_bilinear(pix, size))
        exp = T(g[f"attn_mask_{i}"])
        resized = torch.nn.functional.interpolate(logits, size=size, mode="bilinear", align_corners=False).flatten(2)
        clear = resized.abs() > 1e-4 * resized.abs().max()
        got = m.cpu().bool()
        assert torch.equal(got[clear], exp[clear]), f"size {size}"
        assert (got != exp).float().mean().item() < 1e-3
        assert torch.equal(ro.cpu().bool(), ~got.all(-1))
    assert n >= 2


@pytest.mark.parametrize("B,Q,C,H,W", [(2, 100, 256, 64, 64), (1, 7, 64, 5, 13), (2, 200, 256, 16, 24), (1, 112, 32, 33, 8)])
def test_k3_bf16(ops, B, Q, C, H, W):
    """bf16 operands on the bf16 matrix cores, fp32 accumulation and output: against the exact fp32 products of the
    same bf16-rounded inputs (a bf16 x bf16 product is exact in fp32; only the summation order differs).  Ragged pixel
    counts, fewer / more than 112 queries, and the pixel-major transpose."""
    g = torch.Generator().manual_seed(31)
    emb = torch.randn(B, Q, C, generator=g).to(torch.bfloat16)
    pix = torch.randn(B, C, H, W, generator=g).to(torch.bfloat16)
    pix_t = ops.nchw_to_pixel_major_bf16(dev(pix))
    assert torch.equal(pix_t.cpu(), pix.reshape(B, C, H * W).transpose(1, 2).contiguous())
    out = ops.mask_einsum_bf16(dev(emb), dev(pix), pix_t)
    ref = torch.einsum("bqc,bchw->bqhw", emb.float(), pix.float())
    assert out.dtype == torch.float32
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("B,Q,C,H,W", [(2, 20, 64, 8, 12),      # 2 query steps, the second with 3 lane groups empty; 1.5 strips
                                       (1, 100, 256, 64, 64),   # the production shape at a small map
                                       (2, 112, 128, 16, 40),   # all 7 query steps full, 640 pixels = 10 strips, 2 channel groups
                                       (3, 36, 64, 24, 31),     # pixel ranges that end inside a 32-pixel step (744 pixels)
                                       (1, 200, 64, 8, 8),      # more than 112 queries: two library GEMMs
                                       (1, 12, 64, 2, 2)])      # HW % 8 != 0: two library GEMMs
def test_k3_bf16_backward(ops, B, Q, C, H, W):
    """bf16-autocast backward of the einsum: against the fp64 products of the SAME bf16-rounded operands (grad rounded to
    bf16 as torch's .to(bfloat16) does), so that only the fp32 accumulation order and the final rounding of the bf16
    outputs differ; g_emb run-to-run identical."""
    g = torch.Generator().manual_seed(32)
    emb = torch.randn(B, Q, C, generator=g).to(torch.bfloat16)
    pix = torch.randn(B, C, H, W, generator=g).to(torch.bfloat16)
    go = torch.randn(B, Q, H, W, generator=g)
    e, p = dev(emb).requires_grad_(True), dev(pix).requires_grad_(True)
    out = ops.mask_einsum_bf16(e, p, ops.nchw_to_pixel_major_bf16(p)) if Q <= 112 else None
    gob = go.to(torch.bfloat16).double()
    ge_ref = torch.einsum("bqhw,bchw->bqc", gob, pix.double())
    gp_ref = torch.einsum("bqc,bqhw->bchw", emb.double(), gob)
    if out is not None:
        out.backward(dev(go))
        ge, gp = e.grad, p.grad
    else:
        ge, gp = ops.mask_einsum_bf16_bwd(dev(emb), dev(pix), dev(go))
    assert ge.dtype == torch.bfloat16 and gp.dtype == torch.bfloat16 and gp.shape == pix.shape
    # one bf16 rounding of the result (2^-9 relative) on top of an fp32 sum
    torch.testing.assert_close(ge.double().cpu(), ge_ref, rtol=4e-3, atol=4e-3 * float(ge_ref.abs().max()) / 16)
    torch.testing.assert_close(gp.double().cpu(), gp_ref, rtol=4e-3, atol=4e-3 * float(gp_ref.abs().max()) / 16)
    ge2, gp2 = ops.mask_einsum_bf16_bwd(dev(emb), dev(pix), dev(go))
    assert torch.equal(ge2, ge) and torch.equal(gp2, gp)
    assert ops.mask_einsum_bf16_bwd_applies(Q, C, H * W) == (Q <= 112 and (H * W) % 8 == 0)


@pytest.mark.parametrize("B,Q,C,H,W", [(2, 20, 64, 8, 12),      # one row tile + 4, one super-step of queries with 3 lane groups empty
                                       (1, 100, 256, 64, 64),   # the production shape at a small map: 4 channel chunks, 7 query tiles
                                       (2, 200, 256, 20, 36),   # two query chunks (config 4), pixel count not a multiple of 16 or 64
                                       (1, 16, 128, 2, 2),      # a single 4-pixel step, queries a whole super-step
                                       (3, 36, 64, 50, 50),     # pixel ranges that end inside a 16-pixel step
                                       (1, 10, 32, 4, 4)])      # outside the kernels' shapes (C % 64, Q % 4): two library GEMMs
def test_k3_backward(ops, B, Q, C, H, W):
    """Both gradients of the einsum (HF:2046 under autograd) from wm2f_mask_einsum_bwd against fp64 autograd of the same
    einsum, and g_emb run-to-run identical (fixed summation order, no atomics)."""
    g = torch.Generator().manual_seed(6)
    emb, pix = torch.randn(B, Q, C, generator=g), torch.randn(B, C, H, W, generator=g)
    go = torch.randn(B, Q, H, W, generator=g)
    e0, p0 = emb.double().requires_grad_(), pix.double().requires_grad_()
    torch.einsum("bqc,bchw->bqhw", e0, p0).backward(go.double())
    assert ops.mask_einsum_bwd_applies(Q, C, H * W) == (C % 64 == 0 and Q % 4 == 0)
    e1, p1 = dev(emb).requires_grad_(), dev(pix).requires_grad_()
    ops.mask_einsum(e1, p1).backward(dev(go))
    # |g_emb| ~ sqrt(HW), |g_pix| ~ sqrt(Q): fp32 sums of that many products
    torch.testing.assert_close(e1.grad.cpu().double(), e0.grad, rtol=1e-4, atol=2e-5 * (H * W) ** 0.5 + 1e-4)
    torch.testing.assert_close(p1.grad.cpu().double(), p0.grad, rtol=1e-4, atol=1e-4)
    ge, gp = ops.mask_einsum_bwd(dev(emb), dev(pix), dev(go))
    assert torch.equal(ge, e1.grad) and torch.equal(gp, p1.grad)
    only_e, none_p = ops.mask_einsum_bwd(dev(emb), dev(pix), dev(go), True, False)
    assert none_p is None and torch.equal(only_e, ge)
    none_e, only_p = ops.mask_einsum_bwd(dev(emb), dev(pix), dev(go), False, True)
    assert none_e is None and torch.equal(only_p, gp)


# ----------------------------------------------------------------------------------------- K2
@pytest.mark.parametrize("tag", ["small", "q100"])
def test_k2_golden(ops, tag):
    g = load_golden(f"k2_masked_xattn_{tag}.npz")
    H = int(g["n_heads"])
    q, k, v = T(g["q_proj"]), T(g["k_proj"]), T(g["v_proj"])  # (Q|N, B, E)
    E = q.shape[-1]
    D = E // H
    mask = T(g["mask"])
    qb = (q.transpose(0, 1) * (1.0 / math.sqrt(D))).contiguous()
    kb, vb = k.transpose(0, 1).contiguous(), v.transpose(0, 1).contiguous()
    row_open = (~mask.all(-1)).to(torch.int32)
    ctx = ops.masked_xattn(dev(qb), dev(kb), dev(vb), dev(mask.to(torch.uint8)), dev(row_open), H)  # (B,Q,E)
    out = torch.nn.functional.linear(ctx.cpu(), T(g["out_proj_weight"]), T(g["out_proj_bias"])).transpose(0, 1)
    torch.testing.assert_close(out, T(g["out"]), rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("B,H,Q,N,D,use_mask", [(2, 8, 100, 1024, 32, True), (1, 8, 100, 1000, 32, True),
                                                (2, 2, 10, 37, 32, True), (1, 4, 200, 256, 32, True),
                                                (2, 8, 100, 512, 32, False), (1, 2, 50, 300, 64, True),
                                                (1, 4, 20, 130, 16, True),
                                                # N % 16 == 0: the full-tile kernel, incl. waves with no tile (N = 16), odd tile
                                                # counts per wave (the half-iteration on a dead tile) and all head sizes
                                                (1, 4, 20, 16, 32, True), (1, 2, 130, 80, 32, True), (2, 8, 100, 208, 32, True),
                                                (1, 2, 50, 1040, 64, True), (1, 4, 20, 144, 16, True), (1, 8, 100, 4096, 32, False)])
def test_k2_random(ops, B, H, Q, N, D, use_mask):
    g = torch.Generator().manual_seed(7)
    E = H * D
    q = torch.randn(B, Q, E, generator=g) * 0.5
    k = torch.randn(B, N, E, generator=g)
    v = torch.randn(B, N, E, generator=g)
    mask = torch.rand(B, Q, N, generator=g) < 0.7
    mask[0, 0] = True  # fully blocked row -> attends everywhere
    mask[0, 1, :-1] = True
    mask[0, 1, -1] = False
    sh = lambda t, n: t.view(B, n, H, D).permute(0, 2, 1, 3)
    ref = O.masked_attention_core(sh(q, Q), sh(k, N), sh(v, N), mask if use_mask else torch.zeros_like(mask))
    ref = ref.permute(0, 2, 1, 3).reshape(B, Q, E)
    if use_mask:
        ro = (~mask.all(-1)).to(torch.int32)
        out = ops.masked_xattn(dev(q), dev(k), dev(v), dev(mask.to(torch.uint8)), dev(ro), H)
    else:
        out = ops.masked_xattn(dev(q), dev(k), dev(v), None, None, H)
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("B,H,Q,N,D", [(2, 8, 100, 1024, 32), (1, 2, 37, 80, 32), (1, 4, 130, 272, 16), (1, 2, 50, 2064, 64)])
def test_k2_full_tile_kernel_matches_general(ops, B, H, Q, N, D):
    """The N % 16 == 0 kernel (log2-domain softmax, buffer addressing) against the general kernel on the same inputs.
    The library takes the full-tile kernel when the mask's address is dword-aligned; the same mask bytes at an odd
    address go through the general kernel (no environment knob: the production library reads none)."""
    g = torch.Generator().manual_seed(N + Q)
    E = H * D
    q, k, v = dev(torch.randn(B, Q, E, generator=g) * 0.5), dev(torch.randn(B, N, E, generator=g)), dev(torch.randn(B, N, E, generator=g))
    mask = torch.rand(B, Q, N, generator=g) < 0.8
    mask[0, 0] = True
    ro = dev((~mask.all(-1)).to(torch.int32))
    m8 = dev(mask.to(torch.uint8))
    odd = torch.empty(m8.numel() + 8, dtype=torch.uint8, device=m8.device)[1:1 + m8.numel()].view_as(m8)
    odd.copy_(m8)
    assert m8.data_ptr() % 4 == 0 and odd.data_ptr() % 4 == 1 and odd.is_contiguous()
    outs = [ops.masked_xattn(q, k, v, odd, ro, H).clone(), ops.masked_xattn(q, k, v, m8, ro, H).clone()]
    torch.testing.assert_close(outs[1], outs[0], rtol=2e-5, atol=5e-6)
    assert not torch.equal(outs[1], outs[0]) or N < 64  # two different kernels did run (different rounding)


@pytest.mark.parametrize("B,H,Q,N,D,use_mask", [(2, 8, 100, 256, 32, True), (1, 2, 10, 37, 32, True),
                                                (1, 4, 50, 130, 32, False), (1, 2, 30, 100, 64, True),
                                                (1, 4, 20, 70, 16, True),
                                                # more queries than one workgroup's tiles: dK / dV sum over query chunks
                                                # (regression: the chunks overwrote each other)
                                                (2, 8, 200, 300, 32, True), (1, 2, 53, 283, 64, True), (1, 1, 146, 114, 16, True)])
def test_k2_backward(ops, B, H, Q, N, D, use_mask):
    g = torch.Generator().manual_seed(17)
    E = H * D
    q = torch.randn(B, Q, E, generator=g) * 0.5
    k = torch.randn(B, N, E, generator=g)
    v = torch.randn(B, N, E, generator=g)
    go = torch.randn(B, Q, E, generator=g)
    mask = torch.rand(B, Q, N, generator=g) < 0.6
    mask[0, 0] = True
    if not use_mask:
        mask = torch.zeros_like(mask)
    sh = lambda t, n: t.view(B, n, H, D).permute(0, 2, 1, 3)
    q0, k0, v0 = q.clone().requires_grad_(), k.clone().requires_grad_(), v.clone().requires_grad_()
    ref = O.masked_attention_core(sh(q0, Q), sh(k0, N), sh(v0, N), mask).permute(0, 2, 1, 3).reshape(B, Q, E)
    ref.backward(go)
    q1, k1, v1 = dev(q).requires_grad_(), dev(k).requires_grad_(), dev(v).requires_grad_()
    ro = (~mask.all(-1)).to(torch.int32)
    out = ops.masked_xattn(q1, k1, v1, dev(mask.to(torch.uint8)) if use_mask else None, dev(ro) if use_mask else None, H)
    out.backward(dev(go))
    torch.testing.assert_close(q1.grad.cpu(), q0.grad, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(k1.grad.cpu(), k0.grad, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(v1.grad.cpu(), v0.grad, rtol=1e-4, atol=2e-5)


# ----------------------------------------------------------------------------------------- K4
@pytest.mark.parametrize("NL,B,Q,Tmax,kind", [(3, 4, 100, 16, "randn"), (2, 3, 100, 16, "ties"), (1, 5, 10, 24, "randn"), (2, 2, 7, 7, "ties"),
                                              (1, 3, 200, 40, "randn"), (1, 2, 1, 5, "randn"), (1, 2, 130, 1, "randn"), (2, 2, 64, 65, "ties"),
                                              (10, 16, 100, 16, "randn")])
def test_lsa_batched_equals_scipy(ops, NL, B, Q, Tmax, kind):
    """ops.lsa_batched (the assignment on the device, csrc/lsa.hip) returns scipy.optimize.linear_sum_assignment's indices BIT for
    BIT on every (level, image) problem: random costs, tie-heavy small-integer costs (the tie rule and the scan order decide),
    fewer targets than queries (solved transposed) and more, a different target count per image, single rows / columns."""
    from scipy.optimize import linear_sum_assignment
    g = torch.Generator().manual_seed(NL * 1000 + Q + Tmax)
    if kind == "randn":
        cost = torch.randn(NL, B, Q, Tmax, generator=g)
    else:
        cost = torch.randint(0, 3, (NL, B, Q, Tmax), generator=g).float()
    counts = [int(x) for x in torch.randint(1, Tmax + 1, (B,), generator=g)]
    counts[0] = Tmax
    matched = [min(Q, c) for c in counts]
    rows, cols = ops.lsa_batched(dev(cost), dev(torch.tensor(counts, dtype=torch.int32)), max(matched))
    rows, cols = rows.cpu().numpy(), cols.cpu().numpy()
    for l in range(NL):
        for b in range(B):
            r, c = linear_sum_assignment(cost[l, b, :, :counts[b]].numpy())
            assert np.array_equal(rows[l, b, :matched[b]], r) and np.array_equal(cols[l, b, :matched[b]], c), (l, b)


def test_k4_golden_cost_and_indices(ops):
    g = load_golden("k4_matcher.npz")
    wc, wm, wd = [float(x) for x in g["weights"]]
    B = g["mask_logits"].shape[0]
    counts = [g[f"mask_labels_{i}"].shape[0] for i in range(B)]
    for tgt_dtype in (torch.float32, torch.uint8):
        tgt = torch.cat([T(g[f"mask_labels_{i}"]) for i in range(B)]).to(tgt_dtype)
        cls = torch.cat([T(g[f"class_labels_{i}"]) for i in range(B)])
        cost = ops.matcher_cost(dev(T(g["mask_logits"])[None]), dev(T(g["class_logits"])[None]), dev(tgt), counts,
                                dev(cls), dev(T(g["points"])[None]), wc, wm, wd)[0].cpu()
        for i in range(B):
            c = cost[i, :, :counts[i]]
            torch.testing.assert_close(c, T(g[f"cost_{i}"]), rtol=1e-5, atol=1e-5)
            r, col = O.hungarian(c)
            assert np.array_equal(r.numpy(), g[f"row_{i}"]) and np.array_equal(col.numpy(), g[f"col_{i}"])


def test_k4_multi_level_ragged(ops):
    g = torch.Generator().manual_seed(8)
    NL, B, Q, h, w, Ht, Wt, P, C1 = 3, 3, 25, 16, 20, 64, 80, 500, 4
    ml = torch.randn(NL, B, Q, h, w, generator=g) * 2
    cl = torch.randn(NL, B, Q, C1, generator=g)
    counts = [11, 0, 3]
    tgt = (torch.rand(sum(counts), Ht, Wt, generator=g) < 0.3).float()
    cls = torch.randint(0, C1 - 1, (sum(counts),), generator=g)
    pts = torch.rand(NL, B, P, 2, generator=g)
    cost = ops.matcher_cost(dev(ml), dev(cl), dev(tgt), counts, dev(cls), dev(pts), 2.0, 5.0, 5.0).cpu()
    off = 0
    for b in range(B):
        for lvl in range(NL):
            if counts[b]:
                ref = O.matcher_cost(ml[lvl, b], cl[lvl, b], tgt[off:off + counts[b]], cls[off:off + counts[b]],
                                     pts[lvl, b:b + 1], 2.0, 5.0, 5.0)
                torch.testing.assert_close(cost[lvl, b, :, :counts[b]], ref, rtol=1e-5, atol=1e-5)
        off += counts[b]


@pytest.mark.parametrize("h,w,P,counts", [(300, 500, 2000, [20, 3]), (120, 501, 1100, [2, 17]), (64, 64, 1024, [5, 0])])
def test_k4_band_form(ops, h, w, P, counts):
    """P >= 1024: wm2f_matcher_cost groups the points by band of map rows and samples the predictions from LDS (18 / 4 bands / one
    band here; widths with and without 16-byte rows; more than 16 targets = two target chunks; an image without targets; points
    outside [0, 1], on the first row and beyond the last).  Same cost as the oracle, identical bits on a second run (the grouping
    is a stable counting sort), and the same cost for the points in another order up to summation order."""
    g = torch.Generator().manual_seed(18)
    NL, B, Q, Ht, Wt, C1 = 2, 2, 7, 96, 80, 4
    ml = torch.randn(NL, B, Q, h, w, generator=g) * 2
    cl = torch.randn(NL, B, Q, C1, generator=g)
    tgt = (torch.rand(sum(counts), Ht, Wt, generator=g) < 0.3).float()
    cls = torch.randint(0, C1 - 1, (sum(counts),), generator=g)
    pts = torch.rand(NL, B, P, 2, generator=g) * 1.1 - 0.05
    pts[:, :, :4, 1] = torch.tensor([0.0, 0.2 / h, 1.0, 1.0 - 0.2 / h])
    args = (dev(ml), dev(cl), dev(tgt), counts, dev(cls))
    cost = ops.matcher_cost(*args, dev(pts), 2.0, 5.0, 5.0)
    assert torch.equal(cost, ops.matcher_cost(*args, dev(pts), 2.0, 5.0, 5.0))
    perm = torch.randperm(P, generator=g)
    torch.testing.assert_close(ops.matcher_cost(*args, dev(pts[:, :, perm].contiguous()), 2.0, 5.0, 5.0), cost, rtol=1e-5, atol=1e-5)
    cost, off = cost.cpu(), 0
    for b in range(B):
        for lvl in range(NL):
            if counts[b]:
                ref = O.matcher_cost(ml[lvl, b], cl[lvl, b], tgt[off:off + counts[b]], cls[off:off + counts[b]],
                                     pts[lvl, b:b + 1], 2.0, 5.0, 5.0)
                torch.testing.assert_close(cost[lvl, b, :, :counts[b]], ref, rtol=1e-5, atol=1e-5)
        off += counts[b]


@pytest.mark.parametrize("R,n,k", [(7, 37632, 9408), (3, 1000, 250), (2, 64, 64), (5, 5000, 1), (4, 2049, 2048),
                                   (2, 40000, 300)])  # the last: more candidates than LDS holds -> the stock top-k behind the same call
def test_select_top_points_equals_topk_set(ops, R, n, k):
    """wm2f_select_top_points: the SET torch.topk returns (HF:688-704), written in index order; ties at the threshold go to the
    lowest indices; NaN ranks highest; entries beyond k are the caller's."""
    g = torch.Generator().manual_seed(23)
    score = -torch.randn(R, n, generator=g).abs()
    ties = n <= 38400  # (the stock top-k behind the fallback picks its own members among equal scores)
    if ties:
        score[0, : n // 2] = torch.round(score[0, : n // 2] * 4) / 4  # many exact ties, some at the threshold
    if n > 100 and ties:
        score[1, 17] = float("nan")
        score[1, 5] = 0.0
        score[-1, :] = -1.0  # a constant row: the first k indices
    pts = torch.rand(R, n, 2, generator=g)
    out = ops.select_top_points(dev(score), dev(pts), k, k + 3).cpu()
    assert out.shape == (R, k + 3, 2)
    key = torch.where(torch.isnan(score), torch.full_like(score, float("inf")), score)
    # the reference set: sort by (score descending, index ascending), take k, then index order
    order = torch.sort(-key.double() * 1.0, dim=1, stable=True)[1][:, :k]
    ref_idx = torch.sort(order, dim=1)[0]
    ref = torch.gather(pts, 1, ref_idx[..., None].expand(-1, -1, 2))
    assert torch.equal(out[:, :k], ref)
    # and it is a top-k set in torch's sense: same multiset of scores as torch.topk
    tk = torch.topk(key, k, dim=1)[0]
    assert torch.equal(torch.sort(torch.gather(key, 1, ref_idx), dim=1, descending=True)[0], tk)


@pytest.mark.parametrize("B,N,C", [(3, 1000, 256), (2, 37, 4), (1, 5, 8)])
def test_add_broadcast(ops, B, N, C):
    g = torch.Generator().manual_seed(29)
    a, p = torch.randn(B, N, C, generator=g), torch.randn(1, N, C, generator=g)
    assert torch.equal(ops.add_broadcast(dev(a), dev(p)).cpu(), a + p)


# ----------------------------------------------------------------------------------------- point sampling
def test_point_sample_fwd_bwd(ops):
    g = torch.Generator().manual_seed(9)
    N, H, W, P = 5, 12, 17, 300
    feat = torch.randn(N, H, W, generator=g)
    pts = torch.rand(N, P, 2, generator=g) * 1.2 - 0.1
    go = torch.randn(N, P, generator=g)
    f0 = feat.clone().requires_grad_()
    ref = torch.nn.functional.grid_sample(f0[:, None], 2 * pts[:, :, None] - 1, align_corners=False)[:, 0, :, 0]
    ref.backward(go)
    f1 = dev(feat).requires_grad_()
    out = ops.point_sample(f1, dev(pts))
    out.backward(dev(go))
    torch.testing.assert_close(out.detach().cpu(), ref.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(f1.grad.cpu(), f0.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(out.detach().cpu(), O.sample_point(feat[:, None], pts)[:, 0], rtol=1e-5, atol=1e-6)
    u8 = (feat > 0).to(torch.uint8)
    out8 = ops.point_sample(dev(u8), dev(pts)).cpu()
    torch.testing.assert_close(out8, O.sample_point(u8[:, None].float(), pts)[:, 0], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("B,C,G,H,W,Hs,Ws", [(2, 64, 32, 32, 32, 16, 16), (1, 32, 8, 20, 28, 10, 14), (2, 16, 4, 9, 12, 5, 7),
                                             (1, 256, 32, 64, 64, 32, 32), (1, 8, 2, 6, 8, 6, 8)])
def test_group_norm_act(ops, B, C, G, H, W, Hs, Ws):
    """The FPN tails (HF:1395-1405): GroupNorm + bilinear upsample-add, and GroupNorm + ReLU, against the stock ops."""
    g = torch.Generator().manual_seed(H * W + C)
    x = torch.randn(B, C, H, W, generator=g) * 2.0 + 0.7
    up = torch.randn(B, C, Hs, Ws, generator=g)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    F = torch.nn.functional
    ref = F.group_norm(x, G, gamma, beta, 1e-5) + F.interpolate(up, size=(H, W), mode="bilinear", align_corners=False)
    out = ops.group_norm_act_(dev(x.clone()), G, dev(gamma), dev(beta), 1e-5, up=dev(up))
    torch.testing.assert_close(out.cpu(), ref, rtol=2e-5, atol=2e-5)
    ref2 = torch.relu(F.group_norm(x, G, gamma, beta, 1e-5))
    out2 = ops.group_norm_act_(dev(x.clone()), G, dev(gamma), dev(beta), 1e-5, relu=True)
    torch.testing.assert_close(out2.cpu(), ref2, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("B,C,G,H,W,use_bias", [(2, 64, 32, 8, 8, True), (1, 256, 32, 20, 28, True), (2, 48, 4, 6, 10, False),
                                                (1, 40, 8, 3, 4, True)])
def test_group_norm_tokens(ops, B, C, G, H, W, use_bias):
    """Input projection tail (HF:1341-1357): bias + GroupNorm written transposed into its rows of the token buffer."""
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3
    bias = torch.randn(C, generator=g) if use_bias else None
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    xb = x + (bias[None, :, None, None] if use_bias else 0)
    ref = torch.nn.functional.group_norm(xb, G, gamma, beta, 1e-5).flatten(2).transpose(1, 2)
    S, start = H * W + 13, 5
    tokens = torch.full((B, S, C), 7.0)
    out = ops.group_norm_tokens_(dev(x), None if bias is None else dev(bias), G, dev(gamma), dev(beta), 1e-5, dev(tokens), start).cpu()
    torch.testing.assert_close(out[:, start:start + H * W], ref, rtol=2e-5, atol=2e-5)
    assert bool((out[:, :start] == 7.0).all()) and bool((out[:, start + H * W:] == 7.0).all())  # other rows untouched


@pytest.mark.parametrize("N,C,H,W,Ho,Wo", [(2, 5, 64, 64, 8, 8), (1, 3, 50, 84, 13, 20), (2, 4, 16, 16, 16, 16), (1, 2, 9, 12, 18, 24),
                                           (1, 6, 256, 256, 32, 32)])
def test_resize_bilinear(ops, N, C, H, W, Ho, Wo):
    """Down / identity / up: == F.interpolate(mode="bilinear", align_corners=False)."""
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(H + Wo))
    ref = torch.nn.functional.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False)
    torch.testing.assert_close(ops.resize_bilinear(dev(x), (Ho, Wo)).cpu(), ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("N,C,H,W", [(2, 5, 16, 24), (1, 3, 2, 8), (2, 64, 64, 64), (1, 7, 30, 40)])
def test_bias_relu_maxpool(ops, N, C, H, W):
    """ResNet stem tail: MaxPool2d(3, 2, 1)(ReLU(x + bias)) in one pass == the stock ops, bit for bit (max and add commute)."""
    g = torch.Generator().manual_seed(H + W)
    x, bias = torch.randn(N, C, H, W, generator=g), torch.randn(C, generator=g)
    ref = torch.nn.functional.max_pool2d(torch.relu(x + bias[None, :, None, None]), 3, 2, 1)
    out = ops.bias_relu_maxpool(dev(x), dev(bias))
    assert out.shape == ref.shape and torch.equal(out.cpu(), ref)


def test_fused_elementwise(ops):
    g = torch.Generator().manual_seed(21)
    x = torch.randn(3, 16, 6, 10, generator=g)
    bias, res = torch.randn(16, generator=g), torch.randn(3, 16, 6, 10, generator=g)
    for r, relu in ((None, True), (res, True), (res, False), (None, False)):
        ref = x + bias[None, :, None, None] + (0 if r is None else r)
        ref = torch.relu(ref) if relu else ref
        out = ops.bias_act_(dev(x.clone()), dev(bias), None if r is None else dev(r), relu)
        torch.testing.assert_close(out.cpu(), ref, rtol=1e-6, atol=1e-6)
    for shape in ((2, 5, 40, 52), (1, 3, 64, 132), (2, 7, 32, 32)):  # H*W/4 >= 256: the row form (1 and 3 chunks with tails, exact fit)
        x = torch.randn(*shape, generator=g)
        bias, res = torch.randn(shape[1], generator=g), torch.randn(*shape, generator=g)
        for r, relu in ((None, True), (res, True), (res, False)):
            ref = x + bias[None, :, None, None] + (0 if r is None else r)
            ref = torch.relu(ref) if relu else ref
            out = ops.bias_act_(dev(x.clone()), dev(bias), None if r is None else dev(r), relu)
            assert torch.equal(out.cpu(), ref)  # same additions in the same order
    rows, C = 77, 256
    a, b = torch.randn(2, rows, C, generator=g) * 3, torch.randn(2, rows, C, generator=g)
    gamma, beta, pos = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(rows, C, generator=g)
    ref = torch.nn.functional.layer_norm(a + b, (C,), gamma, beta, 1e-5)
    out, outp = ops.add_layernorm(dev(a), dev(b), dev(gamma), dev(beta), 1e-5, pos=dev(pos))
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(outp.cpu(), ref + pos[None], rtol=1e-5, atol=1e-5)
    out2 = ops.add_layernorm(dev(a), None, dev(gamma), dev(beta), 1e-5)
    torch.testing.assert_close(out2.cpu(), torch.nn.functional.layer_norm(a, (C,), gamma, beta, 1e-5), rtol=1e-5, atol=1e-5)


def test_cpu_tensor_is_refused(ops):
    from weed_instance_segmentation_amd._lib import Wm2fError
    with pytest.raises(Wm2fError):
        ops.mask_einsum(torch.randn(1, 4, 16), torch.randn(1, 16, 2, 2))


@pytest.mark.parametrize("N,C,H,W", [(2, 16, 64, 64), (1, 3, 8, 8), (2, 5, 24, 40), (1, 256, 256, 256), (3, 2, 16, 520)])
def test_resize_pyramid_equals_three_bilinear_resizes(ops, N, C, H, W):
    """wm2f_resize_pyramid: the 1/2, 1/4 and 1/8 size bilinear resizes in one pass -- bit for bit the generic kernel's
    output for each size (2 x 2 means with weights exactly 0.5) and torch's CPU interpolate to round-off."""
    g = torch.Generator().manual_seed(H * 7 + W)
    x = torch.randn(N, C, H, W, generator=g) * 3.0
    ys = ops.resize_pyramid(dev(x))
    for k, y in zip((1, 2, 3), ys):
        size = (H >> k, W >> k)
        assert y.shape == (N, C, *size)
        if size[1] % 4 == 0:
            assert torch.equal(y, ops.resize_bilinear(dev(x), size))
        ref = torch.nn.functional.interpolate(x, size=size, mode="bilinear", align_corners=False)
        torch.testing.assert_close(y.cpu(), ref, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        ops.resize_pyramid(dev(torch.zeros(1, 1, 12, 16)))


@pytest.mark.parametrize("M,K,N,relu,ln,res,pos", [(700, 256, 256, False, False, False, False), (4096 + 37, 256, 288, False, False, False, False),
                                                   (1000, 256, 256, False, True, True, False), (2 * 336, 1024, 256, False, True, True, True),
                                                   (16, 64, 256, True, False, False, False), (5, 128, 288, True, True, False, False),
                                                   (172032 // 8, 256, 256, False, True, True, True)])
def test_token_linear_fused_epilogues(ops, M, K, N, relu, ln, res, pos):
    """wm2f_token_linear_fwd (fp32 MFMA token GEMM with bias / ReLU / residual + LayerNorm / + pos fused) against the same
    chain of stock torch ops in fp64 on the CPU; exact-integer operands pin the fragment layout; ragged token counts (not a
    multiple of 16, fewer tokens than waves) exercise the tile split."""
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.1
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g) if res else None
    gamma, beta = (torch.randn(N, generator=g), torch.randn(N, generator=g)) if ln else (None, None)
    rows = M // 2 if (pos and M % 2 == 0) else M
    pe = torch.randn(rows, N, generator=g) if pos else None
    ref = torch.nn.functional.linear(x.double(), w.double(), b.double())
    if relu:
        ref = ref.relu()
    if ln:
        if res:
            ref = ref + r.double()
        ref = torch.nn.functional.layer_norm(ref, (N,), gamma.double(), beta.double(), 1e-5)
    out = ops.token_linear(dev(x), dev(w), dev(b), relu=relu, residual=dev(r) if res else None,
                           ln=(dev(gamma), dev(beta), 1e-5) if ln else None, pos=dev(pe) if pos else None)
    out_pos = None
    if pos:
        out, out_pos = out
    scale = ref.abs().max().item()
    assert (out.cpu().double() - ref).abs().max().item() <= 3e-6 * scale * math.sqrt(K)
    if pos:
        refp = ref + pe.double().repeat(M // rows, 1)
        assert (out_pos.cpu().double() - refp).abs().max().item() <= 3e-6 * refp.abs().max().item() * math.sqrt(K)
    assert ops.token_linear_applies(dev(x), dev(w))
    if not ln:
        xi = torch.randint(-3, 4, (M, K), generator=g).float()
        wi = torch.randint(-3, 4, (N, K), generator=g).float()
        bi = torch.randint(-5, 6, (N,), generator=g).float()
        exp = torch.nn.functional.linear(xi, wi, bi)
        assert torch.equal(ops.token_linear(dev(xi), dev(wi), dev(bi), relu=relu).cpu(), exp.relu() if relu else exp)
        # feature-group-major output (N / G, M, G): the same numbers at other addresses (G = 36 for N = 288: K1's head-major
        # operand rows; G = 64 / 4 for other splits), ragged last token tile included
        want = exp.relu() if relu else exp
        for G in ((36, 4) if N == 288 else (64, 4)):
            got = ops.token_linear(dev(xi), dev(wi), dev(bi), relu=relu, out_group=G)
            assert got.shape == (N // G, M, G)
            assert torch.equal(got.cpu(), want.view(M, N // G, G).permute(1, 0, 2))


@pytest.mark.parametrize("B,H,Q,N,use_mask", [(2, 8, 100, 1024, True), (1, 8, 100, 4096, True), (1, 4, 20, 16, True),
                                              (1, 2, 130, 80, True), (2, 8, 100, 208, True), (2, 8, 100, 512, False),
                                              (1, 8, 200, 16384, True)])
def test_k2_bf16_forward(ops, B, H, Q, N, use_mask):
    """wm2f_masked_xattn_bf16_fwd (bf16 q / k / v as the in_proj Linears emit them under autocast, bf16 MFMA products, fp32
    softmax): against the oracle's masked attention on the SAME bf16 values in fp32.  The only rounding the kernel adds is P
    to bf16 before the second product (relative 2^-9 per weight, averaged over the open keys): 4e-3 of the output range.
    Fully blocked rows (attend everywhere), a single open key, no mask at all, waves without a tile (N = 16), odd tile
    counts per wave, more than 112 queries (two query chunks)."""
    D = 32
    g = torch.Generator().manual_seed(7 + N)
    E = H * D
    q = (torch.randn(B, Q, E, generator=g) * 0.5).to(torch.bfloat16)
    k = torch.randn(B, N, E, generator=g).to(torch.bfloat16)
    v = torch.randn(B, N, E, generator=g).to(torch.bfloat16)
    mask = torch.rand(B, Q, N, generator=g) < 0.7
    mask[0, 0] = True  # fully blocked row -> attends everywhere
    mask[0, 1] = True
    mask[0, 1, N // 2] = False  # a single open key
    if not use_mask:
        mask = None
    assert ops.masked_xattn_bf16_applies(dev(q), dev(k), dev(v), H)
    row_open = None if mask is None else (~mask.all(-1)).to(torch.int32)
    out = ops.masked_xattn(dev(q), dev(k), dev(v), None if mask is None else dev(mask.to(torch.uint8)),
                           None if mask is None else dev(row_open), H)
    assert out.dtype == torch.float32
    sp = lambda t, n_: t.float().view(B, n_, H, D).permute(0, 2, 1, 3)
    ref = O.masked_attention_core(sp(q, Q), sp(k, N), sp(v, N), mask if mask is not None else torch.zeros(B, Q, N, dtype=torch.bool))
    ref = ref.permute(0, 2, 1, 3).reshape(B, Q, E)
    err = (out.cpu() - ref).abs().max().item()
    assert err <= 4e-3 * ref.abs().max().item(), (err, ref.abs().max().item())
    if mask is not None:  # the single-open-key row is that key's v exactly (p = 1, l = 1)
        torch.testing.assert_close(out[0, 1].cpu(), v[0, N // 2].float(), rtol=0, atol=1e-6)
    # fp32 operands still take the fp32 kernel
    assert not ops.masked_xattn_bf16_applies(dev(q.float()), dev(k.float()), dev(v.float()), H)


@pytest.mark.parametrize("B,H,Q,N", [(2, 8, 100, 1024), (1, 8, 100, 4096), (1, 4, 37, 272), (1, 2, 200, 512)])
def test_k2_bf16_autograd(ops, B, H, Q, N):
    """Training under autocast: bf16 forward and backward kernels (Q = 200: two query chunks, the fp32 backward on fp32
    copies) -- against the oracle's autograd in fp32 on the same bf16 values.  p, dS and the staged grad_out are rounded to
    bf16 as matrix operands: 1e-2 of each gradient's range."""
    D = 32
    g = torch.Generator().manual_seed(3)
    E = H * D
    q = (torch.randn(B, Q, E, generator=g) * 0.5).to(torch.bfloat16)
    k = torch.randn(B, N, E, generator=g).to(torch.bfloat16)
    v = torch.randn(B, N, E, generator=g).to(torch.bfloat16)
    mask = torch.rand(B, Q, N, generator=g) < 0.7
    mask[0, 0] = True
    go = torch.randn(B, Q, E, generator=g)
    qd, kd, vd = dev(q).requires_grad_(), dev(k).requires_grad_(), dev(v).requires_grad_()
    out = ops.masked_xattn(qd, kd, vd, dev(mask.to(torch.uint8)), dev((~mask.all(-1)).to(torch.int32)), H)
    out.backward(dev(go))
    qr, kr, vr = q.float().requires_grad_(), k.float().requires_grad_(), v.float().requires_grad_()
    sp = lambda t, n_: t.view(B, n_, H, D).permute(0, 2, 1, 3)
    ref = O.masked_attention_core(sp(qr, Q), sp(kr, N), sp(vr, N), mask).permute(0, 2, 1, 3).reshape(B, Q, E)
    ref.backward(go)
    for got, want in ((qd.grad, qr.grad), (kd.grad, kr.grad), (vd.grad, vr.grad)):
        assert got.dtype == torch.bfloat16
        assert (got.float().cpu() - want).abs().max().item() <= 1e-2 * want.abs().max().item()


@pytest.mark.parametrize("rows,pos_rows,x_bf16,want_lp,use_res", [(4096, 1024, True, True, True), (1000, 500, True, True, True),
                                                                 (777, 777, False, False, True), (130, 0, True, True, True),
                                                                 (3, 0, False, False, False), (5000, 2500, False, False, True)])
def test_add_layernorm_train(ops, rows, pos_rows, x_bf16, want_lp, use_res):
    """ops.add_layernorm_train (residual add + LayerNorm of the encoder layers in training, with the bf16 copy and y + pos from
    the same pass and ONE backward pass) against the same chain of stock torch ops with autograd, in fp64 on the CPU: all three
    outputs, and the gradients of x, residual, gamma, beta and pos when every output carries a gradient (and when only some do).
    Ragged row counts (not a multiple of the 128-row workgroup range), no residual, no pos; two backward runs give identical
    bits (gamma / beta partials are added in workgroup order)."""
    g = torch.Generator().manual_seed(rows)
    C = 256
    x = torch.randn(rows, C, generator=g) * 2
    if x_bf16:
        x = x.to(torch.bfloat16)
    res = torch.randn(rows, C, generator=g) if use_res else None
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    pos = torch.randn(pos_rows, C, generator=g) if pos_rows else None
    gy, glp = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g).to(torch.bfloat16)
    gyp = torch.randn(rows, C, generator=g)
    if x_bf16:
        gyp = gyp.to(torch.bfloat16)

    def run(with_gy=True):
        xd = dev(x).requires_grad_()
        rd = dev(res).requires_grad_() if use_res else None
        gd, bd = dev(gamma).requires_grad_(), dev(beta).requires_grad_()
        pd = dev(pos).requires_grad_() if pos is not None else None
        y, ylp, yp = ops.add_layernorm_train(xd, rd, gd, bd, 1e-5, pos=pd, want_bf16=want_lp, pos_bf16=x_bf16)
        outs, gs = [], []
        if with_gy:
            outs.append(y); gs.append(dev(gy))
        if want_lp:
            outs.append(ylp); gs.append(dev(glp))
        if pos is not None:
            outs.append(yp); gs.append(dev(gyp))
        torch.autograd.backward(outs, gs)
        return (y, ylp, yp), (xd.grad, None if rd is None else rd.grad, gd.grad, bd.grad, None if pd is None else pd.grad)

    (y, ylp, yp), grads = run()
    # reference in fp64
    xr = x.double().requires_grad_()
    rr = res.double().requires_grad_() if use_res else None
    gr, br = gamma.double().requires_grad_(), beta.double().requires_grad_()
    pr = pos.double().requires_grad_() if pos is not None else None
    yr = torch.nn.functional.layer_norm(xr + rr if use_res else xr, (C,), gr, br, 1e-5)
    loss = (yr * gy.double()).sum()
    if want_lp:
        loss = loss + (yr * glp.double()).sum()
    if pos is not None:
        ypr = yr + pr.repeat(rows // pos_rows, 1)
        loss = loss + (ypr * gyp.double()).sum()
    loss.backward()
    torch.testing.assert_close(y.cpu().double(), yr.detach(), rtol=1e-5, atol=2e-5)
    if want_lp:
        assert torch.equal(ylp, y.to(torch.bfloat16))
    if pos is not None:
        torch.testing.assert_close(yp.float().cpu().double(), ypr.detach(), rtol=1e-2 if x_bf16 else 1e-5, atol=3e-2 if x_bf16 else 2e-5)
    gx, gres, gg, gb, gp = grads
    tol = dict(rtol=2e-2, atol=3e-2) if x_bf16 else dict(rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(gx.float().cpu().double(), xr.grad, **tol)
    if use_res:
        torch.testing.assert_close(gres.cpu().double(), rr.grad, rtol=1e-4, atol=1e-4)
    scale = float(gr.grad.abs().max())
    assert (gg.cpu().double() - gr.grad).abs().max().item() <= 2e-5 * scale * math.sqrt(rows)
    assert (gb.cpu().double() - br.grad).abs().max().item() <= 2e-5 * float(br.grad.abs().max()) * math.sqrt(rows) + 1e-4
    if pos is not None:
        torch.testing.assert_close(gp.cpu().double(), pr.grad, rtol=1e-4, atol=1e-3)
    _, grads2 = run()
    for a_, b_ in zip(grads, grads2):
        assert (a_ is None and b_ is None) or torch.equal(a_, b_)
    if want_lp or pos is not None:  # a subset of the outputs carries a gradient (the last layer's y feeds no residual stream ...)
        _, g3 = run(with_gy=False)
        assert all(torch.isfinite(t).all() for t in g3 if t is not None)


@pytest.mark.parametrize("M,N,K", [(1000, 256, 256), (5000, 96, 256), (4097, 192, 256), (3000, 1024, 256), (3000, 256, 1024),
                                   (70, 288, 256), (63, 256, 256), (20000, 256, 256), (130, 8, 8), (777, 520, 264)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_token_wgrad(ops, M, N, K, dtype):
    """wm2f_token_wgrad_bf16 / _f32: dW = dy^T x and db = column sums of dy for the token Linears of the pixel decoder (bf16
    or fp32 operands, fp32 accumulation, partial tiles added in split order) against the same products in fp64 on the CPU.
    bf16 products are exact in fp32 and fp32 products are rounded once, so the summation order (and that rounding) is all
    that separates the two: a few fp32 ulps of sqrt(M) x the largest term.  Exact small-integer operands pin the transposed fragment reads (ds_read_b64_tr_b16), the XOR swizzle of the LDS
    image and the accumulator layout bit for bit; ragged token counts, feature counts that are not multiples of the 256-wide
    block (zero-filled through the buffer range check) and several column blocks (N or K = 1024) are included; two runs
    give identical bits (no atomics)."""
    g = torch.Generator().manual_seed(M + N + K)
    dy = torch.randn(M, N, generator=g).to(dtype)
    x = torch.randn(M, K, generator=g).to(dtype)
    assert ops.token_wgrad_applies(dev(dy), dev(x))
    dw, db = ops.token_wgrad(dev(dy), dev(x))
    ref_w = dy.double().t() @ x.double()
    ref_b = dy.double().sum(0)
    tol = 4e-6 * math.sqrt(M) * 3.0 * 3.0  # |dy|, |x| reach ~3 sigma
    assert dw.shape == (N, K) and dw.dtype == torch.float32 and db.shape == (N,)
    assert (dw.cpu().double() - ref_w).abs().max().item() <= tol, (dw.cpu().double() - ref_w).abs().max().item()
    assert (db.cpu().double() - ref_b).abs().max().item() <= tol
    dw2, db2 = ops.token_wgrad(dev(dy), dev(x))
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    # exact integers: every product and every partial sum is exact in fp32
    dyi = torch.randint(-3, 4, (M, N), generator=g).to(dtype)
    xi = torch.randint(-3, 4, (M, K), generator=g).to(dtype)
    dwi, dbi = ops.token_wgrad(dev(dyi), dev(xi))
    assert torch.equal(dwi.cpu(), (dyi.float().t() @ xi.float())) and torch.equal(dbi.cpu(), dyi.float().sum(0))
    dwn, dbn = ops.token_wgrad(dev(dyi), dev(xi), want_bias=False)
    assert dbn is None and torch.equal(dwn, dwi)


def test_linear_tokens_autograd_under_bf16_autocast(ops):
    """ops.linear_tokens (what the pixel decoder's encoder layers call in training): under bf16 autocast the same output as
    F.linear bit for bit, the same input gradient, and weight / bias gradients that agree with F.linear's autograd to bf16
    rounding (the library's come back rounded to bf16, the kernel's in fp32 -- compared against fp64); without autocast or
    without autograd it IS F.linear."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 700, 256, generator=g)
    w = (torch.randn(192, 256, generator=g) * 0.05)
    b = torch.randn(192, generator=g)
    go = torch.randn(3, 700, 192, generator=g)
    res = {}
    for name in ("wm2f", "torch"):
        xv, wv, bv = dev(x).requires_grad_(), dev(w).requires_grad_(), dev(b).requires_grad_()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = ops.linear_tokens(xv, wv, bv) if name == "wm2f" else torch.nn.functional.linear(xv, wv, bv)
        y.backward(dev(go).to(y.dtype))
        res[name] = (y.detach(), xv.grad, wv.grad, bv.grad)
    (ya, gxa, gwa, gba), (yb, gxb, gwb, gbb) = res["wm2f"], res["torch"]
    assert ya.dtype == torch.bfloat16 and torch.equal(ya, yb)
    assert gwa.dtype == torch.float32 and gxa.dtype == torch.float32
    torch.testing.assert_close(gxa, gxb, rtol=2e-2, atol=2e-2)
    gob, xb16 = go.to(torch.bfloat16).double().reshape(-1, 192), x.to(torch.bfloat16).double().reshape(-1, 256)
    ref_w, ref_b = gob.t() @ xb16, gob.sum(0)
    assert (gwa.cpu().double() - ref_w).abs().max().item() <= 1e-4 * ref_w.abs().max().item()
    assert (gba.cpu().double() - ref_b).abs().max().item() <= 1e-4 * ref_b.abs().max().item()
    assert (gwb.cpu().double() - ref_w).abs().max().item() <= 2e-2 * ref_w.abs().max().item()  # the library's, for scale
    # fp32 training (no autocast): the same output bits, gradients to fp32 round-off of the fp64 products
    xv, wv, bv = dev(x).requires_grad_(), dev(w).requires_grad_(), dev(b).requires_grad_()
    y32 = ops.linear_tokens(xv, wv, bv)
    assert y32.dtype == torch.float32 and torch.equal(y32, torch.nn.functional.linear(dev(x), dev(w), dev(b)))
    y32.backward(dev(go))
    rw, rb = go.double().reshape(-1, 192).t() @ x.double().reshape(-1, 256), go.double().reshape(-1, 192).sum(0)
    assert (wv.grad.cpu().double() - rw).abs().max().item() <= 1e-5 * rw.abs().max().item()
    assert (bv.grad.cpu().double() - rb).abs().max().item() <= 1e-5 * rb.abs().max().item()
    torch.testing.assert_close(xv.grad.cpu().double(), go.double() @ w.double(), rtol=1e-4, atol=1e-4)
    with torch.no_grad():  # no autograd: plain F.linear
        assert torch.equal(ops.linear_tokens(dev(x), dev(w), dev(b)), torch.nn.functional.linear(dev(x), dev(w), dev(b)))


@pytest.mark.parametrize("shapes,B", [([(25, 42), (50, 84), (100, 167)], 1), ([(7, 11), (13, 21), (25, 42)], 2),
                                      ([(3, 5), (6, 9), (12, 17)], 2), ([(13, 13), (25, 25), (50, 50)], 1)])
def test_k1_streaming_kernel_on_pyramids_that_are_not_1_2_4(ops, shapes, B):
    """Input sizes that are not multiples of 32 (BASELINE config 5: 1333 x 800 -> 25x42 / 50x84 / 100x167) give level sizes
    that only roughly double.  The streaming kernel takes them (variant 4 refuses a shape it cannot run, so a pass here IS
    that kernel): queries mapped to tiles by their reference points, window origins by division, up to 5 x 5 + 9 x 9 + 16 x 16
    queries a tile.  Both operand forms, local offsets (windows) and far ones (slow path), against the oracle and against
    the direct-gather kernel."""
    H, D, L, P = 8, 32, 3, 4
    g = torch.Generator().manual_seed(21)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(B, S, H, D, generator=g)
    ref_pts = O.reference_points(shapes, 1)[0].contiguous()
    norm = torch.tensor([[ww, hh] for hh, ww in shapes], dtype=torch.float32)
    for spread in (3.0, 12.0):
        off = (torch.rand(B, S, H, L, P, 2, generator=g) * 2 - 1) * spread
        logits = torch.randn(B, S, H, L * P, generator=g)
        loc = ref_pts[None, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
        aw = torch.softmax(logits, -1).view(B, S, H, L, P)
        ref = O.msdeform_attn_core(value, shapes, loc, aw)
        out_u = ops.ms_deform_attn_variant(dev(value), shapes, dev(loc), dev(aw), variant=4)
        out_f = ops.ms_deform_attn_variant(dev(value), shapes, dev(off), dev(logits), dev(ref_pts), fused=True, variant=4)
        out_d = ops.ms_deform_attn_variant(dev(value), shapes, dev(loc), dev(aw), variant=1)
        torch.testing.assert_close(out_u.cpu(), ref, rtol=1e-4, atol=1e-5)
        # the fused form rebuilds the sampling coordinate (ref * W - 0.5 + offset) instead of taking it from `loc`: at a
        # level 167 pixels wide one fp32 ulp of a coordinate is 1.5e-5 px -- the dependency's own (ref + off / W) * W - 0.5
        # carries the same noise -- and a unit-variance value map turns that into a few 1e-5 of output
        torch.testing.assert_close(out_f.cpu(), ref, rtol=1e-4, atol=2e-5 * max(1.0, shapes[2][1] / 32))
        torch.testing.assert_close(out_u, out_d, rtol=1e-4, atol=1e-5)
    assert not ops.k1_lanes_applies(shapes, S, D, P, B, H)  # the lane-major rows stay with the exact pyramids


# ----------------------------------------------------------------------------------------- point sampling over levels
@pytest.mark.parametrize("NL,N,M,H,W,P", [(3, 7, 5, 64, 64, 300),      # one band per map
                                          (2, 6, 4, 150, 256, 1000),   # 64-row bands, the last one ragged, points on band seams
                                          (1, 9, 9, 33, 50, 257),      # pixel count not a multiple of 4
                                          (4, 3, 3, 8, 12, 40),
                                          # >= 4096 points per map: the forward's LDS band form (two bands), square / odd / ragged maps
                                          (2, 5, 4, 256, 256, 5000), (1, 4, 3, 101, 77, 4100), (2, 3, 3, 150, 256, 4096)])
def test_point_sample_levels_forward_and_both_backwards(ops, NL, N, M, H, W, P):
    """sample_point (HF:245-274 = grid_sample, bilinear, align_corners False, zero padding) over level maps that are not
    stacked: forward against torch's grid_sample, and the two backward forms -- global atomics (any index) and the LDS
    band form for distinct indices (maps overwritten, untouched maps stay zero) -- against autograd of the same."""
    g = torch.Generator().manual_seed(41)
    maps = [torch.randn(N, H, W, generator=g) for _ in range(NL)]
    pts = torch.rand(NL, M, P, 2, generator=g) * 1.1 - 0.05  # some points outside [0, 1]
    pts[:, :, :8, 1] = torch.tensor([63.5, 64.0, 64.49, 64.5, 127.5, 128.0, 0.0, H - 0.01]) / H  # band seams and borders
    if P >= 4096:  # the forward band form's seam: top-corner rows (H + 1) // 2 - 1 and (H + 1) // 2, and the rows just outside the image
        hb = (H + 1) // 2
        pts[:, :, 8:14, 1] = torch.tensor([hb - 0.75, hb - 0.5, hb + 0.25, hb + 0.5, 0.25, H - 0.25]) / H
        pts[:, :, 14:18, 0] = torch.tensor([0.25, W - 0.25, -0.3, W + 0.3]) / W
    index = torch.stack([torch.randperm(N, generator=g)[:M] for _ in range(NL)]).to(torch.int32)
    go = torch.randn(NL, M, P, generator=g)
    refs, ref_grads = [], []
    for l in range(NL):
        ml = maps[l].clone().requires_grad_()
        sel = ml[index[l].long()][:, None]                                  # (M, 1, H, W)
        out = torch.nn.functional.grid_sample(sel, 2.0 * pts[l][:, None] - 1.0, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0, 0]
        out.backward(go[l])
        refs.append(out.detach())
        ref_grads.append(ml.grad)
    for unique in (False, True):
        dm = [dev(m).requires_grad_() for m in maps]
        out = ops.point_sample_levels(dm, dev(pts), dev(index), unique_index=unique)
        torch.testing.assert_close(out.cpu(), torch.stack(refs), rtol=1e-5, atol=1e-5)
        out.backward(dev(go))
        for l in range(NL):
            torch.testing.assert_close(dm[l].grad.cpu(), ref_grads[l], rtol=1e-4, atol=1e-5)
            untouched = torch.ones(N, dtype=torch.bool)
            untouched[index[l].long()] = False
            assert float(dm[l].grad[dev(untouched)].abs().max() if untouched.any() else 0.0) == 0.0
