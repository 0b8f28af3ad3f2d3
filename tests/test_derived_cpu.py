"""derived.py, the one cache for what the inference path derives from parameters (DESIGN.md "Derived weights"), on the
host: every derivation site against every way its sources can change, and that the cache stays out of the modules."""
import copy
import gc
import io
import math
import weakref

import pytest
import torch

from weed_instance_segmentation_amd import drop_derived, ops
from weed_instance_segmentation_amd.backbone_resnet import BottleNeckLayer, ConvLayer
from weed_instance_segmentation_amd.derived import derived, derived_peek
from weed_instance_segmentation_amd.modeling import MaskedCrossAttention, MSDeformAttn, SelfAttention


def _same(a, b):
    """torch.equal with the same dtype, over a tensor or a tuple of tensors."""
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def _fold(layer):
    c, bn = layer.convolution, layer.normalization
    scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
    return (c.weight * scale[:, None, None, None]).contiguous(), (bn.bias - bn.running_mean * scale).contiguous()


def _stir_batchnorm(m):
    for bn in m.modules():
        if isinstance(bn, torch.nn.BatchNorm2d):
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.data.uniform_(0.5, 1.5)
            bn.bias.data.uniform_(-0.2, 0.2)
    return m


class Site:
    """One derivation site: build() a module, run() it under no_grad, its `owner` and `name` in the cache, the parameter a
    mutation writes, and the derivation by hand."""
    fold = False

    def inputs(self, dtype):
        g = torch.Generator().manual_seed(1)
        return [torch.randn(*s, generator=g).to(dtype) for s in self.shapes]

    def run(self, m, dtype=torch.float32):
        with torch.no_grad():
            return m(*self.inputs(dtype))

    def owner(self, m):
        return m


class ConvSite(Site):
    name, shapes, fold = "fold", [(1, 8, 6, 5)], True

    def build(self):
        return _stir_batchnorm(ConvLayer(8, 16)).eval()

    def param(self, m):
        return m.convolution.weight

    def hand(self, m):
        return _fold(m)


class BottleneckSite(ConvSite):
    def build(self):
        return _stir_batchnorm(BottleNeckLayer(8, 16, 2)).eval()

    def owner(self, m):
        return m.layer[1]

    def param(self, m):
        return m.layer[1].convolution.weight

    def hand(self, m):
        return _fold(m.layer[1])


class SelfAttentionSite(Site):
    name, shapes = "qk", [(1, 3, 16), (1, 3, 16)]

    def build(self):
        return SelfAttention(16, 2).eval()

    def param(self, m):
        return m.q_proj.weight

    def hand(self, m):
        return (torch.cat([m.q_proj.weight * m.scaling, m.k_proj.weight], 0).contiguous(),
                torch.cat([m.q_proj.bias * m.scaling, m.k_proj.bias], 0).contiguous())


class QueryWeightSite(Site):
    name = "q"

    def build(self):
        m = MaskedCrossAttention(16, 2).eval()
        m.in_proj_bias.data.uniform_(-0.5, 0.5)
        return m

    def run(self, m, dtype=torch.float32):
        return m._q_weight()

    def param(self, m):
        return m.in_proj_weight

    def hand(self, m):
        sc = 1.0 / math.sqrt(m.head_dim)
        return (m.in_proj_weight[:16] * sc).contiguous(), (m.in_proj_bias[:16] * sc).contiguous()


class OffsetsLogitsSite(Site):
    def __init__(self, lanes):
        self.lanes, self.name = lanes, "offsets_logits_cat_lanes" if lanes else "offsets_logits_cat"

    def build(self):
        return MSDeformAttn(256, 8).eval()

    def run(self, m, dtype=torch.float32):
        return m._offsets_logits_weight(lanes=self.lanes)

    def param(self, m):
        return m.sampling_offsets.weight

    def hand(self, m):
        so, aw = m.sampling_offsets, m.attention_weights
        w, b = torch.cat([so.weight, aw.weight], 0), torch.cat([so.bias, aw.bias], 0)
        if self.lanes:
            idx = ops.k1_lane_order(8)
            w, b = w[idx], b[idx]
        return w.contiguous(), b.contiguous()


SITES = {"conv_layer": ConvSite(), "bottleneck": BottleneckSite(), "self_attention": SelfAttentionSite(),
         "q_weight": QueryWeightSite(), "offsets_logits": OffsetsLogitsSite(False), "offsets_logits_lanes": OffsetsLogitsSite(True)}


# --------------------------------------------------------------------------------------------------------- mutations
# each takes (site, module) and returns the dtype the module computes in afterwards
def _in_place(site, m):
    with torch.no_grad():
        site.param(m).mul_(-1.5)
    return torch.float32


def _data_assign(site, m):
    p = site.param(m)
    p.data = p.data * 2
    return torch.float32


def _double(site, m):
    m.double()
    return torch.float64


def _load_assign(site, m):
    torch.manual_seed(77)
    m.load_state_dict(site.build().state_dict(), assign=True)
    return torch.float32


def _running_var(site, m):
    with torch.no_grad():
        site.owner(m).normalization.running_var.mul_(3.0)
    return torch.float32


def _data_in_place_then_drop(site, m):
    site.param(m).data.mul_(2)
    drop_derived(m)
    return torch.float32


MUTATIONS = {"in_place": _in_place, "data_assign": _data_assign, "double": _double, "load_state_dict_assign": _load_assign,
             "running_var": _running_var, "data_in_place_then_drop": _data_in_place_then_drop}
CASES = [(s, k) for s in SITES for k in MUTATIONS if k != "running_var" or SITES[s].fold]


@pytest.mark.parametrize("site_name,mutation", CASES)
def test_a_changed_source_is_picked_up(site_name, mutation):
    site = SITES[site_name]
    torch.manual_seed(0)
    m = site.build()
    first = site.run(m)
    assert _same(derived_peek(site.owner(m), site.name), site.hand(m))
    dtype = MUTATIONS[mutation](site, m)
    second = site.run(m, dtype)
    fresh = site.build().to(dtype)  # never run, given the same parameters and buffers
    fresh.load_state_dict(m.state_dict())
    assert derived_peek(site.owner(fresh), site.name) is None
    assert _same(second, site.run(fresh, dtype))
    assert _same(derived_peek(site.owner(m), site.name), site.hand(m))
    assert not _same(second, first)


# ------------------------------------------------------------------------------------------------------ the helper
def test_no_change_is_the_same_object_and_one_make():
    owner, calls = type("D", (), {})(), []
    w, b = torch.randn(4, 3, requires_grad=True), None

    def make():
        calls.append(1)
        return w * 2

    a = derived(owner, "x", (w, b), make)
    assert derived(owner, "x", (w, b), make) is a and derived_peek(owner, "x") is a and len(calls) == 1
    assert not a.requires_grad  # make runs under no_grad
    assert derived_peek(owner, "y") is None and derived_peek(torch.nn.Module(), "x") is None
    pair = derived(owner, "pair", (w,), lambda: (w + 1, w - 1))  # a tuple of tensors is a value too
    assert derived(owner, "pair", (w,), lambda: None) is pair
    drop_derived(owner)
    assert derived_peek(owner, "x") is None
    assert derived(owner, "x", (w, b), make) is not a and len(calls) == 2


@pytest.mark.parametrize("site_name", list(SITES))
def test_sites_keep_the_object_without_a_change(site_name):
    site = SITES[site_name]
    torch.manual_seed(0)
    m = site.build()
    a = site.run(m)
    kept = derived_peek(site.owner(m), site.name)
    assert _same(site.run(m), a)
    again = derived_peek(site.owner(m), site.name)
    assert all(x is y for x, y in zip(again, kept))


@pytest.mark.parametrize("change", ["object", "version", "storage", "device", "dtype", "shape", "none"])
def test_every_field_of_the_rule_recomputes(change):
    owner, calls = type("D", (), {})(), []
    w, bias = torch.nn.Parameter(torch.randn(4, 3)), torch.randn(4)

    def get(srcs):
        return derived(owner, "x", srcs, lambda: (calls.append(1), srcs[0].detach().clone())[1])

    if change == "device":  # the host has one device: a stand-in whose only difference between the calls is that field
        w = type("T", (), dict(_version=0, data_ptr=lambda s: 64, device=torch.device("cpu"), dtype=torch.float32,
                               shape=torch.Size((4, 3)), detach=lambda s: torch.zeros(4, 3)))()
    a = get((w, bias))
    if change == "object":
        w2 = torch.nn.Parameter(w.detach())  # the same storage, version and shape: another tensor
        assert w2.data_ptr() == w.data_ptr() and w2._version == w._version
        w = w2
    elif change == "version":
        with torch.no_grad():
            w.add_(1.0)
    elif change == "storage":
        w.data = w.data.clone()
    elif change == "device":
        w.device = torch.device("meta")
    elif change == "dtype":
        w.data = w.data.double()
    elif change == "shape":
        w.data = w.data.view(3, 4)
    elif change == "none":
        bias = None
    b = get((w, bias))
    assert b is not a and len(calls) == 2
    assert get((w, bias)) is b and len(calls) == 2


# -------------------------------------------------------------------------------------------- nothing enters the module
@pytest.mark.parametrize("site_name", ["bottleneck", "self_attention", "q_weight", "offsets_logits_lanes"])
def test_nothing_enters_the_module(site_name):
    site = SITES[site_name]
    torch.manual_seed(0)
    m = site.build()
    before = {n: sorted(vars(s)) for n, s in m.named_modules()}
    keys = sorted(m.state_dict())
    out = site.run(m)
    site.run(m)
    assert {n: sorted(vars(s)) for n, s in m.named_modules()} == before and sorted(m.state_dict()) == keys
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)
    assert derived_peek(site.owner(loaded), site.name) is None
    assert _same(site.run(loaded), out)
    dup = copy.deepcopy(m)
    assert derived_peek(site.owner(dup), site.name) is None
    assert _same(site.run(dup), out)
    assert derived_peek(site.owner(dup), site.name)[0] is not derived_peek(site.owner(m), site.name)[0]


def test_the_cache_dies_with_its_owner():
    site = SITES["bottleneck"]
    m = site.build()
    site.run(m)
    refs = [weakref.ref(t) for t in derived_peek(site.owner(m), site.name)]
    assert all(r() is not None for r in refs)
    del m
    gc.collect()
    assert all(r() is None for r in refs)


def test_drop_derived_reaches_every_submodule():
    site = SITES["bottleneck"]
    m = site.build()
    site.run(m)
    owners = [s for s in m.modules() if derived_peek(s, "fold") is not None]
    assert len(owners) == 4  # three layers and the shortcut
    drop_derived(m)
    assert all(derived_peek(s, "fold") is None for s in m.modules())
