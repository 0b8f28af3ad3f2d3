"""ResNet backbone (stock PyTorch-ROCm ops: MIOpen convolutions, BatchNorm).

Out of the hot-path scope: kept as plain torch.nn so the drop-in module is
self-contained.  Sub-module and parameter names follow transformers' ResNetBackbone so that the
reference's checkpoints (`save_pretrained` / `from_pretrained`, train.py:224, :245) round-trip:
  embedder.embedder.{convolution,normalization}
  encoder.stages.S.layers.J.{shortcut,layer.K}.{convolution,normalization}
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops
from .derived import derived


def _infer_gpu(x: torch.Tensor) -> bool:
    """Inference on the GPU in fp32 without autocast."""
    return (not torch.is_grad_enabled()) and x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled("cuda")


def _fused_ok(x: torch.Tensor) -> bool:
    """Inference on the GPU with a float4-friendly map: use the fused bias(+residual)+ReLU pass."""
    return _infer_gpu(x) and (x.shape[-1] * x.shape[-2]) % 4 == 0


def _split_1x1(conv: nn.Conv2d, x: torch.Tensor, w: torch.Tensor) -> bool:
    """Inference 1x1 convolution that the split-bf16 kernel covers (ops.conv1x1, any map size)."""
    return (ops.CONV1X1_SPLIT and _infer_gpu(x) and conv.kernel_size == (1, 1) and conv.padding == (0, 0)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.stride[0] == conv.stride[1]
            and ops.conv1x1_applies(x, w, conv.stride[0]))


def _split_3x3(conv: nn.Conv2d, x: torch.Tensor, w: torch.Tensor) -> bool:
    """Inference 3x3 convolution that the split-bf16 kernel covers (ops.conv3x3, any map size)."""
    return (ops.CONV3X3_SPLIT and _infer_gpu(x) and conv.kernel_size == (3, 3) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.stride[0] == conv.stride[1]
            and ops.conv3x3_applies(x, w, conv.stride[0]))


def _folded(layer: nn.Module, conv: nn.Conv2d, bn: nn.BatchNorm2d):
    """Inference-time BatchNorm folding: conv(x, w) * g/sqrt(v+eps) + (b - m*g/sqrt(v+eps)) == conv(x, w', b').
    Derived for `layer`, the owner of conv and bn, so redone only after a parameter or statistic changes."""
    def make():
        scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
        return (conv.weight * scale[:, None, None, None]).contiguous(), (bn.bias - bn.running_mean * scale).contiguous()
    p, s = bn._parameters, bn._buffers  # (read directly: five Module.__getattr__ calls cost more than the lookup itself)
    return derived(layer, "fold", (conv._parameters["weight"], p["weight"], p["bias"], s["running_mean"], s["running_var"]), make)


class ConvLayer(nn.Module):
    def __init__(self, cin, cout, kernel_size=3, stride=1, activation=True):
        super().__init__()
        self.convolution = nn.Conv2d(cin, cout, kernel_size, stride, kernel_size // 2, bias=False)
        self.normalization = nn.BatchNorm2d(cout)
        self.activation = nn.ReLU() if activation else nn.Identity()

    def forward(self, x, residual=None, extra_bias=None, force_relu=False):
        """`residual` / `extra_bias` / `force_relu` let a bottleneck fold its shortcut add and final ReLU
        into this layer's epilogue (inference only)."""
        c = self.convolution
        relu = force_relu or isinstance(self.activation, nn.ReLU)
        if not self.training and not torch.is_grad_enabled():
            # inference: convolution with folded BatchNorm statistics; bias (+ residual) + ReLU in ONE pass
            w, b = _folded(self, c, self.normalization)
            if extra_bias is not None:
                b = b + extra_bias
            if _split_1x1(c, x, w) and (residual is None or relu):
                # 1x1: one split-bf16 GEMM with bias (+ residual) + ReLU in its store
                ws = ops.split_weight_cached(self, "conv", w)
                return ops.conv1x1(x, w, b, residual, relu, c.stride[0], w_split=ws)
            if _split_3x3(c, x, w) and residual is None and relu:
                # 3x3: one split-bf16 implicit GEMM with bias + ReLU in its store; the folded w is the cache's identity,
                # so a new fold (weight or BatchNorm version) re-splits
                ws = ops.split_weight_cached(self, "conv3x3", w, tap_major=True)
                return ops.conv3x3(x, w, b, True, c.stride[0], w_split=ws)
            if _fused_ok(x):
                y = torch.nn.functional.conv2d(x, w, None, c.stride, c.padding)
                if (y.shape[-1] * y.shape[-2]) % 4 == 0:
                    return ops.bias_act_(y, b, residual, relu)
                y = y + b[None, :, None, None]
            else:
                y = torch.nn.functional.conv2d(x, w, b, c.stride, c.padding)
            if residual is not None:
                y = y + residual
            return torch.relu(y) if relu else y
        y = self.normalization(c(x))
        if residual is not None:
            y = y + residual
        return torch.relu(y) if relu else y


class ShortCut(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.convolution = nn.Conv2d(cin, cout, 1, stride, bias=False)
        self.normalization = nn.BatchNorm2d(cout)

    def forward(self, x):
        return self.normalization(self.convolution(x))

    def folded_raw(self, x):
        """Inference: the shortcut convolution WITHOUT its folded bias, and that bias (the bottleneck adds it
        in its fused epilogue)."""
        c = self.convolution
        w, b = _folded(self, c, self.normalization)
        if _split_1x1(c, x, w):
            ws = ops.split_weight_cached(self, "conv", w)
            return ops.conv1x1(x, w, None, stride=c.stride[0], w_split=ws), b
        return torch.nn.functional.conv2d(x, w, None, c.stride), b


class BottleNeckLayer(nn.Module):
    def __init__(self, cin, cout, stride, reduction=4, downsample_in_bottleneck=False):
        super().__init__()
        red = cout // reduction
        self.shortcut = ShortCut(cin, cout, stride) if (cin != cout or stride != 1) else nn.Identity()
        self.layer = nn.Sequential(
            ConvLayer(cin, red, 1, stride if downsample_in_bottleneck else 1),
            ConvLayer(red, red, 3, 1 if downsample_in_bottleneck else stride),
            ConvLayer(red, cout, 1, activation=False),
        )
        self.activation = nn.ReLU()

    def forward(self, x):
        if not self.training and not torch.is_grad_enabled():
            h = self.layer[1](self.layer[0](x))
            if isinstance(self.shortcut, ShortCut):
                out = self._conv3_plus_shortcut(h, x)
                if out is not None:
                    return out
                sc, sc_bias = self.shortcut.folded_raw(x)
                return self.layer[2](h, residual=sc, extra_bias=sc_bias, force_relu=True)
            return self.layer[2](h, residual=x, force_relu=True)
        return self.activation(self.layer(x) + self.shortcut(x))

    def _conv3_plus_shortcut(self, h, x):
        """Inference: relu(conv3(h) + shortcut(x)) as ONE split GEMM over the concatenated K (ops.conv1x1_dual),
        or None where that does not apply and the raw shortcut plus conv3's residual epilogue run.  Each convolution keeps
        its own fold and split under its own layer; the block owns only the sum of the two folded biases."""
        if not ops.SHORTCUT_FOLD:
            return None
        l3, sc = self.layer[2], self.shortcut
        c3, cs = l3.convolution, sc.convolution
        w3, b3 = _folded(l3, c3, l3.normalization)
        wsc, bsc = _folded(sc, cs, sc.normalization)
        if not (c3.stride == (1, 1) and _split_1x1(c3, h, w3) and _split_1x1(cs, x, wsc)
                and ops.conv1x1_dual_applies(h, w3, x, wsc, cs.stride[0])):
            return None
        bias = derived(self, "shortcut_bias", (b3, bsc), lambda: b3 + bsc)  # a new fold gives new bias objects
        return ops.conv1x1_dual(h, w3, x, wsc, bias, cs.stride[0], w1_split=ops.split_weight_cached(l3, "conv", w3),
                                w2_split=ops.split_weight_cached(sc, "conv", wsc))


class Stage(nn.Module):
    def __init__(self, cin, cout, stride, depth, dib):
        super().__init__()
        self.layers = nn.Sequential(BottleNeckLayer(cin, cout, stride, downsample_in_bottleneck=dib),
                                    *[BottleNeckLayer(cout, cout, 1, downsample_in_bottleneck=dib) for _ in range(depth - 1)])

    def forward(self, x):
        return self.layers(x)


class _Embedder(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.embedder = ConvLayer(cin, cout, 7, 2)
        self.pooler = nn.MaxPool2d(3, 2, 1)

    def forward(self, x):
        e, pool = self.embedder, self.pooler
        if (not e.training and _fused_ok(x) and isinstance(e.activation, nn.ReLU)
                and (pool.kernel_size, pool.stride, pool.padding, pool.dilation, pool.ceil_mode) == (3, 2, 1, 1, False)):
            # inference: bias + ReLU + 3x3 / 2 max pool in one pass over the raw convolution output
            c = e.convolution
            w, b = _folded(e, c, e.normalization)
            if ((c.stride, c.padding, c.dilation, c.groups) == ((2, 2), (3, 3), (1, 1), 1)
                    and ops.stem_conv_pool_applies(x, w)):
                # 7x7 / 2 convolution, bias, ReLU and pool in one split-bf16 kernel; the folded w is the cache's identity,
                # so a new fold (weight or BatchNorm version) re-splits
                return ops.stem_conv_pool(x, w, b, w_split=ops.split_weight_cached(e, "stem", w, tap_major=True))
            y = torch.nn.functional.conv2d(x, w, None, c.stride, c.padding)
            if y.shape[-2] % 2 == 0 and y.shape[-1] % 8 == 0:
                return ops.bias_relu_maxpool(y, b)
            return pool(torch.relu_(y.add_(b[None, :, None, None])))
        return pool(e(x))


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        hs, depths = cfg["hidden_sizes"], cfg["depths"]
        dib = bool(cfg.get("downsample_in_bottleneck", False))
        first_stride = 2 if cfg.get("downsample_in_first_stage", False) else 1
        stages = [Stage(cfg["embedding_size"], hs[0], first_stride, depths[0], dib)]
        for cin, cout, d in zip(hs[:-1], hs[1:], depths[1:]):
            stages.append(Stage(cin, cout, 2, d, dib))
        self.stages = nn.ModuleList(stages)


class ResNetBackbone(nn.Module):
    def __init__(self, cfg: dict):
        super().__init__()
        if cfg.get("layer_type", "bottleneck") != "bottleneck":
            raise NotImplementedError("ResNetBackbone: only layer_type='bottleneck' is built")
        self.embedder = _Embedder(cfg.get("num_channels", 3), cfg["embedding_size"])
        self.encoder = _Encoder(cfg)
        names = ["stem"] + [f"stage{i + 1}" for i in range(len(cfg["depths"]))]
        out = cfg.get("out_features") or [names[-1]]
        self.out_indices = [names.index(n) for n in out]
        chans = [cfg["embedding_size"]] + list(cfg["hidden_sizes"])
        self.channels = [chans[i] for i in self.out_indices]

    def forward(self, pixel_values: torch.Tensor) -> list[torch.Tensor]:
        x = self.embedder(pixel_values)
        feats = [x]
        for st in self.encoder.stages:
            x = st(x)
            feats.append(x)
        return [feats[i] for i in self.out_indices]


def build_backbone(cfg: dict) -> nn.Module:
    mt = cfg.get("model_type")
    if mt == "resnet":
        return ResNetBackbone(cfg)
    if mt == "swin":
        from .backbone_swin import SwinBackbone
        return SwinBackbone(cfg)
    raise NotImplementedError(f"backbone model_type={mt!r} is not built (resnet and swin are)")
