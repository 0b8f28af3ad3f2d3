"""HIP-graph capture of the label-free forward (inference): one `hipGraphLaunch` instead of ~1 300 kernel launches.

At BASELINE config 2 (B = 8, 1024 x 1024) the forward is GPU-bound and the gain is about 1 %; at the reference's own
evaluation shape (config 1: 256 x 256, batch 2, `models/metrics.py:56`) the eager forward is bound by launch latency
(11 ms for 2 small images) and the captured one is several times faster.

    fwd = GraphedForward(model, example_pixel_values)      # warms up, then captures
    out = fwd(pixel_values)                                # same fields as model(pixel_values=...)

The output tensors are the graph's static buffers: they are overwritten by the next call (clone what must survive).
Shapes and dtype are fixed at capture; a different shape re-captures.  So is the inference precision (`ops.SPLIT_PRECISION`,
`set_inference_precision`): the graph replays the kernels of the level that was current at capture, whatever the level is
at replay; build another GraphedForward to run another level.
"""
from __future__ import annotations

import torch


class GraphedForward:
    """The label-free forward of `model` captured into one HIP graph at the shape, dtype and inference precision
    (`ops.SPLIT_PRECISION`) that are current at capture; replays run that level whatever the flag says by then."""

    def __init__(self, model, example: torch.Tensor, warmup: int = 3):
        if not example.is_cuda:
            from ._lib import Wm2fError
            raise Wm2fError("GraphedForward needs CUDA tensors (HIP graphs)")
        self.model = model.eval()
        self._capture(example, warmup)

    def _capture(self, example, warmup):
        self.static_in = example.clone()
        side = torch.cuda.Stream(device=example.device)
        side.wait_stream(torch.cuda.current_stream(example.device))
        with torch.cuda.stream(side), torch.no_grad():  # library algorithm searches, lazy caches, first-touch allocations
            for _ in range(warmup):
                self.model(pixel_values=self.static_in)
        torch.cuda.current_stream(example.device).wait_stream(side)
        torch.cuda.synchronize(example.device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.static_out = self.model(pixel_values=self.static_in)

    def __call__(self, pixel_values: torch.Tensor):
        if pixel_values.shape != self.static_in.shape or pixel_values.dtype != self.static_in.dtype:
            self._capture(pixel_values, 2)
        self.static_in.copy_(pixel_values)
        self.graph.replay()
        return self.static_out
