"""What every kernel family shares: the kernel timer, pointer and dtype plumbing, and `_launch`, the one call into libwm2f."""
from __future__ import annotations

import ctypes

import torch

from .. import _lib
from .._lib import check, host_i32, load


class KernelTimer:
    """Optional HIP-event timing of individual kernel launches (bench.py's roofline leg).
    Events are recorded on the stream the kernel is launched on (torch's current stream)."""

    def __init__(self):
        self.records: dict[str, list] = {}

    def bracket(self, name, device):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.records.setdefault(name, []).append((a, b))
        return a, b

    def summary(self):
        """name -> (launches, mean microseconds); call after a device synchronize."""
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) * 1e3 / len(v)) for k, v in self.records.items()}


_timer: KernelTimer | None = None


def set_kernel_timer(t: KernelTimer | None) -> None:
    global _timer
    _timer = t


def _p(t: torch.Tensor | None):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _launch(symbol: str, t: torch.Tensor, *args, tag: str | None = None, raw: bool = False, what: str | None = None) -> int:
    """The one way into a libwm2f kernel: `symbol(*args, stream)` with the device guard and the current stream both taken
    from `t`, bracketed as `tag` when a kernel timer is installed (no tag: never timed), its return code checked under the
    symbol's name (`what` where two symbols report under one name).  raw=True hands WM2F_EUNSUPPORTED -- "this shape takes
    the other route" -- back to the caller; every other non-zero code raises all the same."""
    fn = getattr(load(), symbol)
    with torch.cuda.device(t.device):
        stream = _stream(t)
        if tag is None or _timer is None:
            rc = fn(*args, stream)
        else:
            a, b = _timer.bracket(tag, t.device)
            a.record()
            rc = fn(*args, stream)
            b.record()
    if not (raw and rc == _lib.WM2F_EUNSUPPORTED):
        check(rc, what or symbol)
    return rc


# Mixed precision (BASELINE configs 3-5 run under bf16 autocast): the fp32 entry points below get their inputs cast to
# fp32 with autocast switched off inside -- the policy PyTorch itself applies to grid_sample / softmax / layer_norm,
# which is what the dependency's K1 runs through.  The train step's own paths do not go through these casts: K1 takes
# the projection's rows in bf16 and writes bf16 (ms_deform_attn_rows), K2 and K3 run on the bf16 matrix cores
# (masked_xattn_bf16, mask_einsum_bf16), the token Linears' weight gradients read bf16 operands (token_wgrad).
_amp_fwd = torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
_amp_bwd = torch.amp.custom_bwd(device_type="cuda")


def _f32(t):
    """fp32 view of a half-precision tensor for the entry points without autograd (inference, matcher)."""
    return t.float() if isinstance(t, torch.Tensor) and t.dtype in (torch.bfloat16, torch.float16) else t


def _on_gpu(t: torch.Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise _lib.Wm2fError(f"{name} is on {t.device}: the wm2f kernels run on a GPU only (no CPU fallback)")


def _req(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    _on_gpu(t, name)
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


_DTYPE_CODES = {torch.float32: _lib.WM2F_F32, torch.bfloat16: _lib.WM2F_BF16, torch.int32: _lib.WM2F_I32,
                torch.uint8: _lib.WM2F_U8, torch.bool: _lib.WM2F_U8, torch.uint16: _lib.WM2F_U16, torch.int64: _lib.WM2F_I64}


def _dtype_code(t: torch.Tensor, allowed, error: str) -> int:
    """The WM2F_* code of t's dtype, which must be one of `allowed`; TypeError(error) otherwise."""
    if t.dtype not in allowed:
        raise TypeError(error)
    return _DTYPE_CODES[t.dtype]


def _id_maps_dtype(maps: torch.Tensor, who: str, what: str = "a tensor", contiguous: bool = True):
    """The first half of `_id_maps`: (maps, dtype code) of maps that are a tensor on the GPU, fp32, int32 or uint8."""
    if not isinstance(maps, torch.Tensor):
        raise TypeError(f"{who}: expected {what}")
    if contiguous:
        maps = _req(maps, "maps", maps.dtype)
    else:
        _on_gpu(maps, "maps")
    return maps, _dtype_code(maps, (torch.float32, torch.int32, torch.uint8), f"{who}: maps fp32 / int32 / uint8, got {maps.dtype}")


def _id_maps_size(maps: torch.Tensor, who: str, detail: str | None = None, bad: bool = False):
    """The second half: (B, H, W) of maps that are (B, H, W) and not empty."""
    if maps.dim() != 3:
        raise ValueError(f"{who}: maps must be (B, H, W), got {tuple(maps.shape)}")
    B, H, W = (int(v) for v in maps.shape)
    if B == 0 or H == 0 or W == 0 or bad:
        raise ValueError(f"{who}: bad size" + ("" if detail is None else f" {tuple(maps.shape)}{detail}"))
    return B, H, W


def _id_maps(maps: torch.Tensor, who: str, what: str = "a tensor", detail: str | None = None, bad: bool = False,
             contiguous: bool = True):
    """What a wrapper of an id-map kernel (csrc/labelmap.h) opens with: (maps, dtype code, B, H, W) of (B, H, W) maps that
    are on the GPU, fp32, int32 or uint8, and not empty.  `what` completes "expected ..."; an empty map, or `bad` -- the
    caller's own sizes are wrong --, is "bad size", followed by the shape and `detail` where the caller names its sizes.
    contiguous=False leaves a strided view as it is, for a caller that may still refuse the size.  A caller with a check
    of its own between the two halves calls them itself."""
    maps, dt = _id_maps_dtype(maps, who, what, contiguous)
    return (maps, dt, *_id_maps_size(maps, who, detail, bad))


def _id_maps_d2(maps: torch.Tensor, d2: torch.Tensor, who: str, detail: str | None = None, bad: bool = False):
    """`_id_maps` for an op that also reads the maps' `labelmap_distance`: (maps, dtype code, d2, B, H, W).  Its shape
    error names both tensors."""
    maps, dt = _id_maps_dtype(maps, who, "tensors")
    d2 = _req(d2, "d2", torch.int32)
    if maps.dim() != 3 or d2.shape != maps.shape:
        raise ValueError(f"{who}: maps and d2 must be (B, H, W), got {tuple(maps.shape)} and {tuple(d2.shape)}")
    return (maps, dt, d2, *_id_maps_size(maps, who, detail, bad))


def _id_rows(who: str, B: int, ids: torch.Tensor | None, n_ids: torch.Tensor | None, N: int | None):
    """The result rows of a per-instance op as (ids, n_ids, N): without `ids`, row r is id r of [0, N); with `ids` (B, N)
    int32 ascending and `n_ids` (B) of them valid, row r of image b is the raw id ids[b][r]."""
    if (ids is None) != (n_ids is None):
        raise ValueError(f"{who}: ids and n_ids go together")
    if ids is not None:
        ids, n_ids = _req(ids, "ids", torch.int32), _req(n_ids, "n_ids", torch.int32)
        if ids.dim() != 2 or ids.shape[0] != B or n_ids.shape != (B,) or (N is not None and int(N) != ids.shape[1]):
            raise ValueError(f"{who}: shapes disagree")
        N = int(ids.shape[1])
    elif N is None:
        raise ValueError(f"{who}: N is needed without an id list")
    if int(N) < 0:
        raise ValueError(f"{who}: bad size")
    return ids, n_ids, int(N)


def _workspace(nbytes: int, device, floor: int = 1) -> torch.Tensor:
    """`nbytes` of scratch memory, at least `floor`: a workspace query answers -1 for an unsupported size, and the launch
    that follows reports it, so the tensor only has to exist."""
    return torch.empty(max(int(nbytes), floor), device=device, dtype=torch.uint8)


def _levels(level_hw):
    """The host table (h0, w0, h1, w1, ...) of K1's levels."""
    return host_i32([x for hw in level_hw for x in hw])


def _host_desc(desc):
    """A host descriptor table as (contiguous int64 numpy array, its pointer for the C ABI); the array owns the memory."""
    import numpy as np
    d = np.ascontiguousarray(desc, dtype=np.int64)
    return d, d.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _ptr_table(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
