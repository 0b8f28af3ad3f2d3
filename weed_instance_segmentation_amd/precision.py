"""The inference precision of the split-bf16 GEMMs and convolutions: one package-wide level.

    set_inference_precision("high")            # "highest" (default), "high", "medium"
    with inference_precision("medium"):
        out = model(pixel_values=x)

The level is the flag `ops.SPLIT_PRECISION`, read by the split kernels' Python entry points at every call.  "highest" keeps
three bf16 pieces per operand and six products (fp32 accuracy), "high" two pieces and three products (about TF32),
"medium" one piece and one product (bf16 operands, fp32 accumulation).  Training, autocast and `split=False` never reach
these kernels.  A captured `GraphedForward` replays the level that was current at capture.
"""
from __future__ import annotations

from contextlib import contextmanager

from . import ops

LEVELS = ("highest", "high", "medium")


def _checked(level):
    if level is None:
        return "highest"
    if not isinstance(level, str) or level not in LEVELS:
        raise ValueError(f"inference precision {level!r}: one of {LEVELS}")
    return level


def set_inference_precision(level: str | None) -> None:
    """Set the level for every later call; None means "highest".  Raises ValueError for anything else."""
    ops.SPLIT_PRECISION = _checked(level)


def get_inference_precision() -> str:
    """The current level as one of "highest", "high", "medium" (ValueError if `ops.SPLIT_PRECISION` holds anything else)."""
    return _checked(ops.SPLIT_PRECISION)


@contextmanager
def inference_precision(level: str | None):
    """Run the block at `level`, then restore what `ops.SPLIT_PRECISION` held before, exceptions included."""
    level = _checked(level)
    previous = ops.SPLIT_PRECISION
    ops.SPLIT_PRECISION = level
    try:
        yield
    finally:
        ops.SPLIT_PRECISION = previous
