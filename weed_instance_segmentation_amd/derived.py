"""The one cache for what the inference path derives from parameters: folded convolution weights, merged and scaled
projections, the bf16 splits of all of these.  It lives here, keyed by the owner, never in a module's
__dict__: pickling, deepcopy and state_dict do not see it, and it dies with its owner.  (ops.gemm imports this module.)"""
from __future__ import annotations

import weakref

import torch

_CACHE: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()  # owner -> {name: (source refs, source states, value)}


def _none():
    return None


def _state(t):  # what can change under a source that stays the same object
    return None if t is None else (t._version, t.data_ptr(), t.device, t.dtype, t.shape)


def derived(owner, name: str, sources: tuple, make):
    """make() -- a tensor or a tuple of tensors, computed under no_grad -- cached per (owner, name) and redone when any of
    `sources` (tensors, None allowed) is another tensor object (held by weak reference) or has another _version,
    data_ptr(), device, dtype or shape.  A derived tensor that feeds another is just a source of it: a new one is a new
    object.  A write through `.data` changes none of these: call drop_derived after one."""
    entries = _CACHE.get(owner)
    if entries is None:
        entries = _CACHE[owner] = {}
    hit = entries.get(name)
    if hit is not None and len(hit[0]) == len(sources):
        for s, ref, state in zip(sources, hit[0], hit[1]):
            if ref() is not s or _state(s) != state:
                break
        else:
            return hit[2]
    with torch.no_grad():
        value = make()
    entries[name] = (tuple(_none if s is None else weakref.ref(s) for s in sources), tuple(_state(s) for s in sources), value)
    return value


def derived_peek(owner, name: str):
    """What derived(owner, name, ...) last computed, or None; never computes (tests, probes)."""
    hit = _CACHE.get(owner, {}).get(name)
    return None if hit is None else hit[2]


def drop_derived(obj) -> None:
    """Forget everything derived for `obj`, and for each of its submodules when it is an nn.Module.  The call to make
    after writing parameters or buffers through `.data` (p.data.mul_(2), a broadcast into p.data), which no key can see."""
    for owner in (obj.modules() if isinstance(obj, torch.nn.Module) else (obj,)):
        _CACHE.pop(owner, None)
