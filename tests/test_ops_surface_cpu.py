"""The surface of the `ops` package: every name the single-file ops module offered, with its signature or value, and
the three switches that callers assign on the package.

tests/golden/ops_surface.json was recorded from the one-file module before it became a package: its public functions,
classes and constants, plus the private names other modules and tests reach for (`_p`, `_stream`, `check`, `_GRID`)."""
import importlib
import inspect
import json
import os
import pkgutil

import pytest
import torch

from weed_instance_segmentation_amd import ops

with open(os.path.join(os.path.dirname(__file__), "golden", "ops_surface.json")) as f:
    SURFACE = json.load(f)
FLAGS = ("CONV1X1_SPLIT", "CONV3X3_SPLIT", "K1_BWD_DETERMINISTIC")


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_recorded_name_is_unchanged(name):
    want = SURFACE[name]
    assert hasattr(ops, name), f"ops.{name} is gone"
    got = getattr(ops, name)
    if want["kind"] == "constant":
        assert (list(got) if isinstance(got, tuple) else got) == want["value"]
    else:
        assert (inspect.isclass(got) if want["kind"] == "class" else inspect.isfunction(got)), f"ops.{name} is {type(got)}"
        assert str(inspect.signature(got)) == want["signature"]


@pytest.mark.parametrize("flag", FLAGS)
def test_flag_lives_on_the_package_alone(flag):
    """Callers write `ops.<FLAG> = v` and read it back through the package: the name must be defined in ops/__init__
    itself, and no submodule may hold a copy of its own that the assignment would miss."""
    assert flag in ops.__dict__
    for info in pkgutil.iter_modules(ops.__path__):
        sub = importlib.import_module(f"{ops.__name__}.{info.name}")
        assert flag not in sub.__dict__, f"{sub.__name__} has its own {flag}"


@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("value", [None, True, False])
def test_flag_assignment_is_what_readers_see(monkeypatch, flag, value):
    monkeypatch.setattr(ops, flag, value)
    assert getattr(ops, flag) is value and ops.__dict__[flag] is value


@pytest.mark.parametrize("torch_switch", [False, True])
def test_k1_backward_rule_reads_the_package_flag_at_call_time(monkeypatch, torch_switch):
    monkeypatch.setattr(torch, "are_deterministic_algorithms_enabled", lambda: torch_switch)
    monkeypatch.setattr(ops, "K1_BWD_DETERMINISTIC", None)
    assert ops.k1_bwd_deterministic() is torch_switch
    monkeypatch.setattr(ops, "K1_BWD_DETERMINISTIC", True)
    assert ops.k1_bwd_deterministic() is True
    monkeypatch.setattr(ops, "K1_BWD_DETERMINISTIC", False)
    assert ops.k1_bwd_deterministic() is False
    assert ops.k1_bwd_deterministic(True) is True  # the caller's own choice comes before the flag
    monkeypatch.setattr(ops, "K1_BWD_DETERMINISTIC", True)
    assert ops.k1_bwd_deterministic(False) is False
