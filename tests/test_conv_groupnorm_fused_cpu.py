"""Host side of the GroupNorm folding: the group-size predicate, the new names on the ops package and the
C entry points' argument checks that need no device."""
import ctypes
import inspect

import pytest

from weed_instance_segmentation_amd import _lib, ops


@pytest.mark.parametrize("channels,groups,want", [
    (256, 32, True), (256, 64, True), (256, 16, True), (64, 16, True), (192, 12, True),
    (64, 32, False), (256, 8, False), (256, 256, False), (256, 1, False), (250, 32, False), (256, 0, False), (256, -4, False),
])
def test_group_size_predicate(channels, groups, want):
    assert ops.conv_group_stats_applies(channels, groups) is want


def test_switch_lives_on_the_package():
    assert ops.__dict__["CONV_GN_FUSED"] is True
    import importlib
    import pkgutil
    for info in pkgutil.iter_modules(ops.__path__):
        assert "CONV_GN_FUSED" not in importlib.import_module(f"{ops.__name__}.{info.name}").__dict__


def test_new_names_and_signatures():
    assert list(inspect.signature(ops.conv1x1_gn).parameters) == ["x", "weight", "bias", "stride", "w_split", "config",
                                                                  "stats_groups", "norm"]
    assert list(inspect.signature(ops.conv3x3_stats).parameters) == ["x", "weight", "groups", "stride", "w_split", "config"]
    assert list(inspect.signature(ops.group_norm_act_from_stats_).parameters) == ["x", "stats", "groups", "gamma", "beta", "eps",
                                                                                  "up", "relu"]
    assert list(inspect.signature(ops.group_norm_tokens_from_stats_).parameters) == ["x", "stats", "bias", "groups", "gamma",
                                                                                     "beta", "eps", "tokens", "start"]
    for name in ("wm2f_conv1x1_split_gn_fwd", "wm2f_conv3x3_split_stats_fwd", "wm2f_group_norm_act_apply",
                 "wm2f_group_norm_tokens_apply"):
        assert name in _lib.SIGNATURES


def test_entry_points_refuse_bad_arguments_on_the_host():
    """Null pointers and unsupported group sizes come back as WM2F_EINVAL before the device is touched."""
    lib = _lib.load()
    p = ctypes.c_void_p
    buf = ctypes.create_string_buffer(64)
    a = ctypes.cast(buf, p)
    assert lib.wm2f_conv1x1_split_gn_fwd(a, a, None, a, None, 0, None, None, None, 0, 0.0, 0, 1, 32, 64, 4, 4, 1, -1, None) == _lib.WM2F_EINVAL
    assert b"neither" in lib.wm2f_last_error()
    assert lib.wm2f_conv1x1_split_gn_fwd(a, a, None, a, a, 32, None, None, None, 0, 0.0, 0, 1, 32, 64, 4, 4, 1, -1, None) == _lib.WM2F_EINVAL
    assert b"groups of 4, 8 or 16" in lib.wm2f_last_error()
    assert lib.wm2f_conv1x1_split_gn_fwd(a, a, None, a, None, 0, a, a, a, 4, 1e-5, 1, 1, 32, 64, 4, 4, 1, -1, None) == _lib.WM2F_EINVAL
    assert b"+ bias" in lib.wm2f_last_error()
    assert lib.wm2f_conv3x3_split_stats_fwd(a, a, a, a, 2, 1, 32, 64, 4, 4, 1, -1, None) == _lib.WM2F_EINVAL
    assert b"groups of 4, 8 or 16" in lib.wm2f_last_error()
    assert lib.wm2f_conv3x3_split_stats_fwd(a, a, a, None, 8, 1, 32, 64, 4, 4, 1, -1, None) == _lib.WM2F_EINVAL
