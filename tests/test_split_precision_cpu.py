"""The inference precision of the split-bf16 kernels without a GPU: a float64 emulation of the products
each level keeps against the floors of its rule, the prefix property of the piece split, the package flag
`ops.SPLIT_PRECISION` with its environment default and the package-level helpers, and the C ABI's six `_p` symbols."""
import ctypes
import importlib
import inspect
import json
import os
import pkgutil
import re
import subprocess
import sys

import pytest
import torch

import split_gemm_cases as S
import split_precision_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (32, 96, 256, 2048)
TAPS = (1, 9)
P_SYMBOLS = {"wm2f_token_linear_split_fwd_p": "wm2f_token_linear_split_fwd", "wm2f_conv1x1_split_fwd_p": "wm2f_conv1x1_split_fwd",
             "wm2f_conv1x1_split_gn_fwd_p": "wm2f_conv1x1_split_gn_fwd", "wm2f_conv3x3_split_fwd_p": "wm2f_conv3x3_split_fwd",
             "wm2f_conv3x3_split_stats_fwd_p": "wm2f_conv3x3_split_stats_fwd", "wm2f_stem7x7_pool_fwd_p": "wm2f_stem7x7_pool_fwd"}
TOUCHED = ("token_linear", "conv1x1", "conv1x1_gn", "conv3x3", "conv3x3_stats", "stem_conv_pool")


def _flat(family, K, taps):
    """x (M, taps K) and w (N, taps K): every tap of the weight against the same x row, one contraction."""
    x, w, _ = S.operands(family, 16, K, 16, seed=7 * K + taps, taps=taps)
    return x.repeat(1, taps), w.reshape(w.shape[0], -1)


def _emulated_error(family, K, taps, P):
    x, w = _flat(family, K, taps)
    exact = x.double() @ w.double().t()
    mag = x.double().abs() @ w.double().abs().t()
    return ((R.kept_sum(x, w, P) - exact).abs() / mag.clamp_min(1e-300)).max().item()


# ------------------------------------------------------------------------------------------------- the floors, emulated
@pytest.mark.parametrize("taps", TAPS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("family", S.FAMILIES)
def test_emulated_sums_stay_under_the_floors(family, K, taps):
    e2, e1 = _emulated_error(family, K, taps, 2), _emulated_error(family, K, taps, 1)
    print(f"{family} K={K} taps={taps}: two pieces 2^{torch.tensor(e2).log2().item():.1f}, one piece 2^{torch.tensor(e1).log2().item():.1f}")
    assert e2 < R.FLOORS["high"] and e1 < R.FLOORS["medium"]
    assert _emulated_error(family, K, taps, 3) < R.FLOORS["highest"]


@pytest.mark.parametrize("taps", TAPS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("family", ["ints", "bf16"])
def test_bf16_exact_operands_are_exact_at_every_level(family, K, taps):
    x, w = _flat(family, K, taps)
    exact = x.double() @ w.double().t()
    for P in (1, 2, 3):
        assert torch.equal(R.kept_sum(x, w, P), exact), (family, K, taps, P)


def test_the_floors_are_not_vacuous():
    """Each floor separates its level from the one below: on `wide`, one piece misses the two-piece floor and two pieces
    miss the three-piece floor, so a kernel that kept fewer products than its level says would fail its rule."""
    assert _emulated_error("wide", 32, 1, 1) > R.FLOORS["high"]
    assert _emulated_error("wide", 32, 1, 2) > R.FLOORS["highest"]


@pytest.mark.parametrize("family", S.FAMILIES)
def test_first_pieces_of_the_three_piece_split_are_the_p_piece_split(family):
    x, w, _ = S.operands(family, 33, 96, 48, seed=5, taps=9)
    for a in (x, w):
        three = R.split_pieces(a, 3)
        for P in (1, 2):
            got = R.split_pieces(a, P)
            assert len(got) == P and all(torch.equal(g, t) for g, t in zip(got, three))
        assert torch.equal(three[0], R.h_piece(a))
        for p in three:  # every piece is a bf16 value
            assert torch.equal(p.bfloat16().float(), p)
    big = torch.tensor([S.FLT_MAX, -S.FLT_MAX, 3.3961e38, 1.0])
    assert torch.isfinite(R.h_piece(big)).all() and R.h_piece(big)[0].item() == R.BF16_MAX


def test_rule_and_floors():
    assert R.FLOORS == {"highest": 2.0 ** -23, "high": 2.0 ** -14, "medium": 2.0 ** -6} and R.FLOORS["highest"] == S.RULE_FLOOR
    assert R.PIECES == {"highest": 3, "high": 2, "medium": 1}
    for level in R.LEVELS:
        assert R.rule(2e-7 + R.FLOORS[level], 1e-7, level) and not R.rule(2.1e-7 + 1.01 * R.FLOORS[level], 1e-7, level)
    assert [len(R.PRODUCTS[P]) for P in (3, 2, 1)] == [6, 3, 1]
    assert R.PRODUCTS[2] == R.PRODUCTS[3][3:] and R.PRODUCTS[1] == R.PRODUCTS[3][5:]  # the order of the six-product chain


# ------------------------------------------------------------------------------------------------------------ the flag
def test_flag_lives_on_the_package_alone():
    from weed_instance_segmentation_amd import ops
    assert "SPLIT_PRECISION" in ops.__dict__
    for info in pkgutil.iter_modules(ops.__path__):
        sub = importlib.import_module(f"{ops.__name__}.{info.name}")
        assert "SPLIT_PRECISION" not in sub.__dict__, f"{sub.__name__} has its own SPLIT_PRECISION"


@pytest.mark.parametrize("value", [None, "highest", "high", "medium"])
def test_flag_assignment_is_what_readers_see(monkeypatch, value):
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd.ops import gemm
    monkeypatch.setattr(ops, "SPLIT_PRECISION", value)
    assert ops.SPLIT_PRECISION is value and ops.__dict__["SPLIT_PRECISION"] is value
    pieces, suffix = gemm._split_pieces()
    assert pieces == R.PIECES[value or "highest"]
    assert suffix == {3: "", 2: "_p2", 1: "_p1"}[pieces]


@pytest.mark.parametrize("value", ["low", "HIGH", "", 2, True, ("high",)])
def test_bad_value_raises_at_the_call_that_reads_it(monkeypatch, value):
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd.ops import gemm
    monkeypatch.setattr(ops, "SPLIT_PRECISION", value)  # the assignment itself is free
    with pytest.raises(ValueError):
        gemm._split_pieces()
    with pytest.raises(ValueError):
        pkg.get_inference_precision()
    with pytest.raises(ValueError):
        pkg.set_inference_precision(value)
    with pytest.raises(ValueError):
        with pkg.inference_precision(value):
            pass
    assert ops.SPLIT_PRECISION is value  # a refused level changes nothing


def test_package_level_helpers(monkeypatch):
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import ops
    monkeypatch.setattr(ops, "SPLIT_PRECISION", "highest")
    assert pkg.get_inference_precision() == "highest"
    pkg.set_inference_precision("high")
    assert ops.SPLIT_PRECISION == "high" and pkg.get_inference_precision() == "high"
    with pkg.inference_precision("medium"):
        assert ops.SPLIT_PRECISION == "medium"
        with pkg.inference_precision(None):
            assert pkg.get_inference_precision() == "highest"
        assert ops.SPLIT_PRECISION == "medium"
    assert ops.SPLIT_PRECISION == "high"
    with pytest.raises(RuntimeError, match="inside"):
        with pkg.inference_precision("medium"):
            raise RuntimeError("inside")
    assert ops.SPLIT_PRECISION == "high"  # restored on exception
    pkg.set_inference_precision(None)
    assert ops.SPLIT_PRECISION == "highest"


@pytest.mark.parametrize("env,want", [(None, "highest"), ("high", "high"), ("medium", "medium"), ("highest", "highest"),
                                      ("bogus", "bogus")])
def test_environment_default_in_a_fresh_process(env, want):
    """WM2F_SPLIT_PRECISION gives the flag's initial value; a bad one is kept and raises at the first read, like any other."""
    code = ("from weed_instance_segmentation_amd import ops\n"
            "from weed_instance_segmentation_amd.ops import gemm\n"
            "print(ops.SPLIT_PRECISION)\n"
            "try:\n    print(gemm._split_pieces()[0])\nexcept ValueError:\n    print('ValueError')\n")
    e = {k: v for k, v in os.environ.items() if k != "WM2F_SPLIT_PRECISION"}
    if env is not None:
        e["WM2F_SPLIT_PRECISION"] = env
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    flag, pieces = r.stdout.split()
    assert flag == want
    assert pieces == (str(R.PIECES[want]) if want in R.PIECES else "ValueError")


# --------------------------------------------------------------------------------------------------------- the surface
def test_header_declares_and_lib_binds_the_six_symbols():
    from weed_instance_segmentation_amd import _build, _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wm2f.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, base in P_SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        mb = re.search(r"\bint\s+" + base + r"\s*\(([^)]*)\)", header)
        assert m and mb, name
        args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
        base_args = [a.strip() for a in " ".join(mb.group(1).split()).split(",")]
        assert args == base_args[:-1] + ["int pieces", "void* stream"], name  # a trailing `int pieces` before `stream`
        res, argtypes = _lib.SIGNATURES[name]
        bres, bargtypes = _lib.SIGNATURES[base]
        assert res is ctypes.c_int and argtypes == bargtypes[:-1] + [ctypes.c_int, ctypes.c_void_p], name
        assert hasattr(lib, name) and hasattr(lib, base), name


def test_header_states_the_contract_of_each_level():
    header = open(os.path.join(ROOT, "include", "wm2f.h")).read()
    for phrase in ("pieces = 3", "pieces = 2", "pieces = 1", "2^-23", "2^-14", "2^-6", "m.h, h.m, h.h", "WM2F_EINVAL"):
        assert phrase in header, phrase


def test_touched_functions_keep_their_recorded_signatures():
    from weed_instance_segmentation_amd import ops
    with open(os.path.join(ROOT, "tests", "golden", "ops_surface.json")) as f:
        surface = json.load(f)
    # the three entry points that joined ops after the surface was recorded, as they stood before this flag existed
    later = {
        "conv1x1_gn": "(x: 'torch.Tensor', weight: 'torch.Tensor', bias: 'torch.Tensor | None' = None, stride: 'int' = 1, "
                      "w_split: 'torch.Tensor | None' = None, config: 'int' = -1, stats_groups: 'int' = 0, "
                      "norm: 'tuple | None' = None)",
        "conv3x3_stats": "(x: 'torch.Tensor', weight: 'torch.Tensor', groups: 'int', stride: 'int' = 1, "
                         "w_split: 'torch.Tensor | None' = None, config: 'int' = -1)",
        "stem_conv_pool": "(x: 'torch.Tensor', weight: 'torch.Tensor', bias: 'torch.Tensor', w_split: 'torch.Tensor | None' = None, "
                          "split: 'bool' = True, grid: 'int' = 0) -> 'torch.Tensor'",
    }
    for name in TOUCHED:
        want = surface[name]["signature"] if name in surface else later[name]
        assert inspect.isfunction(getattr(ops, name)) and str(inspect.signature(getattr(ops, name))) == want, name
    assert set(TOUCHED) - set(surface) == set(later)


def test_package_reexports_and_graph_docstring():
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import graph, precision
    for name in ("set_inference_precision", "get_inference_precision", "inference_precision"):
        assert getattr(pkg, name) is getattr(precision, name)
    assert "at capture" in graph.__doc__ and "precision" in graph.__doc__
