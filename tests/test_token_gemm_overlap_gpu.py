"""The token kernel's turn boundaries (csrc/token_gemm_split.hip).

What §13.2 changes is WHEN things happen around a k-step's wait and the end of a turn, never what is computed: the
per-step wait is visible to the compiler, which no longer adds waits of its own, and the LayerNorm epilogue keeps two
batches of residual / pos rows in flight.  The candidates that also kept the bias epilogues' stores in flight across the
barrier and walked odd workgroups half a turn out of phase (1, 2, 2, ... tiles per turn) passed this file too; any later
change of that kind has to.  A stale panel, a stale x, a store or load that overtook a wait, or a tile that landed on
the wrong turn would show as wrong or unstable bits.

Token counts, by the CU count C (one persistent workgroup per CU while there are tiles, 8 waves each): wave shares of 0
to 5 tiles, with a fourth turn under a 1, 2, 2, ... walk and with ragged last tiles.  The counts below C * 16 give an odd
number of workgroups on any C (1 and 17 workgroups, and C - 1 where C is even).

Per case: exact small integers equal the fp64 reference (bias epilogues; the LayerNorm epilogue is not exact on integers
and is held to the forms of test_token_gemm_tail_gpu.py), randn is held to the rule of tests/split_gemm_cases.py, ten
repeats give the same bits, the first M rows of a run at M + 48 are the run at M, and the run at M equals the same rows
computed in row chunks of 16 * 7 + 3, of C * 16 and of one chunk per half -- other tile distributions, other phases, other
turns, the same bits."""
import functools
import math

import pytest
import torch

import split_gemm_cases as S

pytestmark = pytest.mark.gpu

M_FORMS = {
    "1": lambda C: 1,
    "16": lambda C: 16,
    "16*17": lambda C: 16 * 17,
    "16C-11": lambda C: 16 * C - 11,
    "16(C+1)": lambda C: 16 * (C + 1),
    "16(8C+1)": lambda C: 16 * (8 * C + 1),
    "16(16C+3)-5": lambda C: 16 * (16 * C + 3) - 5,
    "16(24C+C/2)": lambda C: 16 * (24 * C + C // 2),
    "16(40C+7)-9": lambda C: 16 * (40 * C + 7) - 9,
}
LARGEST = ("16(24C+C/2)", "16(40C+7)-9")  # at (32, 256) only
TOKEN_KN = [(32, 256), (96, 288), (288, 1024)]
CASES = [(m, K, N) for m in M_FORMS for (K, N) in TOKEN_KN if m not in LARGEST or (K, N) == (32, 256)]
EXTRA_ROWS = 16 * 3
POS_SHORT = 17
EPS = 1e-5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def n_cu(ops):
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=2)
def _case(family, M, K, N):
    """Inputs of M + EXTRA_ROWS tokens on the device (the run at M takes the first M rows), computed once per case:
    x, w, bias, gamma, beta, residual, pos with one row per token, pos with POS_SHORT rows."""
    Mx = M + EXTRA_ROWS
    seed = 7 * M + 3 * K + N
    x, w, b = S.operands(family, Mx, K, N, seed)
    ints = family == "ints"
    gamma, beta = S.extra((N,), seed + 1), S.extra((N,), seed + 2)
    if N <= 288:
        r, pos_m, pos_s = S.extra((Mx, N), seed + 3, ints), S.extra((Mx, N), seed + 4, ints), S.extra((POS_SHORT, N), seed + 5, ints)
    else:
        r = pos_m = pos_s = torch.zeros(1, N)
    return tuple(t.cuda() for t in (x, S.as_w1x1(w), b, gamma, beta, r, pos_m, pos_s))


def _ln(x, ws, b, r, gamma, beta, N, pos=None):
    """The LayerNorm epilogue through the C ABI, which takes any pos_rows (ops.token_linear wants it to divide M):
    out, or (out, out + pos[token % pos_rows])."""
    from weed_instance_segmentation_amd.ops._core import _launch, _p
    M, K = x.shape
    x, r = x.contiguous(), r.contiguous()
    out = torch.empty(M, N, device=x.device)
    out_pos = torch.empty_like(out) if pos is not None else None
    pos_rows = 0 if pos is None else pos.shape[0]
    if pos is not None:
        pos = pos.contiguous()
    _launch("wm2f_token_linear_split_fwd", x, _p(x), _p(ws), _p(b), _p(r), _p(gamma), _p(beta), _p(pos), _p(out), _p(out_pos),
            M, K, N, 0, pos_rows, EPS, 0)
    return out if pos is None else (out, out_pos)


def _runs(ops, case, ws, lo, hi):
    """Every epilogue family the shape is built for, on rows lo .. hi of the case: {name: output (rows first)}."""
    xx, w, b, gamma, beta, rr, pos_m, pos_s = case
    N = w.shape[0]
    x = xx[lo:hi]
    outs = {"bias": ops.token_linear(x, w, b, w_split=ws), "relu": ops.token_linear(x, w, b, relu=True, w_split=ws)}
    if N == 288:
        outs["group"] = ops.token_linear(x, w, b, relu=True, out_group=36, w_split=ws).permute(1, 0, 2)  # (rows, 8, 36)
    if N <= 288:
        r = rr[lo:hi]
        outs["ln"] = _ln(x, ws, b, r, gamma, beta, N)
        outs["ln_pos_m"], outs["ln_pos_m+"] = _ln(x, ws, b, r, gamma, beta, N, pos=pos_m[lo:hi])
        # row t of the whole run takes pos_s[t % POS_SHORT]: a chunk that starts at lo sees the table rotated by lo
        rot = pos_s[(torch.arange(POS_SHORT, device=pos_s.device) + lo) % POS_SHORT]
        outs["ln_pos_s"], outs["ln_pos_s+"] = _ln(x, ws, b, r, gamma, beta, N, pos=rot)
    return outs


def _chunked(ops, case, ws, M, step):
    parts = [_runs(ops, case, ws, lo, min(lo + step, M)) for lo in range(0, M, step)]
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


@pytest.mark.parametrize("m_form,K,N", CASES)
def test_values_against_fp64(ops, n_cu, m_form, K, N):
    M = M_FORMS[m_form](n_cu)
    for family in ("ints", "randn"):
        case = _case(family, M, K, N)
        xx, w, b, gamma, beta, rr, pos_m, pos_s = case
        x = xx[:M]
        ws = ops.split_weight(w)
        outs = _runs(ops, case, ws, 0, M)
        for relu in (False, True):
            out = outs["relu" if relu else "bias"]
            assert out.shape == (M, N)
            ref, mag, _ = S.token_ref(x, w, b, relu)
            what = f"token overlap M={M} K={K} N={N} relu={relu} {family}"
            if family == "ints":
                assert torch.equal(out, ref.float()), what
            else:
                e = S.rel_err(out, ref, mag)
                e32 = S.rel_err(S.token_fp32(ops, x, w, b, relu), ref, mag)
                print(f"{what}: e {e:.3e} e32 {e32:.3e}")
                assert S.rule(e, e32), (what, e, e32)
        if "group" in outs:  # feature-group major: the row-major bits, permuted
            assert torch.equal(outs["group"], outs["relu"].view(M, N // 36, 36)), (M, K, N, family)
        if "ln" in outs:
            r = rr[:M]
            lnp = (gamma, beta, EPS)
            ref, _, _ = S.token_ref(x, w, b, residual=r, ln=lnp)
            out32 = S.token_fp32(ops, x, w, b, residual=r, ln=lnp)
            e32 = (out32.double() - ref).abs().max().item()
            for name in ("ln", "ln_pos_m", "ln_pos_s"):
                out = outs[name]
                e = (out.double() - ref).abs().max().item()
                print(f"token overlap + {name} M={M} K={K} N={N} {family}: e {e:.3e} e32 {e32:.3e}")
                assert torch.isfinite(out).all()
                assert e <= 2 * e32 + 1e-6, (name, M, K, N, family, e, e32)
                assert e <= 3e-6 * ref.abs().max().item() * math.sqrt(K), (name, M, K, N, family, e)
                assert torch.equal(out, outs["ln"]), (name, M, K, N, family)  # pos changes nothing in `out`
            # the second output is one fp32 addition on the first
            rows = torch.arange(M, device=x.device)
            assert torch.equal(outs["ln_pos_m+"], outs["ln"] + pos_m[:M]), (M, K, N, family)
            assert torch.equal(outs["ln_pos_s+"], outs["ln"] + pos_s[rows % POS_SHORT]), (M, K, N, family)


@pytest.mark.parametrize("m_form,K,N", CASES)
def test_same_bits_however_the_rows_are_cut(ops, n_cu, m_form, K, N):
    M = M_FORMS[m_form](n_cu)
    case = _case("randn", M, K, N)
    ws = ops.split_weight(case[1])
    base = _runs(ops, case, ws, 0, M)
    for i in range(10):  # ten repeats of one call
        again = _runs(ops, case, ws, 0, M)
        for name, out in base.items():
            assert torch.equal(again[name], out), ("repeat", i, name, M, K, N)
    long = _runs(ops, case, ws, 0, M + EXTRA_ROWS)  # another tile distribution over workgroups, waves and turns
    for name, out in base.items():
        assert torch.equal(long[name][:M], out), ("prefix", name, M, K, N)
    for what, step in (("16*7+3", 16 * 7 + 3), ("C*16", n_cu * 16), ("halves", max(1, (M + 1) // 2))):
        cut = _chunked(ops, case, ws, M, step)
        for name, out in base.items():
            assert torch.equal(cut[name], out), ("chunks of " + what, name, M, K, N)
