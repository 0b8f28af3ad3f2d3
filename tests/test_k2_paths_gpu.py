"""K2 masked cross-attention (csrc/masked_xattn.hip) on the GPU, every kernel the launchers dispatch to
against fp64: the case table of tests/k2_cases.py (one case at least per template instantiation, value families that drive
the online softmax and its lazy rescale, structured masks) under the accuracy rule stated there -- no worse than twice the
stock fp32 route against fp64 (bf16: no worse than the stock bf16 route), per tensor and per row; lse against a
log-sum-exp; exact zeros, exact rows and bit reproducibility where the arithmetic promises them.

Every case prints its errors (`k2 <case> <tensor>: fro fused / stock, row fused / stock`; run with -s).  The rule, the derived
terms and the errors measured on an MI355X are in DESIGN.md §4.4 ("Tests")."""
import pytest
import torch

import k2_cases as K

pytestmark = pytest.mark.gpu

GRADS = ("grad_q", "grad_k", "grad_v")
FWD_IDS = [c.name for c in K.CASES]
BWD_IDS = [c.name for c in K.BACKWARD_CASES]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


def _at_odd_address(m8):
    """The same mask bytes at an address that is 1 mod 4: the launcher then takes the general forward."""
    odd = torch.empty(m8.numel() + 8, dtype=torch.uint8, device=m8.device)[1:1 + m8.numel()].view_as(m8)
    odd.copy_(m8)
    assert m8.data_ptr() % 4 == 0 and odd.data_ptr() % 4 == 1 and odd.is_contiguous()
    return odd


def _fused(ops, c, x, aligned=None):
    """ops.masked_xattn on a case's device inputs: out, lse (the tensor the forward saves for its backward) and, for a
    backward case, the three gradients."""
    dt = torch.bfloat16 if c.dtype == K.BF16 else torch.float32
    q, k, v = (x[n].to(dt).requires_grad_() for n in ("q", "k", "v"))
    m8 = x["m8"]
    if m8 is not None and not (c.aligned if aligned is None else aligned):
        m8 = _at_odd_address(m8)
    out = ops.masked_xattn(q, k, v, m8, x["row_open"], c.heads)
    res = {"out": out.detach(), "lse": out.grad_fn.saved_tensors[-1]}
    assert res["out"].dtype == torch.float32 and res["lse"].shape == (c.B, c.heads, c.Q)
    if c.bwd is not None and aligned is None:
        res.update(zip(GRADS, torch.autograd.grad(out, (q, k, v), x["go"])))
        assert all(res[n].dtype == dt for n in GRADS)
    return res


def _extras(c, ref, e):
    """The derived additive terms of DESIGN.md §4.4 per tensor, as (Frobenius term, worst-row term); fp32 cases only: the
    log2-domain roundings on the full-tile forward's lse (the gradients' derived slack is taken off row by row in _errors)."""
    ex = {n: (0.0, 0.0) for n in e}
    if c.dtype != K.F32:
        return ex
    t = K.lse_term(c.fwd.kernel, ref["smag"], ref["lse"].abs().max().item())
    ex["lse"] = (t, t)
    for n, (a, b) in ex.items():
        if a or b:
            print(f"k2 {c.name} {n}: derived terms {a:.3e} (Frobenius) {b:.3e} (worst row)")
    return ex


def _errors(c, got, ref, stock):
    """name -> (fro fused, fro stock, row fused, row stock); lse: absolute error in both slots (bf16: Frobenius); the
    gradients of the fp32 cases with cancelling rows (k2_cases.cancelling) relative to the magnitude of their terms, with
    `stock` holding the fp32 flash comparator's gradients in its two orders (the worse counts); the others relative to the reference, the kernel's after
    k2_cases.grad_slack, row by row."""
    e = {}
    for n in got:
        if n == "lse":
            f = K.abs_err if c.dtype == K.F32 else K.fro_err
            e[n] = (f(got[n], ref[n]), f(stock[n], ref[n])) * 2
        elif n in GRADS and c.dtype == K.F32:
            cancels = K.cancelling(c)  # then: against the terms, comparator attention_flash_fp32, no slack
            f = K.grad_errs(got[n], ref, n, c.heads, cancels, slack=not cancels)
            sts = [K.grad_errs(t, ref, n, c.heads, cancels, slack=False) for t in (stock[n] if cancels else [stock[n]])]
            st = (max(a for a, _ in sts), max(b for _, b in sts))
            if not cancels:
                raw = K.grad_errs(got[n], ref, n, c.heads, cancels, slack=False)
                print(f"k2 {c.name} {n}: fused before the derived slack: fro {raw[0]:.3e} row {raw[1]:.3e}")
            e[n] = (f[0], st[0], f[1], st[1])
        else:
            e[n] = (K.fro_err(got[n], ref[n]), K.fro_err(stock[n], ref[n]),
                    K.row_err(got[n], ref[n], c.heads), K.row_err(stock[n], ref[n], c.heads))
        print(f"k2 {c.name} [{c.values} {c.mask}] {n}: fro fused {e[n][0]:.3e} stock {e[n][1]:.3e}  row fused {e[n][2]:.3e} stock {e[n][3]:.3e}")
    return e


_CACHE = {}


def _run(ops, name):
    """One evaluation per case, shared by the tests: device inputs, the kernel's results, and their errors and the stock
    route's against the fp64 reference (computed on the device, dropped once measured)."""
    if name not in _CACHE:
        c = K.BY_NAME[name]
        q, k, v, go, m, ro = K.case_inputs(c)
        x = {"q": q.cuda(), "k": k.cuda(), "v": v.cuda(), "go": go.cuda(), "m": None if m is None else m.cuda(),
             "m8": None if m is None else m.to(torch.uint8).cuda(), "row_open": None if ro is None else ro.cuda()}
        got = _fused(ops, c, x)
        go_d = x["go"] if c.bwd is not None else None
        ref = K.attention(x["q"], x["k"], x["v"], x["m"], c.heads, go_d)
        slack = c.dtype == K.F32 and not K.cancelling(c)
        ref.update(K.error_scales(x["q"], x["k"], x["v"], x["m"], c.heads, go_d, got["lse"] if slack else None))
        if c.dtype == K.F32:
            stock = K.attention(x["q"], x["k"], x["v"], x["m"], c.heads, go_d, dtype=torch.float32)
            if go_d is not None and K.cancelling(c):
                flash = [K.attention_flash_fp32(x["q"], x["k"], x["v"], x["m"], c.heads, go_d, K.order(o, c.D),
                                                c.fwd.kernel == K.FWD_FULL) for o in K.STOCK_ORDERS]
                stock.update({n: [f[n] for f in flash] for n in GRADS})
        else:
            stock = K.attention_stock_bf16(x["q"], x["k"], x["v"], x["m"], c.heads, go_d)
        err = _errors(c, got, ref, stock)
        if c.dtype == K.F32 and c.values.startswith("wide"):
            # the worst out row of the wide families is the rounding of a few competing scores, and which fp32 summation
            # order of a score has the worse worst row is chance: the stock route's worst row is taken over three orders
            rows = [err["out"][3]] + [K.row_err(K.attention(x["q"], x["k"], x["v"], x["m"], c.heads, dtype=torch.float32,
                                                            perm=K.order(o, c.D))["out"], ref["out"], c.heads) for o in K.STOCK_ORDERS]
            print(f"k2 {c.name} out: stock worst row in three summation orders " + " ".join(f"{r:.3e}" for r in rows))
            err["out"] = err["out"][:3] + (max(rows),)
        mags = {n: ref[n] for n in ("mag_q", "mag_k") if n in ref}
        _CACHE[name] = {"case": c, "x": x, "got": got, "err": err, "extra": _extras(c, ref, err), "m_cpu": m,
                        "ref_out_lse": (ref["out"], ref["lse"]), "mags": mags}
    return _CACHE[name]


def _hold(c, name, e, extra=(0.0, 0.0)):
    if c.dtype == K.F32:
        assert K.rule(e[0], e[1], extra[0]), f"{c.name} {name}: Frobenius fused {e[0]:.3e} stock {e[1]:.3e} (+ {extra[0]:.3e})"
        assert K.rule(e[2], e[3], extra[1]), f"{c.name} {name}: worst row fused {e[2]:.3e} stock {e[3]:.3e} (+ {extra[1]:.3e})"
    else:
        assert e[1] < 2e-2, f"{c.name} {name}: the stock bf16 comparison itself is broken ({e[1]:.3e})"
        assert K.rule_bf16(e[0], e[1]), f"{c.name} {name}: Frobenius fused {e[0]:.3e} stock bf16 {e[1]:.3e}"


@pytest.mark.parametrize("name", FWD_IDS)
def test_forward(ops, name):
    """out and lse of every table case under the accuracy rule, on the kernel the table says."""
    r = _run(ops, name)
    c = r["case"]
    assert K.case_route(c, False) == c.fwd, "the case moved to another forward kernel: retune the table"
    m8 = r["x"]["m8"]
    assert m8 is None or m8.data_ptr() % 4 == 0  # what `aligned` of the route means; an unaligned case copies it to 1 mod 4
    _hold(c, "out", r["err"]["out"], r["extra"]["out"])
    _hold(c, "lse", r["err"]["lse"], r["extra"]["lse"])


@pytest.mark.parametrize("name", BWD_IDS)
def test_backward(ops, name):
    """grad_q, grad_k, grad_v of every backward case under the accuracy rule -- the fp32 full-tile backward included, which
    no shape of the older tests reaches -- and exact zeros in the grad_k / grad_v rows of keys no query attends (the kernels
    zero p by select; a dropped memset or a stale store shows here)."""
    r = _run(ops, name)
    c = r["case"]
    assert K.case_route(c, True) == c.bwd, "the case moved to another backward kernel: retune the table"
    dead = K.unattended_keys(c, r["m_cpu"])
    assert (dead is not None) == (c.mask in K.ZERO_CHECK)
    if dead is not None:
        dead = dead.cuda()
        assert dead.any()
        for n in ("grad_k", "grad_v"):
            assert not r["got"][n][dead].float().abs().max().item() > 0, f"{n}: nonzero in the row of a key nobody attends"
    for n in GRADS:
        if c.dtype == K.BF16 and c.mask == "single_open" and n != "grad_v":
            # one open key per row: p is one-hot, grad_q and grad_k are identically zero and the stock route returns zeros;
            # the kernel's dP - delta is the difference of two D-term fp32 dot products of the same terms, each within
            # D U32 sum |terms| of the exact value, which bf16 operands and the bf16 result round by 2^-8 more at most: 3.8e-6 of
            # the terms, a worst-case count (measured: grad_q 2.5e-8, grad_k 1.7e-9)
            e = K.grad_row_err(r["got"][n], torch.zeros_like(r["got"][n], dtype=torch.float64), r["mags"]["mag_" + n[-1]])
            print(f"k2 {c.name} {n}: worst row / term magnitude {e:.3e}")
            assert e <= 2 * c.D * K.U32 * (1 + 2.0 ** -8) ** 2
            continue
        _hold(c, n, r["err"][n], r["extra"][n])


@pytest.mark.parametrize("name", [c.name for c in K.CASES if c.mask == "single_open" and c.dtype == K.F32])
def test_single_open_key_row_is_that_keys_value_row(ops, name):
    """One open key: p = 1 and l = 1 in its tile, every other tile, wave and split merges with weight 0 -- out is the key's v
    row bit for bit, at both ends of the key axis and on either side of a tile and of a split boundary."""
    r = _run(ops, name)
    c, m = r["case"], r["x"]["m"]
    key = (~m).float().argmax(-1)  # (B, Q)
    want = r["x"]["v"][torch.arange(c.B, device=key.device)[:, None], key]
    assert torch.equal(r["got"]["out"], want)


@pytest.mark.parametrize("name", [c.name for c in K.CASES if c.values == "uniform"])
def test_uniform_scores_give_the_mean_and_log_count(ops, name):
    """k = 0: the reference the case is held to IS the mean of the open v rows and ln(n_open)."""
    r = _run(ops, name)
    c, x = r["case"], r["x"]
    open_ = ~K.effective_mask(r["m_cpu"], c.B, c.Q, c.N).cuda()
    n_open = open_.sum(-1).double()
    v4 = x["v"].double().view(c.B, c.N, c.heads, c.D)
    mean = torch.einsum("bqn,bnhd->bqhd", open_.double(), v4).reshape(c.B, c.Q, -1) / n_open[..., None]
    ref_out, ref_lse = r["ref_out_lse"]
    assert K.fro_err(mean, ref_out) < 1e-12 and K.abs_err(n_open.log()[:, None].expand_as(ref_lse), ref_lse) < 1e-12
    _hold(c, "out", r["err"]["out"], r["extra"]["out"])
    _hold(c, "lse", r["err"]["lse"], r["extra"]["lse"])


FULL_VS_GENERAL = [c.name for c in K.CASES if c.fwd.kernel == K.FWD_FULL and c.mask != "none" and c.values.startswith(("wide", "asc"))]


@pytest.mark.parametrize("name", FULL_VS_GENERAL)
def test_full_tile_forward_against_general(ops, name):
    """The log2-domain, lazily rescaling forward and the general forward (the same mask bytes at an odd address) on the wide
    and ascending families: the general kernel passes the same rule against fp64, the two differ from each other by no more
    than the sum of what the rule allows each, and they are two kernels (different bits)."""
    r = _run(ops, name)
    c, x = r["case"], r["x"]
    assert K.route(c.B, c.heads, c.Q, c.N, c.D, aligned=False).kernel == K.FWD_GENERAL
    gen = _fused(ops, c, x, aligned=False)
    ref_out, ref_lse = r["ref_out_lse"]
    e_full = r["err"]["out"]
    e_gen = (K.fro_err(gen["out"], ref_out), e_full[1], K.row_err(gen["out"], ref_out, c.heads), e_full[3])
    print(f"k2 {c.name} [{c.values} {c.mask}] general out: fro {e_gen[0]:.3e} stock {e_gen[1]:.3e}  row {e_gen[2]:.3e} stock {e_gen[3]:.3e}")
    _hold(c, "general out", e_gen, r["extra"]["out"])
    l_full, l_gen = r["err"]["lse"], K.abs_err(gen["lse"], ref_lse)
    print(f"k2 {c.name} general lse: {l_gen:.3e} full {l_full[0]:.3e} stock {l_full[1]:.3e}")
    assert K.rule(l_gen, l_full[1])
    assert K.fro_err(r["got"]["out"], gen["out"].double()) <= 2 * max(2 * e_full[1], 1e-6)
    assert not torch.equal(r["got"]["out"], gen["out"]) or c.mask == "single_open"


@pytest.mark.parametrize("name", FWD_IDS)
def test_two_calls_give_identical_bits(ops, name):
    """Every output of every route is reproducible bit for bit (splits, waves and chunks merge in a fixed order), except
    grad_k / grad_v of the general backward with accumulate = 1, whose query chunks add atomically."""
    r = _run(ops, name)
    c = r["case"]
    again = _fused(ops, c, r["x"])
    for n, t in r["got"].items():
        if n in ("grad_k", "grad_v") and c.bwd.accumulate:
            assert c.bwd.kernel == K.BWD_GENERAL and c.bwd.q_chunks > 1
            continue
        assert torch.equal(t, again[n]), n
