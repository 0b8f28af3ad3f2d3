"""What the K2 path tests share (csrc/masked_xattn.hip): the route of a call as the launchers decide it,
seeded input generators (value families and mask families), the fp64 reference with its stock fp32 / bf16 comparators, the
error measures with the accuracy rule, and the case table.  A plain module: it imports without a GPU, and every function
works on the device its tensors are on.

The case table is built from the dispatch, not by hand: every template instantiation the launchers can reach
(INSTANTIATIONS) has at least one case with a non-trivial mask, and every case states the route it claims, so a later
retuning that moves a case to another kernel fails a test instead of silently testing something else.

The accuracy rule, its two measures, the families whose gradients are measured against the magnitude of their terms and
the derived terms are stated once, in DESIGN.md §4.4 ("Tests"), with the measured errors; the functions below implement it."""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional

import torch

from oracle import m2f_oracle as O

LN2 = math.log(2.0)
K_TAU = 8.0  # lazy-rescale slack of the full-tile forward, log2 units (masked_xattn_fwd_full_kernel)
WAVES = 4    # waves of a workgroup; wave w of a split walks its tiles w, w + 4, ...
(UNSUPPORTED, FWD_GENERAL, FWD_FULL, BF16_FWD, BWD_GENERAL, BWD_FULL, BF16_BWD) = range(7)
F32, BF16 = 0, 1  # WM2F_F32, WM2F_BF16


class Route(NamedTuple):
    kernel: int
    nqt: int
    q_chunks: int
    n_splits: int
    tiles_per_split: int
    accumulate: int


def route(B, heads, Q, N, D, dtype=F32, backward=False, aligned=True) -> Route:
    """wm2f_masked_xattn_route: the kernel and grid the launchers take for this call (host arithmetic, no GPU)."""
    from weed_instance_segmentation_amd import _lib
    r = (ctypes.c_int32 * 6)()
    rc = _lib.load().wm2f_masked_xattn_route(B, heads, Q, N, D, dtype, int(backward), int(aligned), r)
    assert rc == 0, rc
    return Route(*r)


# Every instantiation the dispatch of masked_xattn.hip can launch, as (kernel, D, NQT, accumulate).  `accumulate` is a
# run-time argument of the general backward; NQT = 4 there means at most 64 queries = one chunk, so (4, 1) does not exist.
INSTANTIATIONS = (
    [(k, D, nqt, 0) for k in (FWD_GENERAL, FWD_FULL) for D in (16, 32) for nqt in (1, 2, 4, 7)]
    + [(k, 64, nqt, 0) for k in (FWD_GENERAL, FWD_FULL) for nqt in (1, 2)]
    + [(BF16_FWD, 32, nqt, 0) for nqt in (1, 2, 4, 7)]
    + [(BWD_GENERAL, D, 4, 0) for D in (16, 32)]
    + [(BWD_GENERAL, D, 7, acc) for D in (16, 32) for acc in (0, 1)]
    + [(BWD_GENERAL, 64, 3, acc) for acc in (0, 1)]
    + [(BWD_FULL, 32, nqt, 0) for nqt in (4, 7)]
    + [(BF16_BWD, 32, nqt, 0) for nqt in (4, 7)])

# ---------------------------------------------------------------------------------------------------------------- values
ASCENDING_STEPS = (4.0, 7.5, 8.5, 12.0)  # log2 units per 16-key tile: both sides of K_TAU between neighbouring tiles
# a wave walks every fourth tile, so its own running maximum moves by 4 steps per iteration: these put THAT on both sides
ASCENDING_WAVE_STEPS = (1.9, 2.1)
VALUE_FAMILIES = ("randn", "wide30", "wide150", "asc4", "asc7.5", "asc8.5", "asc12", "asc1.9", "asc2.1", "desc12",
                  "outlier", "uniform", "offset_v")
OUTLIER_BOOST = 100.0


def outlier_keys(N: int):
    """The four keys of the `outlier` family: both ends, the middle, and the first key of the second tile."""
    return [0, N - 1, N // 2, 16 % N if N > 17 else 1 % N]


def values(family: str, B: int, heads: int, Q: int, N: int, D: int, seed: int):
    """q (B, Q, E) pre-scaled, k, v (B, N, E), grad_out (B, Q, E): fp32 CPU tensors from a seeded CPU generator.
      randn     q = 0.5 randn, the rest randn: logit standard deviation 0.5 sqrt(D) (the existing tests' data)
      wideS     logit standard deviation S (30, 150): q = randn S / sqrt(D)
      ascS      the scores rise by S log2 units per 16-key tile (+ noise of 0.1 log2 units): dimension 0 of q is 1, of k
                S ln 2 * tile; the other dimensions of q are 0.01 randn
      descS     the mirror image: the first tile holds the maximum, no rescale after it
      outlier   randn with dimensions 0 .. 3 reserved: row r of q has 10 in dimension r % 4, key outlier_keys(N)[c] has 10
                in dimension c, so one key per row scores 100 and the rest 0.5 sqrt(D - 4) randn
      uniform   k = 0: out is the mean of the open v rows, lse = ln(n_open)
      offset_v  randn with v + 1000: cancels in dP - delta"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Q, heads, D, generator=g) * 0.5
    k = torch.randn(B, N, heads, D, generator=g)
    v = torch.randn(B, N, heads, D, generator=g)
    go = torch.randn(B, Q, heads, D, generator=g)
    tile = (torch.arange(N) // 16).float()
    if family == "randn":
        pass
    elif family.startswith("wide"):
        q = q * (2.0 * float(family[4:]) / math.sqrt(D))
    elif family.startswith("asc") or family.startswith("desc"):
        step = float(family[3:] if family.startswith("asc") else family[4:])
        ramp = tile if family.startswith("asc") else (tile.max() - tile)
        q = q * 0.02
        q[..., 0] = 1.0
        k[..., 0] = (ramp * (step * LN2))[None, :, None]
    elif family == "outlier":
        q[..., :4] = 0.0
        k[..., :4] = 0.0
        rows = torch.arange(Q)
        for c, j in enumerate(outlier_keys(N)):
            q[:, rows[rows % 4 == c], :, c] = 10.0
            k[:, j, :, c] = OUTLIER_BOOST / 10.0
    elif family == "uniform":
        k = torch.zeros_like(k)
    elif family == "offset_v":
        v = v + 1000.0
    else:
        raise ValueError(family)
    E = heads * D
    return q.reshape(B, Q, E), k.reshape(B, N, E), v.reshape(B, N, E), go.reshape(B, Q, E)


# ----------------------------------------------------------------------------------------------------------------- masks
MASK_FAMILIES = ("bernoulli", "blob", "leading_dead", "trailing_dead", "single_open", "all_blocked_rows", "none",
                 "no_row_open")
DEAD_TILES = 9  # leading_dead / trailing_dead: more than two rounds of a workgroup's four waves
ZERO_CHECK = ("blob", "leading_dead", "trailing_dead", "single_open")  # families with keys no query attends


def key_grid(N: int):
    """(h, w), h * w = N, h the largest factor up to sqrt(N): the feature map the keys are the pixels of."""
    h = max(d for d in range(1, int(math.isqrt(N)) + 1) if N % d == 0)
    return h, N // h


def single_open_keys(N: int, tiles_per_split: int):
    """Where single_open puts the one open key: both ends, both sides of the first tile boundary and of the first split
    boundary."""
    ks = [0, N - 1]
    for kk in (15, 16, 16 * tiles_per_split - 1, 16 * tiles_per_split):
        if 0 < kk < N - 1 and kk not in ks:
            ks.append(kk)
    return ks


def mask(family: str, B: int, Q: int, N: int, seed: int, tiles_per_split: int = 1):
    """(mask (B, Q, N) bool with True = blocked, or None; row_open (B, Q) int32 or None) on the CPU, seeded.
      bernoulli         independent bytes, 70 % blocked; row 0 of image 0 fully blocked (rows with one open key: single_open)
      blob              one open rectangle per query on the key_grid, at most a sixth of its height: whole key tiles, waves
                        and splits are blocked for a query, and the keys of the map's rightmost eighth are attended by nobody
      leading_dead      the first DEAD_TILES key tiles blocked for every query, 50 % of the rest
      trailing_dead     the last DEAD_TILES key tiles blocked for every query
      single_open       one open key per row, cycling through single_open_keys
      all_blocked_rows  bernoulli 60 % with fully blocked rows (row_open = 0): row 0, the last row and, from 32 queries
                        on, the whole second 16-query tile
      none              no mask at all
      no_row_open       bernoulli with at least one open key per row, passed WITHOUT row_open"""
    if family == "none":
        return None, None
    g = torch.Generator().manual_seed(seed)
    rows = torch.arange(Q)
    if family == "bernoulli":
        m = torch.rand(B, Q, N, generator=g) < 0.7
        m[0, 0] = True
    elif family == "blob":
        h, w = key_grid(N)
        m = torch.ones(B, Q, h, w, dtype=torch.bool)
        hh = torch.randint(1, max(1, h // 6) + 1, (B, Q), generator=g)
        y0 = (torch.rand(B, Q, generator=g) * (h - hh + 1).float()).long().clamp_max(h - 1)
        wb = w - max(1, w // 8)  # the rightmost eighth of the map is a border no rectangle reaches
        ww = torch.randint(2, wb + 1, (B, Q), generator=g)  # at least two open keys: one-hot rows belong to single_open
        x0 = (torch.rand(B, Q, generator=g) * (wb - ww + 1).float()).long().clamp_max(wb - 1)
        for b in range(B):
            for r in range(Q):
                m[b, r, y0[b, r]:y0[b, r] + hh[b, r], x0[b, r]:x0[b, r] + ww[b, r]] = False
        m = m.view(B, Q, N)
    elif family in ("leading_dead", "trailing_dead"):
        dead = DEAD_TILES * 16
        assert N >= dead + 32, "the dead tiles need live ones beside them"
        m = torch.rand(B, Q, N, generator=g) < 0.5
        if family == "leading_dead":
            m[:, :, :dead] = True
            m[:, rows, dead + rows % (N - dead)] = False
        else:
            m[:, :, N - dead:] = True
            m[:, rows, rows % (N - dead)] = False
    elif family == "single_open":
        ks = torch.tensor(single_open_keys(N, tiles_per_split))
        m = torch.ones(B, Q, N, dtype=torch.bool)
        m[:, rows, ks[rows % len(ks)]] = False
    elif family == "all_blocked_rows":
        m = torch.rand(B, Q, N, generator=g) < 0.6
        m[:, rows, (7 * rows) % N] = False
        m[:, 0] = True
        m[:, Q - 1] = True
        if Q >= 32:
            m[:, 16:32] = True
    elif family == "no_row_open":
        m = torch.rand(B, Q, N, generator=g) < 0.7
        m[:, rows, (7 * rows) % N] = False
        return m, None
    else:
        raise ValueError(family)
    return m, (~m.all(-1)).to(torch.int32)


def effective_mask(m, B, Q, N):
    """The mask the attention applies: a fully blocked row attends everywhere (HF:1912-1914); no mask = all open."""
    if m is None:
        return torch.zeros(B, Q, N, dtype=torch.bool)
    return m & ~m.all(-1, keepdim=True)


def split_tiles(N: int, rt: Route, split: int):
    """The key tiles [t0, t1) of a split under a route (empty for a trailing split without tiles)."""
    n_tiles = -(-N // 16)
    t0 = min(split * rt.tiles_per_split, n_tiles)
    return t0, min(t0 + rt.tiles_per_split, n_tiles)


# ------------------------------------------------------------------------------------------------------------ references
def _heads(t, heads):
    B, n, E = t.shape
    return t.view(B, n, heads, E // heads).permute(0, 2, 1, 3)


def _flat(t):
    B, H, n, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, n, H * D)


def _chunks(q, k, v, m, grad_out, dtype, chunk):
    """`chunk` images at a time (the score tensor of a large case stays at a few tens of MB): slice, q, k, v in `dtype`,
    the mask as the attention applies it (B', Q, N) bool, grad_out or None."""
    B, Q, _ = q.shape
    N = k.shape[1]
    for b0 in range(0, B, chunk):
        sl = slice(b0, min(B, b0 + chunk))
        mc = torch.zeros(sl.stop - b0, Q, N, dtype=torch.bool, device=q.device) if m is None else m[sl]
        yield (sl, q[sl].to(dtype), k[sl].to(dtype), v[sl].to(dtype), mc & ~mc.all(-1, keepdim=True),
               None if grad_out is None else grad_out[sl].to(dtype))


def _scores(qc, kc, mm, heads):
    return torch.matmul(_heads(qc, heads), _heads(kc, heads).transpose(-1, -2)).masked_fill(mm[:, None], float("-inf"))


def attention(q, k, v, m, heads: int, grad_out=None, dtype=torch.float64, chunk: int = 8, perm=None):
    """oracle.m2f_oracle.masked_attention_core in `dtype` on the tensors' device: {"out" (B, Q, E), "lse" (B, heads, Q)} and,
    with grad_out, "grad_q", "grad_k", "grad_v" by autograd.  lse is torch.logsumexp of the masked scores.  float64 is the
    reference, float32 the stock fp32 route.  `perm` (a permutation of range(D)) reorders the head dimension of q and k: the
    same scores, summed in another order."""
    names = ("out", "lse") if grad_out is None else ("out", "lse", "grad_q", "grad_k", "grad_v")
    res = {n: [] for n in names}
    if perm is not None:
        D = q.shape[-1] // heads
        idx = (torch.arange(heads)[:, None] * D + torch.as_tensor(perm)[None, :]).flatten().to(q.device)
        q, k = q[..., idx], k[..., idx]
    for sl, qc, kc, vc, mm, go in _chunks(q, k, v, m, grad_out, dtype, chunk):
        qc, kc, vc = (t.detach().requires_grad_(go is not None) for t in (qc, kc, vc))
        out = _flat(O.masked_attention_core(_heads(qc, heads), _heads(kc, heads), _heads(vc, heads), mm))
        res["out"].append(out.detach())
        with torch.no_grad():
            res["lse"].append(torch.logsumexp(_scores(qc, kc, mm, heads), -1))
        if go is not None:
            for n, gr in zip(names[2:], torch.autograd.grad(out, (qc, kc, vc), go)):
                res[n].append(gr)
    return {n: torch.cat(ts) for n, ts in res.items()}


LOG2E, LN2F = 1.4426950408889634, 0.6931471805599453


def attention_flash_fp32(q, k, v, m, heads: int, grad_out, perm, log2_forward: bool, chunk: int = 8):
    """The comparator of the gradients of the cancelling families: the kernels' flash arithmetic in plain fp32 torch ops.
    Forward: out, and lse stored as ONE fp32 number per row -- in the log2 domain as the full-tile forward works
    (scores of q log2 e, lse = m ln 2 + ln sum 2^(s - m)) when log2_forward.  Backward recomputed from them, with the scores
    evaluated AGAIN and independently, as the kernels do (the backward multiplies Q K^T in its own orientation and, after a
    full-tile forward, in another domain): here with the head dimension in the order `perm`.  p = exp(s - lse),
    delta = sum_d dO out as a sum of its own, dS = p (dP - delta), grad_q = dS k, grad_k = dS^T q, grad_v = p^T dO.
    That independent rounding of a score of magnitude |s|, U32 |s| in p and different from key to key, is what separates a
    flash backward from the stock route on these families; with the forward's own score bits the comparator is as accurate as
    the stock route (ramps: grad_q 4e-8 of the terms instead of 1e-6 to 3e-6).  Same gradient keys as attention()."""
    res = {n: [] for n in ("grad_q", "grad_k", "grad_v")}
    D = q.shape[-1] // heads
    idx = (torch.arange(heads)[:, None] * D + torch.as_tensor(perm)[None, :]).flatten().to(q.device)
    with torch.no_grad():
        for sl, qc, kc, vc, mm, go in _chunks(q, k, v, m, grad_out, torch.float32, chunk):
            qh, kh, vh, gh = (_heads(t, heads) for t in (qc, kc, vc, go))
            if log2_forward:
                s2 = _scores(qc * LOG2E, kc, mm, heads)
                mx = s2.amax(-1)
                lse = mx * LN2F + torch.log(torch.exp2(s2 - mx[..., None]).sum(-1))
                out = torch.matmul(torch.softmax(s2 * LN2F, -1), vh)
            else:
                s = _scores(qc, kc, mm, heads)
                lse, out = torch.logsumexp(s, -1), torch.matmul(torch.softmax(s, -1), vh)
            p = torch.exp(_scores(qc[..., idx], kc[..., idx], mm, heads) - lse[..., None])
            ds = p * (torch.matmul(gh, vh.transpose(-1, -2)) - (gh * out).sum(-1)[..., None])
            for n, t in zip(res, (torch.matmul(ds, kh), torch.matmul(ds.transpose(-1, -2), qh), torch.matmul(p.transpose(-1, -2), gh))):
                res[n].append(_flat(t))
    return {n: torch.cat(ts) for n, ts in res.items()}


def error_scales(q, k, v, m, heads: int, grad_out=None, lse_given=None, chunk: int = 8):
    """The fp64 bookkeeping beside the reference: {"smag": the largest sum_d |q_d k_d| over the open (query, key) pairs, the
    scores' rounding scale} and, with grad_out, "mag_q" (B, heads, Q), "mag_k", "mag_v" (B, heads, N) (grad_magnitudes) and,
    with `lse_given` (the lse a backward kernel read), "lsemax_q / _k / _v" and "lse2_q / _k / _v" (lse_propagation)."""
    names = [] if grad_out is None else ["mag_q", "mag_k", "mag_v"]
    if grad_out is not None and lse_given is not None:
        names += ["lsemax_q", "lse2_q", "lsemax_k", "lse2_k", "lsemax_v", "lse2_v"]
    res, smag = {n: [] for n in names}, 0.0
    with torch.no_grad():
        for sl, qc, kc, vc, mm, go in _chunks(q, k, v, m, grad_out, torch.float64, chunk):
            qh, kh, vh = (_heads(t, heads) for t in (qc, kc, vc))
            sa = torch.matmul(qh.abs(), kh.abs().transpose(-1, -2))
            smag = max(smag, sa.masked_fill(mm[:, None], 0.0).amax().item())
            if go is None:
                continue
            gh, s = _heads(go, heads), _scores(qc, kc, mm, heads)
            p = torch.softmax(s, -1)
            out = torch.matmul(p, vh)
            vals = list(grad_magnitudes(p, qh, kh, vh, gh, out))
            if lse_given is not None:
                d = (lse_given[sl].double() - torch.logsumexp(s, -1)).abs()
                ds = p * (torch.matmul(gh, vh.transpose(-1, -2)) - (gh * out).sum(-1)[..., None])
                gq = torch.matmul(ds, kh)  # grad_q: an lse error d scales the row by e^d, to first order d x the row itself
                vals += [d * gq.abs().amax(-1), d * gq.norm(dim=-1), *lse_propagation(p, d, qh, vh, gh, out)]
            for n, t in zip(names, vals):
                res[n].append(t)
    return {"smag": smag, **{n: torch.cat(ts) for n, ts in res.items()}}


def grad_magnitudes(p, q, k, v, go, out):
    """Per row of grad_q (B, H, Q), grad_k and grad_v (B, H, N): the sum of the magnitudes of the terms the row is a sum of,
    with dS = p (dP - delta), dP = dO v^T, delta = sum_d dO out:
      grad_q[q] = sum_n dS[q, n] k[n]  ->  sum_n p (|dO| |v|^T + |dO| . |out|) max_d |k[n]|
      grad_k[n] = sum_q dS[q, n] q[q]  ->  sum_q p (|dO| |v|^T + |dO| . |out|) max_d |q[q]|
      grad_v[n] = sum_q p[q, n] dO[q]  ->  sum_q p max_d |dO[q]|
    dP and delta enter with the magnitudes of THEIR terms (sum_d |dO_d v_d|, sum_d |dO_d out_d|): both are fp32 dot
    products whose rounding scales with those, however small the products come out.
    All arguments (B, H, rows, D) / p (B, H, Q, N), any float dtype."""
    dp = torch.matmul(go.abs(), v.abs().transpose(-1, -2))
    w = p * (dp + (go.abs() * out.abs()).sum(-1)[..., None])
    return ((w * k.abs().amax(-1)[:, :, None, :]).sum(-1), (w * q.abs().amax(-1)[..., None]).sum(-2),
            (p * go.abs().amax(-1)[..., None]).sum(-2))


def lse_propagation(p, d, q, v, go, out):
    """What an error d (B, H, Q) of the stored lse does to grad_k and grad_v, to first order.  The backward recomputes
    p = exp(s - lse), so every p and dS = p (dP - delta) of query row q is scaled by e^d[q]:
      |change of grad_k[n]| <= sum_q d[q] |dS[q, n]| |q[q]|,   |change of grad_v[n]| <= sum_q d[q] p[q, n] |dO[q]|
    (and grad_q[q] changes by d[q] grad_q[q]).  Returned per row (B, H, N) with |.| = max_d (for the worst-row measure) and
    = the 2-norm (for the Frobenius measure): (k max, k 2-norm, v max, v 2-norm).  fp64 arguments."""
    ds = (p * (torch.matmul(go, v.transpose(-1, -2)) - (go * out).sum(-1)[..., None])).abs() * d[..., None]
    pv = p * d[..., None]
    return ((ds * q.abs().amax(-1)[..., None]).sum(-2), (ds * q.norm(dim=-1)[..., None]).sum(-2),
            (pv * go.abs().amax(-1)[..., None]).sum(-2), (pv * go.norm(dim=-1)[..., None]).sum(-2))


def attention_stock_bf16(q, k, v, m, heads: int, grad_out=None):
    """The stock bf16-autocast route on bf16 q, k, v: a bf16 product, an fp32 softmax rounded to bf16, a bf16 product, with
    autograd through the same ops.  lse is the fp32 log-sum-exp of the bf16 scores."""
    B, Q, _ = q.shape
    N = k.shape[1]
    qc, kc, vc = (t.detach().to(torch.bfloat16).requires_grad_(grad_out is not None) for t in (q, k, v))
    mm = torch.zeros(B, Q, N, dtype=torch.bool, device=q.device) if m is None else m & ~m.all(-1, keepdim=True)
    s = torch.matmul(_heads(qc, heads), _heads(kc, heads).transpose(-1, -2)).masked_fill(mm[:, None], float("-inf"))
    p = torch.softmax(s.float(), -1).to(torch.bfloat16)
    out = _flat(torch.matmul(p, _heads(vc, heads)))
    res = {"out": out.detach(), "lse": torch.logsumexp(s.detach().float(), -1)}
    if grad_out is not None:
        gs = torch.autograd.grad(out, (qc, kc, vc), grad_out.to(torch.bfloat16))
        res.update(zip(("grad_q", "grad_k", "grad_v"), gs))
    return res


# --------------------------------------------------------------------------------------------------------- measure, rule
TINY = 1e-30  # as in test_swin_attn_bwd_gpu.py: magnitudes fp32 does not hold count as zero


def fro_err(x, ref) -> float:
    """Relative Frobenius error; a non-finite value counts as an infinite error; a zero reference wants a zero."""
    x = x.double()
    if not torch.isfinite(x).all():
        return float("inf")
    rn = ref.norm().item()
    if rn < TINY:
        return 0.0 if x.norm().item() < TINY else float("inf")
    return ((x - ref).norm() / rn).item()


def row_err(x, ref, heads: int) -> float:
    """max over the (batch, token, head) rows of max_d |x - ref| / max_d |ref|.  A row whose reference is below TINY is
    measured against TINY (exactly zero rows: any nonzero value there is an infinite error)."""
    x = x.double()
    if not torch.isfinite(x).all():
        return float("inf")
    B, n, E = ref.shape
    d = (x - ref).abs().view(B, n, heads, E // heads).amax(-1)
    r = ref.abs().view(B, n, heads, E // heads).amax(-1)
    e = torch.where(r == 0, torch.where(d == 0, 0.0, float("inf")).to(d.dtype), d / r.clamp_min(TINY))
    return e.max().item()


def grad_fro_err(x, ref, mag) -> float:
    """A gradient's error relative to its error scale: ||x - ref||_F / ||mag||_F (mag from grad_magnitudes, one value per
    row).  A gradient whose terms are all zero wants zeros."""
    x = x.double()
    if not torch.isfinite(x).all():
        return float("inf")
    mn = mag.norm().item()
    if mn < TINY:
        return 0.0 if x.norm().item() < TINY else float("inf")
    return ((x - ref).norm() / mn).item()


def grad_row_err(x, ref, mag) -> float:
    """max over the (batch, token, head) rows of max_d |x - ref| / mag[row]; a row without terms (mag = 0: a key nobody
    attends) wants exact zeros."""
    x = x.double()
    if not torch.isfinite(x).all():
        return float("inf")
    B, H, n = mag.shape
    d = (x - ref).abs().view(B, n, H, -1).amax(-1).permute(0, 2, 1)
    e = torch.where(mag == 0, torch.where(d == 0, 0.0, float("inf")).to(d.dtype), d / mag.clamp_min(TINY))
    return e.max().item()


def abs_err(x, ref) -> float:
    x = x.double()
    return float("inf") if not torch.isfinite(x).all() else (x - ref).abs().max().item()


def rule(e: float, e_stock: float, extra: float = 0.0) -> bool:
    """fp32: no worse than twice the stock fp32 route, floor 1e-6; `extra` is one of the derived terms below."""
    return e <= max(2.0 * e_stock, 1e-6) + extra


U32 = 2.0 ** -24  # unit roundoff of fp32


def lse_term(kernel: int, smag: float, lse_max: float) -> float:
    """What the full-tile forward adds to lse beyond the stock route's roundings: it works in the log2
    domain, so q is multiplied by log2 e (one rounding per element: U32 sum_d |q_d k_d| on a score), the running maximum is
    multiplied back by ln 2 (one rounding: U32 |m|, |m| <= |lse|), and the two constants are themselves fp32 roundings of
    log2 e and ln 2 whose product is 1 only to within U32 (another U32 |m|)."""
    return U32 * (smag + 2.0 * lse_max) if kernel in (FWD_FULL, BF16_FWD) else 0.0


# Gradients of these value families and of the single_open mask are measured against the magnitude of their terms
# (grad_errs(terms=True)) and compared with the kernels' flash arithmetic in plain fp32 torch ops (attention_flash_fp32, the
# worse of its two summation orders STOCK_ORDERS) under the unmodified factor-2 rule: p is one-hot or nearly so on their rows (one open key; scores 30 to 150 standard deviations wide;
# one outlier; a ramp of which a mask can leave one key in the top tile), so dS = p (dP - delta) cancels, to exactly zero
# where p is one-hot, and the stock softmax backward, which subtracts its own sum_n p dP, returns that zero: against it a
# correct flash backward (separate delta, p recomputed from a stored lse) has an unbounded relative error.  Every other
# family keeps the plain measures and the stock comparator.
CANCELLING_VALUES = ("wide", "asc", "desc", "outlier")


def cancelling(c) -> bool:
    return c.mask == "single_open" or c.values.startswith(CANCELLING_VALUES)


def grad_slack(ref, name: str):
    """(rows (B, H, n), Frobenius scalar): the absolute error a correct flash backward carries in gradient `name` of a
    NON-cancelling family beyond a summation order, where its arithmetic differs from the stock route's:
      * it recomputes p = exp(s - lse) from the ONE fp32 number per row the forward stored, so that number's error reaches
        every p and dS of the row in full (lse_propagation, with the MEASURED error of the lse the backward read, which the
        lse rule bounds on its own); the stock route normalises p by its row sum;
      * worst row only: delta = sum_d dO out is a separate fp32 sum from dP = sum_d dO v, so sum_n dS is zero only to one
        rounding of the terms, U32 x their magnitude (grad_magnitudes; measured need: 0.31 of it), where the stock route's
        softmax backward subtracts its own sum_n p dP.
    The cancelling families have no slack: their comparator is attention_flash_fp32."""
    t = name[-1]
    return ref["lsemax_" + t] + U32 * ref["mag_" + t], ref["lse2_" + t].norm().item()


def grad_errs(x, ref, name: str, heads: int, terms: bool, slack: bool):
    """(Frobenius, worst row) error of gradient `name` against ref[name].  terms: both relative to the magnitude of the
    terms (the cancelling families); else the plain measures, relative to the reference.  slack: grad_slack is taken off
    each row's (and the tensor's) absolute error first -- the kernel under test; the stock route is measured raw.  A row
    (tensor) whose denominator is zero wants what is left to be zero."""
    x, g, t = x.double(), ref[name], name[-1]
    if not torch.isfinite(x).all():
        return float("inf"), float("inf")
    B, n, E = g.shape
    rows = lambda a: a.abs().view(B, n, heads, E // heads).amax(-1).permute(0, 2, 1)
    d_rows, d_fro = rows(x - g), (x - g).norm().item()
    if slack:
        s_rows, s_fro = grad_slack(ref, name)
        d_rows, d_fro = (d_rows - s_rows).clamp_min(0.0), max(0.0, d_fro - s_fro)
    den_rows, den_fro = (ref["mag_" + t], ref["mag_" + t].norm().item()) if terms else (rows(g), g.norm().item())
    e = torch.where(den_rows == 0, torch.where(d_rows == 0, 0.0, float("inf")).to(d_rows.dtype), d_rows / den_rows.clamp_min(TINY))
    fro = d_fro / den_fro if den_fro >= TINY else (0.0 if d_fro < TINY else float("inf"))
    return fro, e.max().item()


# summation orders of a score other than the natural one: of the stock scores (wide families, out), of the flash comparator's
# recomputed scores (cancelling families, gradients)
STOCK_ORDERS = ("reversed", "interleaved")


def order(name: str, D: int):
    return list(range(D - 1, -1, -1)) if name == "reversed" else list(range(0, D, 2)) + list(range(1, D, 2))


def rule_bf16(e: float, e_stock: float) -> bool:
    """bf16: no worse than the stock bf16 route (margin 1.0), whose own error stays below 2e-2."""
    return e_stock < 2e-2 and e <= e_stock


# ------------------------------------------------------------------------------------------------------------ case table
class Case(NamedTuple):
    name: str
    B: int
    heads: int
    Q: int
    N: int
    D: int
    dtype: int
    values: str
    mask: str
    fwd: Route                   # the route the table claims for the forward ...
    bwd: Optional[Route] = None  # ... and for the backward of a backward case
    aligned: bool = True         # False: the mask is handed over at an odd address (general forward at N % 16 == 0)

    @property
    def seed(self) -> int:
        return 1000 * self.N + 10 * self.Q + self.D + self.B


def _c(name, B, heads, Q, N, D, dtype, vals, msk, fwd, bwd=None, aligned=True):
    return Case(name, B, heads, Q, N, D, dtype, vals, msk, Route(*fwd), None if bwd is None else Route(*bwd), aligned)


G, F, BG, BF = FWD_GENERAL, FWD_FULL, BWD_GENERAL, BWD_FULL
# Shapes: per (kernel, D, NQT) the fewest queries that give the NQT (10 / 20 / 40 / 100 -> 1 / 2 / 4 / 7 query tiles; 130 and
# 146 -> two chunks) and few keys, except where the point of the case needs tiles: the value families that act along the key
# axis and the dead-tile masks run at N = 464 / 528 / 656 (29 / 33 / 41 tiles).  The routes are what
# wm2f_masked_xattn_route returned when the table was written; test_k2_cases_cpu.py holds them to it.
CASES = [
    # ---- fp32, D = 32: general forward (N % 16 != 0, or an odd mask address) and general backward
    _c("g32_q1", 2, 2, 10, 37, 32, F32, "randn", "bernoulli", (G, 1, 1, 1, 3, 0), (BG, 4, 1, 1, 3, 0)),
    _c("g32_q2", 1, 4, 20, 130, 32, F32, "outlier", "no_row_open", (G, 2, 1, 3, 3, 0), (BG, 4, 1, 3, 3, 0)),
    _c("g32_q4_odd_address", 1, 4, 64, 464, 32, F32, "asc8.5", "leading_dead", (G, 4, 1, 8, 4, 0), (BG, 4, 1, 8, 4, 0), False),
    _c("g32_q7", 1, 2, 100, 283, 32, F32, "wide30", "blob", (G, 7, 1, 5, 4, 0), (BG, 7, 1, 5, 4, 0)),
    _c("g32_q7_two_chunks", 1, 2, 130, 300, 32, F32, "offset_v", "all_blocked_rows", (G, 7, 2, 5, 4, 0), (BG, 7, 2, 5, 4, 1)),
    # ---- fp32, D = 32: full-tile forward
    _c("f32_q1_wave_without_tile", 1, 4, 16, 16, 32, F32, "randn", "all_blocked_rows", (F, 1, 1, 1, 1, 0), (BG, 4, 1, 1, 1, 0)),
    _c("f32_q2", 1, 4, 32, 464, 32, F32, "asc7.5", "trailing_dead", (F, 2, 1, 8, 4, 0), (BG, 4, 1, 8, 4, 0)),
    _c("f32_q4", 2, 4, 40, 528, 32, F32, "asc12", "blob", (F, 4, 1, 9, 4, 0), (BG, 4, 1, 9, 4, 0)),
    _c("f32_q7_full_chunk", 1, 2, 112, 464, 32, F32, "wide150", "single_open", (F, 7, 1, 8, 4, 0), (BG, 7, 1, 8, 4, 0)),
    _c("f32_q7_odd_tiles_per_wave", 2, 16, 100, 464, 32, F32, "asc2.1", "bernoulli", (F, 7, 1, 8, 4, 0), (BG, 7, 1, 8, 4, 0)),
    _c("f32_q7_wide150", 1, 2, 100, 464, 32, F32, "wide150", "bernoulli", (F, 7, 1, 8, 4, 0), (BG, 7, 1, 8, 4, 0)),
    _c("f32_q7_no_mask", 2, 8, 100, 208, 32, F32, "randn", "none", (F, 7, 1, 4, 4, 0), (BG, 7, 1, 4, 4, 0)),
    # ---- fp32, D = 32: full-tile backward, both NQT (the first reference tests this kernel gets)
    _c("bf32_q4", 32, 8, 40, 464, 32, F32, "randn", "blob", (F, 4, 1, 1, 29, 0), (BF, 4, 1, 4, 8, 0)),
    _c("bf32_q7", 32, 8, 100, 528, 32, F32, "outlier", "all_blocked_rows", (F, 7, 1, 1, 33, 0), (BF, 7, 1, 4, 9, 0)),
    _c("bf32_q4_values", 32, 8, 40, 464, 32, F32, "asc8.5", "leading_dead", (F, 4, 1, 1, 29, 0), (BF, 4, 1, 4, 8, 0)),
    _c("bf32_q7_values", 32, 8, 100, 528, 32, F32, "offset_v", "trailing_dead", (F, 7, 1, 1, 33, 0), (BF, 7, 1, 4, 9, 0)),
    _c("bf32_q4_wide", 32, 8, 40, 464, 32, F32, "wide150", "no_row_open", (F, 4, 1, 1, 29, 0), (BF, 4, 1, 4, 8, 0)),
    _c("bf32_q7_single", 32, 8, 100, 528, 32, F32, "outlier", "single_open", (F, 7, 1, 1, 33, 0), (BF, 7, 1, 4, 9, 0)),
    # ---- fp32, D = 16
    _c("g16_q1", 1, 4, 10, 70, 16, F32, "uniform", "bernoulli", (G, 1, 1, 2, 3, 0), (BG, 4, 1, 2, 3, 0)),
    _c("g16_q2", 1, 4, 20, 130, 16, F32, "randn", "all_blocked_rows", (G, 2, 1, 3, 3, 0), (BG, 4, 1, 3, 3, 0)),
    _c("g16_q4", 1, 2, 40, 283, 16, F32, "desc12", "blob", (G, 4, 1, 5, 4, 0), (BG, 4, 1, 5, 4, 0)),
    _c("g16_q7", 1, 2, 100, 300, 16, F32, "wide30", "single_open", (G, 7, 1, 5, 4, 0), (BG, 7, 1, 5, 4, 0)),
    _c("g16_q7_two_chunks", 1, 1, 146, 114, 16, F32, "randn", "bernoulli", (G, 7, 2, 2, 4, 0), (BG, 7, 2, 2, 4, 1)),
    _c("f16_q1", 1, 4, 16, 144, 16, F32, "uniform", "no_row_open", (F, 1, 1, 3, 3, 0)),
    _c("f16_q2_empty_split", 1, 26, 20, 656, 16, F32, "asc4", "blob", (F, 2, 1, 10, 5, 0)),
    _c("f16_q4_empty_split_bwd", 6, 19, 40, 592, 16, F32, "asc1.9", "leading_dead", (F, 4, 1, 3, 13, 0), (BG, 4, 1, 9, 5, 0)),
    _c("f16_q7", 1, 2, 100, 464, 16, F32, "desc12", "trailing_dead", (F, 7, 1, 8, 4, 0), (BG, 7, 1, 8, 4, 0)),
    # ---- fp32, D = 64 (forward: at most 2 query tiles per workgroup; backward: 3)
    _c("g64_q1", 1, 2, 10, 100, 64, F32, "randn", "bernoulli", (G, 1, 1, 2, 4, 0), (BG, 3, 1, 2, 4, 0)),
    _c("g64_q2_two_chunks", 1, 2, 53, 283, 64, F32, "outlier", "blob", (G, 2, 2, 5, 4, 0), (BG, 3, 2, 5, 4, 1)),
    _c("f64_q1", 1, 2, 16, 464, 64, F32, "asc8.5", "single_open", (F, 1, 1, 8, 4, 0), (BG, 3, 1, 8, 4, 0)),
    _c("f64_q2", 1, 2, 48, 464, 64, F32, "wide30", "leading_dead", (F, 2, 2, 8, 4, 0), (BG, 3, 1, 8, 4, 0)),
    # ---- bf16 (D = 32, N % 16 == 0): the value families whose stock bf16 route is a reference at all -- it rounds the
    # scores to bf16 (2^-9 relative), which at logits of tens is an error in p of tens of percent and above its 2e-2 bound
    _c("b_q1", 1, 4, 16, 16, 32, BF16, "randn", "bernoulli", (BF16_FWD, 1, 1, 1, 1, 0), (BF16_BWD, 4, 1, 1, 1, 0)),
    _c("b_q2", 1, 4, 20, 464, 32, BF16, "randn", "blob", (BF16_FWD, 2, 1, 8, 4, 0), (BF16_BWD, 4, 1, 8, 4, 0)),
    _c("b_q4", 32, 8, 40, 464, 32, BF16, "randn", "leading_dead", (BF16_FWD, 4, 1, 1, 29, 0), (BF16_BWD, 4, 1, 4, 8, 0)),
    _c("b_q4_no_mask", 1, 4, 37, 272, 32, BF16, "randn", "none", (BF16_FWD, 4, 1, 5, 4, 0), (BF16_BWD, 4, 1, 5, 4, 0)),
    _c("b_q7", 2, 8, 100, 528, 32, BF16, "randn", "all_blocked_rows", (BF16_FWD, 7, 1, 9, 4, 0), (BF16_BWD, 7, 1, 9, 4, 0)),
    # (with one open key per row grad_q and grad_k are identically zero: held to the dot products' rounding bound instead of
    # the margin-1.0 rule, which has no floor; grad_v and the rows of unattended keys as everywhere)
    _c("b_q7_single", 1, 2, 112, 464, 32, BF16, "randn", "single_open", (BF16_FWD, 7, 1, 8, 4, 0), (BF16_BWD, 7, 1, 8, 4, 0)),
    _c("b_q7_two_chunks_fp32_bwd", 1, 2, 130, 464, 32, BF16, "randn", "trailing_dead", (BF16_FWD, 7, 2, 8, 4, 0), (BG, 7, 2, 8, 4, 1)),
]
BY_NAME = {c.name: c for c in CASES}
BACKWARD_CASES = [c for c in CASES if c.bwd is not None]


def case_route(c: Case, backward: bool) -> Route:
    """The route wm2f_masked_xattn_route gives a case.  A bf16 case with more than 112 queries runs its backward on the fp32
    entry point (ops/k2.py)."""
    dtype = F32 if backward and c.dtype == BF16 and c.Q > 112 else c.dtype
    return route(c.B, c.heads, c.Q, c.N, c.D, dtype, backward, c.aligned or backward)


def instantiation(c: Case, backward: bool):
    r = c.bwd if backward else c.fwd
    return (r.kernel, c.D, r.nqt, r.accumulate)


def case_inputs(c: Case):
    """q, k, v, grad_out (fp32, rounded to bf16 values for a bf16 case), mask (bool or None), row_open: CPU tensors."""
    q, k, v, go = values(c.values, c.B, c.heads, c.Q, c.N, c.D, c.seed)
    if c.dtype == BF16:
        q, k, v, go = (t.bfloat16().float() for t in (q, k, v, go))
    m, ro = mask(c.mask, c.B, c.Q, c.N, c.seed + 1, (c.bwd or c.fwd).tiles_per_split)
    return q, k, v, go, m, ro


def unattended_keys(c: Case, m):
    """(B, N) bool: keys blocked in every row of their image, in a case where no row is fully blocked (such a row attends
    everywhere).  grad_k / grad_v are exactly zero there: the kernels zero p by select."""
    if m is None or c.mask not in ZERO_CHECK or bool(m.all(-1).any()):
        return None
    return m.all(1)
