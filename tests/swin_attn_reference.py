"""Float64 restatement of the shifted-window attention contract (include/wm2f.h, wm2f_swin_window_attn_fwd), written from
the contract's bullet list with index arithmetic only -- no roll, no window partition -- so that it shares no code with
either route of backbone_swin.Layer.  test_swin_attn_cpu.py pins it against the stock route on CPU; the GPU tests use it
as the reference of the kernel."""
import torch


def window_slots(H, W, ws, shift):
    """Per window (row-major over (wy, wx)) and slot (i * ws + j):
    tok (nW, L) token index py * W + px in the image (0 where padding), real (nW, L) bool, region (nW, L) shift-mask id."""
    nWy, nWx = -(-H // ws), -(-W // ws)
    Hp, Wp = nWy * ws, nWx * ws
    r = torch.arange(Hp).view(nWy, 1, ws, 1).expand(nWy, nWx, ws, ws)  # rolled-frame row of (wy, wx, i, j)
    c = torch.arange(Wp).view(1, nWx, 1, ws).expand(nWy, nWx, ws, ws)
    py, px = (r + shift) % Hp, (c + shift) % Wp  # padded-frame position the slot's token comes from and goes back to
    real = (py < H) & (px < W)
    tok = torch.where(real, py * W + px, torch.zeros_like(py))
    region = torch.zeros_like(py)
    if shift > 0:
        region = 3 * ((r >= Hp - ws).long() + (r >= Hp - shift).long()) + ((c >= Wp - ws).long() + (c >= Wp - shift).long())
    f = lambda t: t.reshape(nWy * nWx, ws * ws)
    return f(tok), f(real), f(region)


def gather_windows(t, pad_row, tok, real):
    """(B, H*W, E) image-order rows -> (B, nW, L, E) window-order rows; padding slots hold pad_row (zeros if None)."""
    g = t[:, tok]
    pad = torch.zeros(t.shape[-1], dtype=t.dtype, device=t.device) if pad_row is None else pad_row.to(t.dtype)
    return torch.where(real.to(t.device)[None, :, :, None], g, pad)


def relative_bias(table, ws):
    """(heads, L, L): table[(i1 - i2 + ws - 1) (2 ws - 1) + (j1 - j2 + ws - 1), head] for query slot 1, key slot 2."""
    s = torch.arange(ws * ws)
    i, j = s // ws, s % ws
    idx = (i[:, None] - i[None, :] + ws - 1) * (2 * ws - 1) + (j[:, None] - j[None, :] + ws - 1)
    return table[idx.to(table.device)].permute(2, 0, 1)


def shift_mask(region):
    """(nW, L, L): -100 where query and key region ids differ, else 0."""
    diff = region[:, :, None] != region[:, None, :]
    return torch.where(diff, torch.full((), -100.0, dtype=torch.float64), torch.zeros((), dtype=torch.float64))


def scatter_windows(o, tok, real, B, N):
    """(B, nW, L, E) window-order rows -> (B, N, E) image order; padding slots are dropped."""
    out = torch.zeros(B, N, o.shape[-1], dtype=o.dtype, device=o.device)
    out[:, tok[real]] = o[:, real]
    return out


def swin_window_attention_reference(q, k, v, table, dims, heads, ws, shift, k_pad=None, v_pad=None):
    """The contract in float64 on the tensors' device.  q, k, v (B, H*W, heads*D); table ((2 ws - 1)^2, heads)."""
    H, W = dims
    q, k, v, table = q.double(), k.double(), v.double(), table.double()
    k_pad = None if k_pad is None else k_pad.double()
    v_pad = None if v_pad is None else v_pad.double()
    B, N, E = q.shape
    D = E // heads
    tok, real, region = (t.to(q.device) for t in window_slots(H, W, ws, shift))
    L = ws * ws
    split = lambda t: t.view(B, -1, L, heads, D).permute(0, 1, 3, 2, 4)  # (B, nW, heads, L, D)
    qw = split(gather_windows(q, None, tok, real))  # a padding query's output is never written
    kw, vw = split(gather_windows(k, k_pad, tok, real)), split(gather_windows(v, v_pad, tok, real))
    s = qw @ kw.transpose(-1, -2) * D ** -0.5 + relative_bias(table, ws)[None, None]
    if shift > 0:
        s = s + shift_mask(region).to(s.device)[None, :, None]
    o = torch.softmax(s, dim=-1) @ vw  # padding tokens are keys like any other: not masked
    o = o.permute(0, 1, 3, 2, 4).reshape(B, -1, L, E)
    return scatter_windows(o, tok, real, B, N)
