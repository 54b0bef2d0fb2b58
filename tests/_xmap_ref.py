"""References for the per-character attention maps (wd_xattn_maps, forward(return_attention=), the samplers' attention=).

record_maps         the oracle's own attn2 softmax of the three tapped SpatialTransformers (the last one of the input blocks, the
                    middle one, the last one of the output blocks: unet.py:1645-1832), summed over heads: oracle.unet_oracle.
                    cross_attention already returns (out, probs) and transformer_block drops the probabilities, so the recorder
                    wraps that function for the length of one forward.  Nothing under oracle/ is edited.
xattn_maps_spec     what wd_xattn_maps computes from raw operands, in float64: LayerNorm -> scores against the fp32 folded matrix
                    mq -> softmax per head -> head sum; the first attention of the pair form in full before it.
accumulate_fp32     the accumulate form replayed on the host: acc + w * m with the product and the sum rounded to fp32 one after
                    the other (numpy float32 arithmetic rounds every operation).
weight_table        the samplers' weight table from first principles."""
import math
import re

import numpy as np
import torch

from oracle import unet_oracle as U

_ATTN2 = re.compile(r"(input_blocks\.(\d+)\.\d+|middle_block\.\d+|output_blocks\.(\d+)\.\d+)\.transformer_blocks\.(\d+)\.attn2\.$")


def tapped_prefixes(seen):
    """Of the attn2 prefixes one forward went through, in call order: (last of the input blocks, middle, last of the outputs)."""
    ins = [p for p in seen if p.startswith("input_blocks.")]
    mid = [p for p in seen if p.startswith("middle_block.")]
    outs = [p for p in seen if p.startswith("output_blocks.")]
    assert ins and len(mid) == 1 and outs, seen
    return ins[-1], mid[0], outs[-1]


def record_maps(monkeypatch, orc, x, t, context, y):
    """(eps, [m_in, m_mid, m_out]) of one oracle forward; m_i float64 [B, h_i, w_i, L], the attn2 probabilities summed over heads."""
    seen, probs = [], {}
    real = U.cross_attention

    def spy(sd, p, xx, ctx, heads):
        out, attn = real(sd, p, xx, ctx, heads)
        if _ATTN2.search(p):
            seen.append(p)
            probs[p] = attn.detach()
        return out, attn

    monkeypatch.setattr(U, "cross_attention", spy)
    try:
        with torch.no_grad():
            eps = orc(x, t, context, y)
    finally:
        monkeypatch.setattr(U, "cross_attention", real)
    B, _, H, W = x.shape
    maps = []
    for p in tapped_prefixes(seen):
        a = probs[p].double()                      # [B, heads, N, L]
        s = int(round(math.sqrt(H * W / a.shape[2])))
        assert (H // s) * (W // s) == a.shape[2], (p, a.shape)
        maps.append(a.sum(1).reshape(B, H // s, W // s, a.shape[3]))
    return eps, maps


def _ln(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def xattn_maps_spec(x, B, hw, heads, L, gb, bb, mq_b, first=None, eps=1e-5):
    """float64 maps [B * hw][L].  x [B * hw][c]; gb, bb: the tapped attention's LayerNorm; mq_b: its fp32 folded matrix
    [B][heads * L][c] (as wd_xattn_fold wrote it).  first = (ga, ba, mq_a, mo_a, bias_a): the attention that runs before it,
    xa = x + bias + softmax(LN(x) . Mq_a^T) . Mo_a."""
    x = x.double()
    c = x.shape[1]
    if first is not None:
        ga, ba, mq_a, mo_a, bias_a = (v.double() for v in first)
        s = torch.einsum("btn,bkn->btk", _ln(x, ga, ba, eps).view(B, hw, c), mq_a).view(B, hw, heads, L)
        p = torch.softmax(s, -1).reshape(B, hw, heads * L)
        x = (torch.einsum("btk,bkn->btn", p, mo_a) + bias_a).reshape(B * hw, c) + x
    s = torch.einsum("btn,bkn->btk", _ln(x, gb.double(), bb.double(), eps).view(B, hw, c), mq_b.double()).view(B, hw, heads, L)
    return torch.softmax(s, -1).sum(2).reshape(B * hw, L)


def accumulate_fp32(acc, w, m):
    """acc + w * m as the kernel evaluates it: fp32 product, rounded, then fp32 sum, rounded.  numpy arrays / scalars."""
    prod = (np.float32(w) * np.asarray(m, dtype=np.float32)).astype(np.float32)
    return (np.asarray(acc, dtype=np.float32) + prod).astype(np.float32)


def weight_table(rows, steps, timestep_of, window):
    """(fp32 table [rows], N).  steps: (row, calls_model) per visited step in loop order; timestep_of(row) -> t; window: True or
    (t_hi, t_lo).  1/N (one fp32 division) at the N model-calling steps inside the window, 0 elsewhere."""
    sel = [r for r, fwd in steps if fwd and (window is True or window[1] <= timestep_of(r) <= window[0])]
    w = np.zeros(rows, dtype=np.float32)
    if sel:
        w[sel] = np.float32(1.0) / np.float32(len(sel))
    return w, len(sel)
