"""Host specification of the forward attention kernels (csrc/wd_attn.hip, csrc/wd_xattn.hip) for their tests.  No GPU.

  attention_fp64   softmax(q k^T * scale) v in fp64 on the same fp32 operands: the reference of every GPU test.
  emulate_mfma     the arithmetic class of attn_mfma_kernel in torch: q pre-scaled by scale * log2(e) in fp32, operands split into
                   bf16 hi / lo, three products (hi.hi, hi.lo, lo.hi) accumulated in fp32, fp32 scores, the online exp2 softmax
                   over 32-key sub-blocks with the lazily moved maximum (FA_LAZY), P split the same way for P.V, the key-split
                   merge of the 64-query form.  It is not bit-exact (the MFMA's order of summation and v_exp_f32 are the
                   hardware's), it bounds what the arithmetic class alone costs on an input.  ``force_alpha_one`` is the bug the
                   staircase inputs exist for: the rescale of the running state skipped after the first block.
  emulate_fp32     the class of attn_kernel / attn_small_kernel: fp32 scores, exp softmax, fp32 P.V.
  staircase        the input builder, and STAIRCASE / SMALL_STAIRCASE / XATTN_STAIRCASE: the cases the GPU tests run and
                   tests/test_attn_ref_host.py gates."""
import math

import torch

FA_LAZY = 8.0   # csrc/wd_attn.hip: log2 headroom of the running maximum
LOG2E = 1.44269504088896340736


def heads_of(t, B, n, H, d):
    """[B * n][H * d] -> [B][H][n][d]"""
    return t.reshape(B, n, H, d).permute(0, 2, 1, 3)


def rows_of(t):
    """[B][H][n][d] -> [B * n][H * d]"""
    B, H, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * n, H * d)


def attention_fp64(q, k, v, B, H, nq, nk, d, scale):
    """q [B * nq][H * d], k / v [B * nk][H * d] (any float type) -> [B * nq][H * d] fp64."""
    qh, kh, vh = heads_of(q.double(), B, nq, H, d), heads_of(k.double(), B, nk, H, d), heads_of(v.double(), B, nk, H, d)
    att = torch.softmax(qh @ kh.transpose(-1, -2) * float(scale), -1)
    return rows_of(att @ vh)


def logits_fp64(q, k, B, H, nq, nk, d, scale):
    """The logits in nats [B][H][nq][nk] (fp64): their span is what a staircase case is about."""
    return heads_of(q.double(), B, nq, H, d) @ heads_of(k.double(), B, nk, H, d).transpose(-1, -2) * float(scale)


def _split(x):
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def _mm3(a, b):
    """a @ b as the MFMA kernels form it: both operands split-bf16, and per 16-deep step of the reduction index three products
    - lo.hi, hi.lo, hi.hi, in the kernels' order - each added to the fp32 accumulator with one rounding (the 16 products of a
    step are exact in fp32 and summed here without further rounding: the hardware's own order inside a step is not modelled)."""
    ah, al = (t.double() for t in _split(a))
    bh, bl = (t.double() for t in _split(b))
    acc = torch.zeros(a.shape[:-1] + b.shape[-1:], dtype=torch.float32)
    for c in range(0, a.shape[-1], 16):
        e = slice(c, c + 16)
        for x, y in ((al, bh), (ah, bl), (ah, bh)):
            acc = (acc.double() + x[..., e] @ y[..., e, :]).float()
    return acc


def emulate_mfma(q, k, v, B, H, nq, nk, d, scale, ksplit=None, force_alpha_one=False, force_merge_one=False, stats=None):
    """attn_mfma_kernel's arithmetic on the host -> [B * nq][H * d] fp32.  ksplit None: as wd_attention dispatches (nq <= 64).
    stats: a dict that receives 'rescales' (rescales with a live accumulator, summed over the 32-query wave groups) and
    'max_exp2' (the largest exponential argument, log2 units: > 0 when the lazy maximum was exceeded within the headroom)."""
    ksplit = nq <= 64 if ksplit is None else ksplit
    f32 = torch.float32
    sc = torch.tensor(float(scale), dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    qs = heads_of(q.float(), B, nq, H, d) * sc                                  # [B][H][nq][d]
    kh, vh = heads_of(k.float(), B, nk, H, d), heads_of(v.float(), B, nk, H, d)
    s_all = _mm3(qs, kh.transpose(-1, -2).contiguous())                          # [B][H][nq][nk] fp32, log2 units
    ngrp = 2 if ksplit else 1
    wave = torch.arange(nq) // 32                                                # the 32 queries of a wave rescale together
    nwave = int(wave.max()) + 1
    state = []
    live, max_arg = 0, -1e30
    for grp in range(ngrp):
        m = torch.full((B, H, nq), -1e30, dtype=f32)
        lsum = torch.zeros(B, H, nq, dtype=f32)
        o = torch.zeros(B, H, nq, d, dtype=f32)
        for k0 in range(0, nk, 32):
            if ksplit and (k0 // 32) % 2 != grp:
                continue
            s = s_all[..., k0:k0 + 32]
            bm = s.max(-1).values
            fire = bm > m + FA_LAZY                                              # [B][H][nq]
            pad = torch.zeros(B, H, nwave * 32, dtype=torch.bool)
            pad[..., :nq] = fire
            any_fire = pad.view(B, H, nwave, 32).any(-1)[..., wave]              # __any over the wave
            m_new = torch.where(any_fire, torch.maximum(m, bm), m)
            alpha = torch.exp2(m - m_new)
            first = m < -1e29
            live += int((any_fire & ~first)[..., ::32].sum())
            if force_alpha_one:
                alpha = torch.where(first, alpha, torch.ones_like(alpha))
            m = m_new
            lsum = lsum * alpha
            o = o * alpha[..., None]
            arg = s - m[..., None]
            max_arg = max(max_arg, float(arg.max()))
            p = torch.exp2(arg)
            lsum = lsum + p.sum(-1)
            o = o + _mm3(p, vh[..., k0:k0 + 32, :])
        state.append((m, lsum, o))
    m, lsum, o = state[0]
    if ksplit:
        m1, l1, o1 = state[1]                                                    # (idle when nk <= 32: m1 = -1e30, l1 = 0)
        mt = torch.maximum(m, m1)
        a0, a1 = torch.exp2(m - mt), torch.exp2(m1 - mt)
        if force_merge_one:  # the second bug a staircase shows: the two key groups' states added as if their maxima were equal
            a0, a1 = torch.ones_like(a0), torch.ones_like(a1)
        lsum = lsum * a0 + l1 * a1
        o = o * a0[..., None] + o1 * a1[..., None]
    if stats is not None:
        stats.update(rescales=live, max_exp2=max_arg)
    return rows_of(o * (1.0 / lsum)[..., None])


def emulate_fp32(q, k, v, B, H, nq, nk, d, scale):
    """attn_kernel / attn_small_kernel's arithmetic class: a chain of d fused multiply-adds per score and of nk per output element
    (one rounding each, in the kernels' order), fp32 throughout, the maximum subtracted before exp."""
    qh, kh, vh = (heads_of(t.double(), B, n, H, d) for t, n in ((q, nq), (k, nk), (v, nk)))
    s = torch.zeros(B, H, nq, nk, dtype=torch.float32)
    for c in range(d):
        s = (s.double() + qh[..., :, None, c] * kh[..., None, :, c]).float()
    s = s * torch.tensor(float(scale), dtype=torch.float32)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    p = p * (1.0 / p.sum(-1, keepdim=True))
    o = torch.zeros(B, H, nq, d, dtype=torch.float32)
    for j in range(nk):
        o = (o.double() + p[..., :, j, None].double() * vh[..., None, j, :]).float()
    return rows_of(o)


def staircase(B, H, nq, nk, d, scale, step, period, descending=False, c=4.0, seed=0):
    """(q, k, v, off): 0.5 * randn operands whose logits carry a staircase.  q[:, h*d] = c for every head and
    k[j, h*d] = bf16(off_j / (c * scale)): the hi plane of that key column holds the value, its lo plane is zero, so every logit
    of key j gains the same off_j' = c * scale * k[j, h*d] nats (off_j up to the bf16 rounding of the column).  off_j = step *
    (j // period) ascending - the maximum moves at every stair - or, descending, step * ((nk - 1 - j) // period): the maximum
    sits in the first block and never moves.  off: [nk] nats as built."""
    g = torch.Generator().manual_seed(1000 * seed + nq + nk + d)
    inner = H * d
    q = torch.randn(B * nq, inner, generator=g) * 0.5
    k = torch.randn(B * nk, inner, generator=g) * 0.5
    v = torch.randn(B * nk, inner, generator=g) * 0.5
    j = torch.arange(nk)
    off = float(step) * ((nk - 1 - j) // period if descending else j // period).double()
    col = (off / (c * float(scale))).float().to(torch.bfloat16).float()
    q[:, ::d] = c
    k.view(B, nk, H, d)[:, :, :, 0] = col[None, :, None]
    return q, k, v, col.double() * c * float(scale)


def _layer_norm(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def xattn_operands(B, hw, c, heads, L, seed=0, step=0, period=1, cq=4.0):
    """Operands of one folded cross-attention, as tests/test_gpu_kernels.py draws them: x, k, v, wq, wo, bo and the two LayerNorms
    (ga, be: before the attention; ga2, be2: the one that follows).  step > 0: a staircase of step * (j // period) nats over the
    keys.  The query is to_q(LN(x)), so the constant query column of staircase() is made from the LayerNorm itself: ga[0] = 0 and
    be[0] = 1 make LN(x)[:, 0] = 1 exactly, row h*d of wq is cq at column 0 and zero elsewhere, k[j, h*d] carries the stairs."""
    g = torch.Generator().manual_seed(1000 * seed + hw + c + L)
    d = c // heads
    o = dict(x=torch.randn(B * hw, c, generator=g) * 1.5 + 0.3, k=torch.randn(B * L, c, generator=g) * 0.5,
             v=torch.randn(B * L, c, generator=g) * 0.5, wq=torch.randn(c, c, generator=g) / c ** 0.5,
             wo=torch.randn(c, c, generator=g) / c ** 0.5, bo=torch.randn(c, generator=g) * 0.1)
    for i, n in enumerate(("ga", "be", "ga2", "be2")):
        o[n] = torch.randn(c, generator=g) * 0.2 + (1.0 if i % 2 == 0 else 0.0)
    if step:
        scale = d ** -0.5
        off = float(step) * (torch.arange(L) // period).double()
        col = (off / (cq * scale)).float().to(torch.bfloat16).float()
        o["ga"][0], o["be"][0] = 0.0, 1.0
        o["wq"][::d] = 0.0
        o["wq"][::d, 0] = cq
        o["k"].view(B, L, heads, d)[:, :, :, 0] = col[None, :, None]
    return o


def xattn_fp64(o, B, hw, c, heads, L, eps=1e-5):
    """(mq, mo, out, ln): the folded matrices [B][heads * L][c], out = x + to_out(attention(to_q(LN(x)), K, V)) and the LayerNorm
    that follows (unet.py:164-279,337-345), fp64."""
    d = c // heads
    scale = d ** -0.5
    t = {n: a.double() for n, a in o.items()}
    kh, vh = heads_of(t["k"], B, L, heads, d), heads_of(t["v"], B, L, heads, d)            # [B][h][L][d]
    wq_h, wo_h = t["wq"].view(heads, d, c), t["wo"].view(c, heads, d)
    mq = scale * torch.einsum("bhjc,hcn->bhjn", kh, wq_h).reshape(B, heads * L, c)
    mo = torch.einsum("bhjc,nhc->bhjn", vh, wo_h).reshape(B, heads * L, c)
    n1 = _layer_norm(t["x"], t["ga"], t["be"], eps).view(B, hw, c)
    s = torch.einsum("btn,bkn->btk", n1, mq).view(B, hw, heads, L)
    p = torch.softmax(s, -1).reshape(B, hw, heads * L)
    out = (torch.einsum("btk,bkn->btn", p, mo) + t["bo"]).reshape(B * hw, c) + t["x"]
    return mq, mo, out, _layer_norm(out, t["ga2"], t["be2"], eps)


def emulate_xattn16(o, B, hw, c, heads, L, eps=1e-5):
    """xattn16_kernel's arithmetic class: fp32 fold and LayerNorm, split-bf16 products for the scores and the output, fp32 softmax."""
    d = c // heads
    scale = torch.tensor(d ** -0.5, dtype=torch.float32)
    t = {n: a.float() for n, a in o.items()}
    kh, vh = heads_of(t["k"], B, L, heads, d), heads_of(t["v"], B, L, heads, d)
    mq = (torch.einsum("bhjc,hcn->bhjn", kh, t["wq"].view(heads, d, c)) * scale).reshape(B, heads * L, c)
    mo = torch.einsum("bhjc,nhc->bhjn", vh, t["wo"].view(c, heads, d)).reshape(B, heads * L, c)
    n1 = _layer_norm(t["x"], t["ga"], t["be"], eps).view(B, hw, c)
    s = _mm3(n1, mq.transpose(-1, -2).contiguous()).view(B, hw, heads, L)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    p = (p * (1.0 / p.sum(-1, keepdim=True))).reshape(B, hw, heads * L)
    return (_mm3(p, mo) + t["bo"]).reshape(B * hw, c) + t["x"]


def _sc(d):
    return d ** -0.5


# (B, H, nq, nk, d, scale, step, period, descending): attn_mfma_kernel in both forms (nq <= 64: KSPLIT), wd_attention_packed on the
# same operands, and attn_kernel through WDIFF_ATTN_GENERIC.  step 7 nats = 10.1 log2 units > FA_LAZY: the rescale fires with a live
# accumulator at every stair; 3 and 4 nats stay under it: exponentials above 1, a rescale every third / second stair.  No period
# but the last is a multiple of 32: stairs fall inside sub-blocks as well as between them.
STAIRCASE = [
    (2, 2, 70, 200, 80, _sc(80), 7, 48, False),    # 128-query form, KS = 5
    (2, 2, 70, 200, 80, _sc(80), 7, 48, True),     # ... descending: the maximum never moves
    (2, 3, 40, 200, 96, _sc(96), 7, 48, False),    # KSPLIT, KS = 6: the groups' maxima differ at the merge
    (2, 4, 64, 130, 16, _sc(16), 7, 24, False),    # KSPLIT, KS = 1, the odd group one block short
    (2, 4, 64, 130, 16, _sc(16), 7, 20, True),     # KSPLIT descending: the odd group's maximum one stair below the even group's
    (1, 2, 129, 779, 80, _sc(80), 4, 100, False),  # 128-query form, the product's context length, exponentials up to 2^5.8
    (1, 2, 129, 300, 64, _sc(64), 3, 20, False),   # 128-query form, KS = 4, a rescale every third stair
    (2, 2, 33, 160, 32, _sc(32), 7, 32, False),    # KSPLIT, KS = 2, period = the sub-block: each group sees every second stair
    (2, 1, 100, 96, 48, _sc(48), 7, 20, False),    # 128-query form, KS = 3
]
# ... of which attn_kernel (WDIFF_ATTN_GENERIC) runs those on which the all-fp32 class meets the host gate as well: its scores are
# chains of d fp32 FMAs at the magnitude of the largest logit, 1.2e-5 and 1.6e-5 from fp64 on the d = 64 / step 3 and d = 96 cases
GENERIC_STAIRCASE = [STAIRCASE[i] for i in (0, 1, 3, 4, 7, 8)]
# (B, H, nq, nk, d, scale, descending): attn_small_kernel<10> / <0>, a 7-nat stair at every key (period 1)
SMALL_STAIRCASE = [(2, 4, 70, 10, 80, _sc(80), False), (2, 3, 90, 16, 16, _sc(16), False), (2, 4, 70, 10, 80, _sc(80), True)]
# (B, hw, c, heads, L, step, period): wd_xattn_fold + its consumers, the stairs put into K before the fold
XATTN_STAIRCASE = [(2, 70, 320, 4, 10, 7, 5), (2, 33, 64, 4, 10, 7, 1)]


def span_nats(q, k, B, H, nq, nk, d, scale):
    lg = logits_fp64(q, k, B, H, nq, nk, d, scale)
    return float((lg.max(-1).values - lg.min(-1).values).max())


def max_rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


assert math.isclose(7 * LOG2E, 10.099, abs_tol=1e-3)  # the step that clears FA_LAZY
