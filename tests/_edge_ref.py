"""The small kernels at the two ends of every forward, sampling step and training step (csrc/wd_misc.hip: the timestep and token
embeddings, im2col, the layout changes, the DDPM update, the noise fill, noise_images, the EMA, the timestep advance), restated
on the host from their specification in include/wdiff_hip.h and from nothing in the library, with the shapes they are tested at.
A test helper (not collected); tests/test_edge_ref_host.py holds it to the oracle and to plain torch.

Functions with a bit-for-bit promise are numpy fp32 in the kernel's operation order: numpy rounds every fp32 operation once and
fuses nothing, which is the rounding the kernels are held to (their translation unit compiles with contraction off).

    ddpm_update    a * (x - b * eps) + s * z,  z = 0 for t <= 1           (a, b, s = ca[t], cb[t], cs[t])
    guided_eps     torch.lerp(second, first, scale): ``first - (first - second) * (1 - scale)`` from |scale| = 0.5 on,
                   ``second + scale * (first - second)`` below - at the weights of GUIDE_SCALES, where the product is exact, so
                   that ATen's fused and the kernel's unfused form are one value (tests/test_gpu_interp.py)
    noise_images   sa[t_b] * x + sb[t_b] * eps
    ema_update     ema * fp32(beta) + fp32(1.0 - beta) * p,  1 - beta taken in double first
    nchw_to_tokens / tokens_to_nchw     the two permutations, [B][c][hw] <-> [B * hw][c]
    im2col3x3      [B * h * w][kpad], column tap * cin + ci, zero padding, zeros in columns 9 cin .. kpad
    embed_tokens   table[clamp(id)] + pe[r % seq_len], fp32
    advance        max(t + delta, 0)
    planes         ``_guard.split_planes``: hi = bf16(v), lo = bf16(v - hi)

Functions compared in float64 (the kernel calls cosf / sinf / expf, which promise no bits):

    timestep_embedding   cos | sin of the fp32 product fp32(t) * freqs
    emb_combine          silu(time[t] + label[clamp(y_b)]), or silu(time[t]) without a label; row t * B + b

Device draws are ``tests/_philox_ref.py`` under the key (seed, sample_offset + b, tag, e4) that tests/test_gpu_noise.py pins; that
file evaluates log, sqrt, sin and cos in float64, so a device draw is held to it within test_gpu_noise's bound DRAW_TOL * radius
and bit for bit only against another device evaluation of the same key (``draws``)."""
import functools

import numpy as np
import torch

from tests import _philox_ref as P

# grid_for() in csrc/wd_misc.hip caps a launch at 2048 blocks of 256 threads: a kernel with more work items than this takes a
# second pass of its grid-stride loop
GRID_CAP_ITEMS = 2048 * 256
BLOCK = 256
DRAW_TOL = 16.0 * 2.0 ** -24      # |z_dev - z_ref| <= DRAW_TOL * radius (derived in tests/test_gpu_noise.py)
GUIDE_SCALES = (3.0, 0.25)        # one weight on each branch of lerp; 1 - 3 = -2 and 0.25 are powers of two
EMA_BETAS = (0.995, 0.9999)
PLANE_BOUND = (2.0 ** -16, 1e-6)  # |got - ref| <= 2^-16 |ref| + 1e-6: two bf16 roundings (tests/test_gpu_interp.py)
TEMB_BOUND = 2e-5                 # absolute, |arg| up to 999 rad (tests/test_gpu_kernels.py)

f32 = np.float32


def _a(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def rand(shape, seed, scale=1.0):
    """Seeded fp32 normals, the inputs of every case."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------------------------------------ bit for bit
def ddpm_update(x, eps, ca, cb, cs, t, z=None):
    """x after one update at timestep t; x, eps, z fp32 of one shape (z may be None for t <= 1: it is not read)."""
    x, eps = _a(x).astype(f32), _a(eps).astype(f32)
    a, b, s = f32(_a(ca)[t]), f32(_a(cb)[t]), f32(_a(cs)[t])
    zz = np.zeros_like(x) if t <= 1 else _a(z).astype(f32)
    inner = (x - (b * eps).astype(f32)).astype(f32)
    return _t(((a * inner).astype(f32) + (s * zz).astype(f32)).astype(f32))


def guided_eps(first, second, scale):
    assert scale in GUIDE_SCALES, "lerp is stated only where its product is exact"
    return torch.lerp(second, first, scale)


def noise_images(x, eps, t, sa, sb):
    """x, eps fp32 [B][n]; t int64 [B]; the tables fp32."""
    x, eps, t = _a(x).astype(f32), _a(eps).astype(f32), _a(t)
    a, b = _a(sa).astype(f32)[t][:, None], _a(sb).astype(f32)[t][:, None]
    return _t(((a * x).astype(f32) + (b * eps).astype(f32)).astype(f32))


def ema_update(ema, p, beta):
    ema, p = _a(ema).astype(f32), _a(p).astype(f32)
    b, omb = f32(beta), f32(1.0 - float(beta))
    return _t(((ema * b).astype(f32) + (omb * p).astype(f32)).astype(f32))


def nchw_to_tokens(x):
    """[B][c][hw] -> [B * hw][c]."""
    x = _a(x)
    B, c, hw = x.shape
    out = np.empty((B * hw, c), dtype=x.dtype)
    for ch in range(c):
        out[:, ch] = x[:, ch, :].reshape(B * hw)
    return _t(out)


def tokens_to_nchw(tok, B):
    """[B * hw][c] -> [B][c][hw]."""
    tok = _a(tok)
    hw, c = tok.shape[0] // B, tok.shape[1]
    out = np.empty((B, c, hw), dtype=tok.dtype)
    for ch in range(c):
        out[:, ch, :] = tok[:, ch].reshape(B, hw)
    return _t(out)


def im2col3x3(x, kpad):
    """x [B][cin][h][w] -> fp32 [B * h * w][kpad]."""
    x = _a(x).astype(f32)
    B, cin, h, w = x.shape
    assert kpad >= 9 * cin
    xp = np.zeros((B, cin, h + 2, w + 2), dtype=f32)
    xp[:, :, 1:h + 1, 1:w + 1] = x
    out = np.zeros((B, h, w, kpad), dtype=f32)
    for tap in range(9):
        dy, dx = tap // 3, tap % 3
        for ci in range(cin):
            out[:, :, :, tap * cin + ci] = xp[:, ci, dy:dy + h, dx:dx + w]
    return _t(out.reshape(B * h * w, kpad))


def embed_tokens(ids, table, pe, seq_len):
    """ids [rows] of any integer type (clamped into the table), table fp32 [vocab][c], pe fp32 [>= seq_len][c] or None."""
    ids, table = _a(ids).astype(np.int64), _a(table).astype(f32)
    v = table[np.clip(ids, 0, table.shape[0] - 1)]
    if pe is not None:
        v = (v + _a(pe).astype(f32)[np.arange(ids.shape[0]) % seq_len]).astype(f32)
    return _t(v)


def advance(t, delta):
    return max(int(t) + int(delta), 0)


# ------------------------------------------------------------------------------------------------ float64
def temb_freqs(dim):
    """The caller's fp32 table exp(-ln(1e4) k / half), with the reference's op order (unet.py:96-116)."""
    half = dim // 2
    return torch.exp(-np.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)


def timestep_embedding(t, freqs):
    """float64 [batch][2 half]."""
    arg = (_a(t).astype(f32)[:, None] * _a(freqs).astype(f32)[None, :]).astype(f32).astype(np.float64)
    return _t(np.concatenate([np.cos(arg), np.sin(arg)], axis=1))


def emb_combine(time, label, y, B):
    """float64 [T * B][ted]; label None: no label term (y unused)."""
    time = _a(time).astype(np.float64)
    v = np.repeat(time[:, None, :], B, axis=1)
    if label is not None:
        label = _a(label).astype(np.float64)
        v = v + label[np.clip(_a(y).astype(np.int64), 0, label.shape[0] - 1)][None, :, :]
    return _t((v / (1.0 + np.exp(-v))).reshape(-1, time.shape[1]))


def within(got, ref, bound):
    """(ok, worst err / tol) of |got - ref| <= rel |ref| + abs, per element, in float64."""
    rel, ab = bound
    got, ref = got.double(), ref.double()
    ratio = (got - ref).abs() / (rel * ref.abs() + ab)
    return bool((ratio <= 1.0).all()), float(ratio.max())


# ------------------------------------------------------------------------------------------------ draws
@functools.lru_cache(maxsize=None)
def draws(batch, n_per_sample, seed, sample_offset, tag):
    """(z, r) float64 [batch][n_per_sample] of the specification, computed once per key and read-only."""
    z, r = P.randn(batch, n_per_sample, seed, sample_offset, tag, with_r=True)
    z.setflags(write=False)
    r.setflags(write=False)
    return z, r


def draws_within(got, ref):
    """Worst |got - z| / (DRAW_TOL * r) of device draws ``got`` against ref = (z, r); a draw of radius 0 must be 0."""
    z, r = ref
    got = _a(got).astype(np.float64).reshape(z.shape)
    zero = r == 0.0
    assert np.isfinite(got).all() and (got[zero] == 0.0).all()
    ratio = np.zeros_like(z)
    ratio[~zero] = np.abs(got - z)[~zero] / (DRAW_TOL * r[~zero])
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------ the cases
# Per kernel that walks its work items in a grid-stride loop: the smallest shapes at which it can go wrong.  ``big``: more items
# than GRID_CAP_ITEMS with a ragged tail (not a multiple of the block) and, where the items are grouped by sample, the second pass
# beginning INSIDE the last sample, so that the sample index and the index inside the sample are both taken mid-row there.
# The others: under one block, ragged, batch 1 and 3.
CASES = {
    "wd_ema_update": [dict(n=GRID_CAP_ITEMS + 1031), dict(n=1), dict(n=203)],
    "wd_ddpm_step": [dict(batch=5, n=4 * 104860), dict(batch=1, n=4), dict(batch=3, n=4 * 67)],
    "wd_ddpm_step_cfg": [dict(batch=5, n=4 * 104860), dict(batch=1, n=4), dict(batch=3, n=4 * 67)],
    "wd_randn": [dict(batch=5, n=4 * 104860), dict(batch=1, n=4), dict(batch=3, n=4 * 67)],
    "wd_noise_images": [dict(batch=3, n=174763), dict(batch=1, n=1), dict(batch=3, n=67)],  # n % 4 != 0: the scalar kernel
    # (kpad = 64 as in the product: with kpad = 256 every item count is a multiple of the block)
    "wd_im2col3x3": [dict(batch=9, cin=4, h=5, w=203, kpad=64), dict(batch=1, cin=1, h=1, w=1, kpad=32),
                     dict(batch=3, cin=4, h=1, w=1, kpad=64)],
    "wd_nchw_to_tokens": [dict(batch=9, c=4, hw=14564, ld=32), dict(batch=1, c=4, hw=5, ld=32), dict(batch=3, c=4, hw=21, ld=32)],
    "wd_tokens_to_nchw": [dict(batch=9, c=4, hw=14564, ld=32), dict(batch=1, c=4, hw=5, ld=32), dict(batch=3, c=4, hw=21, ld=32)],
    "wd_embed_tokens": [dict(rows=32773, seq_len=10, vocab=53, c=64), dict(rows=1, seq_len=10, vocab=53, c=64),
                        dict(rows=13, seq_len=5, vocab=7, c=8)],
    "wd_emb_combine": [dict(T=1171, B=7, ted=256, ncls=339), dict(T=1, B=1, ted=64, ncls=3), dict(T=5, B=3, ted=64, ncls=11)],
}


def items(kernel, c):
    """(work items of the launch, items per sample or 0): how the kernel counts them."""
    if kernel == "wd_ema_update":
        return c["n"], 0
    if kernel in ("wd_ddpm_step", "wd_ddpm_step_cfg", "wd_randn"):
        return c["batch"] * (c["n"] // 4), c["n"] // 4           # one float4 per item
    if kernel == "wd_noise_images":
        return c["batch"] * c["n"], c["n"]
    if kernel == "wd_im2col3x3":
        return c["batch"] * c["h"] * c["w"] * c["kpad"], c["h"] * c["w"] * c["kpad"]
    if kernel in ("wd_nchw_to_tokens", "wd_tokens_to_nchw"):
        return c["batch"] * c["c"] * c["hw"], c["c"] * c["hw"]
    if kernel == "wd_embed_tokens":
        return c["rows"] * (c["c"] // 4), 0                      # four columns per item
    if kernel == "wd_emb_combine":
        return c["T"] * c["B"] * (c["ted"] // 4), 0
    raise KeyError(kernel)


def is_big(kernel, c):
    return items(kernel, c)[0] > GRID_CAP_ITEMS


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


def params(kernel):
    """The argvalues and ids of pytest.mark.parametrize."""
    return dict(argvalues=CASES[kernel], ids=[case_id(c) for c in CASES[kernel]])


# wd_timestep_embedding (one thread per (sample, frequency), no stride loop): t spans 0 .. 999; 1000 rows = the table form
TEMB_T = {"ragged": [0, 1, 2, 17, 500, 998, 999], "table": list(range(1000))}
TEMB_DIMS = (320, 64)
# wd_advance_timestep (one block of 256): batch around the block, delta -1 down to the clamp, one skip delta
ADVANCE_BATCH = (1, 256, 257, 1000)
ADVANCE_STEPS = ((2, -1), (1, -1), (0, -1), (640, -7), (3, -7))


def step_tables(T=1000):
    """(ca, cb, cs, sqrt_ah, sqrt_1m_ah): the fp32 tables the callers tabulate, with the reference's op order (train.py:180-236)."""
    beta = torch.linspace(1e-4, 0.02, T)
    alpha = 1.0 - beta
    ah = torch.cumprod(alpha, dim=0)
    return 1 / torch.sqrt(alpha), (1 - alpha) / torch.sqrt(1 - ah), torch.sqrt(beta), torch.sqrt(ah), torch.sqrt(1 - ah)
