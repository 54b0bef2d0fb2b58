"""Specifications for the PHOSCnet recogniser (worddiffusion_amd/phoscnet.py, csrc/wd_phoscnet.hip), written from
include/wdiff_hip.h and the published network layout, not from the kernels:

  * the five streaming kernels in numpy, every operation rounded to fp32 in the header's order (the kernel tests compare the
    planes / the resize bit for bit with these);
  * the network as a plain-torch float64 function of a ``state_dict`` (thirteen 3x3 convolutions + ReLU, two 2x2 max-pools,
    temporal pyramid max pooling over [1, 2, 5], two three-layer MLP heads), in the style of ``oracle/``.
"""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
CONV_KEYS = (0, 2, 5, 7, 10, 12, 14, 16, 18, 20, 22, 24, 26)   # indices of the convolutions in ``conv``
POOL_BEFORE = (5, 10)                                          # a 2x2 / 2 max-pool stands before these
CONV_CH = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 256), (256, 256), (256, 256),
           (256, 512), (512, 512), (512, 512))
LEVELS = (1, 2, 5)
N_FEAT, N_PHOS, N_PHOC = 4096, 165, 604
GAIN = math.sqrt(2.0)  # every >= 2-D weight of the golden model is the synthetic one times this (keeps the ReLU stack's scale)


def state_dict_shapes():
    out = []
    for k, (ci, co) in zip(CONV_KEYS, CONV_CH):
        out += [(f"conv.{k}.weight", (co, ci, 3, 3)), (f"conv.{k}.bias", (co,))]
    for head, n in (("phos", N_PHOS), ("phoc", N_PHOC)):
        for k, (i, o) in zip((0, 3, 6), ((N_FEAT, 4096), (4096, 4096), (4096, n))):
            out += [(f"{head}.{k}.weight", (o, i)), (f"{head}.{k}.bias", (o,))]
    return out


def golden_state_dict(seed=7):
    """The weights of tests/golden/phoscnet.npz: ``synthetic_tensor(key, shape, seed)``, every >= 2-D one times sqrt(2) in fp32."""
    from worddiffusion_amd.synthetic import synthetic_tensor
    sd = {}
    for k, s in state_dict_shapes():
        t = torch.from_numpy(synthetic_tensor(k, s, seed))
        sd[k] = t * torch.tensor(GAIN, dtype=torch.float32) if len(s) >= 2 else t
    return sd


def weights_crc(sd) -> int:
    """CRC-32 of the fp32 bytes of every entry, in ``state_dict_shapes`` order."""
    crc = 0
    for k, _ in state_dict_shapes():
        crc = zlib.crc32(np.ascontiguousarray(sd[k].detach().cpu().numpy().astype(np.float32)).tobytes(), crc)
    return crc & 0xFFFFFFFF


# ---- the network in float64 ------------------------------------------------------------------------------------------------
def tpp_torch(x, levels=LEVELS):
    """Temporal pyramid max pooling of an NCHW map: per level L, k = ceil(w / L) columns per bin, k * L - w zero columns of which
    the smaller half goes left, the maximum over the whole height and each run of k columns; flattened channel-major."""
    n, _, h, w = x.shape
    out = []
    for L in levels:
        k = -(-w // L)
        pad = k * L - w
        xp = F.pad(x, [pad // 2, pad - pad // 2], value=0.0)
        out.append(F.max_pool2d(xp, (h, k), stride=(h, k)).reshape(n, -1))
    return torch.cat(out, 1)


def network_f64(sd, x, want_stats=False):
    """-> dict(features, phos_logits, phoc_logits, phos, phoc) in float64 (+ ``conv_stats``: (mean, abs-max) per convolution)."""
    p = {k: v.detach().double().cpu() for k, v in sd.items()}
    h = x.detach().double().cpu()
    stats = []
    for j, k in enumerate(CONV_KEYS):
        if j:
            h = torch.relu(h)
        if k in POOL_BEFORE:
            h = F.max_pool2d(h, (2, 2), stride=2)
        h = F.conv2d(h, p[f"conv.{k}.weight"], p[f"conv.{k}.bias"], padding=1)
        stats.append((float(h.mean()), float(h.abs().max())))
    feat = tpp_torch(torch.relu(h))
    out = {"features": feat}
    for head in ("phos", "phoc"):
        y = feat
        for k in (0, 3, 6):
            if k:
                y = torch.relu(y)
            y = F.linear(y, p[f"{head}.{k}.weight"], p[f"{head}.{k}.bias"])
        out[head + "_logits"] = y
    out["phos"] = torch.relu(out["phos_logits"])
    out["phoc"] = torch.sigmoid(out["phoc_logits"])
    if want_stats:
        out["conv_stats"] = stats
    return out


# ---- the kernels in fp32 numpy ---------------------------------------------------------------------------------------------
def split_np(v):
    """(hi, lo) bit patterns (uint16) of the split-bf16 planes of fp32 ``v``: hi = bf16(v) round to nearest even, lo = bf16(v - hi)."""
    def bf16(a):
        u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
        return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)
    v = np.asarray(v, dtype=F32)
    hi = bf16(v)
    hif = (hi.astype(np.uint32) << 16).view(F32)
    return hi, bf16((v - hif).astype(F32))


def relu_pool_np(x, batch, h, w, pool):
    """x fp32 [batch*h*w][c] -> fp32 [batch*h'*w'][c]: max over the 2x2 window (pool 2, floor), then v > 0 ? v : +0."""
    c = x.shape[1]
    m = np.asarray(x, dtype=F32).reshape(batch, h, w, c)
    if pool == 2:
        ho, wo = h // 2, w // 2
        m = m[:, :2 * ho, :2 * wo].reshape(batch, ho, 2, wo, 2, c).max(axis=(2, 4))
    out = np.where(m > 0, m, F32(0.0)).astype(F32)
    return out.reshape(-1, c)


def tpp_np(x, batch, h, w, levels=LEVELS):
    """x fp32 [batch*h*w][c] -> fp32 [batch][c * sum(levels)], column = offset(level) + ch * L + bin."""
    c = x.shape[1]
    m = np.asarray(x, dtype=F32).reshape(batch, h, w, c)
    out = np.zeros((batch, c * sum(levels)), dtype=F32)
    off = 0
    for L in levels:
        k = -(-w // L)
        left = (k * L - w) // 2
        for j in range(L):
            x0, x1 = max(j * k - left, 0), min((j + 1) * k - left, w)
            v = np.zeros((batch, c), dtype=F32)
            if x1 > x0:
                win = m[:, :, x0:x1].reshape(batch, -1, c).max(axis=1)
                v = np.where(win > 0, win, F32(0.0)).astype(F32)
            out[:, off + np.arange(c) * L + j] = v
        off += c * L
    return out


def _taps(n_dst, n_src):
    n = np.maximum((2 * np.arange(n_dst, dtype=np.int64) + 1) * n_src - n_dst, 0)
    i0 = n // (2 * n_dst)
    i1 = np.minimum(i0 + 1, n_src - 1)
    return i0, i1, ((n - i0 * 2 * n_dst).astype(F32) / F32(2 * n_dst)).astype(F32)


def resize_np(x, h, w, bgr=False):
    """x fp32 [B][C][hs][ws] -> [B][C][h][w], the header's operation order, every operation rounded to fp32."""
    x = np.asarray(x, dtype=F32)
    if bgr:
        x = x[:, ::-1]
    y0, y1, ly = _taps(h, x.shape[2])
    x0, x1, lx = _taps(w, x.shape[3])
    wx, wy = (F32(1.0) - lx).astype(F32), (F32(1.0) - ly).astype(F32)
    r0, r1 = x[:, :, y0], x[:, :, y1]
    top = ((wx * r0[..., x0]).astype(F32) + (lx * r0[..., x1]).astype(F32)).astype(F32)
    bot = ((wx * r1[..., x0]).astype(F32) + (lx * r1[..., x1]).astype(F32)).astype(F32)
    return ((wy[:, None] * top).astype(F32) + (ly[:, None] * bot).astype(F32)).astype(F32)


def finish_np(phos, phoc):
    """relu(phos) | sigmoid(phoc); the sigmoid in float64 (the kernel is held to 1e-6 of it)."""
    phos = np.asarray(phos, dtype=F32)
    a = np.where(phos > 0, phos, F32(0.0)).astype(np.float64)
    return np.concatenate([a, 1.0 / (1.0 + np.exp(-np.asarray(phoc, dtype=np.float64)))], axis=1)


def score_np(pred, table, table_norm=None, target=None):
    """fp32 cosine scores [B][V] = dot / max(|x| |y|, 1e-8) (products and sums in fp32, lane-strided like the kernel), the FIRST
    maximum per row and the score of ``target`` (NaN outside [0, V))."""
    pred, table = np.asarray(pred, dtype=F32), np.asarray(table, dtype=F32)

    def dot(a, b):  # 64 strided partial sums, then their sum
        ab = (a * b).astype(F32)
        d = ab.shape[-1]
        n = -(-d // 64) * 64
        prod = np.zeros(ab.shape[:-1] + (n,), dtype=F32)
        prod[..., :d] = ab
        return prod.reshape(ab.shape[:-1] + (-1, 64)).sum(axis=-2, dtype=F32).sum(axis=-1, dtype=F32)
    xn = np.sqrt(dot(pred, pred)).astype(F32)
    yn = np.sqrt(dot(table, table)).astype(F32) if table_norm is None else np.asarray(table_norm, dtype=F32)
    dots = dot(pred[:, None, :], table[None, :, :])
    scores = (dots / np.maximum((xn[:, None] * yn[None, :]).astype(F32), F32(1e-8))).astype(F32)
    best = first_max(scores)
    tsc = None
    if target is not None:
        t = np.asarray(target)
        ok = (t >= 0) & (t < table.shape[0])
        tsc = np.where(ok, scores[np.arange(len(t)), np.where(ok, t, 0)], F32(np.nan)).astype(F32)
    return scores, best, scores[np.arange(len(best)), best], tsc


def first_max(scores):
    """The reference's loop (``if temp > mx``): the first index that holds the row maximum."""
    best = np.zeros(scores.shape[0], dtype=np.int32)
    for b, row in enumerate(np.asarray(scores)):
        mx, at = -np.inf, 0
        for j, s in enumerate(row):
            if s > mx:
                mx, at = s, j
        best[b] = at
    return best


def write_alphabet_csv(golden_dir, path, version="eng"):
    """The reference's shape-count table travels as data inside tests/golden/phosc.npz; written back in its csv form."""
    import os
    g = np.load(os.path.join(golden_dir, "phosc.npz"), allow_pickle=False)
    with open(path, "w") as f:
        for letter, row in zip(g[f"{version}:letters"], g[f"{version}:table"]):
            f.write(",".join([str(letter)] + [str(int(v)) for v in row]) + "\r\n")
    return path


def cosine_f64(pred, table):
    """float64 cosine [B][V] = dot / max(|x| |y|, 1e-8)."""
    p, t = torch.as_tensor(pred).double(), torch.as_tensor(table).double()
    return (p @ t.T) / torch.clamp(p.norm(dim=1)[:, None] * t.norm(dim=1)[None, :], min=1e-8)
