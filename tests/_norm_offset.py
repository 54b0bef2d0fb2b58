"""Normalisation on inputs whose group mean is far from zero: the input builder, the bound, the references and a numpy emulator
of the GroupNorm statistics producers, shared by test_norm_offset_host.py (CPU) and test_gpu_norm_offset.py (GPU).

Why: every consumer of GroupNorm statistics forms var = sumsq / n - mean^2 in double.  That difference multiplies the relative
error of sumsq by (mean / std)^2 + 1, so a producer that accumulates v * v in fp32 anywhere (error 2^-24 of the running sum per
add) loses (mean / std)^2 * 6e-8 of the variance: 2.4e-4 at mean / std = 64.  nn.GroupNorm in fp32 torch has no such term.

The bound of every check here is bound(path_tol, ref_err): the tolerance the path's ordinary test already uses, or four times the
error of the reference's own fp32 arithmetic against fp64 on the same input, whichever is larger.  It never comes from the
kernel's output.  test_norm_offset_host.py shows that ref_err <= path_tol / 2 everywhere except r = 256."""
import numpy as np
import torch
import torch.nn.functional as F

from tests._common import max_rel

R = (0, 4, 16, 64, 256)      # the ladder of mean / std
KINDS = ("same", "neg", "mixed")
TOL_PLANES = 3e-5            # max_rel of GroupNorm / LayerNorm operand planes (test_groupnorm_silu_planes, test_layernorm_and_split)
TOL_STATS = 1e-5             # max_rel of the statistics (test_gemm_fused_groupnorm_statistics)
GN_TOK = 32                  # tokens per chunk of wd_gn_stats (wd_gn_nchunk)

# (B, hw, c, cpg) of every GroupNorm the GPU file runs: the wd_gn_stats shapes, then the output shapes of the fused producers
GN_STATS_SHAPES = [(2, 64, 320, 10), (1, 100, 64, 2), (2, 256, 640, 20), (1, 32, 1280, 40)]
GN_FOLD_SHAPE = (2, 160, 64, 2)
GN_PRODUCER_SHAPES = [(5, 64, 64, 2), (2, 128, 640, 20), (3, 256, 320, 10), (4, 64, 320, 10), (5, 64, 320, 20), (2, 64, 64, 2),
                      (3, 35, 64, 2), (2, 64, 80, 10)]
LN_SHAPES = [(37, 64), (5, 1280), (64, 64)]


def rk_cases():
    """(r, kind) of a GPU case: the whole ladder for "same"; "neg" and "mixed" at r = 64 only."""
    return [(r, "same") for r in R] + [(64, "neg"), (64, "mixed")]


def bound(path_tol, ref_err):
    return max(path_tol, 4.0 * ref_err)


def group_means(B, ng, r, kind, seed):
    """[B, ng] means in units of the group's std."""
    if kind == "same":
        return torch.full((B, ng), float(r), dtype=torch.float64)
    if kind == "neg":
        return torch.full((B, ng), -float(r), dtype=torch.float64)
    assert kind == "mixed"
    g = torch.Generator().manual_seed(seed * 7919 + 13)
    m = (torch.randint(0, 3, (B, ng), generator=g).double() - 1.0) * r  # -r, 0 or +r per (sample, group)
    m.view(-1)[:3] = torch.tensor([r, 0.0, -r], dtype=torch.float64)[: m.numel()]  # (all three occur)
    return m


def offset_input(rows, c, cpg, r, kind, seed):
    """fp32 [B * hw, c] whose every (sample, group) has std 1 and mean +r ("same"), -r ("neg"), or one of +r / 0 / -r drawn per
    (sample, group) ("mixed": a mean taken from the wrong group or sample shows).  rows = (B, hw), or B * hw for one sample."""
    B, hw = rows if isinstance(rows, tuple) else (1, rows)
    ng = c // cpg
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, hw, ng, cpg, generator=g, dtype=torch.float64)
    z = (z - z.mean(dim=(1, 3), keepdim=True)) / z.std(dim=(1, 3), keepdim=True, unbiased=False)
    z = z + group_means(B, ng, r, kind, seed)[:, None, :, None]
    return z.reshape(B * hw, c).float()


def offset_rows(rows, c, r, seed):
    """LayerNorm input: fp32 [rows, c], every row std 1 and mean +r or -r (alternating)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, c, generator=g, dtype=torch.float64)
    z = (z - z.mean(1, keepdim=True)) / z.std(1, keepdim=True, unbiased=False)
    sign = torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0).double()
    return (z + (sign * r)[:, None]).float()


def affine(c, seed):
    g = torch.Generator().manual_seed(seed + 101)
    return torch.randn(c, generator=g), torch.randn(c, generator=g)


def gn_ref(x, B, hw, cpg, gamma, beta, eps, silu, dtype=torch.float64):
    """F.group_norm (+ SiLU) of token-major x [B * hw, c] in `dtype` on the CPU -> [B * hw, c]."""
    c = x.shape[1]
    v = x.cpu().to(dtype).reshape(B, hw, c).permute(0, 2, 1)
    y = F.group_norm(v, c // cpg, gamma.cpu().to(dtype), beta.cpu().to(dtype), eps)
    if silu:
        y = F.silu(y)
    return y.permute(0, 2, 1).reshape(B * hw, c)


def gn_ref_err(x, B, hw, cpg, gamma, beta, eps, silu):
    """(fp64 reference, max_rel of the fp32 reference against it)."""
    ref = gn_ref(x, B, hw, cpg, gamma, beta, eps, silu)
    return ref, max_rel(gn_ref(x, B, hw, cpg, gamma, beta, eps, silu, torch.float32), ref)


def ln_ref_err(x, gamma, beta, eps):
    ref = F.layer_norm(x.cpu().double(), (x.shape[1],), gamma.cpu().double(), beta.cpu().double(), eps)
    r32 = F.layer_norm(x.cpu().float(), (x.shape[1],), gamma.cpu().float(), beta.cpu().float(), eps)
    return ref, max_rel(r32, ref)


def var_err(part, x, B, hw, cpg, part_cpg=None):
    """max relative error of the variance recomputed in double from part [B, nchunk, c / part_cpg, 2] against the fp64 variance of
    the same values x [B * hw, c] (groups of cpg channels).  For diagnosis: the planes bound is what is asserted."""
    c = x.shape[1]
    part_cpg = part_cpg or cpg
    p = part.cpu().double().sum(1).reshape(B, c // cpg, cpg // part_cpg, 2).sum(2)
    n = hw * cpg
    mean = p[..., 0] / n
    var = p[..., 1] / n - mean * mean
    ref = x.cpu().double().reshape(B, hw, c // cpg, cpg).var(dim=(1, 3), unbiased=False)
    return float(((var - ref).abs() / ref).max())


# ---- numpy emulator of the statistics producers + wd_gn_apply's arithmetic (no GPU; the plane split is not modelled)
def emulate_gn(x, B, hw, cpg, gamma, beta, eps, exact):
    """GroupNorm of x [B * hw, c] (fp32) the way the kernels compute it -> float64 array of the fp32 results.

    exact=False: the statistics as wd_gn_stats accumulated them before the producers went to double - per chunk of 32 tokens
    each thread adds v and v * v over its 16 tokens (every other token) in fp32, and only the sums over the group's channels, the
    two token halves and the chunks are in double.
    exact=True: plain sums and sums of squares in double (what the partials guarantee now).
    Both: var = sumsq / n - mean^2 in double, mean and 1 / sqrt(var + eps) rounded to fp32, y = v * sc + sh with
    sc = rstd * gamma, sh = beta - mean * sc in fp32 (gn_apply_kernel)."""
    x = np.asarray(x, dtype=np.float32)
    c = x.shape[1]
    ng = c // cpg
    v = x.reshape(B, hw, c)
    if exact:
        d = v.astype(np.float64)
        s, q = d.sum(1), (d * d).sum(1)  # [B, c]
    else:
        s = np.zeros((B, c), np.float64)
        q = np.zeros((B, c), np.float64)
        for t0 in range(0, hw, GN_TOK):
            for y in range(2):
                ss = np.zeros((B, c), np.float32)
                qq = np.zeros((B, c), np.float32)
                for t in range(t0 + y, min(hw, t0 + GN_TOK), 2):
                    ss = ss + v[:, t]
                    qq = qq + v[:, t] * v[:, t]
                s += ss
                q += qq
    s, q = s.reshape(B, ng, cpg).sum(2), q.reshape(B, ng, cpg).sum(2)
    n = float(hw * cpg)
    mean = s / n
    var = np.maximum(q / n - mean * mean, 0.0)
    mean32 = np.repeat(mean.astype(np.float32), cpg, 1)[:, None, :]
    rstd32 = np.repeat((1.0 / np.sqrt(var + eps)).astype(np.float32), cpg, 1)[:, None, :]
    ga, be = np.asarray(gamma, np.float32), np.asarray(beta, np.float32)
    sc = rstd32 * ga
    sh = be - mean32 * sc
    return (v * sc + sh).astype(np.float32).reshape(B * hw, c).astype(np.float64)


# ---- the model-level case: SMALL base UNet with every GroupNorm's input pushed 16 std away from zero
MODEL_R = 16.0


GN_FEEDERS = ("in_layers.2.bias", "out_layers.3.bias", "skip_connection.bias", "input_blocks.0.0.bias", ".op.bias", ".conv.bias",
              "proj_out.bias")  # the convolutions whose output (alone, or summed with a residual / embedding row) a GroupNorm reads


def offset_model_state(U, cfg, sd, variant, inp, r=MODEL_R):
    """A copy of the fp32 state_dict `sd` with + r * (std of that convolution's output at the test input `inp`, measured on the
    unmodified weights by the fp64 oracle) added to the bias of every convolution that feeds a GroupNorm."""
    import torch.nn.functional as TF
    sd64 = {k: v.double() for k, v in sd.items()}
    by_ptr = {v.data_ptr(): k for k, v in sd64.items()}
    stds = {}
    conv = TF.conv2d

    def conv_hook(x, w, b=None, *a, **k):
        y = conv(x, w, b, *a, **k)
        if b is not None and b.data_ptr() in by_ptr:
            stds[by_ptr[b.data_ptr()]] = float(y.std())
        return y

    TF.conv2d = conv_hook
    try:
        with torch.no_grad():
            U.UNetOracle(cfg, sd64, variant)(inp["x"], inp["t"], inp["context"], inp["y"])
    finally:
        TF.conv2d = conv
    out = {k: v.clone() for k, v in sd.items()}
    hit = [k for k in out if k.endswith(GN_FEEDERS) and k in stds]  # (parameters the forward never runs are left alone)
    assert hit, "no GroupNorm-feeding convolution was seen by the oracle run"
    for k in hit:
        out[k] = (out[k].double() + r * stds[k]).float()
    return out, hit
