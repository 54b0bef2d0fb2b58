"""GroupNorm on the GPU when a group's mean is far from zero (tests/_norm_offset.py): every producer of (sum, sum of squares)
partials feeding a consumer, at mean / std = 0, 4, 16, 64, 256.  The consumer's result is compared with fp64 F.group_norm (+ SiLU)
of the producer's own fp32 output read back, so GEMM error is not counted; the bound is bound(path_tol, ref_err) - the tolerance
the path's ordinary test uses, or four times torch's own fp32 error on the same values - never the kernel's output.  The relative
error of var recomputed from `part` is printed with every case (diagnosis only).  LayerNorm, two-pass everywhere, is the control.

WDIFF_NORM_OFFSET_LOG=<file>: every measured line is appended there too (profiles/norm_offset_errors.txt was made that way)."""
import ctypes as C
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests import _norm_offset as NO  # noqa: E402
from tests._common import SMALL, make_args, max_rel, rel_err  # noqa: E402
from worddiffusion_amd import UNetModel  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.engine import conv_gather_table, geglu_interleave  # noqa: E402
from worddiffusion_amd.synthetic import synthetic_inputs, synthetic_tensor  # noqa: E402

DEV = "cuda:0"
RK = NO.rk_cases()
RK_IDS = [f"r{r}-{k}" for r, k in RK]
EPS = 1e-5


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _planes(x):
    hi = x.to(torch.bfloat16)
    return torch.stack([hi, (x - hi.float()).to(torch.bfloat16)], 0).contiguous()


def _unplanes(p):
    return p[0].float() + p[1].float()


def _pack(w):
    lib = N.lib()
    wp = _planes(w.to(DEV))
    wf = torch.empty_like(wp)
    N.check(lib.wd_gemm_pack_w(wp[0].data_ptr(), wp[1].data_ptr(), wp.shape[1], wp.shape[2], wf[0].data_ptr(), wf[1].data_ptr(), _st()),
            "wd_gemm_pack_w")
    return wf


def _record(path, shape, r, kind, err, ref_err, bnd, verr=float("nan")):
    line = (f"{path:34s} {str(shape):22s} r={r:<3d} {kind:5s} err {err:.2e}  ref_fp32 {ref_err:.2e}  bound {bnd:.2e}  "
            f"var_err {verr:.2e}")
    print(line)
    log = os.environ.get("WDIFF_NORM_OFFSET_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


def _group_offsets(B, n, cpg, r, kind, seed):
    """[B, n]: the offset of every (sample, channel), constant inside a group."""
    return NO.group_means(B, n // cpg, r, kind, seed).repeat_interleave(cpg, 1).float()


def _apply_and_check(path, x, part, nchunk, part_cpg, B, hw, c, cpg, r, kind, silu=1):
    """wd_gn_apply of x [B * hw, c] (device fp32) with `part` against fp64 GroupNorm (+ SiLU) of the same values."""
    lib = N.lib()
    ga, be = NO.affine(c, c + hw)
    gd, bd = ga.to(DEV), be.to(DEV)
    pl = torch.zeros(2, B * hw, c, dtype=torch.bfloat16, device=DEV)
    N.check(lib.wd_gn_apply(x.data_ptr(), x.shape[1], B, hw, c, cpg, part.data_ptr(), nchunk, part_cpg, gd.data_ptr(), bd.data_ptr(),
                            EPS, silu, pl[0].data_ptr(), pl[1].data_ptr(), c, 0, None, None, _st()), "wd_gn_apply")
    torch.cuda.synchronize()
    _check_planes(path, _unplanes(pl).cpu(), x, part, B, hw, c, cpg, part_cpg, r, kind, ga, be, silu)


def _check_planes(path, got, x, part, B, hw, c, cpg, part_cpg, r, kind, ga, be, silu):
    xc = x.cpu()[:, :c]
    ref, ref_err = NO.gn_ref_err(xc, B, hw, cpg, ga, be, EPS, silu)
    err, bnd = max_rel(got, ref), NO.bound(NO.TOL_PLANES, ref_err)
    verr = NO.var_err(part, xc, B, hw, cpg, part_cpg)
    _record(path, (B, hw, c, cpg), r, kind, err, ref_err, bnd, verr)
    assert torch.isfinite(got).all() and torch.isfinite(part).all()
    assert err <= bnd, f"{path}: planes max_rel {err:.3g} > {bnd:.3g} (var from part off by {verr:.3g})"


# ------------------------------------------------------------------------------------------ wd_gn_stats -> wd_gn_apply
@pytest.mark.parametrize("r,kind", RK, ids=RK_IDS)
@pytest.mark.parametrize("B,hw,c,cpg,part_cpg", [(2, 64, 320, 10, 10), (1, 100, 64, 2, 2), (2, 256, 640, 20, 10), (1, 32, 1280, 40, 40)],
                         ids=["2x64x320", "ragged_chunk", "part_cpg10_under_20", "c4_over_256"])
def test_gn_stats_feeds_gn_apply(B, hw, c, cpg, part_cpg, r, kind):
    lib = N.lib()
    x = NO.offset_input((B, hw), c, cpg, r, kind, seed=hw + c + r).to(DEV)
    nchunk = lib.wd_gn_nchunk(hw)
    part = torch.full((B, nchunk, c // part_cpg, 2), float("nan"), dtype=torch.float64, device=DEV)
    N.check(lib.wd_gn_stats(x.data_ptr(), c, B, hw, c, part_cpg, part.data_ptr(), _st()), "wd_gn_stats")
    _apply_and_check("gn_stats->gn_apply", x, part, nchunk, part_cpg, B, hw, c, cpg, r, kind)


@pytest.mark.parametrize("r,kind", RK, ids=RK_IDS)
def test_gn_stats_folded_chunks_feed_gn_apply(r, kind):
    B, hw, c, cpg = NO.GN_FOLD_SHAPE
    lib = N.lib()
    x = NO.offset_input((B, hw), c, cpg, r, kind, seed=hw + c + r).to(DEV)
    nchunk = lib.wd_gn_nchunk(hw)
    part = torch.full((B, nchunk, c // cpg, 2), float("nan"), dtype=torch.float64, device=DEV)
    fold = torch.full((B, 1, c // cpg, 2), float("nan"), dtype=torch.float64, device=DEV)
    N.check(lib.wd_gn_stats(x.data_ptr(), c, B, hw, c, cpg, part.data_ptr(), _st()), "wd_gn_stats")
    N.check(lib.wd_gn_fold_chunks(part.data_ptr(), B, nchunk, c // cpg, fold.data_ptr(), _st()), "wd_gn_fold_chunks")
    _apply_and_check("gn_stats->fold->gn_apply", x, fold, 1, cpg, B, hw, c, cpg, r, kind)


# ------------------------------------------------------------------------------------------ wd_gemm stat_part
def _conv_gemm(B, hh, ww, cin, n, cpg, r, kind, *, tile=0, w_layout=0, ksplit=1, tickets=False, where="bias", gn_cpg=0, off_cpg=0, want=()):
    """3x3 convolution of unit-variance rows with weights scaled for a unit-variance result; the offset of every (sample, group)
    enters through `bias` (one row: the offsets of sample 0) or `rowvec` (per sample); off_cpg: the width of the groups that
    share an offset when the consumer's groups are wider than the statistics groups.  Returns (out, part, nchunk, planes)."""
    lib = N.lib()
    hw, m = hh * ww, B * hh * ww
    g = torch.Generator().manual_seed(n + hh + cin + r)
    x = torch.randn(m, cin, generator=g)
    w = torch.randn(n, 9 * cin, generator=g) / (9 * cin) ** 0.5
    off = _group_offsets(B, n, off_cpg or cpg, r, kind, seed=n + r)
    bias = off[0].clone() if where == "bias" else torch.randn(n, generator=g) * 0.1
    tab, _, _ = conv_gather_table(hh, ww, "same")
    a = N.WdGemmArgs()
    s0 = N.WdSrc()
    pl, tabd = _planes(x.to(DEV)), torch.from_numpy(tab).to(DEV)
    s0.hi, s0.lo, s0.gather = pl[0].data_ptr(), pl[1].data_ptr(), tabd.data_ptr()
    s0.ld, s0.c, s0.ntaps, s0.hw_src = cin, cin, 9, hw
    a.src[0] = s0
    a.nsrc, a.npass = 1, 3
    wp = _pack(w) if w_layout == 3 else _planes(w.to(DEV))
    a.w_hi, a.w_lo, a.w_layout, a.tile = wp[0].data_ptr(), wp[1].data_ptr(), w_layout, tile
    if tile == 64080:
        a.slab_rows = ww
    a.m, a.n, a.ktot, a.hw_out = m, n, 9 * cin, hw
    bd = bias.to(DEV)
    a.bias = bd.data_ptr()
    if where == "rowvec":
        rv = off.to(DEV)
        a.rowvec, a.rowvec_ld = rv.data_ptr(), n
    out = torch.full((m, n), float("nan"), device=DEV)
    a.out_f32, a.out_ld = out.data_ptr(), n
    a.ksplit = ksplit
    ws = torch.empty(8 * m * n, device=DEV)
    if ksplit != 1:
        a.ws, a.ws_floats = ws.data_ptr(), ws.numel()
    tk = torch.zeros(1024, dtype=torch.int32, device=DEV)
    if tickets:
        a.tickets, a.ntickets = tk.data_ptr(), tk.numel()
    opl = torch.zeros(2, m, n, dtype=torch.bfloat16, device=DEV)
    ga, be = NO.affine(n, n + hw)
    gd, bed = ga.to(DEV), be.to(DEV)
    if gn_cpg:
        a.out_hi, a.out_lo, a.out_pl_ld = opl[0].data_ptr(), opl[1].data_ptr(), n
        a.gn_gamma, a.gn_beta, a.gn_eps, a.gn_silu, a.gn_cpg = gd.data_ptr(), bed.data_ptr(), EPS, 1, gn_cpg
    most = torch.empty(B, max(1, hw // 64), n // cpg, 2, dtype=torch.float64, device=DEV)  # (the resolved tile decides nchunk)
    a.stat_part, a.stat_cpg = most.data_ptr(), cpg
    res = N.WdGemmArgs()
    assert lib.wd_gemm_check(C.byref(a), C.byref(res)) == 0
    kern = lib.wd_gemm_check_kernel(C.byref(a)).decode()
    assert kern in want, f"{kern} (tile {res.tile}, ksplit {res.ksplit})"
    if ksplit == 0:
        assert res.ksplit > 1, "the case is about the combine: K must be cut"
    bm = 64 if (res.ksplit > 1 or res.tile in (64320, 64080, 64064)) else res.tile // 1000
    nchunk = max(1, hw // bm)
    part = torch.full((B, nchunk, n // cpg, 2), float("nan"), dtype=torch.float64, device=DEV)
    a.stat_part = part.data_ptr()
    N.check(lib.wd_gemm(C.byref(a), _st()), "wd_gemm")
    torch.cuda.synchronize()
    assert int(tk.abs().sum()) == 0
    return out, part, nchunk, (_unplanes(opl).cpu(), ga, be)


GEMM_CASES = {
    # name: (B, hh, ww, cin, n, cpg, keywords)
    "v2_two_samples_per_panel": (5, 8, 8, 64, 64, 2, dict(want=("K_V2", "K_V4"))),
    "m16_one_panel_per_sample": (2, 8, 16, 64, 640, 20, dict(want=("K_V2", "K_V4", "K_M16"))),
    "v2_offset_in_rowvec": (5, 8, 8, 64, 64, 2, dict(want=("K_V2", "K_V4"), where="rowvec")),
    "gemmw_64320": (3, 8, 32, 64, 320, 10, dict(want=("K_GEMMW",), tile=64320, w_layout=3)),
    "combine_second_launch": (4, 4, 16, 320, 320, 10, dict(want=("K_V2", "K_V4", "K_M16"), ksplit=0)),
    "combine_tickets": (4, 4, 16, 320, 320, 10, dict(want=("K_V2", "K_V4", "K_M16"), ksplit=0, tickets=True)),
    "gemmq_64080": (5, 4, 16, 64, 320, 10, dict(want=("K_GEMMQ",), tile=64080, w_layout=3, off_cpg=20)),
}


@pytest.mark.parametrize("r,kind", RK, ids=RK_IDS)
@pytest.mark.parametrize("case", list(GEMM_CASES))
def test_gemm_epilogue_statistics_feed_gn_apply(case, r, kind):
    B, hh, ww, cin, n, cpg, kw = GEMM_CASES[case]
    out, part, nchunk, _ = _conv_gemm(B, hh, ww, cin, n, cpg, r, kind, **kw)
    gcpg = kw.get("off_cpg", cpg)  # (K_GEMMQ: statistics per 10 channels under the consumer's groups of 20)
    _apply_and_check("gemm stat_part " + case, out, part, nchunk, cpg, B, hh * ww, n, gcpg, r, kind)


@pytest.mark.parametrize("r,kind", RK, ids=RK_IDS)
def test_gemmq_serves_the_groupnorm_in_the_launch(r, kind):
    """tile 64080 with gn_gamma: the planes are SiLU(GroupNorm(result)) from the launch itself (wd_gn_tile)."""
    B, hh, ww, cin, n, cpg, kw = GEMM_CASES["gemmq_64080"]
    out, part, nchunk, (got, ga, be) = _conv_gemm(B, hh, ww, cin, n, cpg, r, kind, gn_cpg=20, **kw)
    _check_planes("gemmq gn_* in the launch", got, out, part, B, hh * ww, n, 20, cpg, r, kind, ga, be, 1)


@pytest.mark.parametrize("r,kind", [(0, "same"), (64, "same"), (64, "mixed"), (256, "same")])
def test_combine_launch_serves_the_groupnorm(r, kind):
    """K cut + gn_gamma: wd_gn_tile in the combine launch (64 x 40 tiles)."""
    B, hh, ww, cin, n, cpg, kw = GEMM_CASES["combine_second_launch"]
    out, part, nchunk, (got, ga, be) = _conv_gemm(B, hh, ww, cin, n, cpg, r, kind, gn_cpg=10, **kw)
    _check_planes("combine gn_* in the launch", got, out, part, B, hh * ww, n, 10, cpg, r, kind, ga, be, 1)


# ------------------------------------------------------------------------------------------ wd_ff_fused stat_part
@pytest.mark.parametrize("where", ["b2", "resid"])
@pytest.mark.parametrize("r,kind", RK, ids=RK_IDS)
def test_ff_fused_statistics_feed_gn_apply(r, kind, where):
    """m = 128 tokens = two samples of 64, c = 320, inner = 128, statistics per 10 channels: the result is driven to the offset
    through b2 (per group) or through the residual (per sample and group)."""
    lib = N.lib()
    m, c, inner, hw, cpg = 128, 320, 128, 64, 10
    B = m // hw
    assert lib.wd_ff_supported(c, inner)
    g = torch.Generator().manual_seed(inner + r)
    x = torch.randn(m, c, generator=g)
    w1 = torch.randn(2 * inner, c, generator=g) / c ** 0.5
    b1 = torch.randn(2 * inner, generator=g)
    w2 = torch.randn(c, inner, generator=g) / inner ** 0.5
    off = _group_offsets(B, c, cpg, r, kind, seed=c + r)
    b2 = off[0].clone() if where == "b2" else torch.randn(c, generator=g) * 0.1
    res = torch.randn(m, c, generator=g) * 0.5
    if where == "resid":
        res = res + off.repeat_interleave(hw, 0)
    w1f, w2f = _pack(geglu_interleave(w1, 16)), _pack(w2)
    b1d, b2d, resd = geglu_interleave(b1, 16).to(DEV), b2.to(DEV), res.to(DEV)
    xp = _planes(x.to(DEV))
    a = N.WdFfArgs()
    a.x_hi, a.x_lo, a.x_ld = xp[0].data_ptr(), xp[1].data_ptr(), c
    a.m, a.c, a.inner, a.npass = m, c, inner, 3
    a.w1_hi, a.w1_lo, a.b1 = w1f[0].data_ptr(), w1f[1].data_ptr(), b1d.data_ptr()
    a.w2_hi, a.w2_lo, a.b2 = w2f[0].data_ptr(), w2f[1].data_ptr(), b2d.data_ptr()
    a.resid, a.resid_ld = resd.data_ptr(), c
    out = torch.full((m, c), float("nan"), device=DEV)
    a.out_f32, a.out_ld = out.data_ptr(), c
    part = torch.full((B, 1, c // cpg, 2), float("nan"), dtype=torch.float64, device=DEV)
    a.stat_part, a.stat_cpg, a.hw_out = part.data_ptr(), cpg, hw
    N.check(lib.wd_ff_fused(C.byref(a), _st()), "wd_ff_fused")
    torch.cuda.synchronize()
    _apply_and_check("ff_fused stat_part, offset in " + where, out, part, 1, cpg, B, hw, c, cpg, r, kind)


# ------------------------------------------------------------------------------------------ wd_conv3x3_in part
@pytest.mark.parametrize("r,kind", RK, ids=RK_IDS)
def test_input_convolution_statistics_feed_gn_apply(r, kind):
    lib = N.lib()
    B, cin, H, W, cout = 1, 1, 1, 16, 64
    hw, cpg = H * W, cout // 32
    assert lib.wd_conv3x3_in_supported(cin, H, W, cout)
    g = torch.Generator().manual_seed(cout + r)
    x = torch.randn(B, cin, H, W, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin) ** 0.5  # (H = 1: three of the nine taps see the image)
    bias = _group_offsets(B, cout, cpg, r, kind, seed=cout + r)[0].clone()
    nchunk = lib.wd_conv3x3_in_nchunk(hw)
    xd, wd, bd = x.to(DEV), wt.to(DEV), bias.to(DEV)
    out = torch.full((B * hw, cout), float("nan"), device=DEV)
    part = torch.full((B, nchunk, 32, 2), float("nan"), dtype=torch.float64, device=DEV)
    N.check(lib.wd_conv3x3_in(xd.data_ptr(), B, cin, H, W, wd.data_ptr(), bd.data_ptr(), cout, out.data_ptr(), cout, part.data_ptr(),
                              cpg, _st()), "wd_conv3x3_in")
    torch.cuda.synchronize()
    _apply_and_check("conv3x3_in part", out, part, nchunk, cpg, B, hw, cout, cpg, r, kind)


# ------------------------------------------------------------------------------------------ consumers inside other kernels
def _stats_of(x, B, hw, c, cpg):
    lib = N.lib()
    nchunk = lib.wd_gn_nchunk(hw)
    part = torch.full((B, nchunk, c // cpg, 2), float("nan"), dtype=torch.float64, device=DEV)
    N.check(lib.wd_gn_stats(x.data_ptr(), x.shape[1], B, hw, c, cpg, part.data_ptr(), _st()), "wd_gn_stats")
    return part, nchunk


def _gn_conv_refs(x, B, hh, ww, cpg, ga, be, silu, wt, bias):
    """conv3x3(SiLU?(GroupNorm(x))) + bias, token-major input x [B * hw, c] -> NCHW, in fp64 and the fp32 reference's error."""
    c = x.shape[1]

    def run(dt):
        y = NO.gn_ref(x, B, hh * ww, cpg, ga, be, EPS, silu, dt).reshape(B, hh, ww, c).permute(0, 3, 1, 2)
        return F.conv2d(y, wt.to(dt), bias.to(dt), padding=1)

    ref = run(torch.float64)
    return ref, max_rel(run(torch.float32), ref)


@pytest.mark.parametrize("r", [0, 64])
def test_gemm_a32_staging_consumes_offset_statistics(r):
    """wd_gemm_args.a32*: GroupNorm + SiLU applied while the 64 x 320 kernel stages the fp32 rows, (3, 8, 32, 64 -> 320, 9 taps)."""
    lib = N.lib()
    B, hh, ww, cin, n = 3, 8, 32, 64, 320
    hw, m, cpg = hh * ww, B * hh * ww, cin // 32
    x = NO.offset_input((B, hw), cin, cpg, r, "mixed" if r else "same", seed=cin + r)
    g = torch.Generator().manual_seed(17 + r)
    ga, be = torch.randn(cin, generator=g) * 0.3 + 1, torch.randn(cin, generator=g) * 0.2
    wt = torch.randn(n, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    bias = torch.randn(n, generator=g)
    ref, ref_err = _gn_conv_refs(x, B, hh, ww, cpg, ga, be, 1, wt, bias)
    xd = x.to(DEV)
    part, nchunk = _stats_of(xd, B, hw, cin, cpg)
    tab, _, _ = conv_gather_table(hh, ww, "same")
    tabd = torch.from_numpy(tab).to(DEV)
    a = N.WdGemmArgs()
    s0 = N.WdSrc()
    s0.gather, s0.ld, s0.c, s0.ntaps, s0.hw_src = tabd.data_ptr(), cin, cin, 9, hw
    a.src[0] = s0
    a.nsrc, a.npass = 1, 3
    wf = _pack(wt.permute(0, 2, 3, 1).reshape(n, 9 * cin))
    a.w_hi, a.w_lo, a.w_layout, a.tile, a.slab_rows = wf[0].data_ptr(), wf[1].data_ptr(), 3, 64320, ww
    a.m, a.n, a.ktot, a.hw_out, a.ksplit = m, n, 9 * cin, hw, 1
    bd, gd, bed = bias.to(DEV), ga.to(DEV), be.to(DEV)
    a.bias = bd.data_ptr()
    out = torch.full((m, n), float("nan"), device=DEV)
    a.out_f32, a.out_ld = out.data_ptr(), n
    a.a32, a.a32_ld, a.a32_part = xd.data_ptr(), cin, part.data_ptr()
    a.a32_nchunk, a.a32_pcpg, a.a32_cpg = nchunk, cpg, cpg
    a.a32_gamma, a.a32_beta, a.a32_eps, a.a32_silu = gd.data_ptr(), bed.data_ptr(), EPS, 1
    assert lib.wd_gemm_check_kernel(C.byref(a)) == b"K_GEMMW"
    N.check(lib.wd_gemm(C.byref(a), _st()), "wd_gemm a32")
    torch.cuda.synchronize()
    got = out.cpu().reshape(B, hh, ww, n).permute(0, 3, 1, 2)
    err, bnd = rel_err(got, ref), NO.bound(3e-5, ref_err)  # (rel_err < 3e-5: test_gemm_groupnorm_of_the_input_while_staging)
    _record("gemm a32 staging", (B, hw, cin, cpg), r, "mixed" if r else "same", err, ref_err, bnd)
    assert torch.isfinite(out).all() and err <= bnd


@pytest.mark.parametrize("r", [0, 64])
def test_fused_transformer_front_consumes_offset_statistics(r):
    """wd_ff_fused with x_in (the whole SpatialTransformer, B = 4 at 8 x 32, c = 320): its GroupNorm of x_in reads `part`.  The
    residual stream tok2 = tok + attention(tok), tok = GroupNorm(x_in) Wpi^T + b - which does not carry x_in itself - is compared
    with the launch chain proj_in -> wd_xattn_pair fed with the planes of the fp64 GroupNorm; the 1e-5 of
    test_fused_transformer_launch_equals_the_chain, or four times what the fp32 reference GroupNorm changes in that chain."""
    from tests.test_gpu_st_fused import _Block
    lib = N.lib()
    blk = _Block(4)
    B, hw, c, m, cpg = blk.B, blk.hw, blk.c, blk.m, blk.c // 32
    kind = "mixed" if r else "same"
    x = NO.offset_input((B, hw), c, cpg, r, kind, seed=c + hw + r)
    blk.x = x.to(DEV)
    blk.part.fill_(float("nan"))
    N.check(lib.wd_gn_stats(blk.x.data_ptr(), c, B, hw, c, cpg, blk.part.data_ptr(), _st()), "wd_gn_stats")
    _, _, tok2 = blk.fused()

    def chain_tok2(dt):
        gn = NO.gn_ref(x, B, hw, cpg, blk.gn_g, blk.gn_b, 1e-6, 0, dt).float().to(DEV)
        pl = _planes(gn)
        a = N.WdGemmArgs()
        s0 = N.WdSrc()
        s0.hi, s0.lo, s0.ld, s0.c, s0.ntaps, s0.hw_src = pl[0].data_ptr(), pl[1].data_ptr(), c, c, 1, hw
        a.src[0], a.nsrc, a.npass = s0, 1, 3
        a.w_hi, a.w_lo, a.w_layout, a.tile, a.ksplit = blk.pi_w[0].data_ptr(), blk.pi_w[1].data_ptr(), 3, 64320, 1
        a.m, a.n, a.ktot, a.hw_out = m, c, c, hw
        a.bias = blk.pi_b.data_ptr()
        tok = torch.full((m, c), float("nan"), device=DEV)
        a.out_f32, a.out_ld = tok.data_ptr(), c
        N.check(lib.wd_gemm(C.byref(a), _st()), "proj_in")
        out = torch.full((m, c), float("nan"), device=DEV)
        n3 = torch.zeros(2, m, c, dtype=torch.bfloat16, device=DEV)
        (qa, oa, ba, _), (qb, ob, bb, _) = blk.folds
        g2, b2 = blk.n2_g.data_ptr(), blk.n2_b.data_ptr()
        N.check(lib.wd_xattn_pair(tok.data_ptr(), c, B, hw, c, 1e-5, blk.heads, blk.L, g2, b2, qa.data_ptr(), oa.data_ptr(), ba.data_ptr(),
                                  g2, b2, qb.data_ptr(), ob.data_ptr(), bb.data_ptr(), out.data_ptr(), c, blk.n3_g.data_ptr(),
                                  blk.n3_b.data_ptr(), 1e-5, n3[0].data_ptr(), n3[1].data_ptr(), c, _st()), "wd_xattn_pair")
        torch.cuda.synchronize()
        return out.cpu()

    ref = chain_tok2(torch.float64)
    ref_err = max_rel(chain_tok2(torch.float32), ref)
    err, bnd = max_rel(tok2.cpu(), ref), NO.bound(1e-5, ref_err)
    _record("ff_fused x_in front (tok2)", (B, hw, c, cpg), r, kind, err, ref_err, bnd)
    assert torch.isfinite(tok2).all() and err <= bnd


@pytest.mark.parametrize("r", [0, 64])
def test_gn_conv3x3_few_consumes_offset_statistics(r):
    lib = N.lib()
    B, hh, ww, c, oc = 3, 5, 7, 64, 4
    hw, cpg = hh * ww, c // 32
    kind = "mixed" if r else "same"
    x = NO.offset_input((B, hw), c, cpg, r, kind, seed=c + r + 1)
    g = torch.Generator().manual_seed(23 + r)
    ga, be = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    wt = torch.randn(oc, c, 3, 3, generator=g) / (9 * c) ** 0.5
    bias = torch.randn(oc, generator=g)
    ref, ref_err = _gn_conv_refs(x, B, hh, ww, cpg, ga, be, 1, wt, bias)
    xd = x.to(DEV)
    part, nchunk = _stats_of(xd, B, hw, c, cpg)
    out = torch.full((B, oc, hh, ww), float("nan"), device=DEV)
    gd, bed, wd, bid = ga.to(DEV), be.to(DEV), wt.to(DEV), bias.to(DEV)
    N.check(lib.wd_gn_conv3x3_few(xd.data_ptr(), c, B, hh, ww, c, cpg, part.data_ptr(), nchunk, cpg, gd.data_ptr(), bed.data_ptr(), EPS, 1,
                                  wd.data_ptr(), bid.data_ptr(), oc, out.data_ptr(), _st()), "wd_gn_conv3x3_few")
    torch.cuda.synchronize()
    err, bnd = max_rel(out.cpu(), ref), NO.bound(2e-6, ref_err)  # (2e-6: test_gn_silu_conv3x3_few_output_channels)
    _record("gn_conv3x3_few", (B, hw, c, cpg), r, kind, err, ref_err, bnd)
    assert torch.isfinite(out).all() and err <= bnd


@pytest.mark.parametrize("r", [0, 64])
def test_gn_apply2_with_permuted_rows_consumes_offset_statistics(r):
    """wd_gn_apply2: a norm over the concat (a | b), source a written in another row order (perm_a), groups of 4 over two
    statistics arrays kept per 2 channels."""
    lib = N.lib()
    B, hw, ca, cb = 2, 64, 64, 64
    ctot, cpg, pc = ca + cb, 4, 2
    kind = "mixed" if r else "same"
    x = NO.offset_input((B, hw), ctot, cpg, r, kind, seed=ctot + r)
    perm = torch.randperm(hw, generator=torch.Generator().manual_seed(3)).int()  # position t of a sample sits in row perm[t]
    xa_pos, xb = x[:, :ca].contiguous(), x[:, ca:].contiguous()
    xa = torch.empty_like(xa_pos)
    for b in range(B):
        xa[b * hw + perm.long()] = xa_pos[b * hw:(b + 1) * hw]
    xad, xbd, pd = xa.to(DEV), xb.to(DEV), perm.to(DEV)
    pa, nca = _stats_of(xad, B, hw, ca, pc)
    pb, ncb = _stats_of(xbd, B, hw, cb, pc)
    ga, be = NO.affine(ctot, ctot + hw)
    gd, bed = ga.to(DEV), be.to(DEV)
    pl = torch.zeros(2, B * hw, ctot, dtype=torch.bfloat16, device=DEV)
    N.check(lib.wd_gn_apply2(xad.data_ptr(), ca, ca, pa.data_ptr(), nca, pc, 0, xbd.data_ptr(), cb, cb, pb.data_ptr(), ncb, pc, ca, B, hw,
                             cpg, gd.data_ptr(), bed.data_ptr(), EPS, 1, pl[0].data_ptr(), pl[1].data_ptr(), ctot, None, None,
                             pd.data_ptr(), _st()), "wd_gn_apply2")
    torch.cuda.synchronize()
    ref, ref_err = NO.gn_ref_err(x, B, hw, cpg, ga, be, EPS, 1)
    err, bnd = max_rel(_unplanes(pl).cpu(), ref), NO.bound(NO.TOL_PLANES, ref_err)
    _record("gn_apply2 perm_a", (B, hw, ctot, cpg), r, kind, err, ref_err, bnd)
    assert torch.isfinite(_unplanes(pl)).all() and err <= bnd


# ------------------------------------------------------------------------------------------ backward
@functools.lru_cache(maxsize=None)
def _bwd_case(r, silu):
    B, hw, c, cpg = 2, 64, 80, 10
    kind = "mixed" if r else "same"
    x = NO.offset_input((B, hw), c, cpg, r, kind, seed=c + r)
    ga, be = NO.affine(c, c)
    dz = torch.randn(B * hw, c, generator=torch.Generator().manual_seed(5 + r))
    grads = {}
    for dt in (torch.float64, torch.float32):
        xr, gr, br = (t.to(dt).requires_grad_(True) for t in (x, ga, be))
        y = F.group_norm(xr.reshape(B, hw, c).permute(0, 2, 1), c // cpg, gr, br, EPS)
        if silu:
            y = F.silu(y)
        y.permute(0, 2, 1).reshape(B * hw, c).backward(dz.to(dt))
        grads[dt] = (xr.grad, br.grad, gr.grad)
    return x, ga, be, dz, grads, kind


@pytest.mark.parametrize("form", ["fused", "stats_apply"])
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("r", [0, 64])
def test_groupnorm_backward_with_offset_statistics(r, silu, form):
    """wd_gn_bwd_fused and wd_gn_bwd_stats + wd_gn_bwd_apply at (2, 64, 80, 10): dx and [dbeta | dgamma] against fp64 autograd, at
    the 3e-5 max_rel of test_gpu_backward_guard.py or four times fp32 autograd's own error."""
    lib = N.lib()
    B, hw, c, cpg = 2, 64, 80, 10
    x, ga, be, dz, grads, kind = _bwd_case(r, silu)
    xd, dzd, gd, bed = x.to(DEV), dz.to(DEV), ga.to(DEV), be.to(DEV)
    part, nck = _stats_of(xd, B, hw, c, cpg)
    dx = torch.full((B * hw, c), float("nan"), device=DEV)
    common = (xd.data_ptr(), c, dzd.data_ptr(), c, 0, B, hw, c, cpg, part.data_ptr(), nck, cpg, gd.data_ptr(), bed.data_ptr(), 0, EPS, silu)
    if form == "fused":
        assert lib.wd_gn_bwd_fused_supported(hw, c, cpg)
        sums = torch.full((B, 1, 2, c), float("nan"), device=DEV)
        N.check(lib.wd_gn_bwd_fused(*common, sums.data_ptr(), dx.data_ptr(), c, 0, _st()), "wd_gn_bwd_fused")
    else:
        sums = torch.full((B, lib.wd_gn_bwd_nchunk(hw), 2, c), float("nan"), device=DEV)
        N.check(lib.wd_gn_bwd_stats(*common, sums.data_ptr(), _st()), "wd_gn_bwd_stats")
        N.check(lib.wd_gn_bwd_apply(*common, sums.data_ptr(), dx.data_ptr(), c, 0, _st()), "wd_gn_bwd_apply")
    torch.cuda.synchronize()
    tot = sums.cpu().double().sum((0, 1))  # [d beta | d gamma]
    assert torch.isfinite(dx).all() and torch.isfinite(tot).all()
    for name, got, k in (("dx", dx.cpu(), 0), ("dbeta", tot[0], 1), ("dgamma", tot[1], 2)):
        ref_err = max_rel(grads[torch.float32][k], grads[torch.float64][k])
        err, bnd = max_rel(got, grads[torch.float64][k]), NO.bound(3e-5, ref_err)
        _record(f"gn_bwd {form} silu={silu} {name}", (B, hw, c, cpg), r, kind, err, ref_err, bnd)
        assert err <= bnd, name


# ------------------------------------------------------------------------------------------ LayerNorm controls (two-pass)
@pytest.mark.parametrize("r", [0, 256])
@pytest.mark.parametrize("rows,c", [(37, 64), (5, 1280)])
def test_layernorm_control(rows, c, r):
    lib = N.lib()
    x = NO.offset_rows(rows, c, r, seed=rows + c + r)
    ga, be = NO.affine(c, c + rows)
    ref, ref_err = NO.ln_ref_err(x, ga, be, EPS)
    pl = torch.zeros(2, rows, c, dtype=torch.bfloat16, device=DEV)
    xd, gd, bd = x.to(DEV), ga.to(DEV), be.to(DEV)
    N.check(lib.wd_layernorm(xd.data_ptr(), c, rows, c, gd.data_ptr(), bd.data_ptr(), EPS, pl[0].data_ptr(), pl[1].data_ptr(), c, _st()),
            "wd_layernorm")
    torch.cuda.synchronize()
    err, bnd = max_rel(_unplanes(pl).cpu(), ref), NO.bound(NO.TOL_PLANES, ref_err)
    _record("layernorm", (rows, c), r, "rows", err, ref_err, bnd)
    assert torch.isfinite(_unplanes(pl)).all() and err <= bnd


@pytest.mark.parametrize("r", [0, 256])
def test_gemm_layernorm_epilogue_control(r):
    """ln_* of the 64 x 320 kernel at m = k = 64 (n = 320: the tile holds whole rows), the rows' offset in the bias."""
    lib = N.lib()
    m, k, n = 64, 64, 320
    g = torch.Generator().manual_seed(m + k + r)
    x = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) / k ** 0.5
    bias = torch.full((n,), float(r))
    ga, be = NO.affine(n, n)
    xp, wf = _planes(x.to(DEV)), _pack(w)
    a = N.WdGemmArgs()
    s0 = N.WdSrc()
    s0.hi, s0.lo, s0.ld, s0.c, s0.ntaps = xp[0].data_ptr(), xp[1].data_ptr(), k, k, 1
    a.src[0] = s0
    a.nsrc, a.npass = 1, 3
    a.w_hi, a.w_lo, a.w_layout = wf[0].data_ptr(), wf[1].data_ptr(), 3
    a.m, a.n, a.ktot, a.hw_out = m, n, k, 1
    bd, gd, bed = bias.to(DEV), ga.to(DEV), be.to(DEV)
    a.bias = bd.data_ptr()
    out = torch.full((m, n), float("nan"), device=DEV)
    opl = torch.zeros(2, m, n, dtype=torch.bfloat16, device=DEV)
    a.out_f32, a.out_ld = out.data_ptr(), n
    a.out_hi, a.out_lo, a.out_pl_ld = opl[0].data_ptr(), opl[1].data_ptr(), n
    a.ln_gamma, a.ln_beta, a.ln_eps = gd.data_ptr(), bed.data_ptr(), EPS
    assert lib.wd_gemm_check_kernel(C.byref(a)) == b"K_GEMMW"
    N.check(lib.wd_gemm(C.byref(a), _st()), "wd_gemm ln_*")
    torch.cuda.synchronize()
    ref, ref_err = NO.ln_ref_err(out, ga, be, EPS)  # of the launch's own fp32 rows
    err, bnd = max_rel(_unplanes(opl).cpu(), ref), NO.bound(5e-5, ref_err)  # (5e-5: test_gemm_layernorm_of_the_result_rows)
    _record("gemm ln_* epilogue", (m, n), r, "rows", err, ref_err, bnd)
    assert torch.isfinite(_unplanes(opl)).all() and err <= bnd


@pytest.mark.parametrize("r", [0, 256])
def test_folded_cross_attention_layernorm_control(r):
    """wd_xattn_fused at (2, 32, 64, heads 4, L 7) on an offset block input: the LayerNorm in front of the attention and the one
    behind it, against fp64."""
    lib = N.lib()
    B, hw, c, heads, L = 2, 32, 64, 4, 7
    assert lib.wd_xattn_supported(c, heads, L) == 1
    d = c // heads
    g = torch.Generator().manual_seed(hw + c + L + r)
    x = NO.offset_rows(B * hw, c, r, seed=hw + c + r)
    kv = torch.randn(B * L, 2 * c, generator=g) * 0.5
    wq, wo = torch.randn(c, c, generator=g) / c ** 0.5, torch.randn(c, c, generator=g) / c ** 0.5
    bo = torch.randn(c, generator=g) * 0.1
    ga, be, ga2, be2 = (torch.randn(c, generator=g) * 0.2 + (1.0 if i % 2 == 0 else 0.0) for i in range(4))
    scale = d ** -0.5

    def run(dt):
        xd = x.to(dt)
        n1 = F.layer_norm(xd, (c,), ga.to(dt), be.to(dt), EPS)
        hd = lambda t, n: t.reshape(B, n, heads, d).permute(0, 2, 1, 3)  # noqa: E731
        q, k, v = n1 @ wq.to(dt).t(), kv[:, :c].to(dt), kv[:, c:].to(dt)
        att = torch.softmax(hd(q, hw) @ hd(k, L).transpose(-1, -2) * scale, -1)
        o = (att @ hd(v, L)).permute(0, 2, 1, 3).reshape(B * hw, c)
        return o @ wo.to(dt).t() + bo.to(dt) + xd

    ref, ref32 = run(torch.float64), run(torch.float32)
    dev = lambda t: t.contiguous().to(DEV)  # noqa: E731
    xg, kg, vg, wqg, wog, bog, gag, beg, ga2g, be2g = map(dev, (x, kv[:, :c], kv[:, c:], wq, wo, bo, ga, be, ga2, be2))
    mq, mo = torch.zeros(B, heads * L, c, device=DEV), torch.zeros(B, heads * L, c, device=DEV)
    mq_pl = torch.zeros(B, 2, 64, c, dtype=torch.bfloat16, device=DEV)
    mot_pl = torch.zeros(B, 2, c, 64, dtype=torch.bfloat16, device=DEV)
    N.check(lib.wd_xattn_fold(kg.data_ptr(), c, vg.data_ptr(), c, B, heads, L, d, scale, wqg.data_ptr(), wog.data_ptr(), c, mq.data_ptr(),
                              mo.data_ptr(), mq_pl.data_ptr(), mot_pl.data_ptr(), _st()), "wd_xattn_fold")
    out = torch.full((B * hw, c), float("nan"), device=DEV)
    pl = torch.zeros(2, B * hw, c, dtype=torch.bfloat16, device=DEV)
    N.check(lib.wd_xattn_fused(xg.data_ptr(), c, B, hw, c, gag.data_ptr(), beg.data_ptr(), EPS, mq.data_ptr(), mo.data_ptr(), heads, L,
                               bog.data_ptr(), out.data_ptr(), c, ga2g.data_ptr(), be2g.data_ptr(), EPS, pl[0].data_ptr(), pl[1].data_ptr(),
                               c, None, None, _st()), "wd_xattn_fused")
    torch.cuda.synchronize()
    # the attention branch (out - x), where the first LayerNorm shows: 2e-5 of test_folded_cross_attention, relative to the branch
    ref_err = max_rel(ref32 - x, ref - x.double())
    err, bnd = max_rel(out.cpu().double() - x.double(), ref - x.double()), NO.bound(2e-5, ref_err)
    _record("xattn_fused branch (LN in front)", (B * hw, c), r, "rows", err, ref_err, bnd)
    assert torch.isfinite(out).all() and err <= bnd
    # the LayerNorm behind it, of the launch's own fp32 rows
    ref_n, ref_err = NO.ln_ref_err(out, ga2, be2, EPS)
    err, bnd = max_rel(_unplanes(pl).cpu(), ref_n), NO.bound(NO.TOL_PLANES, ref_err)
    _record("xattn_fused LN behind", (B * hw, c), r, "rows", err, ref_err, bnd)
    assert err <= bnd


@pytest.mark.parametrize("r", [0, 256])
def test_layernorm_backward_control(r):
    lib = N.lib()
    rows, c = 37, 64
    x = NO.offset_rows(rows, c, r, seed=rows + c + r + 1)
    ga, _ = NO.affine(c, c + rows)
    dy = torch.randn(rows, c, generator=torch.Generator().manual_seed(9 + r))
    grads = {}
    for dt in (torch.float64, torch.float32):
        xr, gr = x.to(dt).requires_grad_(True), ga.to(dt).requires_grad_(True)
        br = torch.zeros(c, dtype=dt, requires_grad=True)
        F.layer_norm(xr, (c,), gr, br, EPS).backward(dy.to(dt))
        grads[dt] = (xr.grad, gr.grad, br.grad)
    nblk = lib.wd_layernorm_bwd_nblk(rows)
    xd, dyd, gd = x.to(DEV), dy.to(DEV), ga.to(DEV)
    dx = torch.full((rows, c), float("nan"), device=DEV)
    col = torch.full((nblk, 2, c), float("nan"), device=DEV)
    N.check(lib.wd_layernorm_bwd(xd.data_ptr(), c, dyd.data_ptr(), c, rows, c, gd.data_ptr(), EPS, dx.data_ptr(), c, 0, col.data_ptr(),
                                 _st()), "wd_layernorm_bwd")
    torch.cuda.synchronize()
    tot = col.cpu().double().sum(0)  # [d gamma | d beta]
    for name, got, k in (("dx", dx.cpu(), 0), ("dgamma", tot[0], 1), ("dbeta", tot[1], 2)):
        ref_err = max_rel(grads[torch.float32][k], grads[torch.float64][k])
        err, bnd = max_rel(got, grads[torch.float64][k]), NO.bound(3e-5, ref_err)
        _record(f"layernorm_bwd {name}", (rows, c), r, "rows", err, ref_err, bnd)
        assert torch.isfinite(got).all() and err <= bnd, name


# ------------------------------------------------------------------------------------------ the model
def test_model_forward_with_offset_groupnorm_inputs():
    """SMALL base UNet, every GroupNorm-feeding convolution bias + 16 std of that convolution's output: one forward at B = 2
    against the fp64 oracle at the 1e-4 rel_err of the end-to-end contract (the fp32 oracle is inside 2.5e-5:
    test_norm_offset_host.py)."""
    cfg = SMALL
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, 7)) for k, s in U.state_dict_shapes(cfg, "base")}
    inp = synthetic_inputs(2, seed=3, hw=(4, 8), num_classes=cfg["num_classes"])
    sd_off, hit = NO.offset_model_state(U, cfg, sd, "base", inp)
    with torch.no_grad():
        ref = U.UNetOracle(cfg, {k: v.double() for k, v in sd_off.items()}, "base")(inp["x"], inp["t"], inp["context"], inp["y"])
    model = UNetModel(args=make_args(device=DEV), **cfg)
    model.load_state_dict(sd_off, strict=True)
    model = model.to(DEV).eval()
    with torch.no_grad():
        out = model(inp["x"].to(DEV), None, original_images=None, timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV),
                    y=inp["y"].to(DEV))
    err = rel_err(out.cpu(), ref)
    _record("model SMALL base, +16 std biases", tuple(out.shape), 16, "same", err, float("nan"), 1e-4)
    assert torch.isfinite(out).all() and err <= 1e-4
