"""The two ends of the denoising step: wd_gn_conv3x3_few (GroupNorm + SiLU + the 320 -> 4 convolution; a workgroup owns a tile of
4 image rows x 16 columns, a lane four pixels and two channels of a chunk) and wd_conv3x3_in (the 4-channel first convolution as a
direct fp32 kernel with the GroupNorm statistics partials of its result).  Shapes: row blocks taller than the image, ragged
against it and exact; one, two and four column tiles; one channel chunk and five; every store inside a NaN guard band; two
launches give the same bits.  Bound 2e-6 max_rel against fp64, the bar tests/test_gpu_kernels.py sets for the output kernel:
both kernels sum at most 2880 fp32 products per output in a fixed order."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests._common import FULL, SMALL, make_args, max_rel  # noqa: E402
from tests._guard import assert_finite, assert_untouched, guarded  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd import UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs  # noqa: E402

DEV = "cuda:0"


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _unplanes(p):
    return p[0].float() + p[1].float()


# ---------------------------------------------------------------------------------------------- output convolution
OUT_CASES = [  # (h, w, c, oc, silu, chunked statistics)
    (1, 16, 64, 4, 1, False), (2, 32, 64, 3, 1, True), (3, 64, 64, 1, 0, False), (8, 32, 320, 4, 1, True),
    (8, 16, 320, 3, 0, False), (3, 32, 320, 1, 1, True), (2, 64, 320, 4, 1, False), (1, 64, 64, 4, 0, True),
    (8, 64, 64, 4, 1, False), (3, 16, 64, 3, 1, True), (2, 16, 320, 1, 1, False), (1, 32, 320, 4, 1, False),
]


@pytest.mark.parametrize("h,w,c,oc,silu,chunked", OUT_CASES)
def test_output_convolution_tiles(h, w, c, oc, silu, chunked):
    """h in {1, 2, 3, 8} x w in {16, 32, 64} x c in {64, 320}, oc in {1, 3, 4}, SiLU on and off, B = 3; statistics from wd_gn_stats
    (one chunk per 32 positions: nchunk > 1 from 64 positions on) or, `chunked`, from partials of our own cut into 3 chunks of
    uneven length; the output inside a NaN guard band."""
    lib = N.lib()
    B = 3
    g = torch.Generator().manual_seed(1000 * h + 10 * w + c + oc)
    x = torch.randn(B, c, h, w, generator=g) * 2 + 0.3
    gam, bet = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    wt = torch.randn(oc, c, 3, 3, generator=g) / (9 * c) ** 0.5
    bias = torch.randn(oc, generator=g)
    y = F.group_norm(x.double(), 32, gam.double(), bet.double(), eps=1e-5)
    y = F.silu(y) if silu else y
    ref = F.conv2d(y, wt.double(), bias.double(), padding=1)
    hw = h * w
    tok = x.permute(0, 2, 3, 1).reshape(B * hw, c).contiguous().to(DEV)
    cpg = c // 32
    if chunked:
        cuts = [0, hw // 5, hw // 5 + hw // 2, hw]
        t64 = tok.double().reshape(B, hw, 32, cpg)
        part = torch.stack([torch.stack([t64[:, a:b].sum((1, 3)), (t64[:, a:b] ** 2).sum((1, 3))], -1)
                            for a, b in zip(cuts[:-1], cuts[1:])], 1).contiguous()
        nchunk = 3
        assert part.shape == (B, 3, 32, 2)
    else:
        nchunk = lib.wd_gn_nchunk(hw)
        part = torch.zeros(B, nchunk, 32, 2, dtype=torch.float64, device=DEV)
        N.check(lib.wd_gn_stats(tok.data_ptr(), c, B, hw, c, cpg, part.data_ptr(), _st()), "stats")
    assert lib.wd_gn_conv3x3_few_supported(c, w, oc)
    gd, bd, wd, bid = gam.to(DEV), bet.to(DEV), wt.to(DEV), bias.to(DEV)
    outs = []
    for _ in range(2):
        buf, view = guarded(1, B * oc * hw, B * oc * hw + 64, 32, torch.float32, guard_rows=1, device=DEV)
        N.check(lib.wd_gn_conv3x3_few(tok.data_ptr(), c, B, h, w, c, cpg, part.data_ptr(), nchunk, cpg, gd.data_ptr(),
                                      bd.data_ptr(), 1e-5, silu, wd.data_ptr(), bid.data_ptr(), oc, view.data_ptr(), _st()), "gn_conv")
        torch.cuda.synchronize()
        assert_untouched(buf, view, "output")
        assert_finite(view, "output")
        outs.append(view.reshape(B, oc, h, w).clone())
    err = max_rel(outs[0].cpu(), ref)
    print(f"h={h} w={w} c={c} oc={oc} silu={silu} chunked={chunked}: max_rel {err:.3g}")
    assert err < 2e-6
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------- input convolution
IN_CASES = [(3, 4, 8, 32, 320), (2, 4, 2, 16, 320), (5, 3, 4, 16, 64), (1, 1, 1, 16, 64)]


@pytest.mark.parametrize("B,cin,H,W,cout", IN_CASES)
def test_input_convolution_rows_and_statistics(B, cin, H, W, cout):
    lib = N.lib()
    g = torch.Generator().manual_seed(B * 1000 + cin * 100 + H * W + cout)
    x = torch.randn(B, cin, H, W, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.3
    ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1).permute(0, 2, 3, 1).reshape(B * H * W, cout)
    assert lib.wd_conv3x3_in_supported(cin, H, W, cout)
    hw, cpg = H * W, cout // 32
    nchunk = lib.wd_conv3x3_in_nchunk(hw)
    assert nchunk == (hw + 63) // 64
    xd, wd, bd = x.to(DEV), wt.to(DEV), bias.to(DEV)
    ld = cout + 24
    got = []
    for _ in range(2):
        buf, view = guarded(B * hw, cout, ld, 8, torch.float32, device=DEV)
        pbuf, pview = guarded(1, B * nchunk * 32 * 2, B * nchunk * 32 * 2 + 16, 8, torch.float64, guard_rows=1, device=DEV)
        N.check(lib.wd_conv3x3_in(xd.data_ptr(), B, cin, H, W, wd.data_ptr(), bd.data_ptr(), cout, view.data_ptr(), ld,
                                  pview.data_ptr(), cpg, _st()), "conv3x3_in")
        torch.cuda.synchronize()
        assert_untouched(buf, view, "rows")
        assert_untouched(pbuf, pview, "partials")
        assert_finite(view, "rows")
        assert_finite(pview, "partials")
        got.append((view.clone(), pview.reshape(B, nchunk, 32, 2).clone()))
    out, part = got[0]
    err = max_rel(out.cpu(), ref)
    print(f"B={B} cin={cin} {H}x{W} cout={cout}: max_rel {err:.3g}")
    assert err < 2e-6
    assert torch.equal(out, got[1][0]) and torch.equal(part, got[1][1])
    # the partials, chunk by chunk and folded: fp64 sums of the kernel's own fp32 rows
    o64 = out.double().cpu().reshape(B, hw, 32, cpg)
    for j in range(nchunk):
        a, b = 64 * j, min(hw, 64 * j + 64)
        for k, want in enumerate((o64[:, a:b].sum((1, 3)), (o64[:, a:b] ** 2).sum((1, 3)))):
            assert max_rel(part[:, j, :, k].cpu(), want) < 1e-12, (j, k)
    folded = part.cpu().sum(1)
    for k, want in enumerate((o64.sum((1, 3)), (o64 ** 2).sum((1, 3)))):
        assert max_rel(folded[..., k], want) < 1e-12, k
    # ... and wd_gn_apply takes them: planes against fp64 GroupNorm of the fp64 convolution (3e-5: the bound of
    # test_groupnorm_silu_planes for split-bf16 planes)
    gam, bet = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
    gn = F.silu(F.group_norm(ref.reshape(B, hw, cout).permute(0, 2, 1), 32, gam.double(), bet.double(), 1e-5))
    gn = gn.permute(0, 2, 1).reshape(B * hw, cout)
    pl = torch.zeros(2, B * hw, cout, dtype=torch.bfloat16, device=DEV)
    gd, btd = gam.to(DEV), bet.to(DEV)
    N.check(lib.wd_gn_apply(out.data_ptr(), out.stride(0), B, hw, cout, cpg, part.data_ptr(), nchunk, cpg, gd.data_ptr(), btd.data_ptr(),
                            1e-5, 1, pl[0].data_ptr(), pl[1].data_ptr(), cout, 0, None, None, _st()), "apply")
    torch.cuda.synchronize()
    assert max_rel(_unplanes(pl).cpu(), gn) < 3e-5


def test_input_convolution_without_partials_and_predicate():
    """part = NULL writes the rows only; the predicate refuses five input channels, a width past 64 and a sample past 2048 padded
    pixels, and the launcher refuses what the predicate refuses."""
    lib = N.lib()
    B, cin, H, W, cout = 2, 4, 3, 16, 64
    g = torch.Generator().manual_seed(5)
    x, wt = torch.randn(B, cin, H, W, generator=g), torch.randn(cout, cin, 3, 3, generator=g) / 6
    ref = F.conv2d(x.double(), wt.double(), None, padding=1).permute(0, 2, 3, 1).reshape(B * H * W, cout)
    xd, wd = x.to(DEV), wt.to(DEV)
    buf, view = guarded(B * H * W, cout, cout, 0, torch.float32, device=DEV)
    N.check(lib.wd_conv3x3_in(xd.data_ptr(), B, cin, H, W, wd.data_ptr(), None, cout, view.data_ptr(), cout, None, 0, _st()), "conv")
    torch.cuda.synchronize()
    assert_untouched(buf, view, "rows")
    assert max_rel(view.cpu(), ref) < 2e-6
    assert not lib.wd_conv3x3_in_supported(5, 8, 32, 320)
    assert not lib.wd_conv3x3_in_supported(4, 8, 65, 320) and not lib.wd_conv3x3_in_supported(4, 64, 256, 320)
    assert not lib.wd_conv3x3_in_supported(4, 64, 64, 320) and not lib.wd_conv3x3_in_supported(4, 8, 32, 322)
    assert lib.wd_conv3x3_in_supported(4, 8, 32, 320) and lib.wd_conv3x3_in_supported(1, 1, 16, 64)
    assert lib.wd_conv3x3_in(xd.data_ptr(), B, 5, H, W, wd.data_ptr(), None, cout, view.data_ptr(), cout, None, 0, _st()) == N.WD_EINVAL
    assert lib.wd_conv3x3_in(xd.data_ptr(), B, cin, H, W, wd.data_ptr(), None, cout, view.data_ptr(), cout - 4, None, 0, _st()) == N.WD_EINVAL


# ---------------------------------------------------------------------------------------------- engine
def _build(cfg, variant, phosc_on, fuse_in, seed=0, **argkw):
    args = make_args(device=DEV, phosc=1 if phosc_on else 0, **argkw)
    m = fill_module_((UNetModel if variant == "base" else UNetModelPhosc)(args=args, **cfg), seed).to(DEV).eval()
    m.engine.fuse_in = fuse_in
    return m


def _forward(m, variant, inp):
    with torch.no_grad():
        if variant == "base":
            return m(inp["x"].to(DEV), None, original_images=None, timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV),
                     y=inp["y"].to(DEV))
        return m(inp["x"].to(DEV), inp["phosc"].to(DEV) if "phosc" in inp else None, timesteps=inp["t"].to(DEV),
                 context=inp["context"].to(DEV), y=inp["y"].to(DEV))


def _whats(m):
    return [what for _, _, what in next(iter(m.engine._plans.values())).step]


@pytest.mark.parametrize("B", [2, 64])
def test_engine_direct_first_convolution_equals_the_gemm_pair(B):
    """FULL base model: the direct first convolution (default) against im2col + wd_gemm (engine.fuse_in = False, what
    WDIFF_FUSE_IN=0 sets): only the first layer's rounding differs (fp32 products against split-bf16 x 3), so the forwards agree
    far inside 2e-5; one launch fewer."""
    inp = synthetic_inputs(B, seed=11)
    outs, whats = [], []
    for fuse in (True, False):
        m = _build(FULL, "base", False, fuse)
        outs.append(_forward(m, "base", inp))
        whats.append(_whats(m))
    err = max_rel(outs[0].cpu(), outs[1].cpu())
    print(f"B={B}: direct first convolution vs im2col + GEMM max_rel {err:.3g}")
    assert torch.isfinite(outs[0]).all() and err <= 2e-5
    assert len(whats[1]) - len(whats[0]) == 1
    assert "im2col" in whats[1] and "im2col" not in whats[0]
    assert sum(1 for w in whats[0] if w.startswith("input_blocks.0: conv3x3")) == 1


def test_engine_switch_reads_the_environment(monkeypatch):
    """WDIFF_FUSE_IN, read where the other switches are: default on, 0 switches the direct kernel off."""
    monkeypatch.setenv("WDIFF_FUSE_IN", "0")
    m = fill_module_(UNetModel(args=make_args(device=DEV), **SMALL), 0).to(DEV).eval()
    assert m.engine.fuse_in is False
    monkeypatch.delenv("WDIFF_FUSE_IN")
    m = fill_module_(UNetModel(args=make_args(device=DEV), **SMALL), 0).to(DEV).eval()
    assert m.engine.fuse_in is True


def test_engine_keeps_the_gemm_pair_where_the_direct_kernel_does_not_apply():
    """The PHOSC plan, and a base model fed 64 x 256 maps (the non-latent size: the predicate refuses the width), build and run on
    im2col + wd_gemm as before."""
    inp = synthetic_inputs(2, seed=12, phosc_len=769)
    m = _build(FULL, "phosc", True, True)
    out = _forward(m, "phosc", inp)
    assert torch.isfinite(out).all() and "im2col" in _whats(m)
    inp = synthetic_inputs(1, seed=13, hw=(64, 256), num_classes=SMALL["num_classes"])
    m = _build(SMALL, "base", False, True, latent=False)
    out = _forward(m, "base", inp)
    assert out.shape == (1, 4, 64, 256) and torch.isfinite(out).all() and "im2col" in _whats(m)
