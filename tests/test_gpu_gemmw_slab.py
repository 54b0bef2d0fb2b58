"""The slab form of the 64 x 320 weights-to-registers kernel (wd_gemmw_kernel<..., SLAB>, csrc/wd_gemmw.hip): the rows of a 3x3 /
pad 1 / stride 1 source copied into LDS once per 64-channel chunk, the taps read as shifts of the slab row, K walked chunk-major.
Every case runs wd_gemm through the C ABI twice - dbg WD_GEMMW_SLAB_ON (the slab form wherever wd_gemm finds it legal) and dbg WD_GEMMW_SLAB_OFF (the
per-tap form, what WDIFF_GEMMW_SLAB=0 runs) - and checks

  * the slab launch against the fp64 reference (F.conv2d on the fp32 inputs, + the fp64 1x1 of an identity second source) with the
    project's bounds: result and planes rel_err < 2e-5, statistics < 1e-5;
  * the slab launch against the per-tap launch: fp32 result and statistics max_rel < 5e-6 (two summation orders of one product: the
    bound tests/test_gpu_pitch.py sets between two forms of one launch).  The PLANES of the two launches cannot meet that figure: a
    plane pair holds x as bf16(x) + bf16(x - bf16(x)), whose second rounding leaves up to 2^-16 |x| (bf16 keeps 8 significant bits,
    twice), so the encodings of two results 5e-6 apart may differ by 5e-6 + 2 * 2^-16 = 3.55e-5 - measured 1.07e-5 at 8 x 32, B = 2,
    128 channels, where the fp32 results differ by 4.2e-7 and both plane pairs are within 4.1e-6 of fp64.  That sum is their bound;
  * that wd_gemm_check resolved the form the case is about.

Shapes, n = 320: 8 x 32 maps (two image rows per tile) at B = 2 and B = 3 (a tile count that is no multiple of 8: the XCD remap) with
64 (one chunk, no buffer swap), 128 (one swap) and 320 channels (odd chunk count, the step's own K); 16 x 16 and 4 x 64 maps (four and
one image rows per tile); an identity second source; and every epilogue feature at once on a pitched, guard-banded output."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _guard as G  # noqa: E402
from tests._common import FULL, make_args, max_rel, rel_err  # noqa: E402
from tests.test_gpu_pitch import DENSE, PITCH, _case, _conv, _launch, _unpl  # noqa: E402
from worddiffusion_amd import UNetModel  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs  # noqa: E402

DEV = "cuda:0"
SLAB_ON, SLAB_OFF = N.GEMMW_SLAB_ON, N.GEMMW_SLAB_OFF   # wd_gemm_args.dbg: override WDIFF_GEMMW_SLAB for the call; resolved SLAB_ON = slab form taken


def _both(d, P, slab_expected=True, **kw):
    """The case under both switches: (slab launch, per-tap launch), each asserted to have resolved to its form."""
    runs = []
    for bit in (SLAB_ON, SLAB_OFF):
        got = _launch(_case(kernel="K_GEMMW", tile=64320, w_layout=3, dbg=bit, **dict(d, **kw)), P)
        assert got.kernel == "K_GEMMW"
        assert bool(got.resolved[6] & SLAB_ON) == (slab_expected and bit == SLAB_ON), f"dbg {bit:#x} resolved to {got.resolved}"
        runs.append(got)
    return runs


def _figures(d, on, off, stat_cpg=0):
    ref = d["ref"]
    fig = {"out": rel_err(on.win["out"].cpu(), ref), "planes": rel_err(_unpl(on.win["pl"]), ref),
           "out vs per-tap": max_rel(on.win["out"].cpu(), off.win["out"].cpu()),
           "planes vs per-tap": max_rel(_unpl(on.win["pl"]), _unpl(off.win["pl"]))}
    if stat_cpg:
        B, hw, ngr = d["m"] // d["hw_out"], d["hw_out"], ref.shape[1] // stat_cpg
        o = ref.reshape(B, hw, ngr, stat_cpg)
        st, st0 = (g.win["stat"].cpu().reshape(B, -1, ngr, 2).sum(1) for g in (on, off))
        fig["stat"] = max(max_rel(st[..., 0], o.sum(dim=(1, 3))), max_rel(st[..., 1], (o * o).sum(dim=(1, 3))))
        fig["stat vs per-tap"] = max_rel(st, st0)
    return fig


def _assert_bounds(tag, fig):
    print(f"{tag}: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    assert fig["out"] < 2e-5 and fig["planes"] < 2e-5 and fig.get("stat", 0) < 1e-5
    assert fig["out vs per-tap"] < 5e-6 and fig.get("stat vs per-tap", 0) < 5e-6
    assert fig["planes vs per-tap"] < 5e-6 + 2 * 2.0 ** -16


# (map height, map width, samples, channels of the 3x3 source, channels of the identity source)
_SHAPES = [(8, 32, B, cin, 0) for B in (2, 3) for cin in (64, 128, 320)] + [(16, 16, 2, 128, 0), (4, 64, 2, 128, 0), (8, 32, 2, 128, 64)]


@pytest.mark.parametrize("hh,ww,B,cin,c2", _SHAPES)
def test_slab_form_against_fp64_and_the_per_tap_form(hh, ww, B, cin, c2):
    d = _conv(320, c1=cin, c2=c2, hh=hh, ww=ww, B=B, film=False, resid=False)
    on, off = _both(d, DENSE, slab_rows=ww)
    for g in (on, off):
        for key, w in g.win.items():
            G.assert_finite(w, key)
    _assert_bounds(f"{hh} x {ww}, B {B}, {cin} + {c2} channels", _figures(d, on, off))


def test_slab_form_every_epilogue_feature_on_a_pitched_guarded_output():
    """Bias + FiLM row + residual + statistics partials + output planes, every operand a window of a wider NaN-filled buffer with
    guard rows: a store outside an output window changes the pattern, a read outside an operand window brings a NaN in."""
    d = _conv(320, c1=128, c2=64, hh=8, ww=32, B=3, film=True, resid=True)
    on, off = _both(d, PITCH["a"], slab_rows=32, stat_cpg=10)
    for name, buf, view in on.outs:
        G.assert_untouched(buf, view, name)
    for key, w in on.win.items():
        G.assert_finite(w, key)
    _assert_bounds("8 x 32, B 3, 128 + 64 channels, all epilogue features, pitched", _figures(d, on, off, stat_cpg=10))


def test_shapes_the_slab_form_refuses_run_the_per_tap_form_bit_for_bit():
    """A map 24 wide (64 % 24 != 0) and an fp32 source with the consumer's GroupNorm (a32) are not slab shapes: with the switch on
    they resolve to the per-tap form and return the bits of the switch off."""
    d = _conv(320, c1=64, c2=0, hh=8, ww=24, B=2, film=False, resid=False)
    on, off = _both(d, DENSE, slab_expected=False, slab_rows=24)
    assert on.resolved == off.resolved
    assert torch.equal(on.win["out"], off.win["out"]) and torch.equal(on.win["pl"], off.win["pl"])
    g = torch.Generator().manual_seed(24)
    gam, bet = torch.randn(64, generator=g) * 0.3 + 1, torch.randn(64, generator=g) * 0.2
    d = _conv(320, c1=64, c2=0, hh=8, ww=32, B=2, film=False, resid=False)
    on, off = _both(d, DENSE, slab_expected=False, slab_rows=32, a32=dict(gamma=gam, beta=bet, cpg=2, eps=1e-5, silu=1))
    assert on.resolved == off.resolved
    assert torch.equal(on.win["out"], off.win["out"]) and torch.equal(on.win["pl"], off.win["pl"])


def test_engine_slab_switch(monkeypatch):
    """FULL base forward, WDIFF_GEMMW_SLAB=1 against 0: max_rel < 2e-5 at B = 2 (the bar of the earlier rounds; small batches stay on
    the LDS-staged kernels, so this asks that the switch changes nothing there) and at B = 64, where the six 3x3 convolutions of the
    8 x 32 level take the 64 x 320 kernel and the switch picks their form."""
    for B in (2, 64):
        inp = synthetic_inputs(B, seed=5)
        outs = []
        for on in ("0", "1"):
            monkeypatch.setenv("WDIFF_GEMMW_SLAB", on)
            m = UNetModel(args=make_args(device=DEV, phosc=0), **FULL)
            fill_module_(m, 2)
            m = m.to(DEV).eval()
            assert m.engine.gemmw_slab == (on == "1")
            with torch.no_grad():
                outs.append(m(inp["x"].to(DEV), None, original_images=None, timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV),
                              y=inp["y"].to(DEV)))
            del m
        e = max_rel(outs[1].cpu(), outs[0].cpu())
        print(f"FULL base forward, B {B}: slab vs per-tap bit-identical {torch.equal(outs[0], outs[1])}, max_rel {e:.3g}")
        assert torch.isfinite(outs[1]).all()
        assert e < 2e-5
        if B == 64:
            assert not torch.equal(outs[0], outs[1]), "the switch did not reach the 8 x 32 convolutions"
