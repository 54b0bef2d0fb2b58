"""Host gate of tests/_dw_ref.py, the specification tests/test_gpu_dw_guard.py holds wd_dw to: it equals fp64 autograd, and the
element-wise bound of the GPU test tells each of the two wrong variants from it, on the inputs the GPU test uses."""
import pytest
import torch
import torch.nn.functional as F

from tests import _dw_ref as R
from tests._common import max_rel
from worddiffusion_amd.engine import conv_gather_table


@pytest.mark.parametrize("mode,B,Ci,h,w,Co", [("same", 2, 5, 4, 6, 7), ("same", 1, 3, 5, 3, 4), ("down", 2, 5, 6, 8, 3), ("down", 1, 4, 5, 7, 6),
                                              ("up", 2, 3, 3, 4, 5)])
def test_specification_equals_autograd_of_conv2d(mode, B, Ci, h, w, Co):
    g = torch.Generator().manual_seed(B + 3 * Ci + 5 * h)
    x = torch.randn(B, Ci, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(Co, Ci, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if mode == "up" else x
    y = F.conv2d(xin, wt, None, stride=2 if mode == "down" else 1, padding=1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    tab, ho, wo = conv_gather_table(h, w, mode)
    assert (ho, wo) == tuple(y.shape[2:])
    d = dy.permute(0, 2, 3, 1).reshape(B * ho * wo, Co)
    tok = x.permute(0, 2, 3, 1).reshape(B * h * w, Ci)
    got, S = R.dw_ref(d, tok, 9, tab, ho * wo, h * w)
    assert max_rel(got.reshape(Co, Ci, 3, 3), wt.grad) < 1e-12
    assert bool((S >= got.abs() * (1 - 1e-12)).all())


def test_specification_equals_autograd_of_linear():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(37, 6, generator=g, dtype=torch.float64)
    wt = torch.randn(9, 6, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(37, 9, generator=g, dtype=torch.float64)
    F.linear(x, wt).backward(dy)
    got, S = R.dw_ref(dy, x)
    assert max_rel(got, wt.grad) < 1e-12
    assert bool((S >= got.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("case", sorted(R.CONV_CASES))
def test_bound_tells_the_wrong_variants_apart(case, variant):
    """A kernel that read source row 0 for a padding tap, or dropped the last sub-stage of 32 tokens, would miss the bound of the GPU
    test by at least 10x on at least one element."""
    mode, B, h, w, n, c, nslice, _, _, _, npass = R.CONV_CASES[case]
    _misses_by_10x(case, variant, R.conv_inputs(mode, B, h, w, n, c), nslice, npass)


def _misses_by_10x(name, variant, inputs, nslice, npass):
    d, x, tab, hw_out, hw_src = inputs
    dr, xr = R.rounded(d, npass), R.rounded(x, npass)
    ref, S = R.dw_ref(dr, xr, 9, tab, hw_out, hw_src)
    bad, _ = R.dw_ref(dr, xr, 9, tab, hw_out, hw_src, variant=variant)
    ratio = float(((bad - ref).abs() / (R.dw_beta(d.shape[0], nslice) * S)).max())
    print(f"{name} {variant}: largest |wrong - ref| / (beta S) = {ratio:.1f}")
    assert ratio >= 10.0


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("ntaps,nitems,n,nslice,npass", [g for g in R.GROUP_CASES if g[0] == 9])
def test_bound_tells_the_wrong_variants_apart_on_the_grouped_layers(ntaps, nitems, n, nslice, npass, variant):
    for i in range(nitems):
        _misses_by_10x(f"n{n} item {i} of {nitems}", variant, R.conv_inputs(*R.GROUP_MAP, n, n, key=i), nslice, npass)
