"""CPU half of the large-mean normalisation tests (tests/_norm_offset.py): the reference alone stays inside the path tolerances
on every input the GPU file uses, so the bound there is the path tolerance itself (r = 256 excepted, where four times the
reference's own error may be the larger arm); and the record of why the statistics producers sum in double."""
import numpy as np
import pytest
import torch

from oracle import unet_oracle as U
from tests import _norm_offset as NO
from tests._common import SMALL, max_rel, rel_err
from worddiffusion_amd.synthetic import synthetic_inputs, synthetic_tensor

ALL_GN = NO.GN_STATS_SHAPES + [NO.GN_FOLD_SHAPE] + NO.GN_PRODUCER_SHAPES


def _arm(tol, err):
    return "4 * ref_err" if 4.0 * err > tol else "path_tol"


@pytest.mark.parametrize("B,hw,c,cpg", ALL_GN)
def test_groupnorm_reference_is_inside_half_the_tolerance(B, hw, c, cpg):
    ga, be = NO.affine(c, c + hw)
    for silu in (0, 1):
        for r, kind in NO.rk_cases():
            x = NO.offset_input((B, hw), c, cpg, r, kind, seed=hw + c + r)
            _, err = NO.gn_ref_err(x, B, hw, cpg, ga, be, 1e-5, silu)
            print(f"gn ({B},{hw},{c},{cpg}) silu={silu} r={r} {kind}: ref_err {err:.2e} bound {NO.bound(NO.TOL_PLANES, err):.2e} "
                  f"arm {_arm(NO.TOL_PLANES, err)}")
            if r < 256:
                assert err <= NO.TOL_PLANES / 2
            else:
                assert err <= 2 * NO.TOL_PLANES  # (the bound stays the same order as the tolerance: the ladder ends here)


@pytest.mark.parametrize("rows,c", NO.LN_SHAPES)
def test_layernorm_reference_is_inside_half_the_tolerance(rows, c):
    ga, be = NO.affine(c, c + rows)
    for r in (0, 256):
        x = NO.offset_rows(rows, c, r, seed=rows + c + r)
        _, err = NO.ln_ref_err(x, ga, be, 1e-5)
        print(f"ln ({rows},{c}) r={r}: ref_err {err:.2e} bound {NO.bound(NO.TOL_PLANES, err):.2e} arm {_arm(NO.TOL_PLANES, err)}")
        if r < 256:
            assert err <= NO.TOL_PLANES / 2
        else:
            assert err <= 2 * NO.TOL_PLANES


@pytest.mark.parametrize("kind", NO.KINDS)
def test_offset_input_has_the_stated_moments(kind):
    B, hw, c, cpg, r = 3, 40, 64, 2, 64
    x = NO.offset_input((B, hw), c, cpg, r, kind, seed=5).double().reshape(B, hw, c // cpg, cpg)
    mean, std = x.mean(dim=(1, 3)), x.std(dim=(1, 3), unbiased=False)
    assert float((std - 1).abs().max()) < 1e-5
    want = NO.group_means(B, c // cpg, r, kind, 5)
    assert float((mean - want).abs().max()) < 1e-4
    if kind == "mixed":
        assert set(want.flatten().tolist()) == {-64.0, 0.0, 64.0}


def test_fp32_partials_breach_the_tolerance_and_exact_sums_do_not():
    """The finding: with per-thread fp32 accumulation of v and v * v (wd_gn_stats before the producers went to double) GroupNorm
    at mean / std = 64, (hw 64, c 64, cpg 2), is outside the 3e-5 planes tolerance; with the two sums exact and the same apply
    arithmetic it is inside, next to torch's own fp32 result."""
    B, hw, c, cpg, r = 1, 64, 64, 2, 64
    ga, be = NO.affine(c, 1)
    x = NO.offset_input((B, hw), c, cpg, r, "same", seed=11)
    ref, ref_err = NO.gn_ref_err(x, B, hw, cpg, ga, be, 1e-5, 0)
    e32 = max_rel(NO.emulate_gn(x.numpy(), B, hw, cpg, ga.numpy(), be.numpy(), 1e-5, exact=False), ref)
    e64 = max_rel(NO.emulate_gn(x.numpy(), B, hw, cpg, ga.numpy(), be.numpy(), 1e-5, exact=True), ref)
    print(f"r=64 (1,64,64,2): fp32 partials {e32:.2e}, exact sums {e64:.2e}, torch fp32 {ref_err:.2e}")
    assert e32 > NO.TOL_PLANES
    assert e64 <= NO.bound(NO.TOL_PLANES, ref_err) and e64 < NO.TOL_PLANES / 2
    # the ladder: the loss grows like r^2 with fp32 partials and not at all with exact ones
    x0 = NO.offset_input((B, hw), c, cpg, 0, "same", seed=11)
    ref0 = NO.gn_ref(x0, B, hw, cpg, ga, be, 1e-5, 0)
    assert max_rel(NO.emulate_gn(x0.numpy(), B, hw, cpg, ga.numpy(), be.numpy(), 1e-5, exact=False), ref0) < 1e-6


def test_offset_model_fp32_oracle_is_inside_a_quarter_of_the_contract():
    """The model-level case of the GPU file: SMALL base UNet, every GroupNorm-feeding convolution bias + 16 std of its output.  The
    fp32 oracle stays inside 2.5e-5 of the fp64 one, so the 1e-4 end-to-end bound is four times the reference's own error."""
    cfg = SMALL
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, 7)) for k, s in U.state_dict_shapes(cfg, "base")}
    inp = synthetic_inputs(2, seed=3, hw=(4, 8), num_classes=cfg["num_classes"])
    sd_off, hit = NO.offset_model_state(U, cfg, sd, "base", inp)
    assert len(hit) >= 8
    with torch.no_grad():
        o32 = U.UNetOracle(cfg, sd_off, "base")(inp["x"], inp["t"], inp["context"], inp["y"])
        o64 = U.UNetOracle(cfg, {k: v.double() for k, v in sd_off.items()}, "base")(inp["x"], inp["t"], inp["context"], inp["y"])
    err = rel_err(o32, o64)
    print(f"offset model: {len(hit)} biases moved, fp32 oracle vs fp64 rel_err {err:.2e}")
    assert o64.dtype == torch.float64 and err <= 2.5e-5
