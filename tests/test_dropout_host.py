"""Host side of the training dropout: the public helpers of ``worddiffusion_amd.dropout`` against the formulas of the
specification, the layer numbering against the reference's state_dict layout, and the mask reference itself (tests/_dropout_ref.py,
which the GPU tests hold the kernels to) on the properties a dropout mask must have."""
import numpy as np
import pytest

from oracle import unet_oracle as U
from tests import _dropout_ref as R
from tests._common import FULL, SMALL, make_args
from worddiffusion_amd import UNetModel, UNetModelPhosc
from worddiffusion_amd import dropout as DO

KEY = "out_layers.3.weight"


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.999])
def test_threshold_scale_tag(p):
    assert DO.threshold(p) == int(p * 2.0 ** 32 + 0.5) == R.threshold(p)
    assert 0 <= DO.threshold(p) < 2 ** 32
    s = DO.scale(p)
    assert isinstance(s, np.float32) and s == np.float32(1.0 / (1.0 - p)) == R.scale(p)
    for layer in (0, 5, 41):
        assert DO.tag(layer) == 0x80000000 | (0x100 + layer) == R.tag(layer)


@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5])
def test_helpers_refuse_p_outside_the_half_open_interval(p):
    with pytest.raises(ValueError):
        DO.threshold(p)
    with pytest.raises(ValueError):
        DO.scale(p)


@pytest.mark.parametrize("variant", ["base", "phosc"])
def test_layer_ids_follow_the_state_dict_order(variant):
    cls = UNetModel if variant == "base" else UNetModelPhosc
    m = cls(args=make_args(), **FULL)
    want = [k[: -len(KEY)] for k, _ in U.state_dict_shapes(FULL, variant) if k.endswith(KEY)]
    assert len(want) >= 5  # two encoder blocks, two middle, the decoder
    ids = DO.layer_ids(m)
    assert ids == {prefix: i for i, prefix in enumerate(want)}
    if variant == "base":
        assert "res." in ids  # the dead block takes a number (and never runs)


def test_p_outside_the_interval_raises_at_plan_request():
    """nn.Dropout accepts p = 1, so the model constructs; the training plan refuses it before any device work."""
    m = UNetModel(args=make_args(), **SMALL, dropout=1.0).train()
    with pytest.raises(ValueError):
        m.train_engine.plan_train(2, 8, 16, 10)
    with pytest.raises(ValueError):  # nn.Dropout's own check: p outside [0, 1] never constructs
        UNetModel(args=make_args(), **SMALL, dropout=-0.1)


@pytest.mark.parametrize("p,share", [(0.1, 0.900047), (0.5, 0.500003)])
def test_mask_keeps_the_expected_share(p, share):
    """seed 1234, layer 5, rows 7..10 of a 1024 x 320 map (1,310,720 elements): the kept share lies within 1.05e-3 of 1 - p - four
    standard deviations of a binomial share at p = 0.1, sqrt(0.1 * 0.9 / n) = 2.62e-4 each, 2.4 at p = 0.5 - and is the value recorded
    when the specification was written."""
    keep = R.keep_mask(1234, 7, 4, 1024, 320, 5, p)
    assert keep.shape == (4, 1024, 320) and keep.dtype == np.bool_
    got = float(keep.mean())
    print(f"p = {p}: kept share {got:.6f}")
    assert abs(got - (1.0 - p)) < 1.05e-3
    assert abs(got - share) < 5e-7


def test_rows_do_not_depend_on_batching():
    a = R.keep_mask(1234, 7, 4, 64, 64, 5, 0.3)
    b = R.keep_mask(1234, 9, 2, 64, 64, 5, 0.3)
    assert np.array_equal(a[2:], b)
    assert not np.array_equal(a[0], a[1])
    assert not np.array_equal(a, R.keep_mask(1234, 7, 4, 64, 64, 6, 0.3))  # another layer, another mask
    assert not np.array_equal(a, R.keep_mask(1235, 7, 4, 64, 64, 5, 0.3))  # another seed
