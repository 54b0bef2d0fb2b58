"""wd_weighted_mse_loss on the GPU against tests/_wloss_ref.py (itself held to float64 autograd by test_wloss_ref_host.py).

Every fp32 / fp64 operand is a window of a poisoned buffer (tests/_guard.py): a store outside a window or a read outside one shows.
Masks take values k/256, so M_b is exact in double whatever the order of the sum, hence c_b and the whole gradient are exact and
compared by their bits; S_b is a sum of non-negative doubles, good to n * 2^-53 before its one rounding, so the losses are held to
one fp32 ulp; the histogram is the specification's recurrence applied to the device's own per-sample losses, bit for bit."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _wloss_ref as R  # noqa: E402
from tests._guard import assert_finite, assert_untouched, guarded_flat  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402

DEV = "cuda:0"
T = 1000
SHAPES = [(1, 4), (3, 1028), (65, 1024), (257, 8)]


@functools.lru_cache(maxsize=None)
def case(B, n, masked, weighted, live_single=False):
    """Host inputs and the specification's outputs (without a histogram: that is applied to the device's sample losses)."""
    rs = np.random.RandomState(1000 * B + n + 2 * masked + weighted)
    p = rs.standard_normal((B, n)).astype(np.float32)
    e = (0.5 * rs.standard_normal((B, n)) + 0.25).astype(np.float32)
    m = None
    if masked:
        m = (rs.randint(0, 257, (B, n)) / 256.0).astype(np.float32)
        m[rs.rand(B, n) < 0.3] = 0.0
        if not live_single:
            m[B - 1] = 0.0  # one row without a single cell
    t = rs.randint(0, T, B).astype(np.int64)
    if B >= 3:
        t[0], t[1], t[2] = 0, T - 1, T - 1
    else:
        t[0] = T - 1 if masked else 0
    w = None
    if weighted:
        w = rs.uniform(0.0, 2.0, T).astype(np.float32)
        w[0] = 0.0  # the sample at t = 0 weighs nothing (and is still counted)
    ref = R.weighted_mse(p, e, m, t, w)
    return p, e, m, t, w, ref


class Launch:
    """The operands of one call in guarded windows on the device."""

    def __init__(self, p, e, m, t, w, nbins, need_t, hist0=None):
        B, n = p.shape
        self.B, self.n, self.nbins = B, n, nbins
        self.bufs = {}

        def put(name, n_el, dtype, value=None):
            buf, view = guarded_flat(n_el, dtype, device=DEV)
            if value is not None:
                view.copy_(torch.as_tensor(value).reshape(-1))
            self.bufs[name] = (buf, view)
            return view

        self.pred, self.target = put("pred", B * n, torch.float32, p), put("target", B * n, torch.float32, e)
        self.mask = put("mask", B * n, torch.float32, m) if m is not None else None
        self.weights = put("weights", T, torch.float32, w) if w is not None else None
        self.t = torch.as_tensor(t).to(DEV) if need_t else None
        self.grad, self.loss = put("grad", B * n, torch.float32), put("loss", 1, torch.float32)
        self.sample_loss, self.scratch = put("sample_loss", B, torch.float32), put("scratch", 2 * B, torch.float64)
        self.hist = put("hist", 2 * nbins, torch.float64, hist0) if nbins else None

    def args(self, **over):
        ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
        a = dict(pred=ptr(self.pred), target=ptr(self.target), mask=ptr(self.mask), batch=self.B, n_per_sample=self.n, t=ptr(self.t),
                 weights=ptr(self.weights), T=T, grad=ptr(self.grad), loss=ptr(self.loss), sample_loss=ptr(self.sample_loss),
                 hist=ptr(self.hist), nbins=self.nbins, scratch=ptr(self.scratch))
        a.update(over)
        return list(a.values())

    def run(self, **over):
        rc = N.lib().wd_weighted_mse_loss(*self.args(**over), torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize()
        return rc

    def bits(self):
        return {k: buf.clone().view(torch.int32).cpu() for k, (buf, _) in self.bufs.items()}

    def check_guards(self, outputs=("grad", "loss", "sample_loss", "scratch", "hist")):
        for name, (buf, view) in self.bufs.items():
            assert_untouched(buf, view, name)
            if name in outputs:
                assert_finite(view, name)


def hist0_of(nbins):
    """A histogram that already holds something: the launch adds to it."""
    rs = np.random.RandomState(nbins)
    return np.stack([rs.uniform(0.0, 3.0, nbins), rs.randint(0, 5, nbins).astype(np.float64)], 1)


def check_outputs(L, ref, t, hist_before, launches=1):
    B, n = L.B, L.n
    grad = L.grad.cpu().numpy().reshape(B, n)
    assert np.array_equal(grad.view(np.int32), ref["grad"].view(np.int32)), \
        f"grad differs from the specification in {int((grad.view(np.int32) != ref['grad'].view(np.int32)).sum())} element(s)"
    sl = L.sample_loss.cpu().numpy()
    loss = L.loss.cpu().numpy()
    assert int(R.ulp_distance(sl, ref["sample_loss"]).max()) <= 1, "sample_loss more than 1 ulp off"
    assert int(R.ulp_distance(loss, ref["loss"]).max()) <= 1, (float(loss[0]), float(ref["loss"]))
    dead = ~ref["live"]
    assert not grad[dead].any() and not sl[dead].any()
    if L.hist is not None:
        want = np.array(hist_before, np.float64)
        for _ in range(launches):
            want = R.hist_update(want, sl, ref["live"], t, T)
        got = L.hist.cpu().numpy().reshape(-1, 2)
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), (got, want)
        assert got[:, 1].sum() - np.asarray(hist_before)[:, 1].sum() == launches * int(ref["live"].sum())


# ------------------------------------------------------------------------------------------------------------- G1
@pytest.mark.parametrize("nbins", [0, 1, 7])
@pytest.mark.parametrize("weighted", [False, True], ids=["w1", "weights"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("B,n", SHAPES)
def test_against_the_specification(B, n, masked, weighted, nbins):
    p, e, m, t, w, ref = case(B, n, masked, weighted)
    h0 = hist0_of(nbins) if nbins else None
    L = Launch(p, e, m, t, w, nbins, need_t=weighted or nbins > 0, hist0=h0)
    assert L.run() == N.WD_OK
    L.check_guards()
    check_outputs(L, ref, t, h0)
    if masked:
        assert not ref["live"][B - 1] and int(ref["live"].sum()) == B - 1


def test_single_sample_with_a_live_mask():
    """(1, 4) masked, the row alive (the case above has its only row empty)."""
    p, e, m, t, w, ref = case(1, 4, True, True, live_single=True)
    m = m.copy()
    m[0, 1] = 0.5  # (whatever the draw left: at least one cell counts)
    ref = R.weighted_mse(p, e, m, t, w)
    assert ref["live"][0]
    h0 = hist0_of(7)
    L = Launch(p, e, m, t, w, 7, need_t=True, hist0=h0)
    assert L.run() == N.WD_OK
    L.check_guards()
    check_outputs(L, ref, t, h0)


def test_optional_outputs_may_be_null():
    """grad, sample_loss and hist are optional: the loss is the same without them."""
    p, e, m, t, w, ref = case(3, 1028, True, True)
    L = Launch(p, e, m, t, w, 0, need_t=True)
    before = L.bits()
    assert L.run(grad=None, sample_loss=None) == N.WD_OK
    after = L.bits()
    assert torch.equal(before["grad"], after["grad"]) and torch.equal(before["sample_loss"], after["sample_loss"])
    L.check_guards(outputs=("loss", "scratch"))
    assert int(R.ulp_distance(L.loss.cpu().numpy(), ref["loss"]).max()) <= 1


# ------------------------------------------------------------------------------------------------------------- G2
@pytest.mark.parametrize("B,n", [(65, 1024), (257, 8)])
def test_two_launches_give_the_same_bits_and_the_histogram_accumulates(B, n):
    p, e, m, t, w, ref = case(B, n, True, True)
    h0 = hist0_of(7)
    L = Launch(p, e, m, t, w, 7, need_t=True, hist0=h0)
    assert L.run() == N.WD_OK
    first = L.bits()
    check_outputs(L, ref, t, h0, launches=1)
    L.grad.fill_(float("nan"))
    L.sample_loss.fill_(float("nan"))
    L.loss.fill_(float("nan"))
    assert L.run() == N.WD_OK
    second = L.bits()
    for name in ("grad", "loss", "sample_loss", "scratch"):
        assert torch.equal(first[name], second[name]), f"{name}: the second launch gave other bits"
    L.check_guards()
    check_outputs(L, ref, t, h0, launches=2)


# ------------------------------------------------------------------------------------------------------------- G3
def test_invalid_arguments_launch_nothing():
    p, e, m, t, w, _ = case(3, 1028, True, True)
    L = Launch(p, e, m, t, w, 7, need_t=True, hist0=hist0_of(7))
    before = L.bits()
    bad = dict(
        pred_null=dict(pred=None), target_null=dict(target=None), loss_null=dict(loss=None), scratch_null=dict(scratch=None),
        t_null_with_weights=dict(t=None, hist=None, nbins=0), t_null_with_hist=dict(t=None, weights=None),
        batch_0=dict(batch=0), batch_negative=dict(batch=-1), n_0=dict(n_per_sample=0), n_2=dict(n_per_sample=2),
        n_not_multiple_of_4=dict(n_per_sample=1026),
        T_0_with_weights=dict(T=0, hist=None, nbins=0), T_0_with_hist=dict(T=0, weights=None),
        nbins_0_with_hist=dict(nbins=0), nbins_negative_with_hist=dict(nbins=-3),
        pred_misaligned=dict(pred=L.pred.data_ptr() + 4), target_misaligned=dict(target=L.target.data_ptr() + 8),
        mask_misaligned=dict(mask=L.mask.data_ptr() + 4), grad_misaligned=dict(grad=L.grad.data_ptr() + 12),
    )
    for name, over in bad.items():
        assert L.run(**over) == N.WD_EINVAL, name
    after = L.bits()
    for name in before:
        assert torch.equal(before[name], after[name]), f"{name} changed although every call was refused"
    assert L.run() == N.WD_OK  # (the operands themselves are fine)


# ------------------------------------------------------------------------------------------------------------- G4
@pytest.mark.parametrize("B,n", [(1, 4), (3, 1028), (65, 1024)])
def test_unweighted_unmasked_gradient_is_wd_mse_loss_s(B, n):
    """weights = NULL, mask = NULL: c_b = (float)(2 / (B n)) is wd_mse_loss's scale, so the gradients agree bit for bit; the old
    kernel squares in fp32 (half an ulp per term), so the two double sums agree to 2^-24 before the last rounding: 4 ulp."""
    from worddiffusion_amd.optim import mse_loss
    p, e, _, t, _, _ = case(B, n, False, False)
    L = Launch(p, e, None, t, None, 0, need_t=False)
    assert L.run() == N.WD_OK
    L.check_guards()
    old_loss, old_grad = mse_loss(L.pred.reshape(B, n).clone(), L.target.reshape(B, n).clone())
    torch.cuda.synchronize()
    assert torch.equal(L.grad.reshape(B, n).view(torch.int32), old_grad.view(torch.int32))
    assert int(R.ulp_distance(L.loss.cpu().numpy(), old_loss.cpu().numpy()).max()) <= 4
