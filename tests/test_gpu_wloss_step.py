"""The weighted training loss through ``TrainStep`` and ``Diffusion.eval_loss``: FULL base UNet, B = 3, [4, 8, 16] latents (the
smallest training shape test_gpu_training.py runs), explicit t and noise, AdamW at lr 0 so the weights stay those the reference sees.

The reference is ``oracle.unet_oracle`` in float64 under autograd with the weighted loss written in torch; the bars are those of
test_gpu_training.py: per parameter ||g - ref|| < 2e-4 ||ref|| + 1e-7, the loss and every per-sample loss to 1e-5 relative."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ddpm_oracle as D  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402
from tests._common import FULL, make_args  # noqa: E402
from tests._wloss_ref import ulp_distance  # noqa: E402
from tests._train_ref import case_inputs, train_model  # noqa: E402
from worddiffusion_amd import Diffusion  # noqa: E402
from worddiffusion_amd.latents import loss_mask_columns  # noqa: E402
from worddiffusion_amd.optim import FusedAdamW, weighted_mse_loss  # noqa: E402
from worddiffusion_amd.synthetic import synthetic_tensor  # noqa: E402
from worddiffusion_amd.training import TrainStep  # noqa: E402

DEV = "cuda:0"
B, HW, T, BINS = 3, (8, 16), 1000, 20
SEEDS = (55, 103, 3)
TS = torch.tensor([5, 400, 990])  # SNR far above gamma (weight ~ 4e-3), above it, below it (weight 1): bins 0, 8 and 19 of 20


def diffusion():
    return Diffusion(noise_steps=T, img_size=(64, 128), args=make_args(device=DEV))


def soft_mask():
    """[B, 1, h, w] in [0, 1]: a ramp; the dataset's mask of a 40 px word with the padding at 1/4; and a nearly empty sample, the
    dataset's mask of a one-letter word (8 px: one latent column) with the padding at 0.

    The gradient bar's floor of 1e-7 is absolute: it was set for the plain loss, whose d loss / d pred has the scale 2 / (B n).
    A masked sample's row has the scale 2 w_b / (B M_b) instead, so the emptier the mask, the larger the whole backward pass and
    with it the rounding noise on the gradients that are analytically zero (the key biases of the attention layers).  One kept
    column (M_b = 32 of n = 512) keeps ||d loss / d pred|| within about three times the plain loss's at this shape, where that
    floor still means what it meant; a mask of a single cell would multiply it by ten and measure the floor, not the kernels."""
    h, w = HW
    m = torch.zeros(B, 1, h, w)
    m[0, 0] = torch.linspace(0.05, 1.0, h * w).reshape(h, w)
    m[1] = loss_mask_columns(40, h, w, 0.25)
    m[2] = loss_mask_columns(8, h, w, 0.0)
    return m


def other_mask():
    g = torch.Generator().manual_seed(9)
    return torch.rand(HW, generator=g)


def inputs():
    x0, inp, eps = case_inputs(FULL, B, HW, 0, SEEDS)
    return x0, inp, eps


@functools.lru_cache(maxsize=1)
def reference64():
    """float64 oracle forward of x_t -> L = mean_b w_b sum m (pred - eps)^2 / sum m -> autograd: (L, per-sample means, grads)."""
    x0, inp, eps = inputs()
    x_t = D.noise_images(D.schedule(T)[2], x0, TS, eps)
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, SEEDS[0])).double().requires_grad_(True)
          for k, s in U.state_dict_shapes(FULL, "base")}
    pred = U.UNetOracle(FULL, sd, "base", False)(x_t.double(), TS, inp["context"], inp["y"], None)
    m = soft_mask().double().expand(B, 4, *HW)
    per = (m * (pred - eps.double()) ** 2).sum((1, 2, 3)) / m.sum((1, 2, 3))
    w = Diffusion(noise_steps=T).min_snr_weights(5.0).double()[TS]
    loss = (w * per).mean()
    loss.backward()
    return float(loss.detach()), per.detach().numpy(), {k: v.grad for k, v in sd.items() if v.grad is not None}


class Recorder:
    """Stands in for ``TrainStep.lib``: the entry points the step's own body calls, by name (the forward and backward lists hold
    their functions themselves: ``P.step`` / ``P.bwd``, as tools/step_ops.py reads them)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def make_step(record=False, **kw):
    m = train_model(FULL, "base", False, SEEDS[0])
    step = TrainStep(m, diffusion(), FusedAdamW(m.parameters(), lr=0.0), seed=99, **kw)
    if record:
        step.lib = Recorder(step.lib)
    return m, step


def call(step, loss_mask=None):
    """One step on the fixed batch -> (loss bits as a tensor, {name: gradient clone}, per-sample losses or None)."""
    x0, inp, eps = inputs()
    kw = {} if loss_mask is None else dict(loss_mask=loss_mask)
    loss = step(x0.to(DEV), inp["context"].to(DEV), inp["y"].to(DEV), t=TS, noise=eps.to(DEV), **kw).clone()
    torch.cuda.synchronize()
    sl = step._sample_loss.clone() if step._sample_loss is not None else None
    return loss.cpu(), {k: g.clone() for k, g in step.eng.grads().items()}, sl


def same_bits(a, b, what):
    assert torch.equal(a[0], b[0]), f"{what}: the loss differs"
    assert set(a[1]) == set(b[1])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), f"{what}: gradient {k} differs"
    if a[2] is not None and b[2] is not None:
        assert torch.equal(a[2], b[2]), f"{what}: the per-sample losses differ"


# ------------------------------------------------------------------------------------------------------------- G5
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_weighted_masked_step_against_the_float64_reference(use_graph):
    loss_ref, per_ref, gref = reference64()
    m, step = make_step(loss_weights="min_snr", loss_bins=BINS, use_graph=use_graph)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    mask = soft_mask()
    first = call(step, mask)
    assert (step._mgraph is not None) == use_graph and step._graph is None
    loss = float(first[0])
    print(f"loss {loss!r} reference {loss_ref!r}")
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref), (loss, loss_ref)
    sl = step.last_sample_losses.cpu().double().numpy()
    print(f"per-sample losses {sl} reference {per_ref}")
    assert np.all(np.abs(sl - per_ref) <= 1e-5 * np.abs(per_ref)), (sl, per_ref)
    assert set(first[1]) == set(gref), sorted(set(first[1]) ^ set(gref))[:10]
    bad, worst = [], 0.0
    for k, r in gref.items():
        g = first[1][k].cpu().double()
        err, rn = float((g - r).norm()), float(r.norm())
        worst = max(worst, err / rn) if rn > 1e-6 else worst
        if not err < 2e-4 * rn + 1e-7:
            bad.append((k, err, rn))
    print(f"worst relative gradient error {worst:.2e}")
    assert not bad, f"{len(bad)} gradients off the reference: {bad[:8]}"
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k}: lr = 0 moved the parameter"
    same_bits(first, call(step, mask), "a replayed step")
    h = step.loss_by_timestep()
    assert h["edges"].tolist() == list(range(0, T + 1, T // BINS)) and h["count"].dtype == np.int64
    bins = [int(t) * BINS // T for t in TS]
    assert h["count"].tolist() == [2 if k in bins else 0 for k in range(BINS)]
    for b, k in enumerate(bins):  # (l + l) / 2 is exact
        assert h["mean"][k] == np.float64(step.last_sample_losses.cpu().numpy()[b])
    assert np.isnan(h["mean"][[k for k in range(BINS) if k not in bins]]).all()
    step.reset_loss_by_timestep()
    assert not step.loss_by_timestep()["count"].any()


# ------------------------------------------------------------------------------------------------------------- G6
@functools.lru_cache(maxsize=1)
def default_run():
    _, step = make_step(record=True)
    out = call(step)
    return out, list(step.lib.calls), step


def test_a_default_step_is_todays():
    """Built with no new argument: ``wd_mse_loss`` and not the new entry point, nothing of the weighted path allocated, and the
    same bits as a second default step on a fresh identical model."""
    out, calls, step = default_run()
    assert "wd_mse_loss" in calls and "wd_weighted_mse_loss" not in calls, calls
    listed = [fn.__name__ for fn, _, _ in step._P.step] + [fn.__name__ for fn, _, _ in step._P.bwd]
    assert "wd_weighted_mse_loss" not in listed
    assert step._graph is not None and step._mgraph is None
    assert all(getattr(step, a) is None for a in ("_wtab", "_hist", "_sample_loss", "_wscratch", "_mask"))
    with pytest.raises(RuntimeError):
        step.last_sample_losses
    with pytest.raises(RuntimeError):
        step.loss_by_timestep()
    _, again = make_step()
    same_bits(out, call(again), "a second default step")


def test_unit_weights_give_the_default_steps_gradients():
    """``loss_weights = ones``: the new entry point runs (the recorder shows it) and, c_b being wd_mse_loss's scale, every gradient
    is the default step's bit for bit; the loss within 4 fp32 ulp (test_gpu_wloss.py, G4)."""
    out, _, _ = default_run()
    _, step = make_step(record=True, loss_weights=torch.ones(T))
    got = call(step)
    assert "wd_weighted_mse_loss" in step.lib.calls and "wd_mse_loss" not in step.lib.calls, step.lib.calls
    same_bits((out[0], out[1], None), (out[0], got[1], None), "unit weights")
    assert int(ulp_distance(got[0].numpy(), out[0].numpy()).max()) <= 4


def test_a_host_timestep_out_of_range_is_refused():
    _, _, step = default_run()
    x0, inp, eps = inputs()
    with pytest.raises(ValueError):
        step(x0.to(DEV), inp["context"].to(DEV), inp["y"].to(DEV), t=torch.tensor([5, 400, T]), noise=eps.to(DEV))
    with pytest.raises(ValueError):
        step(x0.to(DEV), inp["context"].to(DEV), inp["y"].to(DEV), t=TS, noise=eps.to(DEV), loss_mask=torch.full(HW, 1.5))


# ------------------------------------------------------------------------------------------------------------- G7
def test_alternating_masked_and_unmasked_calls():
    """m, u, m, u on one step (the second masked call with another mask): each result is, bit for bit, that of the same call on a
    step that only ever saw that variant; both captured bodies are kept."""
    kw = dict(loss_weights="min_snr", loss_bins=BINS)
    m1, m2 = soft_mask(), other_mask()
    _, only_m = make_step(**kw)
    want_m = [call(only_m, m1), call(only_m, m2)]
    _, only_u = make_step(**kw)
    want_u = [call(only_u), call(only_u)]
    assert only_m._graph is None and only_u._mgraph is None
    _, step = make_step(**kw)
    got = [call(step, m1), call(step), call(step, m2), call(step)]
    assert step._graph is not None and step._mgraph is not None
    same_bits(got[0], want_m[0], "masked call 1")
    same_bits(got[1], want_u[0], "unmasked call 1")
    same_bits(got[2], want_m[1], "masked call 2")
    same_bits(got[3], want_u[1], "unmasked call 2")
    assert not torch.equal(got[0][2], got[2][2]), "the second mask did not reach the step's buffer"
    assert step.loss_by_timestep()["count"].sum() == 4 * B


# ------------------------------------------------------------------------------------------------------------- G8
def test_eval_loss_is_the_eval_forward_and_leaves_the_model_alone():
    x0, inp, eps = inputs()
    m = train_model(FULL, "base", False, SEEDS[0])
    diff = diffusion()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    args = (x0.to(DEV), inp["context"].to(DEV), inp["y"].to(DEV))
    mask = soft_mask()
    got = diff.eval_loss(m, *args, TS, noise=eps.to(DEV), loss_mask=mask)
    assert m.training and all(mod.training for mod in m.modules()), "the training flags were not put back"
    assert tuple(got.shape) == (B,) and got.is_cuda and bool(torch.isfinite(got).all())
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed"
    assert all(p.grad is None for p in m.parameters())
    x_t, _ = diff.noise_images(args[0], TS, eps=eps.to(DEV))
    m.eval()
    with torch.no_grad():
        pred = m(x_t, timesteps=TS.to(DEV), context=args[1], y=args[2])
    want = weighted_mse_loss(pred, eps.to(DEV), mask=mask, want_grad=False)[2]
    assert torch.equal(got, want)
    # without a mask and without noise: seeded, so two calls agree, and another seed draws other noise
    a, b = diff.eval_loss(m, *args, TS, seed=4), diff.eval_loss(m, *args, TS, seed=4)
    assert torch.equal(a, b) and not torch.equal(a, diff.eval_loss(m, *args, TS, seed=5))
    assert not m.training
