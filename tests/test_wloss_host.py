"""The host side of the weighted training loss: ``Diffusion.min_snr_weights``, the argument validation of ``TrainStep`` and
``optim.weighted_mse_loss`` that happens before anything touches a device, and the loss-mask columns of ``CachedLatentDataset``.
No GPU."""
import math

import numpy as np
import pytest
import torch

from worddiffusion_amd import Diffusion
from worddiffusion_amd import latents as L
from worddiffusion_amd import optim as O
from worddiffusion_amd.training import TrainStep


# ------------------------------------------------------------------------------------------------------ min_snr_weights
def _snr64(diff):
    ah = np.cumprod(1.0 - diff.beta.detach().cpu().numpy().astype(np.float64))
    return ah / (1.0 - ah)


@pytest.mark.parametrize("T,gamma", [(1000, 5.0), (1000, 1.0), (600, 5.0), (1000, 0.03)])
def test_min_snr_weights_are_the_float64_formula_rounded_once(T, gamma):
    diff = Diffusion(noise_steps=T)
    w = diff.min_snr_weights(gamma)
    assert w.dtype == torch.float32 and tuple(w.shape) == (T,) and not w.is_cuda
    snr = _snr64(diff)
    want = np.minimum(snr, gamma) / snr
    got = w.numpy()
    ulp = np.spacing(want.astype(np.float32))
    assert np.all(np.abs(got.astype(np.float64) - want) <= ulp), "more than 1 fp32 ulp from min(SNR, gamma) / SNR"
    assert np.all(got[snr <= gamma] == 1.0), "the weight is exactly 1 wherever SNR <= gamma"
    assert np.any(snr <= gamma) and np.any(snr > gamma)
    order = np.argsort(snr, kind="stable")
    assert np.all(np.diff(got[order]) <= 0), "the weight does not increase with SNR"
    assert np.all(got > 0) and np.all(got <= 1)


def test_min_snr_weights_with_gamma_above_every_snr_are_ones():
    diff = Diffusion(noise_steps=1000)
    snr0 = float(_snr64(diff)[0])
    assert torch.equal(diff.min_snr_weights(2.0 * snr0), torch.ones(1000))
    assert float(diff.min_snr_weights(0.5 * snr0)[0]) < 1.0


@pytest.mark.parametrize("gamma", [0.0, -1.0, float("nan"), float("inf")])
def test_min_snr_weights_reject_a_bad_gamma(gamma):
    with pytest.raises(ValueError):
        Diffusion().min_snr_weights(gamma)


# ------------------------------------------------------------------------------------------------------ TrainStep arguments
@pytest.mark.parametrize("kw", [
    dict(loss_weights="snr"),
    dict(loss_weights=torch.ones(999)),
    dict(loss_weights=torch.ones(1000, dtype=torch.int64)),
    dict(loss_weights=torch.full((1000,), float("nan"))),
    dict(loss_weights=torch.cat([torch.ones(999), torch.tensor([float("inf")])])),
    dict(loss_weights=torch.cat([torch.ones(999), torch.tensor([-1e-3])])),
    dict(loss_weights="min_snr", snr_gamma=0.0),
    dict(loss_weights="min_snr", snr_gamma=float("nan")),
    dict(loss_bins=-1),
    dict(loss_bins=2.5),
    dict(loss_bins=True),
])
def test_train_step_rejects_bad_loss_arguments_before_it_touches_the_model(kw):
    with pytest.raises(ValueError):
        TrainStep(None, Diffusion(noise_steps=1000), None, **kw)


# ------------------------------------------------------------------------------------------------------ weighted_mse_loss arguments
def test_weighted_mse_loss_validates_on_the_host_and_has_no_cpu_path():
    p, e = torch.zeros(2, 4, 2, 4), torch.zeros(2, 4, 2, 4)
    ok_t, ok_w = torch.tensor([0, 9]), torch.ones(10)
    bad = [
        dict(weights=ok_w),                                   # weights without t
        dict(weights=ok_w, t=torch.tensor([0, 10])),          # t outside [0, T)
        dict(weights=ok_w, t=torch.tensor([-1, 3])),
        dict(weights=ok_w, t=torch.tensor([0, 1, 2])),        # not [B]
        dict(weights=ok_w, t=torch.tensor([0.0, 1.0])),       # not integers
        dict(weights=-ok_w, t=ok_t),                          # negative weights
        dict(weights=ok_w * float("nan"), t=ok_t),
        dict(weights=ok_w.reshape(2, 5), t=ok_t),
        dict(mask=torch.ones(4, 2)),                          # none of [h, w], [B, 1, h, w], [B, C, h, w]
        dict(mask=torch.ones(1, 1, 2, 4)),
        dict(mask=torch.ones(2, 4, dtype=torch.int64)),
        dict(mask=torch.full((2, 4), 1.5)),                   # outside [0, 1]
        dict(mask=torch.full((2, 4), -0.5)),
        dict(mask=torch.full((2, 4), float("nan"))),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            O.weighted_mse_loss(p, e, **kw)
    with pytest.raises(ValueError):
        O.weighted_mse_loss(p, torch.zeros(2, 4, 2, 2))       # shapes differ
    with pytest.raises(ValueError):
        O.weighted_mse_loss(torch.zeros(2, 6), torch.zeros(2, 6))  # 6 elements per sample: not a multiple of 4
    with pytest.raises(ValueError):
        O.weighted_mse_loss(torch.zeros(2, 8), torch.zeros(2, 8), mask=torch.ones(8))  # flat rows take a mask of their own shape only
    from worddiffusion_amd._native import NativeError
    with pytest.raises(NativeError):
        O.weighted_mse_loss(p, e, t=ok_t, weights=ok_w, mask=torch.ones(2, 4))  # valid, but on the host: there is no fallback


def test_expand_loss_mask_follows_the_known_region_shapes():
    shape = (3, 4, 2, 8)
    hw = torch.arange(16, dtype=torch.float32).reshape(2, 8) / 16
    per = torch.rand(3, 1, 2, 8, generator=torch.Generator().manual_seed(0))
    full = torch.rand(shape, generator=torch.Generator().manual_seed(1))
    assert torch.equal(O.expand_loss_mask(hw, shape), hw.expand(shape).reshape(3, -1))
    assert torch.equal(O.expand_loss_mask(per, shape), per.expand(shape).reshape(3, -1))
    assert torch.equal(O.expand_loss_mask(full, shape), full.reshape(3, -1))
    b = O.expand_loss_mask(hw > 0.4, shape)
    assert b.dtype == torch.float32 and set(b.unique().tolist()) == {0.0, 1.0}
    assert O.expand_loss_mask(hw, shape).is_contiguous()


def test_check_timesteps():
    assert O.check_timesteps(torch.tensor([0, 999]), 2, 1000) is not None
    for t in (torch.tensor([0, 1000]), torch.tensor([-1, 0]), torch.tensor([1]), torch.tensor([[0, 1]]), torch.tensor([True, False])):
        with pytest.raises(ValueError):
            O.check_timesteps(t, 2, 1000)


def test_eval_loss_validates_on_the_host():
    diff = Diffusion(noise_steps=1000, img_size=(16, 64))
    lat, words, y = torch.zeros(2, 4, 2, 8), torch.zeros(2, 10, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError):
        diff.eval_loss(None, lat, words, y, torch.tensor([0, 1000]))
    with pytest.raises(ValueError):
        diff.eval_loss(None, lat, words, y, torch.tensor([0, 1]), loss_mask=torch.full((2, 8), 2.0))
    with pytest.raises(ValueError):
        diff.eval_loss(None, lat[0], words, y, torch.tensor([0, 1]))


# ------------------------------------------------------------------------------------------------------ the dataset's loss mask
@pytest.mark.parametrize("width,cols", [(0, 0), (1, 1), (8, 1), (9, 2), (255, 32), (256, 32), (300, 32)])
def test_loss_mask_columns(width, cols):
    m = L.loss_mask_columns(width, 8, 32, 0.25)
    assert m.dtype == torch.float32 and tuple(m.shape) == (1, 8, 32)
    assert bool((m[..., :cols] == 1.0).all()) and bool((m[..., cols:] == 0.25).all())
    assert cols == min(math.ceil(width / 8), 32)


def test_loss_mask_columns_rejects_a_bad_width():
    for wd in (-1, 3.5, True):
        with pytest.raises(ValueError):
            L.loss_mask_columns(wd, 8, 32, 0.5)


def _dataset(tmp_path, **kw):
    names = ["a", "bb", "ccc", "dddd"]
    g = torch.Generator().manual_seed(0)
    path = L.save_latent_cache(str(tmp_path / "lat.npz"), {n + ".png": torch.randn(4, 8, 32, generator=g) for n in names})
    rows = [("w0", n, n.upper()) for n in names]
    return L.CachedLatentDataset(rows, {"w0": 0}, L.LatentCache(path), **kw), names


def test_dataset_needs_a_pad_weight_with_width_of(tmp_path):
    with pytest.raises(ValueError):
        _dataset(tmp_path, width_of=lambda name: 8)
    with pytest.raises(ValueError):
        _dataset(tmp_path, pad_weight=0.5)
    for pw in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            _dataset(tmp_path, width_of=lambda name: 8, pad_weight=pw)


@pytest.mark.parametrize("preload", [False, True])
def test_dataset_batches_carry_the_loss_mask(tmp_path, preload):
    widths = {"a.png": 1, "bb.png": 8, "ccc.png": 9, "dddd.png": 256}
    ds, names = _dataset(tmp_path, width_of=widths.__getitem__, pad_weight=0.125)
    if preload:
        assert ds.preload()
    plain, _ = _dataset(tmp_path)
    assert "loss_mask" not in plain[0] and "loss_mask" not in next(plain.batches(2, shuffle=False, pin=False))
    seen = 0
    for b in ds.batches(2, shuffle=True, seed=3, pin=False):
        m = b["loss_mask"]
        assert m.dtype == torch.float32 and tuple(m.shape) == (2, 1, 8, 32)
        for i, name in enumerate(b["image_names"]):
            cols = (widths[name] + 7) // 8
            assert torch.equal(m[i], L.loss_mask_columns(widths[name], 8, 32, 0.125))
            assert bool((m[i, 0, :, :cols] == 1).all()) and bool((m[i, 0, :, cols:] == 0.125).all())
            seen += 1
    assert seen == 4
    assert torch.equal(ds[2]["loss_mask"], L.loss_mask_columns(9, 8, 32, 0.125))
