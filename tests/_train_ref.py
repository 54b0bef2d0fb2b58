"""The float64 training reference the gradient tests share (tests/test_gpu_training.py, tests/test_gpu_shapes.py): one case's inputs,
the oracle's forward -> MSE -> autograd in float64 on the CPU, the comparison with its bars, and the model -> MSELoss -> backward
call of the HIP path.  Every function takes the model's config dict."""
import functools

import numpy as np
import torch

from oracle import ddpm_oracle as D
from oracle import unet_oracle as U
from tests._common import make_args, max_rel
from worddiffusion_amd import UNetModel, UNetModelPhosc
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs, synthetic_tensor

DEV = "cuda:0"


def case_inputs(cfg, B, hw, phosc_len, seeds, noised=False):
    """(model input x, synthetic_inputs batch, eps) for seeds = (model, inputs, eps).  noised: x = noise_images(x0, t, eps) in
    fp32, the first launch of TrainStep's graph (wd_noise_images, bit-identical to it: test_noise_images_and_ema_exact)."""
    inp = synthetic_inputs(B, seed=seeds[1], hw=hw, num_classes=cfg["num_classes"], phosc_len=phosc_len)
    eps = torch.from_numpy(np.random.RandomState(seeds[2]).standard_normal(tuple(inp["x"].shape)).astype(np.float32))
    x = inp["x"]
    if noised:
        x = D.noise_images(D.schedule(1000)[2], x, inp["t"], eps)
    return x, inp, eps


def reference64(cfg, variant, B, hw, phosc_len, seeds, noised=False):
    """float64 oracle forward -> MSE -> autograd: (pred, loss, {name: grad}) of the parameters the loss reaches.  (The last two
    results are kept: the config enters the key as its sorted items.)"""
    return _reference64(tuple(sorted(cfg.items())), variant, B, hw, phosc_len, seeds, noised)


@functools.lru_cache(maxsize=2)
def _reference64(cfg_items, variant, B, hw, phosc_len, seeds, noised):
    cfg = dict(cfg_items)
    x, inp, eps = case_inputs(cfg, B, hw, phosc_len, seeds, noised)
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seeds[0])).double().requires_grad_(True)
          for k, s in U.state_dict_shapes(cfg, variant)}
    orc = U.UNetOracle(cfg, sd, variant, phosc_len > 0)
    pred = orc(x.double(), inp["t"], inp["context"], inp["y"], inp.get("phosc"))
    loss = torch.nn.functional.mse_loss(pred, eps.double())
    loss.backward()
    return pred.detach(), float(loss.detach()), {k: v.grad for k, v in sd.items() if v.grad is not None}


def check_against_reference(pred, loss, grads, ref, label):
    """Per-sample prediction (max_rel < 5e-5), loss (1e-5 relative), the set of parameters with a gradient, every gradient."""
    pred_ref, loss_ref, gref = ref
    pred = pred.detach().cpu().double()
    assert pred.shape == pred_ref.shape
    worst_pred = max(max_rel(pred[b], pred_ref[b]) for b in range(pred.shape[0]))
    assert worst_pred < 5e-5, [b for b in range(pred.shape[0]) if max_rel(pred[b], pred_ref[b]) >= 5e-5]
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref), (loss, loss_ref)
    assert set(grads) == set(gref), sorted(set(grads) ^ set(gref))[:10]
    worst, bad = ("", 0.0), []
    for k, r in gref.items():
        g = grads[k].detach().cpu().double()
        assert tuple(g.shape) == tuple(r.shape), k
        err, rn = float((g - r).norm()), float(r.norm())
        if rn > 1e-6 and err / rn > worst[1]:
            worst = (k, err / rn)
        if not err < 2e-4 * rn + 1e-7:  # (a few gradients are analytically ~0: absolute floor)
            bad.append((k, err, rn))
    print(f"{label}: worst per-sample prediction error {worst_pred:.2e}, worst relative gradient error {worst[1]:.2e} ({worst[0]})")
    assert not bad, f"{len(bad)} gradients off the reference: {bad[:8]}"


def train_model(cfg, variant, phosc_on, seed):
    cls = UNetModel if variant == "base" else UNetModelPhosc
    m = cls(args=make_args(device=DEV, phosc=1 if phosc_on else 0), **cfg)
    fill_module_(m, seed)
    return m.to(DEV).train()


def train_call(m, variant, x, inp, eps, phosc_len):
    """model(...) in train mode -> MSELoss -> loss.backward() (train.py:287-291): (pred, loss, {name: grad})."""
    kw = dict(timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV), y=inp["y"].to(DEV))
    if variant == "base":
        pred = m(x.to(DEV), **kw)
    else:
        pred = m(x.to(DEV), inp["phosc"].to(DEV) if phosc_len else None, **kw)
    loss = torch.nn.MSELoss()(eps.to(DEV), pred)
    loss.backward()
    torch.cuda.synchronize()
    return pred, float(loss.detach()), {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
