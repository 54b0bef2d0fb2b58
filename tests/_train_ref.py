"""The float64 training reference the gradient tests share (tests/test_gpu_training.py, tests/test_gpu_shapes.py): one case's inputs,
the oracle's forward -> MSE -> autograd in float64 on the CPU, the comparison with its bars, and the model -> MSELoss -> backward
call of the HIP path.  Every function takes the model's config dict.  ``RunningReference`` is the same reference for the first B
samples of one pool at many B (tests/test_gpu_train_thresholds.py): per-sample gradients summed in float64."""
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
    return batched_reference64(cfg, variant, x, inp, eps, phosc_len, seeds[0])


def batched_reference64(cfg, variant, x, inp, eps, phosc_len, seed_w):
    """One batched float64 forward -> mse_loss -> backward over the given inputs: (pred, loss, {name: grad})."""
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed_w)).double().requires_grad_(True)
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


def misses_the_gradient_bar(g, r) -> bool:
    """The per-parameter gradient bar of ``check_against_reference``, for one float64 pair (gradient, reference)."""
    return not float((g - r).norm()) < 2e-4 * float(r.norm()) + 1e-7


class RunningReference:
    """The float64 reference of ``reference64`` for the first B samples of one pool, for many B at the cost of one pass over the pool.

    The oracle has no operation that couples samples (GroupNorm is per sample, LayerNorm per token, dropout is off), so with
    S_b = sum((pred_b - eps_b)^2) and n elements per sample
        grad(mse loss of the first B samples) = (sum over b < B of grad S_b) / (B n)
    and the loss is the same expression in S_b itself.  Held: ONE float64 copy of the summed parameter gradients G (346 MB for
    FULL base), the per-sample S_b and predictions, the count of samples folded in, and the gradient of the last advance (what
    ``drop_one_share`` leaves out).  tests/test_train_running_ref_host.py holds ``at`` to the batched ``reference64`` construction."""
    CHUNK = 16  # samples per oracle backward

    def __init__(self, cfg, variant, pool_inputs, pool_eps, phosc_len, seed_w=0):
        self.variant, self.inp, self.eps, self.phosc_len = variant, pool_inputs, pool_eps.double(), phosc_len
        self.sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed_w)).double().requires_grad_(True)
                   for k, s in U.state_dict_shapes(cfg, variant)}
        self.orc = U.UNetOracle(cfg, self.sd, variant, phosc_len > 0)
        self.n = int(self.eps[0].numel())
        self._reset()

    def _reset(self):
        self.count, self.S, self.pred = 0, [], []
        self.G = None      # {name: sum over the samples folded in of grad S_b}, the parameters the loss reaches
        self.last = None   # (first sample, end, {name: gradient}) of the last advance

    def _advance(self, lo, hi):
        s, inp = slice(lo, hi), self.inp
        pred = self.orc(inp["x"][s].double(), inp["t"][s], inp["context"][s], inp["y"][s],
                        inp["phosc"][s] if self.phosc_len else None)
        S = ((pred - self.eps[s]) ** 2).flatten(1).sum(1)
        names = list(self.sd)
        got = torch.autograd.grad(S.sum(), [self.sd[k] for k in names], allow_unused=True)
        g = {k: v for k, v in zip(names, got) if v is not None}
        if self.G is None:
            self.G = {k: v.clone() for k, v in g.items()}
        else:
            assert set(g) == set(self.G)
            for k, v in g.items():
                self.G[k] += v
        self.S += [float(v) for v in S.detach()]
        self.pred += list(pred.detach())
        self.count, self.last = hi, (lo, hi, g)

    def at(self, B):
        """(pred[:B], loss, {name: grad}) of the mse loss over the first B samples: the tuple ``check_against_reference`` takes."""
        assert 1 <= B <= self.eps.shape[0]
        if B < self.count:
            print(f"[running reference] {self.variant}: B = {B} after B = {self.count}: starting over from zero")
            self._reset()
        while self.count < B:
            self._advance(self.count, min(B, self.count + self.CHUNK))
        scale = 1.0 / (B * self.n)
        return torch.stack(self.pred[:B]), sum(self.S[:B]) * scale, {k: v * scale for k, v in self.G.items()}

    def drop_one_share(self):
        """After an ``at(B)`` that advanced by exactly one sample: (parameters whose reference WITHOUT that sample's contribution,
        (G - g_last) / (B n), misses the gradient bar against the reference, parameters asked) over those with reference norm
        > 1e-6 - the teeth of the bar at this B.  None after any other advance."""
        if self.last is None or self.last[1] != self.count or self.last[1] - self.last[0] != 1:
            return None
        scale = 1.0 / (self.count * self.n)
        asked = broken = 0
        for k, G in self.G.items():
            ref = G * scale
            if float(ref.norm()) > 1e-6:
                asked += 1
                broken += misses_the_gradient_bar((G - self.last[2][k]) * scale, ref)
        return broken, asked


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
