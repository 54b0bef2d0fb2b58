"""Cost of the weighted training loss at the training leg's shape (bench.build_model: FULL base UNet, B = 64, [4, 8, 32]
latents; DESIGN.md section 9 "Weighted training loss"):

   python tools/wloss_time.py [--rounds R] [--calls K] [--warmup W] [--precision bf16x3|bf16] [--batch B] [--json PATH]

Three legs in one process, each its own FusedAdamW and TrainStep over the same model:
   plain            TrainStep(...)                                              the default step: wd_mse_loss
   weighted         TrainStep(loss_weights="min_snr", loss_bins=20) + loss_mask  wd_weighted_mse_loss, one hipGraph
   weighted_eager   the same with use_graph=False
After W warm-up calls of every leg: R rounds, in each round every leg in turn runs K calls between two host clock reads around a
device synchronise (the legs interleaved, so drift of the clocks or of the host hits them alike).  Reported per leg: the median
over the rounds of ms per call, and every round."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from worddiffusion_amd import Diffusion  # noqa: E402
from worddiffusion_amd.latents import loss_mask_columns  # noqa: E402
from worddiffusion_amd.optim import FusedAdamW  # noqa: E402
from worddiffusion_amd.synthetic import synthetic_inputs  # noqa: E402
from worddiffusion_amd.training import TrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--precision", default="bf16x3")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wloss_time.json"))
a = ap.parse_args()
dev = "cuda:0"

model, args = bench.build_model(dev, a.precision, "base")
model.train()
ema_model = copy.deepcopy(model).eval().requires_grad_(False)
diff = Diffusion(noise_steps=bench.T, img_size=(64, 256), args=args)
inp = synthetic_inputs(a.batch, seed=7, hw=(8, 32), num_classes=339)
x, ctx, y = inp["x"].to(dev), inp["context"].to(dev), inp["y"].to(dev)
# the dataset's column mask: words of 16 .. 256 px, padding at 1/4
widths = torch.randint(16, 257, (a.batch,), generator=torch.Generator().manual_seed(0))
mask = torch.stack([loss_mask_columns(int(wd), 8, 32, 0.25) for wd in widths]).to(dev)


def leg(masked, **kw):
    opt = FusedAdamW(model.parameters(), lr=1e-4, ema_model=ema_model, ema_beta=0.995, step_start_ema=2000)
    step = TrainStep(model, diff, opt, seed=99, **kw)
    extra = dict(loss_mask=mask, check=False) if masked else dict(check=False)
    return step, (lambda: step(x, ctx, y, **extra))


legs = dict(plain=leg(False),
            weighted=leg(True, loss_weights="min_snr", loss_bins=20),
            weighted_eager=leg(True, loss_weights="min_snr", loss_bins=20, use_graph=False))
for _, fn in legs.values():
    for _ in range(a.warmup):
        loss = fn()
torch.cuda.synchronize()
times = {k: [] for k in legs}
for _ in range(a.rounds):
    for name, (_, fn) in legs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            loss = fn()
        torch.cuda.synchronize()
        times[name].append(1e3 * (time.perf_counter() - t0) / a.calls)
out = dict(device=torch.cuda.get_device_name(0), precision=a.precision, batch=a.batch, rounds=a.rounds, calls_per_round=a.calls,
           warmup_calls=a.warmup, loss_finite=bool(torch.isfinite(loss).all().item()),
           legs={k: dict(ms_per_call_median=statistics.median(v), ms_per_call_min=min(v), ms_per_call_max=max(v),
                         ms_per_call_rounds=v) for k, v in times.items()})
med = {k: v["ms_per_call_median"] for k, v in out["legs"].items()}
out["weighted_over_plain"] = med["weighted"] / med["plain"]
out["weighted_eager_over_plain"] = med["weighted_eager"] / med["plain"]
hist = legs["weighted"][0].loss_by_timestep()
out["weighted_histogram_samples"] = int(hist["count"].sum())
print(json.dumps(out), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
with open(a.json, "w") as f:
    json.dump(out, f, indent=1)
