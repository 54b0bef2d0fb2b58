"""Cost of writer-free guidance at the benchmark's shape (bench.build_model: FULL base UNet, B = 64, [4, 8, 32] latents; DESIGN.md
"Writer-free guidance"):

   python tools/writer_free_time.py [--rounds R] [--steps S] [--calls K] [--precision bf16x3|bf16] [--batch B] [--json PATH]

Sampling, one process, S DDPM steps per call (a schedule of S + 1 noise steps), three calls alternated R times, wall clock around
the call and a device synchronise:
   plain     Diffusion.sampling(...)                                       one forward per step
   mix2      the same model in the reference's interpolation mode (args.interpolation, mix_rate, cfg_scale=3): two forwards per
             step, the plan this feature was modelled on
   guided    Diffusion.sampling(..., guidance="writer_free")               two forwards per step
Training, three models with the same weights, each its own FusedAdamW and TrainStep, alternated R times, K calls between two clock
reads: label_dropout 0 (the step without the argument), 0.1 (one more small launch inside the captured body) and 0 again on a
model of its own - a control for what two model instances differ by before any argument does.
Reported per leg: every round, the median and the spread (max - min) in ms per step / per call."""
import argparse
import copy
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from worddiffusion_amd import Diffusion  # noqa: E402
from worddiffusion_amd.optim import FusedAdamW  # noqa: E402
from worddiffusion_amd.synthetic import synthetic_inputs  # noqa: E402
from worddiffusion_amd.training import TrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--precision", default="bf16x3")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "writer_free_time.json"))
a = ap.parse_args()
dev = "cuda:0"


def summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v), rounds=v)


# ---- sampling
model, args = bench.build_model(dev, a.precision, "base")
diff = Diffusion(noise_steps=a.steps + 1, img_size=(64, 256), args=args)
labels = torch.arange(a.batch, dtype=torch.int64) % 339


def sample(**kw):
    return diff.sampling(model, None, a.batch, "getting", labels, args, seed=1, **kw)


def mix2():
    model.interpolation = True  # (what args.interpolation sets at construction; the weights are the same)
    try:
        random.seed(3)
        return sample(mix_rate=0.37, cfg_scale=3)
    finally:
        model.interpolation = False


calls = dict(plain=sample, mix2=mix2, guided=lambda: sample(guidance="writer_free", cfg_scale=3))
fps = {}
for name, fn in calls.items():  # builds the plan; the timed calls capture their graph like any call
    x = fn()
    fps[name] = diff.last_stats["forwards_per_step"]
torch.cuda.synchronize()
assert fps == dict(plain=1, mix2=2, guided=2), fps
times = {k: [] for k in calls}
for _ in range(a.rounds):
    for name, fn in calls.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = fn()
        torch.cuda.synchronize()
        times[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
out = dict(device=torch.cuda.get_device_name(0), precision=a.precision, batch=a.batch, rounds=a.rounds,
           sampling=dict(steps_per_call=a.steps, unit="ms per step, wall clock around the call", finite=bool(torch.isfinite(x).all().item()),
                         legs={k: summary(v) for k, v in times.items()}))
s = out["sampling"]["legs"]
out["sampling"]["guided_minus_mix2_median"] = s["guided"]["median"] - s["mix2"]["median"]
out["sampling"]["plain_spread"] = s["plain"]["spread"]
out["sampling"]["guided_within_plain_spread_of_mix2"] = bool(s["guided"]["median"] - s["mix2"]["median"] <= s["plain"]["spread"])
del model
torch.cuda.empty_cache()

# ---- training
inp = synthetic_inputs(a.batch, seed=7, hw=(8, 32), num_classes=339)
x0, ctx, y = inp["x"].to(dev), inp["context"].to(dev), inp["y"].to(dev)


def leg(p):
    m, margs = bench.build_model(dev, a.precision, "base")
    m.train()
    ema = copy.deepcopy(m).eval().requires_grad_(False)
    opt = FusedAdamW(m.parameters(), lr=1e-4, ema_model=ema, ema_beta=0.995, step_start_ema=2000)
    step = TrainStep(m, Diffusion(noise_steps=bench.T, img_size=(64, 256), args=margs), opt, seed=99, label_dropout=p)
    return step, (lambda: step(x0, ctx, y, check=False))


# (the control: a second model instance running the same plan as the first, i.e. what two instances differ by on their own)
legs = {"label_dropout_0": leg(0.0), "label_dropout_0.1": leg(0.1), "label_dropout_0_second_model": leg(0.0)}
for _, fn in legs.values():
    for _ in range(a.warmup):
        loss = fn()
torch.cuda.synchronize()
ttimes = {k: [] for k in legs}
for _ in range(a.rounds):
    for name, (_, fn) in legs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            loss = fn()
        torch.cuda.synchronize()
        ttimes[name].append(1e3 * (time.perf_counter() - t0) / a.calls)
keep = legs["label_dropout_0.1"][0].last_writer_keep
out["training"] = dict(calls_per_round=a.calls, warmup_calls=a.warmup, unit="ms per call", loss_finite=bool(torch.isfinite(loss).all().item()),
                       kept_in_last_call=int(keep.sum().item()), legs={k: summary(v) for k, v in ttimes.items()})
t = out["training"]["legs"]
out["training"]["dropout_minus_plain_median"] = t["label_dropout_0.1"]["median"] - t["label_dropout_0"]["median"]
out["training"]["control_minus_plain_median"] = t["label_dropout_0_second_model"]["median"] - t["label_dropout_0"]["median"]
out["training"]["difference_within_plain_spread"] = bool(abs(out["training"]["dropout_minus_plain_median"]) <= t["label_dropout_0"]["spread"])
print(json.dumps(out), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
with open(a.json, "w") as f:
    json.dump(out, f, indent=1)
