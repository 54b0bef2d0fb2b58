"""Diffusion.sampling_ddim (50 steps, eta = 0) against Diffusion.sampling (999 steps) at the headline configuration through the
PRODUCT API: FULL base UNet, B = 64, synthetic weights.  Wall clock per call, 1 warm-up + REPS timed calls each, in one process.
Prints one JSON line (ms per executed step, ms per call, images/s for both samplers); ``--out FILE`` also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from worddiffusion_amd import Diffusion  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--ddim_steps", type=int, default=50)
ap.add_argument("--eta", type=float, default=0.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ddpm_reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()

dev = "cuda:0"
model, args = bench.build_model(dev, os.environ.get("PREC", "bf16x3"), "base")
diff = Diffusion(noise_steps=1000, img_size=(64, 256), args=args)
B = a.batch
words = ["".join("abcdefghij"[int(c)] for c in str(i)).rjust(4, "w") for i in range(B)]
labels = torch.arange(B) % 339


def timed(fn, reps):
    fn()  # warm-up: plan, packed weights, FiLM table buffers
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    assert bool(torch.isfinite(x).all())
    return out


def summary(times, steps):
    med = statistics.median(times)
    return dict(steps=steps, calls_s=[round(t, 4) for t in times], ms_per_call=round(1e3 * med, 2), ms_per_step=round(1e3 * med / steps, 4),
                ms_per_step_min=round(1e3 * min(times) / steps, 4), ms_per_step_max=round(1e3 * max(times) / steps, 4),
                images_per_s=round(B / med, 2))


ddim = timed(lambda: diff.sampling_ddim(model, None, B, words, labels, args, steps=a.ddim_steps, eta=a.eta, seed=5), a.reps)
ddim_stats = dict(diff.last_stats)
ddpm = timed(lambda: diff.sampling(model, None, B, words, labels, args, seed=5), a.ddpm_reps)
res = dict(tool="ddim_bench", device=torch.cuda.get_device_name(0), batch=B, eta=a.eta, timing="wall clock per call, median of the timed calls",
           ddim=summary(ddim, ddim_stats["steps"]), ddpm=summary(ddpm, diff.last_stats["steps"]))
res["call_speedup"] = round(res["ddpm"]["ms_per_call"] / res["ddim"]["ms_per_call"], 2)
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
