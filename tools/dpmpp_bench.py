"""Diffusion.sampling_dpmpp (20 steps, order 2, log-SNR spacing) against Diffusion.sampling_ddim (20 and 50 steps, eta = 0) at the
headline configuration through the PRODUCT API: FULL base UNet, B = 64, synthetic weights.  Wall clock per call, 1 warm-up call each, then REPS
rounds that time the three in turn, in one process.  Prints one JSON line (ms per executed step, ms per call, images/s for the three runs, and
the per-step and per-call ratios); ``--out FILE`` also writes it."""
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
ap.add_argument("--dpmpp_steps", type=int, default=20)
ap.add_argument("--dpmpp_order", type=int, default=2, choices=[1, 2])
ap.add_argument("--dpmpp_spacing", default="logsnr", choices=["logsnr", "time"])
ap.add_argument("--ddim_steps", type=int, default=50)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()

dev = "cuda:0"
model, args = bench.build_model(dev, os.environ.get("PREC", "bf16x3"), "base")
diff = Diffusion(noise_steps=1000, img_size=(64, 256), args=args)
B = a.batch
words = ["".join("abcdefghij"[int(c)] for c in str(i)).rjust(4, "w") for i in range(B)]
labels = torch.arange(B) % 339


def timed(fns, reps):
    """1 warm-up call of each (plan, packed weights, FiLM table buffers), then ``reps`` rounds that time each in turn: a drift
    of the clocks over the run falls on all of them alike."""
    for fn in fns:
        fn()
    out = [[] for _ in fns]
    for _ in range(reps):
        for times, fn in zip(out, fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            assert bool(torch.isfinite(x).all())
    return out


def summary(times, steps):
    med = statistics.median(times)
    return dict(steps=steps, calls_s=[round(t, 4) for t in times], ms_per_call=round(1e3 * med, 2), ms_per_step=round(1e3 * med / steps, 4),
                ms_per_step_min=round(1e3 * min(times) / steps, 4), ms_per_step_max=round(1e3 * max(times) / steps, 4),
                images_per_s=round(B / med, 2))


t_dpmpp, t_same, t_ddim = timed([
    lambda: diff.sampling_dpmpp(model, None, B, words, labels, args, steps=a.dpmpp_steps, order=a.dpmpp_order, spacing=a.dpmpp_spacing,
                                seed=5),
    lambda: diff.sampling_ddim(model, None, B, words, labels, args, steps=a.dpmpp_steps, eta=0.0, seed=5),
    lambda: diff.sampling_ddim(model, None, B, words, labels, args, steps=a.ddim_steps, eta=0.0, seed=5)], a.reps)
dpmpp, ddim_same, ddim = summary(t_dpmpp, a.dpmpp_steps), summary(t_same, a.dpmpp_steps), summary(t_ddim, a.ddim_steps)
res = dict(tool="dpmpp_bench", device=torch.cuda.get_device_name(0), batch=B, order=a.dpmpp_order, spacing=a.dpmpp_spacing,
           timing="wall clock per call, the three timed in turn per round, median of the rounds", dpmpp=dpmpp, ddim_same_steps=ddim_same, ddim=ddim)
res["step_ratio_vs_ddim_same_steps"] = round(dpmpp["ms_per_step"] / ddim_same["ms_per_step"], 4)
res["call_ratio_vs_ddim"] = round(dpmpp["ms_per_call"] / ddim["ms_per_call"], 4)
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
