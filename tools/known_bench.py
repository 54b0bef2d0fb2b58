"""What keeping a known region costs: Diffusion.sampling_ddim (50 steps, eta = 0) at the headline configuration through the
PRODUCT API - FULL base UNet, B = 64, synthetic weights - plain and with a column mask (``known`` / ``known_mask``: one
``wd_known_blend`` launch more in every step), on the same build, in one process, the two calls alternating.  Wall clock per
call around a device synchronise, 1 warm-up + REPS timed calls each.  Prints one JSON line (per variant: the calls, the median,
ms per step, the min-max spread); ``--out FILE`` also writes it.  ``--plain_only`` times the plain call alone (a tree without
the feature: the parent commit's figure); ``--parent FILE`` folds such a result into the output as ``parent_plain``."""
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
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--keep_cols", type=int, default=16, help="the first KEEP_COLS of the 32 latent columns are kept")
ap.add_argument("--plain_only", action="store_true")
ap.add_argument("--parent", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()

dev = "cuda:0"
model, args = bench.build_model(dev, os.environ.get("PREC", "bf16x3"), "base")
diff = Diffusion(noise_steps=1000, img_size=(64, 256), args=args)
B = a.batch
words = ["".join("abcdefghij"[int(c)] for c in str(i)).rjust(4, "w") for i in range(B)]
labels = torch.arange(B) % 339
known = torch.randn(B, 4, 8, 32, generator=torch.Generator().manual_seed(1)) * 0.8
mask = torch.zeros(8, 32)
mask[:, :a.keep_cols] = 1.0

variants = {"plain": lambda: diff.sampling_ddim(model, None, B, words, labels, args, steps=a.ddim_steps, eta=0.0, seed=5)}
if not a.plain_only:
    variants["masked"] = lambda: diff.sampling_ddim(model, None, B, words, labels, args, steps=a.ddim_steps, eta=0.0, seed=5,
                                                    known=known, known_mask=mask)
times = {k: [] for k in variants}
stats = {}
for k, fn in variants.items():  # warm-up: plan, packed weights, FiLM table buffers
    assert bool(torch.isfinite(fn()).all())
    stats[k] = dict(diff.last_stats)
for _ in range(a.reps):  # alternating: a drift of the machine reaches both variants alike
    for k, fn in variants.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times[k].append(time.perf_counter() - t0)


def summary(ts, steps):
    med = statistics.median(ts)
    return dict(steps=steps, calls_s=[round(t, 4) for t in ts], ms_per_call=round(1e3 * med, 2), ms_per_step=round(1e3 * med / steps, 4),
                ms_per_step_min=round(1e3 * min(ts) / steps, 4), ms_per_step_max=round(1e3 * max(ts) / steps, 4),
                spread_pct=round(100 * (max(ts) - min(ts)) / med, 2), images_per_s=round(B / med, 2))


res = dict(tool="known_bench", device=torch.cuda.get_device_name(0), batch=B, ddim_steps=a.ddim_steps, keep_cols=a.keep_cols,
           timing="wall clock per call around a device synchronise, median of the timed calls, variants alternating",
           **{k: summary(ts, stats[k]["steps"]) for k, ts in times.items()})
if "masked" in res:
    res["masked"]["known_noise"] = stats["masked"]["known_noise"]
    res["masked_over_plain"] = round(res["masked"]["ms_per_call"] / res["plain"]["ms_per_call"], 4)
    res["blend_ms_per_step"] = round(res["masked"]["ms_per_step"] - res["plain"]["ms_per_step"], 4)
if a.parent:
    with open(a.parent) as f:
        res["parent_plain"] = json.loads(f.read())["plain"]
    res["plain_over_parent_plain"] = round(res["plain"]["ms_per_call"] / res["parent_plain"]["ms_per_call"], 4)
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
