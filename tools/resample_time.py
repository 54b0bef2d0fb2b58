"""What resampling jumps cost: Diffusion.sampling_ddim (50 steps, eta = 0) at the headline configuration through the PRODUCT
API - FULL base UNet, B = 64, synthetic weights - plain, with a column mask (``known`` / ``known_mask``) and with the mask and
``resample=2, jump=10`` (a walk of 90 down entries and 4 up entries), on the same build, in one process, the three calls
alternating.  The protocol is ``tools/known_bench.py``'s: wall clock per call around a device synchronise, 1 warm-up + REPS timed
calls each.  Prints one JSON line (per variant: the calls, the median, ms per step - for the resampled call ms per DOWN entry,
the up entries' cost folded in - and the min-max spread) and writes it to ``profiles/resample_time.json`` (``--out FILE``).  On a
tree without the feature ``tools/known_bench.py`` gives the plain and masked figures to compare with."""
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
ap.add_argument("--resample", type=int, default=2)
ap.add_argument("--jump", type=int, default=10)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resample_time.json"))
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
kw = dict(steps=a.ddim_steps, eta=0.0, seed=5)

variants = {"plain": lambda: diff.sampling_ddim(model, None, B, words, labels, args, **kw),
            "masked": lambda: diff.sampling_ddim(model, None, B, words, labels, args, known=known, known_mask=mask, **kw),
            "resampled": lambda: diff.sampling_ddim(model, None, B, words, labels, args, known=known, known_mask=mask,
                                                    resample=a.resample, jump=a.jump, **kw)}
times = {k: [] for k in variants}
stats = {}
for k, fn in variants.items():  # warm-up: plan, packed weights, FiLM table buffers
    assert bool(torch.isfinite(fn()).all())
    stats[k] = dict(diff.last_stats)
for _ in range(a.reps):  # alternating: a drift of the machine reaches every variant alike
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


# (a step of the resampled call is a down entry: ``model_calls`` of a call with one forward per step)
res = dict(tool="resample_time", device=torch.cuda.get_device_name(0), batch=B, ddim_steps=a.ddim_steps, keep_cols=a.keep_cols,
           resample=a.resample, jump=a.jump,
           timing="wall clock per call around a device synchronise, median of the timed calls, variants alternating",
           **{k: summary(ts, stats[k]["model_calls"]) for k, ts in times.items()})
res["resampled"].update(walk=stats["resampled"]["walk"], up_entries=stats["resampled"]["walk"] - stats["resampled"]["model_calls"],
                        known_noise=stats["resampled"]["known_noise"])
res["masked"]["known_noise"] = stats["masked"]["known_noise"]
res["masked_over_plain"] = round(res["masked"]["ms_per_call"] / res["plain"]["ms_per_call"], 4)
res["down_entry_over_masked_step"] = round(res["resampled"]["ms_per_step"] / res["masked"]["ms_per_step"], 4)
res["extra_ms_per_down_entry"] = round(res["resampled"]["ms_per_step"] - res["masked"]["ms_per_step"], 4)
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
