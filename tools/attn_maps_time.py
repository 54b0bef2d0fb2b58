"""What the attention maps cost: Diffusion.sampling_ddim (50 steps, eta = 0) at the headline configuration through the PRODUCT
API - FULL base UNet, B = 64, synthetic weights - plain and with ``attention=True`` (three SpatialTransformers leave the one-launch
form for the chained launches, and each gains one ``wd_xattn_maps`` launch per step), on the same build, in one process, the two
calls alternating.  Wall clock per call around a device synchronise, 1 warm-up + REPS timed calls each.  Then the three
``wd_xattn_maps`` launches of the maps plan alone, back to back on one stream between two events (ITERS rounds), and each on its
own.  Prints one JSON line; ``--out FILE`` also writes it (profiles/attn_maps_time.json)."""
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
from worddiffusion_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--ddim_steps", type=int, default=50)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--out", default=None)
a = ap.parse_args()

dev = "cuda:0"
model, args = bench.build_model(dev, os.environ.get("PREC", "bf16x3"), "base")
diff = Diffusion(noise_steps=1000, img_size=(64, 256), args=args)
B = a.batch
words = ["".join("abcdefghij"[int(c)] for c in str(i)).rjust(4, "w") for i in range(B)]
labels = torch.arange(B) % 339

variants = {"plain": lambda: diff.sampling_ddim(model, None, B, words, labels, args, steps=a.ddim_steps, eta=0.0, seed=5),
            "attention": lambda: diff.sampling_ddim(model, None, B, words, labels, args, steps=a.ddim_steps, eta=0.0, seed=5,
                                                    attention=True)}
times = {k: [] for k in variants}
stats, finals = {}, {}
for k, fn in variants.items():  # warm-up: plan, packed weights, FiLM table buffers
    finals[k] = fn()
    assert bool(torch.isfinite(finals[k]).all())
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


# ---- the three maps launches alone (accumulate form, as the step runs them)
lib = N.lib()
P = next(p for p in model.engine._plans.values() if p.maps)
maps_ops = [op for op in P.step if op[0] is lib.wd_xattn_maps]
assert len(maps_ops) == 3
stream = torch.cuda.current_stream().cuda_stream


def timed(ops, iters):
    for fn, fargs, what in ops:
        N.check(fn(*fargs, stream), what)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        for fn, fargs, what in ops:
            fn(*fargs, stream)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters  # us per round


launches = dict(all_three_us=round(timed(maps_ops, a.iters), 2),
                **{what: round(timed([op], a.iters), 2) for op in maps_ops for what in [op[2] + "_us"]})

res = dict(tool="attn_maps_time", device=torch.cuda.get_device_name(0), batch=B, ddim_steps=a.ddim_steps,
           timing="wall clock per call around a device synchronise, median of the timed calls, variants alternating; the launches "
                  "alone: back to back on one stream between two events, mean over the rounds",
           **{k: summary(ts, stats[k]["steps"]) for k, ts in times.items()})
res["attention"]["attention_steps"] = stats["attention"]["attention_steps"]
res["attention_over_plain"] = round(res["attention"]["ms_per_call"] / res["plain"]["ms_per_call"], 4)
res["attention_ms_per_step"] = round(res["attention"]["ms_per_step"] - res["plain"]["ms_per_step"], 4)
res["maps_launches"] = launches
res["final_x_max_rel_attention_vs_plain"] = float((finals["attention"] - finals["plain"]).abs().max() / finals["plain"].abs().max())
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
