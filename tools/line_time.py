"""Cost of line sampling (``windows=``, DESIGN.md "Lines") at the benchmark's model (bench.build_model: FULL base UNet, [4, 8, 32]
latents), model batch 64 throughout:

   python tools/line_time.py [--rounds R] [--steps S] [--precision bf16x3|bf16] [--parent TREE] [--json PATH]

One process, S-step DDIM calls (eta = 0) through the captured graph, three calls alternated R times after one warm-up call each,
wall clock around the call and a device synchronise, reported in ms per step:
   plain      64 plain words                       the call without the argument
   lines8x8   8 lines of 8 words, overlap 2        the same forward at batch 64 + gather and blend per step, line width 242
   lines16x4  16 lines of 4 words, overlap 2       likewise, line width 122
A line step is the plain step at the same model batch plus two small launches (and an update over fewer elements); what that costs
is reported as ``*_minus_plain_median``, not gated.

``--parent TREE``: a built checkout of the parent commit.  The plain leg is then also timed on that tree and on this one in child
processes of their own (``--plain_only``, one process per tree and round, alternated; a child imports the package of the tree it
is given and uses nothing the parent lacks).  The plain path launches the same things on both, so the two medians must agree within
the run-to-run spread the children report: ``plain_vs_parent`` carries both, the difference and the verdict."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--precision", default="bf16x3")
ap.add_argument("--parent", default=None, metavar="TREE")
ap.add_argument("--tree", default=ROOT, help="the checkout whose package is imported (children of --parent)")
ap.add_argument("--plain_only", action="store_true", help="time the plain leg alone and print one JSON line (what a child runs)")
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "line_time.json"))
a = ap.parse_args()

sys.path.insert(0, os.path.abspath(a.tree))
import torch  # noqa: E402

import bench  # noqa: E402
from worddiffusion_amd import Diffusion  # noqa: E402

dev = "cuda:0"
MODEL_BATCH, OVERLAP = 64, 2
WORDS = ["getting", "Moving", "on", "a", "Zebra", "quilt", "Word", "by"]


def summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v), rounds=v)


model, args = bench.build_model(dev, a.precision, "base")
diff = Diffusion(noise_steps=bench.T, img_size=(64, 256), args=args)


def plain():
    labels = torch.arange(MODEL_BATCH, dtype=torch.int64) % 339
    return diff.sampling_ddim(model, None, MODEL_BATCH, [WORDS[i % 8] for i in range(MODEL_BATCH)], labels, args, steps=a.steps, seed=1)


def lines(K):
    n = MODEL_BATCH // K
    lw = diff.line_windows(n, K, overlap=OVERLAP)
    labels = torch.arange(n, dtype=torch.int64) % 339
    return lambda: diff.sampling_ddim(model, None, n, WORDS[:K], labels, args, steps=a.steps, seed=1, windows=lw)


def timed(calls, rounds):
    stats = {}
    for name, fn in calls.items():  # builds the plan; the timed calls capture their graph like any call
        x = fn()
        stats[name] = dict(diff.last_stats, finite=bool(torch.isfinite(x).all().item()), shape=list(x.shape))
        assert stats[name]["graph"] and stats[name]["finite"], (name, stats[name])
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
    return times, stats


if a.plain_only:
    times, _ = timed(dict(plain=plain), a.rounds)
    print(json.dumps(dict(tree=os.path.abspath(a.tree), plain=times["plain"])), flush=True)
    sys.exit(0)

times, stats = timed(dict(plain=plain, lines8x8=lines(8), lines16x4=lines(4)), a.rounds)
assert all(stats[k]["model_batch"] == MODEL_BATCH for k in ("lines8x8", "lines16x4"))
legs = {k: summary(v) for k, v in times.items()}
out = dict(device=torch.cuda.get_device_name(0), precision=a.precision, model_batch=MODEL_BATCH, overlap=OVERLAP, rounds=a.rounds,
           steps_per_call=a.steps, sampler="ddim", unit="ms per step, wall clock around the call", legs=legs,
           line_width={k: stats[k]["line_width"] for k in ("lines8x8", "lines16x4")},
           lines8x8_minus_plain_median=legs["lines8x8"]["median"] - legs["plain"]["median"],
           lines16x4_minus_plain_median=legs["lines16x4"]["median"] - legs["plain"]["median"])
if a.parent:
    del model
    torch.cuda.empty_cache()
    trees = dict(this=ROOT, parent=os.path.abspath(a.parent))
    per = {k: [] for k in trees}
    for _ in range(a.rounds):  # one fresh process per tree and round, alternated: each figure is the median of that process's calls
        for name, tree in trees.items():
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain_only", "--tree", tree, "--rounds", "3", "--steps",
                                  str(a.steps), "--precision", a.precision], check=True, capture_output=True, text=True, timeout=300)
            per[name].append(statistics.median(json.loads(res.stdout.strip().splitlines()[-1])["plain"]))
    cmp_ = {k: summary(v) for k, v in per.items()}
    gap = cmp_["this"]["median"] - cmp_["parent"]["median"]
    spread = max(cmp_["this"]["spread"], cmp_["parent"]["spread"])
    out["plain_vs_parent"] = dict(unit="ms per step; per round the median of 3 calls of a fresh process", legs=cmp_, this_minus_parent_median=gap,
                                  spread=spread, agree_within_spread=bool(abs(gap) <= spread))
print(json.dumps(out), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
with open(a.json, "w") as f:
    json.dump(out, f, indent=1)
