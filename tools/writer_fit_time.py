"""What the frozen-trunk step of writer fitting saves over the full training step (DESIGN.md "Fitting new writers"): FULL base
model, [4, 8, 32] latents, B = 64 and B = 16:

   python tools/writer_fit_time.py [--rounds R] [--calls K] [--warmup W] [--precision bf16x3|bf16] [--new 8] [--json PATH]

Four legs per batch size, each on its own copy of the model (a training engine keeps one live plan), all grown by ``--new`` writer
rows whose ids the batch cycles through:
   full_graph / full_eager       TrainStep(FusedAdamW(model.parameters()))   every weight trains
   frozen_graph / frozen_eager   TrainStep(RowAdamW(label_emb.weight, rows))  the frozen-trunk plan, one wd_adamw_rows launch
After W warm-up calls of every leg: R rounds, in each round every leg in turn runs K calls between two host clock reads around a
device synchronise (the legs interleaved, so drift hits them alike).  Reported per leg: the median over the rounds of ms per call
and every round, plus len(P.step) and len(P.bwd) of both plans; ``frozen_over_full`` is the ratio of the graph legs' medians and
``spread`` the largest (max - min) / median over the rounds of those two legs - the saving counts only where it exceeds that."""
import argparse
import copy
import gc
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from worddiffusion_amd import Diffusion  # noqa: E402
from worddiffusion_amd.optim import FusedAdamW, RowAdamW  # noqa: E402
from worddiffusion_amd.synthetic import synthetic_inputs  # noqa: E402
from worddiffusion_amd.training import TrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--precision", default="bf16x3")
ap.add_argument("--new", type=int, default=8)
ap.add_argument("--batches", type=int, nargs="+", default=[64, 16])
ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                               "writer_fit_time.json"))
a = ap.parse_args()
dev = "cuda:0"

base, args = bench.build_model(dev, a.precision, "base")
base.train()
rows = base.add_writers(a.new, init="mean")
diff = Diffusion(noise_steps=bench.T, img_size=(64, 256), args=args)


def measure(batch):
    inp = synthetic_inputs(batch, seed=7, hw=(8, 32), num_classes=339)
    x, ctx = inp["x"].to(dev), inp["context"].to(dev)
    y = torch.tensor([rows[b % len(rows)] for b in range(batch)], device=dev)
    legs = {}
    for name, frozen, graph in (("full_graph", False, True), ("full_eager", False, False), ("frozen_graph", True, True),
                                ("frozen_eager", True, False)):
        m = copy.deepcopy(base)
        opt = RowAdamW(m.label_emb.weight, rows, lr=1e-4) if frozen else FusedAdamW(m.parameters(), lr=1e-4)
        step = TrainStep(m, diff, opt, seed=99, use_graph=graph)
        legs[name] = (step, (lambda step=step: step(x, ctx, y, check=False)))
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
    out = dict(batch=batch, loss_finite=bool(torch.isfinite(loss).all().item()),
               legs={k: dict(ms_per_call_median=statistics.median(v), ms_per_call_min=min(v), ms_per_call_max=max(v),
                             ms_per_call_rounds=v) for k, v in times.items()},
               launches={k: dict(step=len(legs[k + "_graph"][0]._P.step), bwd=len(legs[k + "_graph"][0]._P.bwd))
                         for k in ("full", "frozen")})
    med = {k: v["ms_per_call_median"] for k, v in out["legs"].items()}
    out["frozen_over_full"] = med["frozen_graph"] / med["full_graph"]
    out["frozen_eager_over_full_eager"] = med["frozen_eager"] / med["full_eager"]
    out["spread"] = max((max(times[k]) - min(times[k])) / med[k] for k in ("full_graph", "frozen_graph"))
    return out


results = []
for batch in a.batches:
    results.append(measure(batch))
    gc.collect()
    torch.cuda.empty_cache()
out = dict(device=torch.cuda.get_device_name(0), precision=a.precision, new_rows=a.new, rounds=a.rounds, calls_per_round=a.calls,
           warmup_calls=a.warmup, batches=results)
print(json.dumps(out), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
with open(a.json, "w") as f:
    json.dump(out, f, indent=1)
