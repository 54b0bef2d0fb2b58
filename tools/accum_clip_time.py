"""Cost of gradient accumulation and global-norm clipping at the training leg's shape (bench.build_model: FULL base UNet,
B = 64 per call, [4, 8, 32] latents, one hipGraph per call; DESIGN.md section 9 "Accumulation and clipping"):

   python tools/accum_clip_time.py [--accumulate A ...] [--max-grad-norm X|none ...] [--steps N] [--warmup W]
                                   [--precision bf16x3|bf16] [--batch B] [--json PATH]

For every (A, X) pair: its own FusedAdamW(max_grad_norm=X) and TrainStep(accumulate=A), W optimiser steps of warm-up, then N
optimiser steps (N * A calls) between two host clock reads around a device synchronise -> ms per call and per optimiser step.
Then, alone and warm, 100 back-to-back launches between two hipEvents, three times each: the norm pass
(wd_grad_sqnorm_multi over the optimiser's table), the accumulate pass (wd_grad_accumulate over the arena) and a
device-to-device copy of the arena, the yardstick (it reads N bytes and writes N bytes)."""
import argparse
import copy
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from worddiffusion_amd import Diffusion  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.optim import FusedAdamW  # noqa: E402
from worddiffusion_amd.synthetic import synthetic_inputs  # noqa: E402
from worddiffusion_amd.training import TrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--accumulate", type=int, nargs="+", default=[1])
ap.add_argument("--max-grad-norm", nargs="+", default=["none"])
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--precision", default="bf16x3")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--json", default=None)
a = ap.parse_args()
dev = "cuda:0"
lib = N.lib()

model, args = bench.build_model(dev, a.precision, "base")
model.train()
ema_model = copy.deepcopy(model).eval().requires_grad_(False)
diff = Diffusion(noise_steps=bench.T, img_size=(64, 256), args=args)
inp = synthetic_inputs(a.batch, seed=7, hw=(8, 32), num_classes=339)
x, ctx, y = inp["x"].to(dev), inp["context"].to(dev), inp["y"].to(dev)

rows, opt, step = [], None, None
for acc in a.accumulate:
    for mg in a.max_grad_norm:
        mgn = None if mg.lower() == "none" else float(mg)
        opt = FusedAdamW(model.parameters(), lr=1e-4, ema_model=ema_model, ema_beta=0.995, step_start_ema=2000, max_grad_norm=mgn)
        step = TrainStep(model, diff, opt, seed=99, accumulate=acc)
        for _ in range(a.warmup * acc):
            step(x, ctx, y)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps * acc):
            loss = step(x, ctx, y)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        row = dict(accumulate=acc, max_grad_norm=mgn, precision=a.precision, batch_per_call=a.batch, optimizer_steps=a.steps,
                   ms_per_call=ms / (a.steps * acc), ms_per_optimizer_step=ms / a.steps,
                   loss_finite=bool(torch.isfinite(loss).all().item()),
                   grad_norm=float(opt.grad_norm.cpu()) if mgn is not None else None)
        rows.append(row)
        print(json.dumps(row), flush=True)


def alone(fn, reps=100, rounds=3):
    """ms per launch: ``reps`` back-to-back launches between two events, warm, ``rounds`` times."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


# the three passes alone, on the last step's arena and an optimiser table with the scratch of the norm pass
if opt.max_grad_norm is None:
    opt = FusedAdamW(model.parameters(), lr=0.0, max_grad_norm=float("inf"))
    opt.step()
arena = step.eng.grad_arena()
other = torch.zeros_like(arena)
n = arena.numel()
torch.cuda.synchronize()
st = torch.cuda.current_stream(dev).cuda_stream
passes = dict(
    norm_pass=alone(lambda: N.check(lib.wd_grad_sqnorm_multi(opt._table.data_ptr(), len(opt.params), opt._chunks,
                                                             opt._partials.data_ptr(), 1.0, opt._clip_ctl.data_ptr(), st),
                                    "wd_grad_sqnorm_multi")),
    accumulate_pass=alone(lambda: N.check(lib.wd_grad_accumulate(other.data_ptr(), arena.data_ptr(), n, 0, 1.0, st),
                                          "wd_grad_accumulate")),
    arena_copy=alone(lambda: other.copy_(arena)))
copy_ms = min(passes["arena_copy"])
alone_out = dict(arena_mb=n * 4 / 1e6, table_chunks=int(opt._chunks), ms=passes,
                 norm_over_copy=min(passes["norm_pass"]) / copy_ms, accumulate_over_copy=min(passes["accumulate_pass"]) / copy_ms,
                 copy_gb_per_s=2 * n * 4 / 1e6 / copy_ms, norm_gb_per_s=n * 4 / 1e6 / min(passes["norm_pass"]),
                 accumulate_gb_per_s=3 * n * 4 / 1e6 / min(passes["accumulate_pass"]))
print(json.dumps(alone_out), flush=True)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), runs=rows, passes_alone=alone_out), f, indent=1)
