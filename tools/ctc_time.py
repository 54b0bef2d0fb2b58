"""Cost of the CTC loss kernel alone (``wd_ctc_loss``; DESIGN.md section 9 "CTC loss") at the shapes of OCR-aware training:
T = 256 steps, C classes, B = 64 samples, targets of L ids.

   python tools/ctc_time.py [--rounds R] [--calls K] [--warmup W] [--batch B] [--json PATH]

Legs: (C, L) = (51, 10), (80, 20), (80, 42) with the gradient, (80, 42) loss only, and (51, 10) replayed from a hipGraph of K calls.
After W warm-up calls of every leg: R rounds, in each round every leg in turn runs K calls between two host clock reads around a
device synchronise (legs interleaved).  Reported per leg: the median over the rounds of microseconds per call, and every round.
The calls of a leg are back to back on one stream, so a leg's figure is the kernel pair's duration, not its launch overhead,
once the duration exceeds the launch cost; the graph leg shows the difference."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from worddiffusion_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ctc_time.json"))
a = ap.parse_args()
dev, T, B = "cuda:0", 256, a.batch
lib = N.lib()


def leg(C, L, grad, graph=False):
    rs = np.random.RandomState(C + L)
    x = torch.from_numpy(rs.standard_normal((T, B, C)).astype(np.float32)).to(dev)
    tg = torch.from_numpy(rs.randint(1, C, (B, L)).astype(np.int32)).to(dev)
    il = torch.full((B,), T, dtype=torch.int32, device=dev)
    tl = torch.full((B,), L, dtype=torch.int32, device=dev)
    g = torch.empty_like(x) if grad else None
    nll, loss = torch.empty(B, device=dev), torch.empty(1, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = lib.wd_ctc_workspace_bytes(T, B, L)
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    keep = (x, tg, il, tl, g, nll, loss, status, work)

    def call():
        N.check(lib.wd_ctc_loss(x.data_ptr(), C, T, B, C, tg.data_ptr(), 0, L, L, il.data_ptr(), tl.data_ptr(), 1.0 / B,
                                g.data_ptr() if grad else None, C, nll.data_ptr(), loss.data_ptr(), status.data_ptr(),
                                work.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream), "wd_ctc_loss")

    if not graph:
        return keep, (lambda: [call() for _ in range(a.calls)]), loss
    call()
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        for _ in range(a.calls):
            call()
    return keep + (cg,), cg.replay, loss


legs = {"C51_L10": leg(51, 10, True), "C80_L20": leg(80, 20, True), "C80_L42": leg(80, 42, True),
        "C80_L42_loss_only": leg(80, 42, False), "C51_L10_graph": leg(51, 10, True, graph=True)}
for _, fn, _ in legs.values():
    for _ in range(a.warmup):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in legs}
for _ in range(a.rounds):
    for name, (_, fn, _) in legs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times[name].append(1e6 * (time.perf_counter() - t0) / a.calls)
out = dict(device=torch.cuda.get_device_name(0), T=T, batch=B, rounds=a.rounds, calls_per_round=a.calls, warmup_rounds=a.warmup,
           loss_finite=all(bool(torch.isfinite(l).all().item()) for _, _, l in legs.values()),
           legs={k: dict(us_per_call_median=statistics.median(v), us_per_call_min=min(v), us_per_call_max=max(v), us_per_call_rounds=v)
                 for k, v in times.items()})
print(json.dumps(out), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
with open(a.json, "w") as f:
    json.dump(out, f, indent=1)
