"""The batch sizes at which the launch plan of the forward changes its kernel forms: builds the FULL model once, plans
B = 1..N at 8 x 32 latents with 10 context tokens (phosc: plus the 769-int PHOSC vector) and prints one line per B whose plan
signature (tests/_plan_sig.py) differs from that of B - 1, with the summary of the difference.  Plans allocate device buffers, so it
needs the GPU; nothing but ``refresh_weights`` launches.  Every plan is released before the next one is built.

    python tools/plan_thresholds.py --variant base --max-batch 260 --out profiles/plan_thresholds_base.txt
    python tools/plan_thresholds.py --variant phosc --max-batch 130 --out profiles/plan_thresholds_phosc.txt
    python tools/plan_thresholds.py --variant base --min-batch 131 --max-batch 260     # a second range: compares 131 with 130

tests/test_plan_thresholds_host.py ties the tables of tests/test_gpu_batch_thresholds.py to the two committed files: a pull request
that moves a planner rule re-runs the scan and the tests then cover the new edges."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import _common as T  # noqa: E402
from tests._plan_sig import diff, signature_at  # noqa: E402
from worddiffusion_amd import UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_  # noqa: E402

PHOSC_LEN = 769

ap = argparse.ArgumentParser()
ap.add_argument("--variant", default="base", choices=["base", "phosc"])
ap.add_argument("--min-batch", type=int, default=1)
ap.add_argument("--max-batch", type=int, required=True)
ap.add_argument("--out", default="", help="also write the lines to this file")
a = ap.parse_args()
assert 1 <= a.min_batch <= a.max_batch

phosc_len = PHOSC_LEN if a.variant == "phosc" else 0
cls = UNetModel if a.variant == "base" else UNetModelPhosc
m = fill_module_(cls(args=T.make_args(device="cuda:0", phosc=1 if phosc_len else 0), **T.FULL), 1).to("cuda:0").eval()
eng = m.engine

lines = [f"# plan thresholds: FULL {a.variant}, 8x32 latents, 10 context tokens" + (f" + {phosc_len} PHOSC ints" if phosc_len else "") +
         f", B = {a.min_batch}..{a.max_batch}; a line per B whose plan differs from that of B - 1 (tools/plan_thresholds.py)"]
print(lines[0], flush=True)
t0 = time.time()
prev = signature_at(eng, a.min_batch - 1, phosc_len) if a.min_batch > 1 else None
for B in range(a.min_batch, a.max_batch + 1):
    sig = signature_at(eng, B, phosc_len)
    if prev is not None and sig != prev:
        lines.append(f"B={B}: {diff(prev, sig)}")
        print(lines[-1], flush=True)
    prev = sig
print(f"[plan_thresholds] {a.max_batch - a.min_batch + 1} plans in {time.time() - t0:.1f} s, {len(lines) - 1} thresholds", file=sys.stderr)
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
