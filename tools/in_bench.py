"""Micro-benchmark of the step's first layer at the headline shape (B = 64, 4 x 8 x 32 latents -> 320 channels): the direct fp32
convolution wd_conv3x3_in against the im2col + wd_gemm pair (WDIFF_FUSE_IN=0), each taken from the engine's own plan and timed as
the plan launches it (hipEvent pair around REP back-to-back repetitions, after warm passes of the whole step)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as B  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402

dev = torch.device("cuda:0")
batch = int(os.environ.get("BATCH", "64"))
REP = int(os.environ.get("REP", "200"))
HEAD = ("im2col", "input_blocks.0")

for fuse in ("0", "1"):
    os.environ["WDIFF_FUSE_IN"] = fuse  # (read when the model's engine is made)
    model, args = B.build_model(dev, "bf16x3", "base")
    run = B.StepRunner(model, args, dev, batch, 0, 0)
    P, st = run.P, run.stream.cuda_stream
    head = [(fn, a, what) for fn, a, what in P.step if what.startswith(HEAD)]
    with torch.cuda.stream(run.stream):
        for _ in range(3):
            P.run_step(st)
        run.stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(run.stream)
        for _ in range(REP):
            for fn, a, what in head:
                N.check(fn(*a, st), what)
        e1.record(run.stream)
        run.stream.synchronize()
    print(f"WDIFF_FUSE_IN={fuse} B={batch}: {' + '.join(getattr(fn, '__name__', str(fn)) for fn, _, _ in head)}: "
          f"{e0.elapsed_time(e1) * 1e3 / REP:.1f} us")
