"""The training leg of bench.py on its own (configs[2] shape: batch 64, base UNet): ms per step in split-bf16 and single-pass bf16.
   python tools/train_time.py [steps] [--dropout P]      (P: nn.Dropout(P) in every ResBlock, DESIGN.md section 9 "Training dropout")"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from worddiffusion_amd import dist as wdist  # noqa: E402

argv = sys.argv[1:]
p_drop = 0.0
if "--dropout" in argv:
    i = argv.index("--dropout")
    p_drop = float(argv[i + 1])
    del argv[i:i + 2]
steps = int(argv[0]) if argv else 30
if p_drop:
    from worddiffusion_amd.layers import ResBlockParams  # noqa: E402
    _build_model = bench.build_model

    def build_model(*a, **k):  # the benchmark's model with UNetModel(..., dropout=P)'s ResBlocks
        model, args = _build_model(*a, **k)
        model.dropout = p_drop
        for mod in model.modules():
            if isinstance(mod, ResBlockParams):
                mod.out_layers[2].p = p_drop
        return model, args

    bench.build_model = build_model
out = bench.train_leg("cuda:0", "bf16x3", int(os.environ.get("B", "64")), steps, 5, 0, 1, torch.cuda.synchronize, wdist)
out["dropout"] = p_drop
print(json.dumps({k: out[k] for k in ("dropout", "ms_per_step", "images_per_sec", "loss_finite", "bf16_single_pass") if k in out}))
kc = out.get("kernel_classes")
if kc:
    print(json.dumps({k: v for k, v in kc.items() if v.get("launches_per_step")}))
