"""The batch sizes at which a launch plan changes its kernel forms: builds the model once, plans B = 1..N and prints one line per B
whose plan signature (tests/_plan_sig.py) differs from that of B - 1, with the summary of the difference.  Plans allocate device
buffers, so it needs the GPU; nothing but ``refresh_weights`` launches.  Every plan is released before the next one is built.

``--variant base | phosc``: the forward of the FULL model at 8 x 32 latents with 10 context tokens (phosc: plus the 769-int PHOSC
vector).

    python tools/plan_thresholds.py --variant base --max-batch 260 --out profiles/plan_thresholds_base.txt
    python tools/plan_thresholds.py --variant phosc --max-batch 130 --out profiles/plan_thresholds_phosc.txt
    python tools/plan_thresholds.py --variant base --min-batch 131 --max-batch 260     # a second range: compares 131 with 130

``--variant vae-dec | vae-enc``: ``plan_decode`` / ``plan_encode`` of an ``AutoencoderKL`` with ``--config`` (block_out_channels, then
``:`` and layers_per_block) at ``--latent HxW`` (the encoder is planned for the images that give such latents).  The encoder plans at
most ``AutoencoderKL.ENCODE_CHUNK`` images.

    python tools/plan_thresholds.py --variant vae-dec --config 128,256:1 --latent 8x32 --max-batch 130 \\
        --out profiles/plan_thresholds_vae_dec_batch.txt
    python tools/plan_thresholds.py --variant vae-enc --config 64,64,128,128:1 --latent 6x26 --max-batch 16 \\
        --out profiles/plan_thresholds_vae_enc_6x26.txt

``--variant train-base | train-phosc``: the training step of the same model and inputs, ``TrainEngine.plan_train`` - its forward
lists and its backward list (``train_signature_at``).

    python tools/plan_thresholds.py --variant train-base --max-batch 72 --out profiles/plan_thresholds_train_base.txt
    python tools/plan_thresholds.py --variant train-phosc --max-batch 32 --out profiles/plan_thresholds_train_phosc.txt

tests/test_plan_thresholds_host.py ties the tables of tests/test_gpu_batch_thresholds.py to the two committed UNet files and
those of tests/test_gpu_train_thresholds.py to the two training files,
tests/test_vae_thresholds_host.py those of tests/_vae_cases.py to the VAE files (``scan_command`` there gives each file's command
line): a pull request that moves a planner rule re-runs the scan and the tests then cover the new edges."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import _common as T  # noqa: E402
from tests._plan_sig import diff, signature_at, train_signature_at  # noqa: E402
from worddiffusion_amd import UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_  # noqa: E402

PHOSC_LEN = 769

scan_at = signature_at
ap = argparse.ArgumentParser()
ap.add_argument("--variant", default="base", choices=["base", "phosc", "train-base", "train-phosc", "vae-dec", "vae-enc"])
ap.add_argument("--min-batch", type=int, default=1)
ap.add_argument("--max-batch", type=int, required=True)
ap.add_argument("--config", default="128,256,512,512:2", help="vae-*: block_out_channels ':' layers_per_block")
ap.add_argument("--latent", default="8x32", help="vae-*: the latent size HxW")
ap.add_argument("--out", default="", help="also write the lines to this file")
a = ap.parse_args()
assert 1 <= a.min_batch <= a.max_batch

if a.variant.startswith("vae-"):
    from worddiffusion_amd.vae import AutoencoderKL
    boc, _, lpb = a.config.partition(":")
    boc, lpb = tuple(int(c) for c in boc.split(",")), int(lpb)
    lh, lw = (int(v) for v in a.latent.split("x"))
    enc = a.variant == "vae-enc"
    assert not enc or a.max_batch <= AutoencoderKL.ENCODE_CHUNK, "the encoder plans no more than ENCODE_CHUNK images"
    f = len(boc) - 1
    m = fill_module_(AutoencoderKL(block_out_channels=boc, layers_per_block=lpb, with_encoder=enc), 1).to("cuda:0").eval()
    eng = m.encoder_engine if enc else m.engine
    h, w = (lh << f, lw << f) if enc else (lh, lw)
    kw = dict(h=h, w=w, planner=eng.plan_encode if enc else eng.plan_decode)
    what = (f"VAE {'encoder' if enc else 'decoder'} block_out_channels={boc} layers_per_block={lpb}, {lh}x{lw} latents "
            f"({lh << f}x{lw << f} images)")
else:
    train = a.variant.startswith("train-")
    variant = a.variant[len("train-"):] if train else a.variant
    phosc_len = PHOSC_LEN if variant == "phosc" else 0
    cls = UNetModel if variant == "base" else UNetModelPhosc
    m = fill_module_(cls(args=T.make_args(device="cuda:0", phosc=1 if phosc_len else 0), **T.FULL), 1).to("cuda:0")
    m = m.train() if train else m.eval()
    eng = m.train_engine if train else m.engine
    if train:
        scan_at = train_signature_at
    kw = dict(phosc_len=phosc_len)
    what = (f"FULL {variant}{' training step' if train else ''}, 8x32 latents, 10 context tokens" +
            (f" + {phosc_len} PHOSC ints" if phosc_len else ""))

lines = [f"# plan thresholds: {what}, B = {a.min_batch}..{a.max_batch}; a line per B whose plan differs from that of B - 1 "
         "(tools/plan_thresholds.py)"]
print(lines[0], flush=True)
t0 = time.time()
prev = scan_at(eng, a.min_batch - 1, **kw) if a.min_batch > 1 else None
for B in range(a.min_batch, a.max_batch + 1):
    sig = scan_at(eng, B, **kw)
    if prev is not None and sig != prev:
        lines.append(f"B={B}: {diff(prev, sig)}")
        print(lines[-1], flush=True)
    prev = sig
print(f"[plan_thresholds] {a.max_batch - a.min_batch + 1} plans in {time.time() - t0:.1f} s, {len(lines) - 1} thresholds", file=sys.stderr)
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
