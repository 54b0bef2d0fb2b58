#!/usr/bin/env python3
"""Golden vectors for writer-style interpolation (``mix_rate``), generated from the REFERENCE itself.

TEST INFRASTRUCTURE - not part of the product.  Run once, where a checkout of the reference is at hand:

    python tools/make_golden_interp.py <reference checkout> tests/golden

Same import stand-ins as ``oracle/make_golden.py``; the reference's modules are imported unmodified from the path on the
command line and only tensors are written.  Weights are ``synthetic_tensor`` fills (none stored).

  interp.npz
      SMALL config with ``num_classes = 339`` (``unet.py:1561`` hard-codes ``randint(0, 338)``), ``args.interpolation = True``,
      ``mix_rate = 0.37``:
      base_* / phosc_*   one eval forward of ``unet.UNetModel`` / ``unetPhosc.UNetModelPhosc`` after ``random.seed(rseed)``:
                         inputs, the pair the model drew (read off its ``label_emb`` lookups), output;
      cfg3_* / cfg0_*    ``train.Diffusion.sampling`` (T = 8, n = 3) driving ``UNetModelPhosc`` with ``cfg_scale`` 3 / 0 after
                         ``random.seed(rseed)``: start latent + recorded per-step noise, the pairs in draw order (14 / 7), the x
                         of every step and every single prediction of the model (two per step / one per step).
"""
from __future__ import annotations

import argparse
import os
import random
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import make_golden as MG  # noqa: E402
import make_golden_samplers as MS  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs  # noqa: E402

np_ = MG.np_
MIX_RATE = 0.37
CFG = dict(MG.SMALL, num_classes=339)


def pair_spy(model):
    """Every ``label_emb`` lookup of the interpolation branch is one id (``unet.py:1565-1568``): s1 then s2 per forward."""
    ids = []
    h = model.label_emb.register_forward_hook(lambda _m, inp, _out: ids.append(int(inp[0].reshape(-1)[0])))
    return ids, h


def gen_forward(out, tag, cls, base_variant, seed, rseed):
    args = MG.make_args(interpolation=True)
    torch.manual_seed(0)
    model = cls(args=args, **CFG).eval()
    fill_module_(model, seed)
    inp = synthetic_inputs(3, seed=seed + 2, hw=(4, 8), in_ch=CFG["in_channels"], num_classes=CFG["num_classes"],
                           max_len=CFG["max_seq_len"])
    ids, h = pair_spy(model)
    random.seed(rseed)
    with torch.no_grad():
        if base_variant:
            y = model(inp["x"], None, original_images=None, timesteps=inp["t"], context=inp["context"].clone(), y=inp["y"],
                      mix_rate=MIX_RATE)
        else:
            y = model(inp["x"], None, timesteps=inp["t"], context=inp["context"].clone(), y=inp["y"], mix_rate=MIX_RATE)
    h.remove()
    assert len(ids) == 2
    out.update({tag + "_x": np_(inp["x"]), tag + "_t": np_(inp["t"]), tag + "_context": np_(inp["context"]),
                tag + "_y": np_(inp["y"]), tag + "_pair": np.array(ids, dtype=np.int64), tag + "_out": np_(y),
                tag + "_seed": np.int64(seed), tag + "_rseed": np.int64(rseed)})
    print(f"[golden] interp {tag}: pair {ids} out mean|.|={np.abs(np_(y)).mean():.4f}")


def gen_traj(out, tag, ref_train, ref_phosc, cfg_scale, seed, rseed, n=3, T=8, word="MOVE"):
    args = MG.make_args(interpolation=True)
    torch.manual_seed(0)
    model = ref_phosc.UNetModelPhosc(args=args, **CFG).eval()
    fill_module_(model, seed)
    labels = torch.tensor([3, 0, 7], dtype=torch.int64)
    ids, h = pair_spy(model)
    xs, preds = [], []
    orig = model.forward

    def fwd(x, *a, **k):
        xs.append(np_(x).copy())
        y = orig(x, *a, **k)
        preds.append(np_(y).copy())
        return y

    model.forward = fwd
    diff = ref_train.Diffusion(noise_steps=T, img_size=(32, 64), args=args)
    random.seed(rseed)
    with MS.NoiseRecorder(seed * 7 + 1) as nr:
        img = diff.sampling(model, MS.IdentityVAE(), n, word, labels, args, mix_rate=MIX_RATE, cfg_scale=cfg_scale)
    model.forward = orig
    h.remove()
    per = 2 if cfg_scale > 0 else 1
    assert len(preds) == per * (T - 1) and len(ids) == 2 * len(preds)
    out.update({tag + "_noise": np.stack(nr.rec), tag + "_x_per_step": np.stack(xs[::per]), tag + "_pred": np.stack(preds),
                tag + "_pairs": np.array(ids, dtype=np.int64).reshape(-1, 2), tag + "_labels": np_(labels),
                tag + "_word": np.array(word), tag + "_T": np.int64(T), tag + "_image": np_(img), tag + "_seed": np.int64(seed),
                tag + "_rseed": np.int64(rseed), tag + "_cfg_scale": np.float64(cfg_scale)})
    print(f"[golden] interp {tag}: {len(preds)} forwards, pairs {np.array(ids).reshape(-1, 2).tolist()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("outdir")
    a = ap.parse_args()
    outdir = os.path.abspath(a.outdir)
    sys.dont_write_bytecode = True
    MG._install_stubs()
    sys.path.insert(0, os.path.abspath(a.reference))
    os.chdir(tempfile.mkdtemp())  # train.py writes two json files into the CWD at import
    torch.set_num_threads(8)

    import unet as ref_unet  # noqa
    import unetPhosc as ref_phosc  # noqa
    import train as ref_train  # noqa

    out = dict(mix_rate=np.float64(MIX_RATE), num_classes=np.int64(CFG["num_classes"]))
    gen_forward(out, "base", ref_unet.UNetModel, True, 71, 1001)
    gen_forward(out, "phosc", ref_phosc.UNetModelPhosc, False, 72, 1002)
    gen_traj(out, "cfg3", ref_train, ref_phosc, 3, 73, 1003)
    gen_traj(out, "cfg0", ref_train, ref_phosc, 0, 74, 1004)
    np.savez_compressed(os.path.join(outdir, "interp.npz"), **out)


if __name__ == "__main__":
    main()
