#!/usr/bin/env python3
"""Golden vectors for writer-free guidance (classifier-free guidance on the writer), generated from the REFERENCE itself.

TEST INFRASTRUCTURE - not part of the product.  Run once, where a checkout of the reference is at hand:

    python tools/make_golden_writer_free.py <reference checkout> tests/golden

Same import stand-ins as ``oracle/make_golden.py``; the reference's modules are imported unmodified from the path on the
command line and only tensors are written.  Weights are ``synthetic_tensor`` fills (none stored).

  writer_free.npz      SMALL config (``num_classes = 11``):
      base_*           ``unet.UNetModel``, one eval forward per variant on the same weights and inputs:
                       ``out_cond`` with ``args.imgConditioned = 0``, ``out_free`` with ``args.imgConditioned = 1`` (the label
                       term left out, unet.py:1578-1579) and ``out_zero`` with ``imgConditioned = 0`` and ``label_emb.weight``
                       zeroed - the construction the PHOSC model needs, shown by the host test to equal ``out_free``;
      phosc_*          ``unetPhosc.UNetModelPhosc``, which has no such flag: ``out_cond`` and ``out_free`` = the zeroed table;
      gb3_* / gb025_*  ``train.Diffusion.sampling`` (T = 8, n = 3, ``cfg_scale`` 3 / 0.25) on the base UNet,
      gp3_* / gp025_*  and on the PHOSC one.  The reference's loop calls its model twice per step with the same arguments
                       (train.py:223-228); here it drives ``TwoForwards``, which sends the first call of a step to the
                       conditional model and the second to the writer-free one, so the loop and the lerp are the reference's
                       own and the two forwards differ at last.  Start latent + recorded per-step noise, the x of every step,
                       every single prediction in call order (cond, free, cond, ...) and the image.
"""
from __future__ import annotations

import argparse
import os
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
CFG = dict(MG.SMALL)


def build(cls, seed, free, flag):
    """The reference model with the synthetic weights of ``seed``.  free: the writer-free one - through
    ``args.imgConditioned = 1`` where the class reads that flag (``flag``), else through a zeroed ``label_emb`` table."""
    args = MG.make_args(imgConditioned=1 if (free and flag) else 0)
    torch.manual_seed(0)
    model = cls(args=args, **CFG).eval()
    fill_module_(model, seed)
    if free and not flag:
        with torch.no_grad():
            model.label_emb.weight.zero_()
    return model, args


def call(model, base, x, t, context, y):
    if base:
        return model(x, None, original_images=None, timesteps=t, context=context.clone(), y=y)
    return model(x, None, timesteps=t, context=context.clone(), y=y)


def gen_forward(out, tag, cls, base, seed):
    inp = synthetic_inputs(3, seed=seed + 2, hw=(4, 8), in_ch=CFG["in_channels"], num_classes=CFG["num_classes"],
                           max_len=CFG["max_seq_len"])
    res = {}
    for name, free, flag in (("cond", False, False), ("free", True, base), ("zero", True, False)):
        if name == "zero" and not base:
            continue
        model, _ = build(cls, seed, free, flag)
        with torch.no_grad():
            res[name] = np_(call(model, base, inp["x"], inp["t"], inp["context"], inp["y"]))
    out.update({tag + "_x": np_(inp["x"]), tag + "_t": np_(inp["t"]), tag + "_context": np_(inp["context"]),
                tag + "_y": np_(inp["y"]), tag + "_seed": np.int64(seed)})
    out.update({f"{tag}_out_{k}": v for k, v in res.items()})
    print(f"[golden] writer_free {tag}: " + ", ".join(f"{k} mean|.|={np.abs(v).mean():.4f}" for k, v in res.items()) +
          f", max|cond - free|={np.abs(res['cond'] - res['free']).max():.4f}")


class TwoForwards:
    """What ``train.Diffusion.sampling`` is handed as its model: call 2k goes to the conditional model, call 2k + 1 to the
    writer-free one (with ``cfg_scale > 0`` the loop makes exactly two calls per step, train.py:223-227)."""

    def __init__(self, cond, free, base):
        self.models, self.base, self.xs, self.preds = (cond, free), base, [], []

    def eval(self):
        return self

    def train(self):
        return self

    def __call__(self, x, _unused, t, context, y, mix_rate=None):
        model = self.models[len(self.preds) % 2]
        self.xs.append(np_(x).copy())
        pred = call(model, self.base, x, t, context, y)
        self.preds.append(np_(pred).copy())
        return pred


def gen_traj(out, tag, ref_train, cls, base, cfg_scale, seed, n=3, T=8, word="MOVE"):
    cond, args = build(cls, seed, False, False)
    free, _ = build(cls, seed, True, base)
    labels = torch.tensor([3, 0, 7], dtype=torch.int64)
    two = TwoForwards(cond, free, base)
    diff = ref_train.Diffusion(noise_steps=T, img_size=(32, 64), args=args)
    with MS.NoiseRecorder(seed * 7 + 1) as nr:
        img = diff.sampling(two, MS.IdentityVAE(), n, word, labels, args, cfg_scale=cfg_scale)
    assert len(two.preds) == 2 * (T - 1)
    out.update({tag + "_noise": np.stack(nr.rec), tag + "_x_per_step": np.stack(two.xs[::2]), tag + "_pred": np.stack(two.preds),
                tag + "_labels": np_(labels), tag + "_word": np.array(word), tag + "_T": np.int64(T), tag + "_image": np_(img),
                tag + "_seed": np.int64(seed), tag + "_cfg_scale": np.float64(cfg_scale)})
    print(f"[golden] writer_free {tag}: {len(two.preds)} forwards, scale {cfg_scale}")


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

    out = dict(num_classes=np.int64(CFG["num_classes"]))
    gen_forward(out, "base", ref_unet.UNetModel, True, 81)
    gen_forward(out, "phosc", ref_phosc.UNetModelPhosc, False, 82)
    gen_traj(out, "gb3", ref_train, ref_unet.UNetModel, True, 3, 83)
    gen_traj(out, "gb025", ref_train, ref_unet.UNetModel, True, 0.25, 84)
    gen_traj(out, "gp3", ref_train, ref_phosc.UNetModelPhosc, False, 3, 85)
    gen_traj(out, "gp025", ref_train, ref_phosc.UNetModelPhosc, False, 0.25, 86)
    np.savez_compressed(os.path.join(outdir, "writer_free.npz"), **out)


if __name__ == "__main__":
    main()
