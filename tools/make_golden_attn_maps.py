#!/usr/bin/env python3
"""Golden vectors for the per-character cross-attention maps (``--attentionMaps 1``), generated from the REFERENCE itself.

TEST INFRASTRUCTURE - not part of the product.  Run once, where a checkout of the reference is at hand:

    python tools/make_golden_attn_maps.py <reference checkout> tests/golden

Same import stand-ins as ``oracle/make_golden.py``; the reference's modules are imported unmodified from the path on the
command line and only tensors are written.  Weights are ``synthetic_tensor`` fills (none stored).

  attn_maps_full.npz
      FULL config (64 x 256: the only geometry the reference's maps path runs at, unet.py:213-216,248-253), B = 2.  An
      ``attentionMaps=0`` ``unet.UNetModel`` is filled with ``fill_module_``; its state dict, renamed by
      ``to_attention_maps_state_dict`` (the middle block is registered as ``middle_block1`` with the flag, unet.py:1336-1364),
      loads strictly into an ``attentionMaps=1`` model.  Asserted here: the two ``eps`` are bit-equal, and each returned map is
      the pure x8 / x16 / x8 replication of its latent-resolution values.  Stored: the inputs, ``eps``, the three maps
      de-replicated ([2, 8, 32, 10], [2, 4, 16, 10], [2, 8, 32, 10]) and the returned ``context`` [2, 10, 320].
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
from worddiffusion_amd.model import remap_attention_maps_state_dict, to_attention_maps_state_dict  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs  # noqa: E402

np_ = MG.np_
SEED, BATCH = 81, 2
FACTORS = (8, 16, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("outdir")
    a = ap.parse_args()
    outdir = os.path.abspath(a.outdir)
    sys.dont_write_bytecode = True
    MG._install_stubs()
    sys.path.insert(0, os.path.abspath(a.reference))
    os.chdir(tempfile.mkdtemp())
    torch.set_num_threads(8)

    import unet as ref_unet  # noqa

    cfg = MG.FULL
    torch.manual_seed(0)
    plain = ref_unet.UNetModel(args=MG.make_args(attentionMaps=0), **cfg).eval()
    fill_module_(plain, SEED)
    torch.manual_seed(0)
    maps_model = ref_unet.UNetModel(args=MG.make_args(attentionMaps=1), **cfg).eval()
    sd = to_attention_maps_state_dict(plain.state_dict())
    maps_model.load_state_dict(sd, strict=True)
    assert list(remap_attention_maps_state_dict(maps_model.state_dict())) == list(plain.state_dict())
    inp = synthetic_inputs(BATCH, seed=SEED + 2, hw=(8, 32), in_ch=cfg["in_channels"], num_classes=cfg["num_classes"],
                           max_len=cfg["max_seq_len"])

    def call(m):
        with torch.no_grad():
            return m(inp["x"], None, original_images=None, timesteps=inp["t"], context=inp["context"].clone(), y=inp["y"])

    eps0 = call(plain)
    eps, a1, a2, a3, ctx = call(maps_model)
    assert torch.equal(eps0, eps), "the attentionMaps=1 model does not compute the attentionMaps=0 model's eps"
    small = []
    for m, f in zip((a1, a2, a3), FACTORS):
        assert tuple(m.shape) == (BATCH, 64, 256, 10), tuple(m.shape)
        s = m[:, ::f, ::f]
        assert torch.equal(m, s.repeat_interleave(f, 1).repeat_interleave(f, 2)), "not a pure replication"
        small.append(np_(s).copy())
    out = dict(x=np_(inp["x"]), t=np_(inp["t"]), context=np_(inp["context"]), y=np_(inp["y"]), eps=np_(eps),
               attn1=small[0], attn2=small[1], attn3=small[2], context_out=np_(ctx), seed=np.int64(SEED),
               factors=np.array(FACTORS, dtype=np.int64),
               maps_keys=np.array([k for k in maps_model.state_dict() if k.startswith("middle_block")]))
    np.savez_compressed(os.path.join(outdir, "attn_maps_full.npz"), **out)
    for n, m in zip(("attn1", "attn2", "attn3"), small):
        print(f"[golden] attn_maps_full {n}: {m.shape} min {m.min():.3f} max {m.max():.3f} sum over chars "
              f"{m.sum(-1).min():.6f} .. {m.sum(-1).max():.6f}")


if __name__ == "__main__":
    main()
