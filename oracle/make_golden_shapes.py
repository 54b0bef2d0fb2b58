#!/usr/bin/env python3
"""Golden forwards of the REFERENCE's own UNets at every shape of ``tests/_shapes.SHAPES`` (TEST INFRASTRUCTURE, run once where
the reference checkout is mounted):

    python oracle/make_golden_shapes.py /path/to/reference tests/golden

One ``fwd_shape_<tag>.npz`` per tag: B = 2, seed 7, no hooks - the inputs, the reference's output and the key / shape lists of its
state_dict; the weights are regenerated from the seed (``worddiffusion_amd.synthetic``).  The reference's ``unet.py`` and
``unetPhosc.py`` are imported unmodified from the path on the command line, with the stand-ins of ``oracle/make_golden.py``;
nothing of the reference's text is copied, only tensors are written."""
from __future__ import annotations

import io
import os
import sys
import tempfile
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle.make_golden import _install_stubs, gen_forward, make_args  # noqa: E402
from tests._shapes import SHAPES, phosc_len  # noqa: E402

BATCH, SEED = 2, 7


def rewrite_without_timestamps(path):
    """``np.savez_compressed`` stamps every member with the time of writing; the same arrays under a fixed date, so that a second
    run of this script writes the same bytes."""
    with np.load(path, allow_pickle=False) as g:
        arrays = {k: g[k] for k in g.files}
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ref, outdir = sys.argv[1], os.path.abspath(sys.argv[2])
    os.makedirs(outdir, exist_ok=True)
    sys.dont_write_bytecode = True
    _install_stubs()
    sys.path.insert(0, os.path.abspath(ref))
    os.chdir(tempfile.mkdtemp())
    torch.set_num_threads(8)

    import unet as ref_unet  # noqa
    import unetPhosc as ref_phosc  # noqa

    for tag, (cfg, variant, hw) in SHAPES.items():
        base = variant == "base"
        cls = ref_unet.UNetModel if base else ref_phosc.UNetModelPhosc
        gen_forward(outdir, "fwd_shape_" + tag, cls, cfg, make_args(phosc=0 if base else 1), SEED, BATCH, hw, base,
                    phosc_len=phosc_len(tag))
        rewrite_without_timestamps(os.path.join(outdir, f"fwd_shape_{tag}.npz"))


if __name__ == "__main__":
    main()
