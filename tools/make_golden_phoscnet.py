"""Golden outputs of the reference's own PHOSCnet (ResPhoSCNetZSL/modules/models.py, imported unmodified) on synthetic weights.

    python tools/make_golden_phoscnet.py <reference checkout> tests/golden

``timm`` is not installed here; ``models.py`` only takes the ``register_model`` decorator from it, so an identity decorator is put
into ``sys.modules`` under ``timm.models.registry`` before the import (as the other golden tools do for their missing imports).
The model is filled with ``synthetic.fill_module_(seed=7)`` and every >= 2-D weight is multiplied by sqrt(2): without that gain
the ReLU stack shrinks the logits to a standard deviation of ~0.07 and the sigmoid hides errors.  Written to
``tests/golden/phoscnet.npz``: two uint8 images [2, 3, 50, 250] from a fixed RandomState, the fp32 outputs (phos, phoc, the 4096
features, both heads' pre-activation logits), the (mean, abs-max) of every convolution's output, the state_dict's keys and shapes
and a CRC of the weights.  The weights themselves are never written: the tests regenerate them from the seed.
"""
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _phoscnet_ref as R  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_  # noqa: E402


def reference_model(checkout: str):
    timm, models, registry = types.ModuleType("timm"), types.ModuleType("timm.models"), types.ModuleType("timm.models.registry")
    registry.register_model = lambda fn: fn
    timm.models, models.registry = models, registry
    sys.modules.update({"timm": timm, "timm.models": models, "timm.models.registry": registry})
    sys.path.insert(0, os.path.join(checkout, "ResPhoSCNetZSL"))
    from modules.models import PHOSCnet
    return PHOSCnet()


def main(checkout: str, out_dir: str):
    torch.manual_seed(0)
    net = fill_module_(reference_model(checkout), 7).eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() >= 2:
                p.mul_(torch.tensor(math.sqrt(2.0), dtype=torch.float32))
    images = np.random.RandomState(20240607).randint(0, 256, size=(2, 3, 50, 250)).astype(np.uint8)
    x = torch.from_numpy(images).float() / 255.0
    stats, logits = [], {}
    hooks = [m.register_forward_hook(lambda _m, _i, o: stats.append((float(o.mean()), float(o.abs().max()))))
             for m in net.conv if isinstance(m, torch.nn.Conv2d)]
    hooks += [net.phos[6].register_forward_hook(lambda _m, _i, o: logits.__setitem__("phos", o.detach().clone())),
              net.phoc[6].register_forward_hook(lambda _m, _i, o: logits.__setitem__("phoc", o.detach().clone()))]
    with torch.no_grad():
        feat = net.temporal_pool(net.conv(x))
        del stats[:]
        out = net(x)
    for hk in hooks:
        hk.remove()
    sd = net.state_dict()
    keys = list(sd)
    path = os.path.join(out_dir, "phoscnet.npz")
    np.savez_compressed(path, images=images, phos=out["phos"].numpy(), phoc=out["phoc"].numpy(), features=feat.numpy(),
                        phos_logits=logits["phos"].numpy(), phoc_logits=logits["phoc"].numpy(),
                        conv_stats=np.array(stats, dtype=np.float64), keys=np.array(keys),
                        shapes=np.array([",".join(str(d) for d in sd[k].shape) for k in keys]),
                        crc=np.array([R.weights_crc(sd)], dtype=np.uint32), seed=np.array([7]), gain=np.array([math.sqrt(2.0)]))
    print(f"[golden] phoscnet: feature std {float(feat.std()):.3f}, phos logit std {float(logits['phos'].std()):.3f}, "
          f"phoc logit std {float(logits['phoc'].std()):.3f}; {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
