"""Host side of the training dropout (``nn.Dropout(p)`` of ``ResBlock.out_layers``, unet.py:616-623; DESIGN.md section 9,
"Training dropout"): the numbers the kernels are keyed with, so that a mask can be reproduced off the device.

One Philox4x32-10 draw covers four consecutive elements of a sample's token-major activation:

    counter = (e4, tag, row & 0xffffffff, row >> 32)      key = (seed & 0xffffffff, seed >> 32)
    idx = token * c + ch,  e4 = idx >> 2,  element idx reads output word idx & 3 and is kept iff word >= threshold(p)

``row`` is the global sample row, ``tag = tag(layer)`` and a kept element is multiplied by ``scale(p)``.

The writer dropout of a training step (DESIGN.md "Writer-free guidance") is one such draw per sample: counter (0, label_tag(), row),
the same key, word 0 against ``threshold(p)``; nothing is scaled.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from ._native import STREAM_DROPOUT0, STREAM_LABEL_DROP, WdDropout  # noqa: F401  (wd_dropout, WD_STREAM_* of include/wdiff_hip.h)

_KEY = "out_layers.3.weight"


def check_p(p: float) -> float:
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must be in [0, 1) to train, got {p}")
    return p


def threshold(p: float) -> int:
    """Element kept iff its 32-bit word >= threshold: int(p * 2**32 + 0.5)."""
    return int(check_p(p) * 2.0 ** 32 + 0.5)


def scale(p: float) -> np.float32:
    """fp32(1 / (1 - p)), the quotient taken in double first (what torch multiplies the kept elements by)."""
    return np.float32(1.0 / (1.0 - check_p(p)))


def tag(layer: int) -> int:
    return 0x80000000 | (STREAM_DROPOUT0 + int(layer))


def label_tag() -> int:
    """The tag of the writer dropout (``wd_label_rows_keep``): one draw per global sample row with counter (0, tag, row), the
    sample keeps its writer iff word 0 >= threshold(p).  Disjoint from every ``tag(layer)``, WD_TAG_KNOWN and the bare timesteps."""
    return 0x80000000 | STREAM_LABEL_DROP


def layer_ids(model) -> Dict[str, int]:
    """{state-dict prefix of a ResBlock (trailing dot included): layer}: the position of the block among the ``state_dict()``
    keys ending in ``out_layers.3.weight``.  Blocks the forward never runs (``res.*``) are numbered too."""
    keys = [k for k in model.state_dict().keys() if k.endswith(_KEY)]
    return {k[: -len(_KEY)]: i for i, k in enumerate(keys)}
