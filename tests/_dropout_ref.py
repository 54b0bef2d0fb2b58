"""The training dropout mask, restated in plain numpy from its specification ("Training dropout") and from
nothing in the library: one Philox4x32-10 draw (tests/_philox_ref.py) per four consecutive elements,

    counter = (e4, tag, row & 0xffffffff, row >> 32)      key = (seed & 0xffffffff, seed >> 32)

with ``idx = token * c + ch`` the token-major position inside one sample (``ch`` the channel inside the norm, ``c`` its channel
count), ``e4 = idx >> 2``, element ``idx`` reading output word ``idx & 3``; ``row = row_base + b`` is the global sample row,
``tag = 0x80000000 | (0x100 + layer)``; an element is kept iff ``word >= int(p * 2**32 + 0.5)`` and a kept one is multiplied by
``float32(1 / (1 - p))``."""
import numpy as np

from tests._philox_ref import counter_words

STREAM = 0x80000000
DROPOUT0 = 0x100


def threshold(p):
    return int(p * 2.0 ** 32 + 0.5)


def scale(p):
    return np.float32(1.0 / (1.0 - p))


def tag(layer):
    return STREAM | (DROPOUT0 + layer)


def keep_mask(seed, row_base, B, hw, c, layer, p):
    """bool [B, hw, c]: True where the element survives."""
    assert (hw * c) % 4 == 0
    row = (np.uint64(int(row_base)) + np.arange(B, dtype=np.uint64))[:, None]
    e4 = np.arange(hw * c // 4, dtype=np.uint64)[None, :]
    words = np.stack(counter_words(seed, row, tag(layer), e4), axis=-1)  # [B, hw * c / 4, 4]: word k is element 4 e4 + k
    return (words >= np.uint64(threshold(p))).reshape(B, hw, c)
