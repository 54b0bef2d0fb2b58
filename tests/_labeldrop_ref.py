"""The writer dropout of a training step, restated in plain numpy from its specification (DESIGN.md "Writer-free guidance") and from
nothing in the library: one Philox4x32-10 draw (tests/_philox_ref.py) per sample,

    counter = (0, tag, row & 0xffffffff, row >> 32)      key = (seed & 0xffffffff, seed >> 32)

with ``row = row_base + b`` the global sample row and ``tag = 0x80000000 | 5`` (WD_STREAM_LABEL_DROP); the sample keeps its writer
term iff output word 0 ``>= int(p * 2**32 + 0.5)``.  Nothing is scaled.

Also here: the float oracle with the writer term per sample (``KeepOracle``), and the one table of draws the GPU tests use."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import unet_oracle as U
from tests._philox_ref import counter_words

STREAM = 0x80000000
LABEL_DROP = 5


def threshold(p):
    return int(p * 2.0 ** 32 + 0.5)


def label_tag():
    return STREAM | LABEL_DROP


def keep_mask(seed, row_base, B, p):
    """bool [B]: True where the sample keeps its writer term."""
    row = np.uint64(int(row_base)) + np.arange(B, dtype=np.uint64)
    word0 = counter_words(seed, row, label_tag(), np.uint64(0))[0]
    return word0 >= np.uint64(threshold(p))


def y_eff(y, keep):
    """The ids label_emb's backward reads: y where kept, -1 where dropped."""
    return np.where(keep, np.asarray(y, dtype=np.int64), np.int64(-1))


# Every (seed, row_base, B, p) the GPU tests draw with, by name.  tests/test_writer_free_host.py asserts that each gives at least
# one kept and one dropped sample: a mask that keeps or drops everything tests nothing.  Chosen by evaluating keep_mask on the host.
# ("kernel B+B": the two launches of B rows at consecutive bases whose union is the 2B-row launch - each half is mixed as well.)
KERNEL_SEED = 1234
STEP_SEED = 77
DRAWS = {
    "kernel B=5 p=0.1": (KERNEL_SEED, 2, 5, 0.1),
    "kernel B=5 p=0.5": (KERNEL_SEED, 2, 5, 0.5),
    "kernel B=5 p=0.1, next rows": (KERNEL_SEED, 7, 5, 0.1),
    "kernel B=5 p=0.5, next rows": (KERNEL_SEED, 7, 5, 0.5),
    "kernel B=3 p=0.1": (KERNEL_SEED, 24, 3, 0.1),
    "kernel B=3 p=0.5": (KERNEL_SEED, 24, 3, 0.5),
    "kernel B=3 p=0.1, next rows": (KERNEL_SEED, 27, 3, 0.1),
    "kernel B=3 p=0.5, next rows": (KERNEL_SEED, 27, 3, 0.5),
    "kernel rows past 2^32": (KERNEL_SEED, (1 << 32) + 6, 5, 0.5),
    "step call 0": (STEP_SEED, 0, 3, 0.5),
    "step call 1": (STEP_SEED, 3, 3, 0.5),
    "step B=6": (STEP_SEED, 0, 6, 0.5),
}


class KeepOracle(U.UNetOracle):
    """``UNetOracle`` with the label term of unet.py:1575-1581 per sample: added where ``keep`` (bool [B]) holds, left out where it
    does not (the ``args.imgConditioned == 1`` branch); ``keep = None`` is the oracle itself."""
    keep = None

    def embed(self, t, y):
        if self.keep is None:
            return super().embed(t, y)
        sd = self.sd
        e = U.timestep_embedding(t, self.cfg["model_channels"], dtype=self.dtype)
        e = F.linear(e, sd["time_embed.0.weight"], sd["time_embed.0.bias"])
        e = F.linear(F.silu(e), sd["time_embed.2.weight"], sd["time_embed.2.bias"])
        keep = torch.as_tensor(np.asarray(self.keep, dtype=bool))
        if bool(keep.any()):
            rows = torch.zeros_like(e)
            rows[keep] = F.embedding(y.long()[keep], sd["label_emb.weight"]).to(e.dtype)
            e = e + rows  # (+ 0.0 where dropped: exact in any precision)
        return e
