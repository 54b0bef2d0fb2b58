"""The model shapes the reference's scripts and constructor can ask for beyond FULL / SMALL / DEEP: ``--num_heads``,
``--num_res_blocks``, ``--emb_dim``, ``--img_size`` and the ``channel_mult`` / ``attention_resolutions`` / ``context_dim`` keywords.

``SHAPES``: tag -> (cfg, variant, latent (h, w)); every cfg is FULL with keys overridden.  A base model needs
``context_dim == ch`` at every level that has a SpatialTransformer: the reference builds ``attn1`` without ``context_dim`` and
calls it with the context (unet.py:337-345).  ``oracle/make_golden_shapes.py`` writes one golden forward of the reference per tag
(``tests/golden/fwd_shape_<tag>.npz``), tests/test_shapes_host.py pins the oracle and this table to them, tests/test_gpu_shapes.py
runs the HIP path.

What each tag is there to reach (the planner picks kernel forms from these numbers, engine.py / train_engine.py):
  heads1, heads2   320 channels with d = 320 / 160: the folded cross-attention pair, the wd_ff_fused front and wd_xattn_fold with a
                   head stride no FULL test gives them
  heads8           heads * L = 80 > 40: wd_xattn_supported refuses, the blocks run plain wd_attention (nk = 10, d = 40) in front of a
                   wd_ff_fused tail
  res2             two ResBlocks per level: three decoder blocks per level, the Upsample behind a SpatialTransformer
  emb96/160/256    widths that are neither 64 nor 320: the generic GEMM forms everywhere (no wd_ff_fused, 256: no folded attention)
  mult12           640 channels at the 4 x 16 level; the decoder GroupNorm behind the Upsample has 640 + 320 channels, cpg = 30, its
                   groups straddle the concat
  mult124          three levels from 64 channels, attention at the lowest (2 x 8) only
  full_8x64        w = 64, the edge of both direct convolutions; full_16x32: 512 tokens; full_8x16: hw = 32 at the lower level, so
                   64-row panels straddle samples; full_6x26: hw = 156 and 39, ragged against every 64-row tile
  phosc_*          the PHOSC variant (self-attention + 779-key cross-attention) with 8 heads, with a 640-channel level, at 128 channels

``BATCHES``: tag -> the batch sizes of the GPU forward test.  They hold ragged tails and b - 1 / b of the planner rules that can be
derived by hand for the shape (the 192-panel rule, ``wdirect_fills_chip`` for the phase Upsample; tests/test_shapes_host.py recomputes both),
plus b - 1 / b of every batch size at which the plan changes its kernel family (``FAMILY_THRESHOLDS``: found by planning every batch
of the sweep, and recomputed by ``test_plans_build_at_every_batch`` of tests/test_gpu_shapes.py)."""
from tests._common import FULL

PHOSC_LEN = 769
CTX_LEN = 10


def _cfg(**kw):
    cfg = dict(FULL)
    cfg.update(kw)
    return cfg


SHAPES = {
    "heads1": (_cfg(num_heads=1), "base", (8, 32)),
    "heads2": (_cfg(num_heads=2), "base", (8, 32)),
    "heads8": (_cfg(num_heads=8), "base", (8, 32)),
    "res2": (_cfg(num_res_blocks=2), "base", (8, 32)),
    "emb96": (_cfg(model_channels=96, context_dim=96), "base", (8, 32)),
    "emb160": (_cfg(model_channels=160, context_dim=160), "base", (8, 32)),
    "emb256": (_cfg(model_channels=256, context_dim=256), "base", (8, 32)),
    "mult12": (_cfg(channel_mult=(1, 2), attention_resolutions=(2,), context_dim=640), "base", (8, 32)),
    "mult124": (_cfg(model_channels=64, channel_mult=(1, 2, 4), attention_resolutions=(4,), context_dim=256), "base", (8, 32)),
    "full_8x64": (_cfg(), "base", (8, 64)),
    "full_16x32": (_cfg(), "base", (16, 32)),
    "full_8x16": (_cfg(), "base", (8, 16)),
    "full_6x26": (_cfg(), "base", (6, 26)),
    "phosc_heads8": (_cfg(num_heads=8), "phosc", (8, 32)),
    "phosc_mult12": (_cfg(channel_mult=(1, 2), attention_resolutions=(1, 2)), "phosc", (8, 32)),
    "phosc_emb128": (_cfg(model_channels=128, context_dim=128), "phosc", (8, 32)),
}

# ---- the batch sizes the issue's table gives: ragged tails and b - 1 / b of the hand-derived planner rules
_B_320 = (1, 2, 3, 5, 8, 16, 17, 31, 32, 33, 47, 48, 64, 65)
_B_NARROW = (1, 2, 3, 5, 8, 16, 17, 32, 33, 64, 65)
_B_WIDE_MAP = (1, 2, 3, 5, 8, 16, 17, 23, 24, 31, 32, 33)
_B_PHOSC = (1, 2, 3, 8, 16, 17, 32, 33, 47, 48, 64, 65)
_LISTED = {
    "heads1": _B_320, "heads2": _B_320, "heads8": _B_320, "res2": _B_320, "mult12": _B_320,
    "emb96": _B_NARROW, "emb160": _B_NARROW, "emb256": _B_NARROW, "mult124": _B_NARROW,
    "full_8x64": _B_WIDE_MAP, "full_16x32": _B_WIDE_MAP,
    "full_8x16": (1, 2, 3, 8, 17, 33, 64, 65, 95, 96, 127, 128, 129),
    "full_6x26": (1, 2, 3, 5, 17, 33, 78, 79),   # (79: the first batch with ceil(156 B / 64) >= 192)
    "phosc_heads8": _B_PHOSC, "phosc_mult12": _B_PHOSC, "phosc_emb128": _B_PHOSC,
}
# ---- the batch sizes b at which the plan of b launches another kernel family than that of b - 1, over B = 1 .. sweep_limit(tag):
# a wd_gemm launch changes its kernel (wd_gemm_check_kernel), a wd_ff_fused launch its form, or the set of launched functions
# changes.  (A tile or K-cut change inside one kernel is no entry.)  tests/test_gpu_shapes.py::test_plans_build_at_every_batch
# recomputes this table from the plans and holds it to that.
FAMILY_THRESHOLDS = {
    "heads1": (2, 7, 16, 32, 39, 48, 63, 64, 65, 97, 129),
    "heads2": (2, 7, 16, 32, 39, 48, 63, 64, 65, 97, 129),
    "heads8": (2, 7, 16, 32, 39, 48, 63, 64, 65, 97, 129),
    "res2": (2, 7, 16, 26, 32, 48, 63, 64, 65, 129),
    "emb96": (),
    "emb160": (64,),
    "emb256": (),
    "mult12": (16, 31, 32, 45, 64, 65, 128, 129),
    "mult124": (),
    "full_8x64": (7, 8, 16, 24, 32, 39),
    "full_16x32": (7, 8, 16, 24, 32, 39),
    "full_8x16": (3, 7, 32, 39, 64, 65, 96, 97, 125, 128),
    "full_6x26": (2, 7, 26, 39, 52, 65, 79, 97, 102, 105),
    "phosc_heads8": (2, 3, 4, 7, 8, 11, 16, 22, 32, 43, 48, 63, 64, 65, 86, 129),
    "phosc_mult12": (4, 6, 7, 8, 11, 16, 22, 31, 32, 43, 48, 64, 65, 128, 129),
    "phosc_emb128": (),
}
BATCHES = {tag: tuple(sorted(set(_LISTED[tag]) | {B for b in FAMILY_THRESHOLDS[tag] for B in (b - 1, b)})) for tag in SHAPES}
assert set(_LISTED) == set(FAMILY_THRESHOLDS) == set(SHAPES)

# the gradient cases of tests/test_gpu_shapes.py (B = 3)
GRAD_TAGS = ("heads1", "heads2", "heads8", "res2", "emb160", "emb256", "mult12", "mult124", "full_6x26", "phosc_heads8",
             "phosc_emb128")


def phosc_len(tag) -> int:
    return PHOSC_LEN if SHAPES[tag][1] == "phosc" else 0


def sweep_limit(tag) -> int:
    """The plan sweep covers B = 1 .. this (B <= 40 for the 512-token maps, which hold twice the rows per sample)."""
    h, w = SHAPES[tag][2]
    return 40 if h * w > 256 else 130


def levels(tag) -> list:
    """(channels, (h, w), has a SpatialTransformer) per level of the UNet, top level first."""
    cfg, _, (h, w) = SHAPES[tag]
    out = []
    for i, m in enumerate(cfg["channel_mult"]):
        out.append((cfg["model_channels"] * m, (h >> i, w >> i), (1 << i) in cfg["attention_resolutions"]))
    return out

