"""The cases of the VAE threshold tests (tests/test_gpu_vae_thresholds.py, tests/test_vae_thresholds_host.py): configs, tags, the
batch sizes at which ``plan_decode`` / ``plan_encode`` change their kernel forms, and the input pools.  Imports without a GPU.

A tag is ``<dec|enc>_<shape>``; its scan is ``profiles/plan_thresholds_vae_<tag>.txt``, written by tools/plan_thresholds.py
(``scan_command(tag)`` is the command line).  Two families (SHAPES):
  batch   block_out_channels (128, 256), one layer per block, 8 x 32 latents (16 x 64 images): the decoder over B = 1..130 (the
          sampling batch of bench.py is 64, and ``Diffusion._finish`` hands ``decode`` whatever batch the sampler ran), the encoder over
          B = 1..16 (``AutoencoderKL.ENCODE_CHUNK``: it plans nothing larger)
  8x64, 16x32, 8x16, 6x26
          (64, 64, 128, 128), one layer per block - factor 8, as in production - at the latent sizes tests/_shapes.py gives the UNet,
          B = 1..16.  8 x 16 latents put two samples into a 128-row panel at the lowest level; 6 x 26 gives hw = 156, 624 and 2496
          (ragged against every tile, no fused statistics), then 9984 = 78 * 128.
THRESHOLDS is the B column of those files, copied; tests/test_vae_thresholds_host.py holds it to them."""
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_W = 11          # fill_module_ seed of every model here
ENCODE_CHUNK = 16    # AutoencoderKL.ENCODE_CHUNK (the host test compares)
SAMPLE_SCALE = (1.0, 0.5, 1.5)  # sample b of a pool is scaled by SAMPLE_SCALE[b % 3]: neighbours differ in GroupNorm statistics

_BATCH_CFG = dict(block_out_channels=(128, 256), layers_per_block=1)
_SHAPE_CFG = dict(block_out_channels=(64, 64, 128, 128), layers_per_block=1)
# shape -> (config, latent (h, w), top of the decoder scan, top of the encoder scan)
SHAPES = {
    "batch": (_BATCH_CFG, (8, 32), 130, ENCODE_CHUNK),
    "8x64": (_SHAPE_CFG, (8, 64), 16, 16),
    "16x32": (_SHAPE_CFG, (16, 32), 16, 16),
    "8x16": (_SHAPE_CFG, (8, 16), 16, 16),
    "6x26": (_SHAPE_CFG, (6, 26), 16, 16),
}
SHAPE_SWEEP = tuple(s for s in SHAPES if s != "batch")
TAGS = tuple(f"{d}_{s}" for s in SHAPES for d in ("dec", "enc"))

# the B column of profiles/plan_thresholds_vae_<tag>.txt
THRESHOLDS = {
    "dec_batch": (3, 4, 5, 6, 7, 9, 10, 11, 13, 16, 17, 22, 33, 64),
    "enc_batch": (9, 10, 11, 13, 16),
    "dec_8x64": (2, 5, 6, 8),
    "enc_8x64": (2, 5, 6, 8),
    "dec_16x32": (2, 5, 6, 8),
    "enc_16x32": (2, 5, 6, 8),
    "dec_8x16": (2, 5, 6, 8),
    "enc_8x16": (2, 8),
    "dec_6x26": (2, 4, 5, 7, 14),
    "enc_6x26": (2, 7, 14),
}
assert set(THRESHOLDS) == set(TAGS)

# 6 x 26 latents: the launches whose output map is the 48 x 208 one (hw = 9984 = 78 * 128), by the prefix of their ``what``; no other
# GEMM of these plans carries fused GroupNorm statistics (hw = 156, 624, 2496 are no multiple of the 128-row panel)
STAT_LEVEL_6x26 = {"dec_6x26": ("up2.us.", "up3."), "enc_6x26": ("encoder.conv_in", "down0.r0.")}


def split(tag) -> tuple:
    """tag -> (direction 'dec' | 'enc', shape)."""
    d, _, s = tag.partition("_")
    assert d in ("dec", "enc") and s in SHAPES, tag
    return d, s


def config(tag) -> dict:
    return SHAPES[split(tag)[1]][0]


def latent_hw(tag) -> tuple:
    return SHAPES[split(tag)[1]][1]


def image_hw(tag) -> tuple:
    f = len(config(tag)["block_out_channels"]) - 1
    h, w = latent_hw(tag)
    return h << f, w << f


def scanned_to(tag) -> int:
    d, s = split(tag)
    return SHAPES[s][2 if d == "dec" else 3]


def scan_file(tag) -> str:
    return os.path.join(ROOT, "profiles", f"plan_thresholds_vae_{tag}.txt")


def scan_command(tag) -> str:
    d, s = split(tag)
    cfg, (h, w) = config(tag), latent_hw(tag)
    return (f"python tools/plan_thresholds.py --variant vae-{d} --config {','.join(str(c) for c in cfg['block_out_channels'])}:"
            f"{cfg['layers_per_block']} --latent {h}x{w} --max-batch {scanned_to(tag)} --out profiles/plan_thresholds_vae_{tag}.txt")


def scan_header(tag) -> str:
    """What the first line of the tag's scan file holds: config, latent size and range."""
    d, _ = split(tag)
    cfg, (h, w), (H, W) = config(tag), latent_hw(tag), image_hw(tag)
    return (f"VAE {'decoder' if d == 'dec' else 'encoder'} block_out_channels={tuple(cfg['block_out_channels'])} "
            f"layers_per_block={cfg['layers_per_block']}, {h}x{w} latents ({H}x{W} images), B = 1..{scanned_to(tag)};")


def batch_sizes(tag) -> tuple:
    """b - 1 and b of every threshold (neighbours that coincide once); a shape-sweep tag also runs B = 1, 2, 3 and an encoder tag the
    full chunk, whose plan every larger batch replays."""
    d, s = split(tag)
    out = {B for b in THRESHOLDS[tag] for B in (b - 1, b)}
    if s in SHAPE_SWEEP:
        out |= {1, 2, 3}
    if d == "enc":
        out.add(ENCODE_CHUNK)
    return tuple(sorted(out))


def pool_size(tag) -> int:
    """The samples a tag's cases read: the pool and its float64 reference are made no larger."""
    return max(batch_sizes(tag))


ORACLE_CASES = [(t, B) for t in TAGS for B in batch_sizes(t)]        # decode / encode of the first B samples against the reference
THRESHOLD_CASES = [(t, b) for t in TAGS for b in THRESHOLDS[t]]      # the run at b against the run at b - 1


def pool_inputs(tag, n=None) -> torch.Tensor:
    """The first ``n`` (default: all) samples of the tag's pool on the CPU in fp32: latents ``randn * 3`` [n, 4, h, w] for a decoder tag, images
    uniform in [-1, 1] [n, 3, H, W] for an encoder tag - the distributions of tests/test_gpu_vae.py and tests/test_gpu_vae_encode.py
    - with sample b scaled by SAMPLE_SCALE[b % 3].  Sample b does not depend on ``n``."""
    d, s = split(tag)
    total = pool_size(tag)
    n = total if n is None else n
    assert 1 <= n <= total, (tag, n)
    g = torch.Generator().manual_seed(1000 + 2 * list(SHAPES).index(s) + (d == "enc"))
    if d == "dec":
        x = torch.randn(total, 4, *latent_hw(tag), generator=g) * 3.0
    else:
        x = torch.rand(total, 3, *image_hw(tag), generator=g) * 2 - 1
    x = x * torch.tensor([SAMPLE_SCALE[b % 3] for b in range(total)]).reshape(total, 1, 1, 1)
    # every sample is its own: a launch that read a neighbour's rows or statistics would not get away with it
    assert len({x[b].numpy().tobytes() for b in range(total)}) == total
    return x[:n].contiguous()


def build_model(tag):
    """The tag's ``AutoencoderKL`` on the CPU (synthetic weights, seed SEED_W; an encoder tag's with its encoder) and its state dict in
    float64 for the references."""
    from worddiffusion_amd.synthetic import fill_module_
    from worddiffusion_amd.vae import AutoencoderKL
    m = fill_module_(AutoencoderKL(with_encoder=split(tag)[0] == "enc", **config(tag)), SEED_W)
    return m, {k: v.double() for k, v in m.state_dict().items()}


def reference(tag, sd, x, chunk=8):
    """float64: ``oracle.vae_oracle.vae_decode`` -> image, or ``tests._vae_encode_ref.vae_encode`` -> (mean, clamped logvar), over ``x``
    in chunks of ``chunk`` samples."""
    from oracle.vae_oracle import vae_decode
    from tests._vae_encode_ref import vae_encode
    cfg = config(tag)
    fn = vae_decode if split(tag)[0] == "dec" else vae_encode
    with torch.no_grad():
        parts = [fn(sd, x[b0:b0 + chunk].double(), cfg["block_out_channels"], cfg["layers_per_block"]) for b0 in range(0, len(x), chunk)]
    if split(tag)[0] == "dec":
        return torch.cat(parts)
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
