"""Plain-torch restatement (dtype of its inputs: the tests run it in float64) of ``AutoencoderKL.encode`` of the published
``diffusers`` model for a state dict in ``diffusers`` naming - test infrastructure, in the style of ``oracle/vae_oracle.py``, whose
ResnetBlock2D / Attention / GroupNorm restatements it shares:

  Encoder.conv_in (3x3) -> per level: layers_per_block x ResnetBlock2D (+ Downsample2D: F.pad(x, (0, 1, 0, 1)), 3x3 stride 2 pad 0,
  every level but the last) -> UNetMidBlock2D [ResnetBlock2D, Attention, ResnetBlock2D] -> GroupNorm -> SiLU -> conv_out (3x3, 2L)
  -> quant_conv (1x1) -> DiagonalGaussianDistribution: mean, logvar = chunk(2, dim=1); logvar = clamp(logvar, -30, 20).
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch
import torch.nn.functional as F

from oracle.vae_oracle import _attention, _conv, _gn, _resnet


def vae_encode_moments(sd: Dict[str, torch.Tensor], x: torch.Tensor, block_out_channels: Sequence[int] = (128, 256, 512, 512),
                       layers_per_block: int = 2) -> torch.Tensor:
    """The output of ``quant_conv``: [B, 2L, h, w], before chunk and clamp."""
    h = _conv(sd, "encoder.conv_in", x, 1)
    n = len(block_out_channels)
    for i in range(n):
        for j in range(layers_per_block):
            h = _resnet(sd, f"encoder.down_blocks.{i}.resnets.{j}", h)
        if i != n - 1:
            k = f"encoder.down_blocks.{i}.downsamplers.0.conv"
            h = F.conv2d(F.pad(h, (0, 1, 0, 1)), sd[k + ".weight"], sd[k + ".bias"], stride=2)
    h = _resnet(sd, "encoder.mid_block.resnets.0", h)
    h = _attention(sd, "encoder.mid_block.attentions.0", h)
    h = _resnet(sd, "encoder.mid_block.resnets.1", h)
    h = _conv(sd, "encoder.conv_out", F.silu(_gn(sd, "encoder.conv_norm_out", h)), 1)
    return _conv(sd, "quant_conv", h, 0)


def vae_encode(sd, x, block_out_channels=(128, 256, 512, 512), layers_per_block=2) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean, clamped logvar) of ``vae.encode(x).latent_dist``."""
    mean, logvar = vae_encode_moments(sd, x, block_out_channels, layers_per_block).chunk(2, dim=1)
    return mean, logvar.clamp(-30.0, 20.0)


def posterior(mean: torch.Tensor, logvar: torch.Tensor, z: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    return scale * (mean + torch.exp(0.5 * logvar) * z)


def kl(mean: torch.Tensor, logvar: torch.Tensor) -> torch.Tensor:
    return 0.5 * torch.sum(mean ** 2 + torch.exp(logvar) - 1.0 - logvar, dim=[1, 2, 3])
