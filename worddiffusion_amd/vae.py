"""The Stable-Diffusion-v1.5 ``AutoencoderKL`` on the HIP kernels of this package: ``decode`` always,
``encode`` when the object is built with ``with_encoder=True`` (``from_pretrained`` sets it when the checkpoint has an encoder).

Reference call sites: ``AutoencoderKL.from_pretrained(args.stable_dif_path, subfolder="vae")`` (``train.py:415``,
``sampling.py:108``) and, at the end of every sampler, ``latents = 1 / 0.18215 * x; image = vae.decode(latents).sample;
image = (image / 2 + 0.5).clamp(0, 1)`` (``train.py:239-247``).  ``diffusers`` is not part of the reference tree: the
architecture below restates the published ``diffusers`` model (``models/autoencoder_kl.py``, ``models/vae.py::Decoder``,
``UNetMidBlock2D``, ``UpDecoderBlock2D``, ``ResnetBlock2D``, ``Attention``, ``Upsample2D``) for the SD-v1.5 VAE config
(block_out_channels (128, 256, 512, 512), layers_per_block 2, latent_channels 4, norm_num_groups 32, eps 1e-6, one
attention head of 512 channels in the mid block).

**Parity unpinned**: neither ``diffusers`` nor any VAE weights exist offline, so the HIP path is
checked against ``oracle/vae_oracle.py`` - a plain-torch restatement of the same published architecture - on synthetic
weights; a real checkpoint in ``diffusers`` layout loads through ``load_state_dict`` / ``from_pretrained`` (state-dict
keys and shapes are the ``diffusers`` ones, both attention namings).

The encoder serves the default training path of the reference, ``images = vae.encode(images.to(torch.float32))
.latent_dist.sample(); images = images * 0.18215`` (``train.py:277-278``, ``trainModifyCondition.py:703-705``), and the making
of a latent cache for ``--vaeFromDict 1`` (``latents.build_latent_cache``).  It restates ``models/vae.py::Encoder`` /
``DownEncoderBlock2D`` / ``Downsample2D`` (zero padding right and bottom, then 3x3 stride 2) / ``DiagonalGaussianDistribution``
of the same published model; forward only (the reference never trains the VAE).  The posterior noise is the package's on-device
Philox stream, keyed by ``(seed, sample_offset + sample index)``, not ``torch.randn``.

A default ``AutoencoderKL()`` stays decoder-only: same ``state_dict`` keys as before the encoder existed, ``encoder.*`` /
``quant_conv.*`` entries of a checkpoint are dropped on load.  There is no CPU fallback: ``decode`` / ``encode`` need the model
on an MI355X.
"""
from __future__ import annotations

import json
import os
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from . import _native as N
from .engine import _NATIVE_WRITES, _PARAM_GEN, Act, Plan, RecipeBook, UNetEngine

SD15_VAE_CONFIG = dict(in_channels=3, out_channels=3, latent_channels=4, block_out_channels=(128, 256, 512, 512),
                       layers_per_block=2, norm_num_groups=32, scaling_factor=0.18215)


class _Resnet(nn.Module):
    """``ResnetBlock2D`` without time embedding (``temb_channels=None``), eps 1e-6, SiLU."""

    def __init__(self, cin: int, cout: int, groups: int):
        super().__init__()
        self.cin, self.cout = cin, cout
        self.norm1 = nn.GroupNorm(groups, cin, eps=1e-6)
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1)
        self.norm2 = nn.GroupNorm(groups, cout, eps=1e-6)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)


class _Attention(nn.Module):
    """``Attention`` of the VAE mid block: GroupNorm, one head over all channels, biased projections, residual."""

    def __init__(self, ch: int, groups: int):
        super().__init__()
        self.ch = ch
        self.group_norm = nn.GroupNorm(groups, ch, eps=1e-6)
        self.to_q = nn.Linear(ch, ch)
        self.to_k = nn.Linear(ch, ch)
        self.to_v = nn.Linear(ch, ch)
        self.to_out = nn.ModuleList([nn.Linear(ch, ch), nn.Dropout(0.0)])


class _Mid(nn.Module):
    def __init__(self, ch: int, groups: int):
        super().__init__()
        self.attentions = nn.ModuleList([_Attention(ch, groups)])
        self.resnets = nn.ModuleList([_Resnet(ch, ch, groups), _Resnet(ch, ch, groups)])


class _Upsampler(nn.Module):
    def __init__(self, ch: int):
        super().__init__()
        self.cin = self.cout = ch
        self.conv = nn.Conv2d(ch, ch, 3, padding=1)


class _UpBlock(nn.Module):
    def __init__(self, cin: int, cout: int, nlayers: int, groups: int, upsample: bool):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet(cin if j == 0 else cout, cout, groups) for j in range(nlayers)])
        if upsample:
            self.upsamplers = nn.ModuleList([_Upsampler(cout)])


class _Decoder(nn.Module):
    def __init__(self, latent: int, out_ch: int, boc: Sequence[int], layers_per_block: int, groups: int):
        super().__init__()
        self.conv_in = nn.Conv2d(latent, boc[-1], 3, padding=1)
        self.mid_block = _Mid(boc[-1], groups)
        rev = list(reversed(boc))
        ups, prev = [], rev[0]
        for i, ch in enumerate(rev):
            ups.append(_UpBlock(prev, ch, layers_per_block + 1, groups, upsample=i != len(rev) - 1))
            prev = ch
        self.up_blocks = nn.ModuleList(ups)
        self.conv_norm_out = nn.GroupNorm(groups, boc[0], eps=1e-6)
        self.conv_out = nn.Conv2d(boc[0], out_ch, 3, padding=1)


class _Downsampler(nn.Module):
    """``Downsample2D``: ``F.pad(x, (0, 1, 0, 1))`` then this 3x3 / stride 2 / padding 0 convolution."""

    def __init__(self, ch: int):
        super().__init__()
        self.cin = self.cout = ch
        self.conv = nn.Conv2d(ch, ch, 3, stride=2, padding=0)


class _DownBlock(nn.Module):
    def __init__(self, cin: int, cout: int, nlayers: int, groups: int, downsample: bool):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet(cin if j == 0 else cout, cout, groups) for j in range(nlayers)])
        if downsample:
            self.downsamplers = nn.ModuleList([_Downsampler(cout)])


class _Encoder(nn.Module):
    def __init__(self, in_ch: int, latent: int, boc: Sequence[int], layers_per_block: int, groups: int):
        super().__init__()
        self.conv_in = nn.Conv2d(in_ch, boc[0], 3, padding=1)
        downs, prev = [], boc[0]
        for i, ch in enumerate(boc):
            downs.append(_DownBlock(prev, ch, layers_per_block, groups, downsample=i != len(boc) - 1))
            prev = ch
        self.down_blocks = nn.ModuleList(downs)
        self.mid_block = _Mid(boc[-1], groups)
        self.conv_norm_out = nn.GroupNorm(groups, boc[-1], eps=1e-6)
        self.conv_out = nn.Conv2d(boc[-1], 2 * latent, 3, padding=1)


class DecoderOutput:
    """What ``vae.decode`` returns in ``diffusers`` (the samplers read ``.sample``)."""

    def __init__(self, sample: torch.Tensor):
        self.sample = sample


def _draw_seed(seed: Optional[int], generator=None) -> int:
    """An explicit ``seed`` wins; a ``generator`` supplies it by one integer draw (re-seeding it reproduces the sample); otherwise
    one draw from torch's global generator, as ``Diffusion.sampling(seed=None)``."""
    if seed is not None:
        return int(seed)
    if generator is not None:
        return int(torch.randint(0, 2 ** 62, (1,), generator=generator, device=generator.device).item())
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class DiagonalGaussianDistribution:
    """The posterior ``vae.encode(x).latent_dist`` of ``diffusers``: ``mean`` and ``logvar`` (clamped to [-30, 20]) are the NCHW
    fp32 outputs of ``wd_vae_posterior``; ``sample`` is one ``wd_posterior_sample`` launch.  ``std`` / ``var`` / ``parameters`` /
    ``kl`` are conveniences off every hot path (plain tensor expressions of the two stored maps)."""

    def __init__(self, mean: torch.Tensor, logvar: torch.Tensor):
        self.mean, self.logvar = mean, logvar

    @property
    def std(self) -> torch.Tensor:
        return torch.exp(0.5 * self.logvar)

    @property
    def var(self) -> torch.Tensor:
        return torch.exp(self.logvar)

    @property
    def parameters(self) -> torch.Tensor:
        """[B, 2L, h, w]: mean | logvar (the clamped logvar: the unclamped moments are not kept)."""
        return torch.cat([self.mean, self.logvar], dim=1)

    def mode(self) -> torch.Tensor:
        return self.mean

    def kl(self) -> torch.Tensor:
        m, lv = self.mean.double(), self.logvar.double()
        return (0.5 * torch.sum(m * m + torch.exp(lv) - 1.0 - lv, dim=[1, 2, 3])).float()

    def sample(self, generator=None, *, seed: Optional[int] = None, sample_offset: int = 0, scale: float = 1.0,
               noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``scale * (mean + std * z)``; sample ``i``'s ``z`` depends on ``(seed, sample_offset + i)`` only.  ``noise`` (same shape)
        replaces the Philox stream (parity tests)."""
        mean = self.mean
        B, n = mean.shape[0], mean[0].numel()
        out = torch.empty_like(mean)
        if noise is not None:
            noise = noise.to(mean.device, torch.float32).contiguous()
            if noise.shape != mean.shape:
                raise ValueError(f"noise must be {tuple(mean.shape)}, got {tuple(noise.shape)}")
        st = torch.cuda.current_stream(mean.device).cuda_stream
        N.check(N.lib().wd_posterior_sample(mean.data_ptr(), self.logvar.data_ptr(), B, n, out.data_ptr(), float(scale),
                                            noise.data_ptr() if noise is not None else None,
                                            0 if noise is not None else _draw_seed(seed, generator), int(sample_offset), st),
                "wd_posterior_sample")
        return out


class AutoencoderKLOutput:
    """What ``vae.encode`` returns in ``diffusers`` (the training loops read ``.latent_dist``)."""

    def __init__(self, latent_dist: DiagonalGaussianDistribution):
        self.latent_dist = latent_dist


class AutoencoderKL(nn.Module):
    """``decode(z).sample`` = image in [-1, 1] nominal range, [B, 3, 8h, 8w]; with ``with_encoder=True`` also
    ``encode(x).latent_dist`` for images [B, 3, H, W] (H, W multiples of ``2**(levels - 1)``)."""

    ENCODE_CHUNK = 16  # images per encoder launch plan: a larger batch runs as replays of it

    def __init__(self, in_channels: int = 3, out_channels: int = 3, latent_channels: int = 4,
                 block_out_channels: Sequence[int] = (128, 256, 512, 512), layers_per_block: int = 2,
                 norm_num_groups: int = 32, scaling_factor: float = 0.18215, with_encoder: bool = False, **_ignored):
        super().__init__()
        if norm_num_groups != 32:
            raise NotImplementedError("the GroupNorm kernels are built for 32 groups (every SD VAE uses 32)")
        if any(c % 64 for c in block_out_channels):
            raise NotImplementedError("block_out_channels must be multiples of 64 (the GEMM streams 64-channel chunks)")
        self.config = SimpleNamespace(in_channels=in_channels, out_channels=out_channels, latent_channels=latent_channels,
                                      block_out_channels=tuple(block_out_channels), layers_per_block=layers_per_block,
                                      norm_num_groups=norm_num_groups, scaling_factor=scaling_factor)
        self.decoder = _Decoder(latent_channels, out_channels, tuple(block_out_channels), layers_per_block, norm_num_groups)
        self.post_quant_conv = nn.Conv2d(latent_channels, latent_channels, 1)
        self.with_encoder = bool(with_encoder)
        if self.with_encoder:
            if not 1 <= latent_channels <= N.VAE_MAX_LATENT:
                raise NotImplementedError(f"wd_vae_posterior is built for 1..{N.VAE_MAX_LATENT} latent channels")
            self.encoder = _Encoder(in_channels, latent_channels, tuple(block_out_channels), layers_per_block, norm_num_groups)
            self.quant_conv = nn.Conv2d(2 * latent_channels, 2 * latent_channels, 1)
        self.encode_chunk = self.ENCODE_CHUNK
        self._engine: Optional[VAEDecoderEngine] = None
        self._enc_engine: Optional[VAEEncoderEngine] = None

    # ---- weights -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _remap(sd: Dict[str, torch.Tensor], with_encoder: bool = False) -> Dict[str, torch.Tensor]:
        """Decoder entries (and, ``with_encoder``, the encoder ones) of a ``diffusers`` AutoencoderKL state dict; the pre-0.14
        attention names (query / key / value / proj_attn) are mapped to to_q / to_k / to_v / to_out.0, 1x1-conv shaped projections
        are flattened."""
        ren = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}
        keep = ("decoder.", "post_quant_conv.") + (("encoder.", "quant_conv.") if with_encoder else ())
        out = {}
        for k, v in sd.items():
            if not k.startswith(keep):
                continue
            parts = k.split(".")
            if "attentions" in parts and parts[-2] in ren:
                k = ".".join(parts[:-2] + [ren[parts[-2]], parts[-1]])
            if "attentions" in k and v.dim() == 4 and ("to_" in k):
                v = v.reshape(v.shape[0], v.shape[1])
            out[k] = v
        return out

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        return super().load_state_dict(self._remap(dict(state_dict), self.with_encoder), strict=strict, **kw)

    @classmethod
    def from_pretrained(cls, path: str, subfolder: Optional[str] = None, **kw) -> "AutoencoderKL":
        """LOCAL directory in ``diffusers`` layout (``config.json`` + ``diffusion_pytorch_model.safetensors`` or ``.bin``);
        nothing is ever downloaded.  The ``.bin`` is read with ``weights_only=True``.  The encoder is built when the checkpoint holds
        ``encoder.*`` entries (every full SD checkpoint does), or when ``with_encoder`` is passed."""
        root = os.path.join(path, subfolder) if subfolder else path
        cfg = dict(SD15_VAE_CONFIG)
        cfg_file = os.path.join(root, "config.json")
        if os.path.isfile(cfg_file):
            with open(cfg_file) as f:
                raw = json.load(f)
            cfg.update({k: raw[k] for k in cfg if k in raw})
        st = os.path.join(root, "diffusion_pytorch_model.safetensors")
        if os.path.isfile(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        else:
            sd = torch.load(os.path.join(root, "diffusion_pytorch_model.bin"), map_location="cpu", weights_only=True)
        with_encoder = kw.get("with_encoder")
        if with_encoder is None:
            with_encoder = any(k.startswith("encoder.") for k in sd)
        model = cls(**cfg, with_encoder=bool(with_encoder))
        model.load_state_dict(sd)
        return model.eval().requires_grad_(False)

    # ---- the one operation the samplers use -------------------------------------------------------------------------------
    @property
    def engine(self) -> "VAEDecoderEngine":
        if self._engine is None:
            self._engine = VAEDecoderEngine(self)
        return self._engine

    def _require_encoder(self):
        if not self.with_encoder:
            raise N.NativeError("this AutoencoderKL was built without its encoder: construct it with with_encoder=True, or load a "
                                "checkpoint that holds encoder.* entries through from_pretrained")

    @property
    def encoder_engine(self) -> "VAEEncoderEngine":
        self._require_encoder()
        if self._enc_engine is None:
            self._enc_engine = VAEEncoderEngine(self)
        return self._enc_engine

    def set_precision(self, mode: str):
        self.engine.set_precision(mode)
        if self.with_encoder:
            self.encoder_engine.set_precision(mode)

    @torch.no_grad()
    def decode(self, z: torch.Tensor, return_dict: bool = True, generator=None):
        if z.dim() != 4 or z.shape[1] != self.config.latent_channels:
            raise ValueError(f"latents must be [B, {self.config.latent_channels}, h, w], got {tuple(z.shape)}")
        if not z.is_cuda:
            raise N.NativeError("worddiffusion_amd runs on an MI355X only: move the latents and the VAE to cuda "
                                "(there is no CPU / eager fallback)")
        sample = self.engine.decode(z.float().contiguous())
        return DecoderOutput(sample) if return_dict else (sample,)

    def forward(self, z):
        return self.decode(z).sample

    # ---- the operation the training loops use -------------------------------------------------------------------------
    def _encode(self, x: torch.Tensor, want_sample: bool, scale: float, seed, sample_offset: int, noise=None):
        self._require_encoder()
        if x.dim() != 4 or x.shape[1] != self.config.in_channels:
            raise ValueError(f"images must be [B, {self.config.in_channels}, H, W], got {tuple(x.shape)}")
        f = 1 << (len(self.config.block_out_channels) - 1)
        if x.shape[2] % f or x.shape[3] % f or x.shape[0] == 0:
            raise ValueError(f"image height and width must be multiples of {f}, got {tuple(x.shape)}")
        if not x.is_cuda:
            raise N.NativeError("worddiffusion_amd runs on an MI355X only: move the images and the VAE to cuda "
                                "(there is no CPU / eager fallback)")
        return self.encoder_engine.encode(x.float().contiguous(), want_sample, scale, seed, sample_offset, noise, max(1, int(self.encode_chunk)))

    @torch.no_grad()
    def encode(self, x: torch.Tensor, return_dict: bool = True):
        """``diffusers``' ``vae.encode(x)``: ``.latent_dist`` with ``mean`` / ``logvar`` [B, L, H / f, W / f]."""
        mean, logvar, _ = self._encode(x, False, 1.0, 0, 0)
        out = AutoencoderKLOutput(DiagonalGaussianDistribution(mean, logvar))
        return out if return_dict else (out.latent_dist,)

    @torch.no_grad()
    def encode_latents(self, x: torch.Tensor, *, seed: Optional[int] = None, sample_offset: int = 0, mode: bool = False,
                       noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``vae.encode(x).latent_dist.sample() * scaling_factor`` (``train.py:277-278``) with the draw and the scale inside the
        encoder's last launch; ``mode=True``: ``scaling_factor * mean``.  Sample ``i``'s noise depends on
        ``(seed, sample_offset + i)`` only."""
        sf = float(self.config.scaling_factor)
        if mode:
            mean, _, _ = self._encode(x, False, 1.0, 0, 0)
            return mean.mul_(sf)
        return self._encode(x, True, sf, _draw_seed(seed) if noise is None else 0, int(sample_offset), noise)[2]


class VAEDecoderEngine(UNetEngine):
    """Launch plan of the decoder out of the UNet engine's building blocks: im2col + GEMM for the two 4-channel
    convolutions, tap-gather GEMMs with fused GroupNorm statistics for every 3x3, nearest-x2 folded into the gather table of
    the upsampler's convolution, the shortcut 1x1 as a second K segment of a block's last 3x3, one attention launch."""

    TILE = 128128  # channel counts are multiples of 128, not of 160

    def __init__(self, model: AutoencoderKL):
        super().__init__(model, "vae")

    # ---- operands -----------------------------------------------------------------------------------------------------
    def _resnets(self):
        d = self.model.decoder
        yield "mid.r0", d.mid_block.resnets[0]
        yield "mid.r1", d.mid_block.resnets[1]
        for i, ub in enumerate(d.up_blocks):
            for j, r in enumerate(ub.resnets):
                yield f"up{i}.r{j}", r

    def _resnet_recipes(self, R: RecipeBook):
        for name, r in self._resnets():
            R.vector(name + ".gn1.g", r.norm1.weight)
            R.vector(name + ".gn1.b", r.norm1.bias)
            R.matrix(name + ".c1.w", r.cout, 9 * r.cin).fwd(r.conv1.weight)
            R.vector(name + ".c1.b", r.conv1.bias)
            R.vector(name + ".gn2.g", r.norm2.weight)
            R.vector(name + ".gn2.b", r.norm2.bias)
            if r.cin != r.cout:
                R.matrix(name + ".c2.w", r.cout, 9 * r.cout + r.cin).fwd(r.conv2.weight) \
                    .fwd(r.conv_shortcut.weight, col_off=9 * r.cout)
                R.vector(name + ".c2.b", r.conv2.bias, r.conv_shortcut.bias)
            else:
                R.matrix(name + ".c2.w", r.cout, 9 * r.cout).fwd(r.conv2.weight)
                R.vector(name + ".c2.b", r.conv2.bias)

    @staticmethod
    def _attention_recipes(R: RecipeBook, at: _Attention):
        ch = at.ch
        R.vector("mid.at.gn.g", at.group_norm.weight)
        R.vector("mid.at.gn.b", at.group_norm.bias)
        R.matrix("mid.at.qkv.w", 3 * ch, ch)
        for i, l in enumerate((at.to_q, at.to_k, at.to_v)):
            R["mid.at.qkv.w"].fwd(l.weight, row_off=i * ch)
        R.vector_cat("mid.at.qkv.b", [at.to_q.bias, at.to_k.bias, at.to_v.bias])
        R.linear("mid.at.o", at.to_out[0])

    def _recipes(self) -> RecipeBook:
        m = self.model
        d = m.decoder
        R = RecipeBook()
        lat = m.config.latent_channels
        self.kpad_in = ((9 * lat + 31) // 32) * 32
        # post_quant_conv (1x1) rides the same im2col operand as a 3x3 whose only non-zero tap is the centre one
        R.matrix("pq.w", lat, self.kpad_in).fwd(m.post_quant_conv.weight, col_off=4 * lat)
        R.vector("pq.b", m.post_quant_conv.bias)
        R.matrix("in.w", d.conv_in.out_channels, self.kpad_in).fwd(d.conv_in.weight)
        R.vector("in.b", d.conv_in.bias)
        self._resnet_recipes(R)
        self._attention_recipes(R, d.mid_block.attentions[0])
        for i, ub in enumerate(d.up_blocks):
            if hasattr(ub, "upsamplers"):
                up = ub.upsamplers[0]
                R.matrix(f"up{i}.us.w", up.cout, 9 * up.cin).fwd(up.conv.weight)
                R.vector(f"up{i}.us.b", up.conv.bias)
        R.vector("out.gn.g", d.conv_norm_out.weight)
        R.vector("out.gn.b", d.conv_norm_out.bias)
        R.matrix("out.w", d.conv_out.out_channels, 9 * d.conv_out.in_channels).fwd(d.conv_out.weight)
        R.vector("out.b", d.conv_out.bias)
        return R

    # ---- plan ---------------------------------------------------------------------------------------------------------
    def _vae_resnet(self, P: Plan, name: str, r: _Resnet, x: Act) -> Act:
        ops = P.step
        B, h, w = self._B, x.h, x.w
        hw, M = h * w, B * h * w
        tab = self._table(h, w, "same")
        need_raw = r.cin != r.cout
        a1, raw = self._gn(P, ops, name + ".gn1", [x], name + ".gn1", 1e-6, True, want_raw=need_raw)
        h1 = self._f32(P, M, r.cout)
        g1 = self._gemm(ops, name + ".conv1", [self._src(a1, r.cin, 9, tab, hw)], name + ".c1.w", M, hw,
                        bias=self._w[name + ".c1.b"], out_f32=h1, out_ld=r.cout, want_stats=True, tile=self.TILE)
        a2, _ = self._gn(P, ops, name + ".gn2", [Act(h1, r.cout, h, w, g1.stats)], name + ".gn2", 1e-6, True)
        out = self._f32(P, M, r.cout)
        if need_raw:
            g2 = self._gemm(ops, name + ".conv2+shortcut", [self._src(a2, r.cout, 9, tab, hw), self._src(raw, r.cin)],
                            name + ".c2.w", M, hw, bias=self._w[name + ".c2.b"], out_f32=out, out_ld=r.cout,
                            want_stats=True, tile=self.TILE)
        else:
            g2 = self._gemm(ops, name + ".conv2", [self._src(a2, r.cout, 9, tab, hw)], name + ".c2.w", M, hw,
                            bias=self._w[name + ".c2.b"], resid=x.t.data_ptr(), resid_ld=r.cout, out_f32=out,
                            out_ld=r.cout, want_stats=True, tile=self.TILE)
        return Act(out, r.cout, h, w, g2.stats)

    def _vae_attention(self, P: Plan, x: Act) -> Act:
        ops = P.step
        B, h, w, c = self._B, x.h, x.w, x.c
        hw, M = h * w, B * h * w
        g, _ = self._gn(P, ops, "mid.at.gn", [x], "mid.at.gn", 1e-6, False)
        qkv = self._f32(P, M, 3 * c)
        self._gemm(ops, "mid.attn.qkv", [self._src(g, c)], "mid.at.qkv.w", M, hw, bias=self._w["mid.at.qkv.b"], out_f32=qkv,
                   out_ld=3 * c, tile=self.TILE)
        o = self._planes(P, M, c)
        self._attention(ops, "mid.attn", qkv.data_ptr(), 3 * c, qkv.data_ptr() + 4 * c, 3 * c, qkv.data_ptr() + 8 * c, 3 * c,
                        1, hw, hw, c, float(c) ** -0.5, o)
        out = self._f32(P, M, c)
        gg = self._gemm(ops, "mid.attn.to_out+residual", [self._src(o, c)], "mid.at.o.w", M, hw, bias=self._w["mid.at.o.b"],
                        resid=x.t.data_ptr(), resid_ld=c, out_f32=out, out_ld=c, want_stats=True, tile=self.TILE)
        return Act(out, c, h, w, gg.stats)

    def plan_decode(self, B: int, H: int, W: int) -> Plan:
        key = ("vae", B, H, W, self.npass)
        P = self._cached_plan(self._plans, key)
        if P is not None:
            return P
        m, lib, dev = self.model, self.lib, self.device
        d = m.decoder
        lat = m.config.latent_channels
        P = self._begin_plan(Plan(), B)
        step = P.step
        P.z_in = torch.zeros((B, lat, H, W), dtype=torch.float32, device=dev)
        zq_tok = self._head_gemm(P, step, "post_quant_conv", P.z_in, "pq", label="im2col(z)", want_stats=False)[0].t
        zq = self._f32(P, B, lat, H, W)
        step.append((lib.wd_tokens_to_nchw, (zq_tok.data_ptr(), lat, B, lat, H * W, zq.data_ptr()), "tokens_to_nchw(z)"))
        cur, _ = self._head_gemm(P, step, "decoder.conv_in", zq, "in", label="im2col(post_quant z)", tile=self.TILE)
        cur = self._vae_resnet(P, "mid.r0", d.mid_block.resnets[0], cur)
        cur = self._vae_attention(P, cur)
        cur = self._vae_resnet(P, "mid.r1", d.mid_block.resnets[1], cur)
        for i, ub in enumerate(d.up_blocks):
            for j, r in enumerate(ub.resnets):
                cur = self._vae_resnet(P, f"up{i}.r{j}", r, cur)
            if hasattr(ub, "upsamplers"):
                cur = self._resample(P, f"up{i}.us", ub.upsamplers[0], cur, "up", tile=self.TILE)
        P.out = torch.empty((B, d.conv_out.out_channels, cur.h, cur.w), dtype=torch.float32, device=dev)
        self._tail_gemm(P, step, "decoder.conv_out", cur, 1e-6, nchw=P.out)
        self._plans[key] = P
        return P

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        self.refresh_weights()
        B, _, H, W = z.shape
        P = self.plan_decode(B, H, W)
        P.z_in.copy_(z, non_blocking=True)
        P.run_step(torch.cuda.current_stream(self.device).cuda_stream)
        return P.out.clone()


class VAEEncoderEngine(VAEDecoderEngine):
    """Launch plan of the encoder out of the same building blocks: im2col + GEMM for the 3-channel ``conv_in``, tap-gather GEMMs
    with fused GroupNorm statistics for every 3x3, ``Downsample2D`` (zero padding right and bottom, stride 2) as the ``down_rb``
    gather table of its convolution, the shortcut 1x1 as a second K segment, one attention launch; the tail (``quant_conv``, chunk,
    clamp, posterior draw, scale, NCHW) is one ``wd_vae_posterior`` launch outside the plan, because its seed changes per call.

    A plan keeps every buffer of its batch, so ``encode`` runs a batch as replays of a plan of at most ``chunk`` images (plus one
    smaller plan for a remainder).  The noise of sample ``i`` is keyed by ``sample_offset + i``: it does not see the chunking."""

    def _resnets(self):
        e = self.model.encoder
        for i, db in enumerate(e.down_blocks):
            for j, r in enumerate(db.resnets):
                yield f"down{i}.r{j}", r
        yield "mid.r0", e.mid_block.resnets[0]
        yield "mid.r1", e.mid_block.resnets[1]

    def _signature(self):
        # (the encoder's own parameters only: a decoder update does not re-pack the encoder's operands)
        if self._ps is None or self._ps_gen != _PARAM_GEN[0]:
            self._ps = list(self.model.encoder.parameters()) + list(self.model.quant_conv.parameters())
            self._ps_gen = _PARAM_GEN[0]
        ps = self._ps
        return (sum(p._version for p in ps) + (_NATIVE_WRITES[0] << 32), hash(tuple(p.data_ptr() for p in ps)), str(ps[0].device))

    def _recipes(self) -> RecipeBook:
        m = self.model
        e = m.encoder
        R = RecipeBook()
        self.kpad_in = ((9 * m.config.in_channels + 31) // 32) * 32
        R.matrix("in.w", e.conv_in.out_channels, self.kpad_in).fwd(e.conv_in.weight)
        R.vector("in.b", e.conv_in.bias)
        self._resnet_recipes(R)
        self._attention_recipes(R, e.mid_block.attentions[0])
        for i, db in enumerate(e.down_blocks):
            if hasattr(db, "downsamplers"):
                ds = db.downsamplers[0]
                R.matrix(f"down{i}.ds.w", ds.cout, 9 * ds.cin).fwd(ds.conv.weight)
                R.vector(f"down{i}.ds.b", ds.conv.bias)
        R.vector("out.gn.g", e.conv_norm_out.weight)
        R.vector("out.gn.b", e.conv_norm_out.bias)
        R.matrix("out.w", e.conv_out.out_channels, 9 * e.conv_out.in_channels).fwd(e.conv_out.weight)
        R.vector("out.b", e.conv_out.bias)
        # quant_conv stays fp32 in the parameter layout: wd_vae_posterior applies it itself (include/wdiff_hip.h)
        R.vector("qc.w", m.quant_conv.weight)
        R.vector("qc.b", m.quant_conv.bias)
        return R

    def plan_encode(self, B: int, H: int, W: int) -> Plan:
        key = ("vae.enc", B, H, W, self.npass)
        P = self._cached_plan(self._plans, key)
        if P is not None:
            return P
        e = self.model.encoder
        P = self._begin_plan(Plan(), B)
        step = P.step
        P.x_in = torch.zeros((B, self.model.config.in_channels, H, W), dtype=torch.float32, device=self.device)
        cur, _ = self._head_gemm(P, step, "encoder.conv_in", P.x_in, "in", label="im2col(x)", tile=self.TILE)
        for i, db in enumerate(e.down_blocks):
            for j, r in enumerate(db.resnets):
                cur = self._vae_resnet(P, f"down{i}.r{j}", r, cur)
            if hasattr(db, "downsamplers"):
                cur = self._resample(P, f"down{i}.ds", db.downsamplers[0], cur, "down_rb", tile=self.TILE)
        cur = self._vae_resnet(P, "mid.r0", e.mid_block.resnets[0], cur)
        cur = self._vae_attention(P, cur)
        cur = self._vae_resnet(P, "mid.r1", e.mid_block.resnets[1], cur)
        _, P.moments = self._tail_gemm(P, step, "encoder.conv_out", cur, 1e-6)  # (token rows: wd_vae_posterior reads them)
        P.lat_hw = (cur.h, cur.w)
        self._plans[key] = P
        return P

    @staticmethod
    def plan_bytes(P: Plan) -> int:
        """Device bytes a plan holds on to (its activations, operand planes and statistics; not the packed weights)."""
        return sum(t.numel() * t.element_size() for t in P.keep + [P.x_in] if isinstance(t, torch.Tensor))

    def encode(self, x: torch.Tensor, want_sample: bool, scale: float, seed: int, sample_offset: int,
               noise: Optional[torch.Tensor], chunk: int):
        """-> (mean, logvar, sample or None), NCHW fp32 [B, L, h, w]."""
        self.refresh_weights()
        m, lib = self.model, self.lib
        B, _, H, W = x.shape
        L = m.config.latent_channels
        f = len(m.config.block_out_channels) - 1
        h, w = H >> f, W >> f
        if (L * h * w) % 4:
            raise ValueError(f"latent_channels * h * w = {L * h * w} must be a multiple of 4 (the Philox stream draws four at a time)")
        dev = self.device
        mean = torch.empty((B, L, h, w), dtype=torch.float32, device=dev)
        logvar = torch.empty_like(mean)
        sample = torch.empty_like(mean) if want_sample else None
        if noise is not None:
            noise = noise.to(dev, torch.float32).contiguous()
            if noise.shape != mean.shape:
                raise ValueError(f"noise must be {tuple(mean.shape)}, got {tuple(noise.shape)}")
        st = torch.cuda.current_stream(dev).cuda_stream
        per = 4 * L * h * w  # bytes of one sample of an output map
        for b0 in range(0, B, chunk):
            nb = min(chunk, B - b0)
            P = self.plan_encode(nb, H, W)
            assert P.lat_hw == (h, w)
            P.x_in.copy_(x[b0:b0 + nb], non_blocking=True)
            P.run_step(st)
            N.check(lib.wd_vae_posterior(P.moments.data_ptr(), 2 * L, self._w["qc.w"].data_ptr(), self._w["qc.b"].data_ptr(), nb, L,
                                         h * w, mean.data_ptr() + b0 * per, logvar.data_ptr() + b0 * per,
                                         sample.data_ptr() + b0 * per if want_sample else None, float(scale),
                                         noise.data_ptr() + b0 * per if noise is not None else None, int(seed),
                                         int(sample_offset) + b0, st), "wd_vae_posterior")
        return mean, logvar, sample
