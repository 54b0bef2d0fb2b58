"""Common body of ``UNetModel`` / ``UNetModelPhosc``: the reference constructor surface and parameter tree,
with the forward handed to the HIP engine.

Constructor kwargs: reference ``unet.py:1126-1156`` / ``unetPhosc.py:781-811`` (identical lists).
Block construction order: ``unet.py:1248-1458``.
"""
from __future__ import annotations

import copy
import os
from typing import Optional

import torch
import torch.nn as nn

from .layers import (CharacterEncoderParams, DownsampleParams, ResBlockParams, SpatialTransformerParams,
                     UpsampleParams, _zero)


def _arg(args, name, default=0):
    return getattr(args, name, default) if args is not None else default


class UNetBase(nn.Module):
    variant = "base"

    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks,
                 attention_resolutions, dropout=0, channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2,
                 num_classes=None, use_checkpoint=False, use_fp16=False, num_heads=-1, num_head_channels=-1,
                 num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False,
                 use_new_attention_order=False, use_spatial_transformer=True, transformer_depth=1,
                 context_dim=768, vocab_size=256, n_embed=None, legacy=False, args=None, max_seq_len=20):
        super().__init__()
        # ---- combinations the reference itself cannot run, or that lie outside the hot path
        if not use_spatial_transformer:
            raise NotImplementedError("use_spatial_transformer=False (AttentionBlock) is never used by the reference")
        if context_dim is None:
            raise AssertionError("context_dim is required with the spatial transformer (unet.py:1163-1164)")
        if dims != 2:
            raise NotImplementedError("dims != 2")
        if resblock_updown:
            raise NotImplementedError("resblock_updown=True raises TypeError in the reference (unet.py:547)")
        if not conv_resample:
            raise NotImplementedError("conv_resample=False builds nn.AvgPool2d(dims, ...) which the reference cannot run")
        if use_scale_shift_norm:
            raise NotImplementedError("use_scale_shift_norm=True is not on the accelerated path")
        if n_embed is not None:
            raise NotImplementedError("n_embed (codebook id prediction) is not on the accelerated path")
        if isinstance(context_dim, (list, tuple)):
            context_dim = list(context_dim)[0]
        if _arg(args, "attentionMaps", 0):
            # (with the flag the reference also registers the middle block under other names, unet.py:1336-1364)
            raise NotImplementedError("args.attentionMaps=1: build the model with attentionMaps=0 and ask a forward for the maps "
                                      "with return_attention= (samplers: attention=); a checkpoint saved by an attentionMaps=1 run "
                                      "loads after remap_attention_maps_state_dict(state_dict)")
        for flag in ("charImages", "ocrTraining", "wrdChrWrStyl"):
            if _arg(args, flag, 0):
                raise NotImplementedError(f"args.{flag}=1 selects an auxiliary head / debugging output that is "
                                          "outside the accelerated denoising path (SURVEY.md 8b)")
        # args.charLevelEmb=1 (the default of unet.py:1871; checkpoints ``ckpt_ema_charLevelEmb.pt``, config.py:61): the base
        # CharacterEncoder flattens the ids, embeds them and views the result back as (B, 10, 320) (unet.py:855-864) - the same
        # tensor as without the flag (tests/golden/fwd_base_full_charlevel.npz: bit-identical output).  The view hard-codes
        # 10 tokens x 320 channels, so the reference itself fails for any other context width.  unetPhosc.py never reads it.
        self.char_level_emb = bool(_arg(args, "charLevelEmb", 0)) and self.variant == "base"
        if self.char_level_emb and context_dim != 320:
            raise NotImplementedError("args.charLevelEmb=1 needs context_dim=320: unet.py:864 views the embedding as "
                                      "(B, 10, 320) and raises for any other width")
        if num_heads == -1 and num_head_channels == -1:
            raise AssertionError("Either num_heads or num_head_channels has to be set")
        if num_heads_upsample == -1:
            num_heads_upsample = num_heads

        self.args = args
        self.image_size = image_size
        self.in_channels = in_channels
        self.model_channels = model_channels
        self.out_channels = out_channels
        self.num_res_blocks = num_res_blocks
        self.attention_resolutions = attention_resolutions
        self.dropout = dropout
        self.channel_mult = channel_mult
        self.conv_resample = conv_resample
        self.num_classes = num_classes
        self.use_checkpoint = use_checkpoint
        self.dtype = torch.float32  # use_fp16 only retypes the input in the reference (convert_* are no-ops)
        self.num_heads = num_heads
        self.num_head_channels = num_head_channels
        self.num_heads_upsample = num_heads_upsample
        self.predict_codebook_ids = False
        self.context_dim = context_dim
        self.max_seq_len = max_seq_len
        self.transformer_depth = transformer_depth
        self.interpolation = bool(_arg(args, "interpolation", False))

        ted = model_channels * 4
        self.time_embed = nn.Sequential(nn.Linear(model_channels, ted), nn.SiLU(), nn.Linear(ted, ted))
        self.word_emb = CharacterEncoderParams(vocab_size, context_dim, max_seq_len)
        self._extra_heads_before_label()
        if num_classes is not None:
            self.label_emb = nn.Embedding(num_classes, ted)

        def heads_for(ch):
            if num_head_channels == -1:
                return num_heads, ch // num_heads
            return ch // num_head_channels, num_head_channels

        def st(ch):
            h, d = heads_for(ch)
            return SpatialTransformerParams(ch, h, d, transformer_depth, context_dim)

        self.input_blocks = nn.ModuleList([nn.Sequential(nn.Conv2d(in_channels, model_channels, 3, padding=1))])
        chans = [model_channels]
        ch, ds = model_channels, 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [ResBlockParams(ch, ted, mult * model_channels, dropout)]
                ch = mult * model_channels
                if ds in attention_resolutions:
                    layers.append(st(ch))
                self.input_blocks.append(nn.Sequential(*layers))
                chans.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(nn.Sequential(DownsampleParams(ch, ch)))
                chans.append(ch)
                ds *= 2
        self.middle_block = nn.Sequential(ResBlockParams(ch, ted, ch, dropout), st(ch),
                                          ResBlockParams(ch, ted, ch, dropout))
        self.output_blocks = nn.ModuleList([])
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                ich = chans.pop()
                layers = [ResBlockParams(ch + ich, ted, model_channels * mult, dropout)]
                ch = model_channels * mult
                if ds in attention_resolutions:
                    layers.append(st(ch))
                if level and i == num_res_blocks:
                    layers.append(UpsampleParams(ch, ch))
                    ds //= 2
                self.output_blocks.append(nn.Sequential(*layers))
        self.out = nn.Sequential(nn.GroupNorm(32, ch), nn.SiLU(),
                                 _zero(nn.Conv2d(model_channels, out_channels, 3, padding=1)))
        self._extra_heads_after_out()
        self._engine = None
        self._train_engine = None
        dev = _arg(args, "device", None)
        if dev is not None and str(dev) != "cpu":
            # the reference moves word_emb to args.device in the constructor (unet.py:1210-1213); callers then
            # .to(device) the whole model, which we leave to them.
            pass

    # hooks for the two variants --------------------------------------------------------------------------
    def _extra_heads_before_label(self):
        pass

    def _extra_heads_after_out(self):
        pass

    # ---------------------------------------------------------------------------------------------------------
    @property
    def engine(self):
        if self._engine is None:
            from .engine import UNetEngine
            self._engine = UNetEngine(self, self.variant)
            mode = os.environ.get("WDIFF_PRECISION")
            if mode:
                self._engine.set_precision(mode)
        return self._engine

    def __deepcopy__(self, memo):
        # ``copy.deepcopy(model)`` is how the reference makes its EMA model (train.py:409); the engine (ctypes
        # handles, device plans) is per-instance and rebuilt lazily by the copy.
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = None if k in ("_engine", "_train_engine", "_anchor") else copy.deepcopy(v, memo)
        return new

    def set_precision(self, mode: str):
        """'bf16x3' (default; split-bf16 MFMA, fp32-class results) or 'bf16' (single pass)."""
        self.__dict__["_precision"] = mode
        self.engine.set_precision(mode)
        if self._train_engine is not None:
            self._train_engine.set_precision(mode)
        return self

    def convert_to_fp16(self):  # no-ops in the reference as well (unet.py:415-419)
        pass

    def convert_to_fp32(self):
        pass

    def _check_common(self, x, timesteps, mix_rate):
        if timesteps is None:
            raise ValueError("timesteps is required")
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"x must be [B,{self.in_channels},H,W], got {tuple(x.shape)}")

    def _check_context(self, context):
        if self.char_level_emb and context is not None and context.shape[1] != 10:
            raise ValueError("args.charLevelEmb=1: context must be [B, 10] (unet.py:864 views the embedding as (B, 10, 320))")

    @property
    def train_engine(self):
        """Forward-with-saved-intermediates + backward launch lists (``train_engine.py``); base variant only."""
        if self._train_engine is None:
            from .train_engine import TrainEngine
            self._train_engine = TrainEngine(self, self.variant)
            mode = self.__dict__.get("_precision") or os.environ.get("WDIFF_PRECISION")
            if mode:
                self._train_engine.set_precision(mode)
        return self._train_engine

    def add_writers(self, k: int, init="mean"):
        """Grows the writer table by ``k`` rows (DESIGN.md "Fitting new writers") and returns the new ids,
        ``list(range(old, old + k))``.  ``label_emb`` becomes an ``nn.Embedding(num_classes + k, ted)`` whose first rows are the old
        ones bit for bit, so ``state_dict()`` keeps the reference's key layout and loads ``strict=True`` into a model built with
        ``num_classes + k``.  ``init``: "mean" (the fp32 mean over the old rows), an int id or a list of ``k`` ids (copies of those
        rows), or a float tensor [k, ted].  The engines are dropped - plans, packed tables and the gradient arena are sized for
        the old table - and rebuilt lazily; an EMA copy is grown by the caller with the same call."""
        if self.num_classes is None:
            raise ValueError("add_writers needs a class-conditional model (num_classes)")
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"k must be an integer >= 1, got {k!r}")
        old_w = self.label_emb.weight.detach()
        old, ted = old_w.shape
        if isinstance(init, str):
            if init != "mean":
                raise ValueError(f"init must be 'mean', a writer id, a list of {k} ids or a float tensor [{k}, {ted}], not {init!r}")
            rows = old_w.float().mean(0, keepdim=True).expand(k, ted)
        elif torch.is_tensor(init) and init.is_floating_point():
            if tuple(init.shape) != (k, ted):
                raise ValueError(f"an init tensor must be [{k}, {ted}], got {tuple(init.shape)}")
            rows = init.detach().to(device=old_w.device, dtype=old_w.dtype)
        else:
            ids = [init] * k if isinstance(init, int) and not isinstance(init, bool) else \
                (init.tolist() if torch.is_tensor(init) else list(init) if isinstance(init, (list, tuple)) else None)
            if ids is None or len(ids) != k or any(isinstance(i, bool) or not isinstance(i, int) for i in ids):
                raise ValueError(f"init must be 'mean', a writer id, a list of {k} ids or a float tensor [{k}, {ted}]")
            if any(i < 0 or i >= old for i in ids):
                raise ValueError(f"every init id must lie in [0, {old})")
            rows = old_w[torch.tensor(ids, dtype=torch.long, device=old_w.device)]
        emb = nn.Embedding(old + k, ted, device=old_w.device, dtype=old_w.dtype)
        with torch.no_grad():
            emb.weight[:old].copy_(old_w)
            emb.weight[old:].copy_(rows)
        emb.weight.requires_grad_(self.label_emb.weight.requires_grad)
        self.label_emb = emb
        self.num_classes = old + k
        self._engine = self._train_engine = None
        return list(range(old, old + k))

    def set_dropout_state(self, seed: int, row_base: int = 0):
        """Keys the training dropout of ``model(...)`` under autograd (``dropout.py``): the Philox seed, and the global row the
        next training forward gives its sample 0 - every forward then advances it by its batch."""
        eng = self.train_engine
        eng.dropout_seed, eng.dropout_row_base = int(seed), int(row_base)
        return self

    def _run(self, x, timesteps, context, y, phosc=None, mix_rate=None, return_attention=False, writer_keep=None):
        """writer_keep: None, a bool / uint8 tensor [B] (nonzero: the sample keeps its writer term) or False (no sample does: the
        reference's ``args.imgConditioned == 1`` forward, unet.py:1578-1579)."""
        autograd = torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters())
        if writer_keep is not None:
            if self.num_classes is None:
                raise ValueError("writer_keep needs a class-conditional model (num_classes)")
            if return_attention is not False:
                raise NotImplementedError("writer_keep together with return_attention")
            if self.interpolation and mix_rate is not None:
                raise NotImplementedError("writer_keep together with mix_rate in interpolation mode")
        if return_attention is not False:
            return self._run_attention(x, timesteps, context, y, phosc, mix_rate, return_attention, autograd)
        if self.training and not autograd and float(self.dropout) > 0:
            # the inference engine has no dropout: running it here would silently skip the layer train mode asks for
            raise NotImplementedError(f"train mode with dropout={self.dropout} outside autograd: the HIP inference path applies "
                                      "no dropout - call model.eval() first (or run under autograd to train)")
        if self.interpolation and mix_rate is not None:
            # unet.py:1558-1573 / unetPhosc.py:1093-1108: one pair of writers per call from Python's global ``random``, the same
            # blended row for every sample; ``y`` is unused.  (Without args.interpolation the reference ignores mix_rate.)
            if autograd:
                raise NotImplementedError("mix_rate under autograd: the reference's training loop never passes it "
                                          "(train.py:287); the interpolation forward is inference-only")
            from .diffusion import draw_style_pairs
            pair = draw_style_pairs(1)[0]
            B = x.shape[0]
            pairs = torch.tensor([pair] * B, dtype=torch.int32)
            m = mix_rate.float().reshape(-1).expand(B) if torch.is_tensor(mix_rate) else torch.full((B,), float(mix_rate))
            out = self.engine.forward(x.float(), timesteps, context, y, phosc, mix=(pairs, m))
            return out.type(x.dtype)
        if autograd:
            # ``predicted_noise = model(...)`` inside the training loop (train.py:287): the result carries a grad_fn whose
            # backward runs the HIP backward list and fills ``param.grad`` (reference layouts), so ``loss.backward()``,
            # ``optimizer.step()`` and ``ema.step_ema`` of the reference loop work unchanged.
            return _HipUNetStep.apply(self, x, timesteps, context, y, phosc, self._grad_anchor(x.device),
                                      writer_keep).type(x.dtype)
        out = self.engine.forward(x.float(), timesteps, context, y, phosc, writer_keep=writer_keep)
        return out.type(x.dtype)

    def _run_attention(self, x, timesteps, context, y, phosc, mix_rate, mode, autograd):
        """``forward(..., return_attention=True | "reference")``: the predicted noise and the per-character attention maps of the
        three SpatialTransformers the reference taps with --attentionMaps 1 (unet.py:1645-1832), each the softmax of the block's
        attn2 summed over heads.  True: ``(eps, attn1, attn2, attn3)``, fp32 [B, h_i, w_i, L] at latent resolution.
        "reference": ``(eps, attn1, attn2, attn3, context)`` as the reference returns them - the maps replicated x8 / x16 / x8
        (its nearest-neighbour F.interpolate, unet.py:1761-1778) and the word encoder's output [B, L, context_dim]."""
        if mode is not True and mode != "reference":
            raise ValueError(f"return_attention must be False, True or 'reference', not {mode!r}")
        if autograd:
            raise NotImplementedError("return_attention under autograd: the attention maps are an inference-only output")
        if self.interpolation and mix_rate is not None:
            raise NotImplementedError("return_attention together with mix_rate")
        if self.training and float(self.dropout) > 0:
            raise NotImplementedError(f"train mode with dropout={self.dropout} outside autograd: call model.eval() first")
        eng = self.engine
        out, maps = eng.forward(x.float(), timesteps, context, y, phosc, attn_maps=True)
        out = out.type(x.dtype)
        if mode is True:
            return (out, *maps)
        B, L = x.shape[0], maps[0].shape[-1]
        P = eng.plan(B, x.shape[2], x.shape[3], L, 0, attn_maps=True)  # (the plan that just ran: its word-encoder planes)
        # (held as split-bf16 operand planes, hi + lo: 16 significant bits of the reference's fp32 tensor)
        ctx = (P.ctx_pl[0].float() + P.ctx_pl[1].float() if eng.npass == 3 else P.ctx_pl[0].float()).reshape(B, L, -1)
        big = [m.repeat_interleave(f, 1).repeat_interleave(f, 2) for m, f in zip(maps, (8, 16, 8))]
        return (out, *big, ctx)

    def _grad_anchor(self, device):
        a = self.__dict__.get("_anchor")
        if a is None or a.device != device:
            a = torch.zeros(1, device=device, requires_grad=True)
            self.__dict__["_anchor"] = a
        return a


_MAPS_KEYS = (("middle_block1.0.0.", "middle_block.0."), ("middle_block1.0.1.", "middle_block.1."),
              ("middle_block1.1.0.", "middle_block.2."))


def _rename_keys(sd, pairs):
    out = type(sd)()
    if hasattr(sd, "_metadata"):
        out._metadata = sd._metadata
    for k, v in sd.items():
        for old, new in pairs:
            if k.startswith(old):
                k = new + k[len(old):]
                break
        if k in out:
            raise KeyError(f"two keys map to {k!r}")
        out[k] = v
    return out


def remap_attention_maps_state_dict(sd):
    """A state dict saved by a reference model built with ``--attentionMaps 1`` -> the keys of this package's models (and of the
    reference without the flag): with the flag the reference registers the middle block as ``middle_block1`` =
    ``[[ResBlock, SpatialTransformer], [ResBlock]]`` (unet.py:1336-1364), so ``middle_block1.0.0.`` -> ``middle_block.0.``,
    ``middle_block1.0.1.`` -> ``middle_block.1.``, ``middle_block1.1.0.`` -> ``middle_block.2.``.  Every other key, and every
    tensor, is passed through; the order is kept."""
    return _rename_keys(sd, _MAPS_KEYS)


def to_attention_maps_state_dict(sd):
    """The inverse of ``remap_attention_maps_state_dict``: this package's keys -> those an ``--attentionMaps 1`` reference loads."""
    return _rename_keys(sd, tuple((new, old) for old, new in _MAPS_KEYS))


class _HipUNetStep(torch.autograd.Function):
    """Autograd node of the HIP training forward.  The parameters are not inputs of the node: their gradients are written
    by the backward kernels into persistent buffers that become ``param.grad`` (added to an existing ``.grad``, as autograd
    would).  ``anchor`` is a dummy leaf that makes autograd schedule the node; x / context get no gradient (train.py never
    asks for one)."""

    @staticmethod
    def forward(ctx, model, x, timesteps, context, y, phosc, anchor, writer_keep=None):
        eng = model.train_engine
        out = eng.forward_train(x.float(), timesteps, context, y, phosc, writer_keep=writer_keep).clone()
        # the plan keeps the intermediates of this forward only until the next one: its identity is checked in backward
        ctx.eng, ctx.fwd = eng, eng.last_forward()
        return out

    @staticmethod
    def backward(ctx, gout):
        ctx.eng.backward(gout.contiguous().float(), forward=ctx.fwd)
        return None, None, None, None, None, None, torch.zeros_like(ctx.eng.model._anchor), None
