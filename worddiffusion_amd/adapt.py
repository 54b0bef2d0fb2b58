"""Fitting new writers: embedding-only adaptation of the writer table ("textual inversion" for ``label_emb``; DESIGN.md "Fitting new
writers").  The workflow, from a handful of word images of one person to samples in their hand:

    latents = vae.encode(images)                              # pixels -> latents
    scores = score_writers(model, diffusion, latents, text, range(model.num_classes), t)
    new = model.add_writers(1, init=int(scores.mean(0).argmin()))      # start from the closest known writer
    losses = fit_writers(model, diffusion, latents, text, torch.full((len(latents),), new[0]), steps=200, batch=8)
    diffusion.sampling_ddim(model, ..., labels=torch.tensor(new))       # any sampler takes the new id

Every weight of the model but the fitted rows stays bit for bit what it was.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _native as N
from .optim import RowAdamW
from .training import TrainStep


def fit_writers(model, diffusion, latents: torch.Tensor, text_features: torch.Tensor, writer_of_sample, steps: int, batch: int,
                lr: float = 1e-3, anchor=None, weight_decay: float = 0.0, ema_model=None, loss_weights=None, loss_mask=None,
                seed: int = 0, phoscLabels: Optional[torch.Tensor] = None, use_graph: bool = True, return_step: bool = False):
    """Optimises the rows ``writer_of_sample`` names (ids of rows added with ``model.add_writers``; one per sample) against the
    noise-prediction loss of ``latents`` [S, C, h, w] / ``text_features`` [S, L], every other parameter frozen: ``steps`` calls of a
    ``TrainStep`` over a ``RowAdamW``, each on ``batch`` samples taken in cyclic order (sample ``(i * batch + j) % S`` is row j of
    call i), so the few samples repeat with fresh (t, eps) under the step's keying invariant.  The timesteps come from a host
    generator seeded with ``seed``.  Returns the per-step losses as one device tensor [steps]; nothing synchronises per step.
    ``loss_mask``: one mask per sample, [S, 1, h, w] or [S, C, h, w], or one [h, w] for all.  ``ema_model``: grown by the caller with
    the same ``add_writers`` call; its fitted rows follow the optimiser's EMA, nothing else of it changes.  ``return_step``: also
    return the ``TrainStep`` (its ``opt`` is the ``RowAdamW``), to go on fitting or to checkpoint the optimiser."""
    if not latents.is_cuda:
        raise N.NativeError("fit_writers runs on the GPU only (no CPU fallback)")
    if latents.dim() != 4:
        raise ValueError(f"latents must be [S, C, h, w], got {tuple(latents.shape)}")
    S, dev = latents.shape[0], latents.device
    if isinstance(steps, bool) or int(steps) != steps or steps < 1 or isinstance(batch, bool) or int(batch) != batch or batch < 1:
        raise ValueError(f"steps and batch must be integers >= 1, got {steps!r} and {batch!r}")
    writers = torch.as_tensor(writer_of_sample).to(torch.int64).reshape(-1).cpu()
    if S < 1 or writers.numel() != S or text_features.shape[0] != S or (phoscLabels is not None and phoscLabels.shape[0] != S):
        raise ValueError("latents, text_features, writer_of_sample (and phoscLabels) must hold one entry per sample")
    per_sample_mask = loss_mask is not None and torch.as_tensor(loss_mask).dim() == 4
    if per_sample_mask and loss_mask.shape[0] != S:
        raise ValueError(f"a per-sample loss_mask must hold {S} masks, got {tuple(loss_mask.shape)}")
    rows = sorted(set(writers.tolist()))
    opt = RowAdamW(model.label_emb.weight, rows, lr=lr, weight_decay=weight_decay, anchor=anchor, ema_model=ema_model)
    step = TrainStep(model, diffusion, opt, seed=seed, use_graph=use_graph, loss_weights=loss_weights)
    text_features, writers = text_features.to(dev), writers.to(dev)
    gen = torch.Generator().manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
    losses = torch.empty(int(steps), dtype=torch.float32, device=dev)
    for i in range(int(steps)):
        idx = (torch.arange(batch) + i * batch) % S
        t = torch.randint(low=1, high=diffusion.noise_steps, size=(batch,), generator=gen)
        idx = idx.to(dev)
        loss = step(latents[idx], text_features[idx], writers[idx], t=t, check=(i == 0),
                    phoscLabels=None if phoscLabels is None else phoscLabels.to(dev)[idx],
                    loss_mask=None if loss_mask is None else (loss_mask.to(dev)[idx] if per_sample_mask else loss_mask))
        losses[i:i + 1].copy_(loss)
    return (losses, step) if return_step else losses


def score_writers(model, diffusion, latents: torch.Tensor, text_features: torch.Tensor, candidates, t, seed: int = 0,
                  chunk: int = 64, phoscLabels: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [S, C] on the device: entry (s, c) is ``diffusion.eval_loss`` of sample s under candidate writer ``candidates[c]``.  Every
    candidate sees the SAME (t, eps) of its sample - ``t`` [S], eps the device Philox stream of ``seed``, row s -, which is what makes
    the scores of one row comparable.  Evaluated in chunks of at most ``chunk`` (sample, candidate) rows, sample-major, through
    ``eval_loss`` with explicit ``noise=``.  ``scores.mean(0).argmin()`` is the closest known writer (an ``add_writers`` init);
    ``scores.argmin(1)`` identifies the writer of every sample."""
    if not latents.is_cuda:
        raise N.NativeError("score_writers runs on the GPU only (no CPU fallback)")
    if latents.dim() != 4:
        raise ValueError(f"latents must be [S, C, h, w], got {tuple(latents.shape)}")
    if isinstance(chunk, bool) or int(chunk) != chunk or chunk < 1:
        raise ValueError(f"chunk must be an integer >= 1, got {chunk!r}")
    S, dev = latents.shape[0], latents.device
    cand = torch.as_tensor(list(candidates) if not torch.is_tensor(candidates) else candidates).to(torch.int64).reshape(-1)
    nc = getattr(model, "num_classes", None)
    if nc is None:
        raise ValueError("score_writers needs a class-conditional model (num_classes)")
    if cand.numel() < 1 or bool(((cand < 0) | (cand >= nc)).any()):
        raise ValueError(f"every candidate must be a writer id in [0, {nc})")
    t = torch.as_tensor(t).reshape(-1)
    if S < 1 or t.numel() != S or text_features.shape[0] != S or (phoscLabels is not None and phoscLabels.shape[0] != S):
        raise ValueError("latents, text_features, t (and phoscLabels) must hold one entry per sample")
    Cn = cand.numel()
    _, eps = diffusion.noise_images(latents, t, seed=int(seed))  # the eps row of every sample, drawn once
    s_idx = torch.arange(S).repeat_interleave(Cn)
    c_idx = torch.arange(Cn).repeat(S)
    out = torch.empty(S * Cn, dtype=torch.float32, device=dev)
    text_features, t_host = text_features.to(dev), t.cpu()
    for lo in range(0, S * Cn, int(chunk)):
        si, ci = s_idx[lo:lo + chunk], c_idx[lo:lo + chunk]
        sd = si.to(dev)
        out[lo:lo + si.numel()] = diffusion.eval_loss(model, latents[sd], text_features[sd], cand[ci].to(dev), t_host[si],
                                                      noise=eps[sd],
                                                      phoscLabels=None if phoscLabels is None else phoscLabels.to(dev)[sd])
    return out.view(S, Cn)
