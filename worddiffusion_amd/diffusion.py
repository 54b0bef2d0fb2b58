"""``Diffusion`` / ``EMA`` / ``label_padding`` with the reference's call surface (``train.py:42-52,140-251``).

Every sampler runs through the one reverse loop of ``Diffusion._denoise``, entirely on the device: the step-invariant
conditioning (word embedding, cross-attention K/V) is computed once, one denoising step (UNet forward(s) + the sampler's
update with on-device Philox noise + its timestep advance) is captured into a hipGraph and replayed once per visited step;
there is no per-step host->device traffic.  What a sampler is to that loop is a ``_Sampler``, fixed on the host before
anything is launched: ``_ddpm`` (``sampling``, ``train.py:221-236``: ``x <- 1/sqrt(a) (x - (1-a)/sqrt(1-ah) eps) + sqrt(b) z``
at t = T-1 .. 1; ``sampling3`` skips the model on most of those steps), ``_ddim`` (``sampling_ddim``: a subsequence) and
``_dpmpp`` (``sampling_dpmpp``: a subsequence spaced in log-SNR, second-order multistep) - it contributes its tables and its one
update launch; the rest of a step's tail is written once (``_step_tail``).  Everything else a public sampler settles before the
loop travels in one ``_Call`` record, built by ``Diffusion._sample``, the prelude and epilogue the public samplers share.
A ``windows=`` call (``line_windows``) samples whole lines through the same loop: the state the tail works on is a line latent, and a
model-calling step cuts it into overlapping windows of the model's width for the forward(s) and averages their predictions back.
A ``resample=`` call (``resample_walk``) walks a table of entries instead of the plain schedule: most are the sampler's steps, some
diffuse the state forward again (``wd_forward_jump``), and every draw is keyed by the walk entry rather than by the timestep.

Facts preserved from the reference: the method is ``sampling`` (``sample`` is provided as
an alias because ``sampling.py:119`` calls it); index 0 of the schedule is never used; with ``cfg_scale > 0``
the reference runs the UNet twice on identical inputs and ``lerp(a, a, w) == a`` bit-for-bit, so one forward per
step is executed (``forwards_per_step = 2`` re-enables the literal behaviour for timing comparisons).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import random
from typing import Callable, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _native as N

C_CLASSES = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"
LETTER2INDEX = {c: i for i, c in enumerate(C_CLASSES)}
MAX_CHARS = 10
TOKENS = {"PAD_TOKEN": 52}
NUM_TOKENS = len(TOKENS)
VOCAB_SIZE = len(C_CLASSES) + NUM_TOKENS
# the alphabet of trainModifyCondition.py:68 / trainGWModifyCondition.py:53: the 52 letters + '_' (a space is written as
# '_', :169) -> 53 classes, vocab_size 54; PAD stays 52, so '_' is id 53 and 'z' (51 + 1) still collides with PAD as in
# train.py
C_CLASSES_UNDERSCORE = C_CLASSES + "_"
LETTER2INDEX_UNDERSCORE = {c: i for i, c in enumerate(C_CLASSES_UNDERSCORE)}
VOCAB_SIZE_UNDERSCORE = len(C_CLASSES_UNDERSCORE) + NUM_TOKENS


def _pad_ids(labels: str, table, num_tokens: int, max_len: int) -> List[int]:
    try:
        ll = [table[ch] + num_tokens for ch in labels]
    except KeyError as e:  # the reference raises KeyError from ``letter2index[i]`` as well (train.py:45)
        raise KeyError(f"character {e.args[0]!r} of {labels!r} is not in the label alphabet") from None
    if len(ll) > max_len:
        raise ValueError(f"word longer than {max_len} characters: {labels!r}")
    return ll + [TOKENS["PAD_TOKEN"]] * (max_len - len(ll))


def label_padding(labels: str, num_tokens: int = NUM_TOKENS, max_len: int = MAX_CHARS) -> List[int]:
    """``train.py:42-52``: letter indices shifted by ``num_tokens`` and right-padded with PAD (52) to 10."""
    return _pad_ids(labels, LETTER2INDEX, num_tokens, max_len)


def label_padding_underscore(labels: str, num_tokens: int = NUM_TOKENS, max_len: int = MAX_CHARS) -> List[int]:
    """``trainModifyCondition.py:166-180`` (same in ``trainGWModifyCondition.py:64-78``): ``labels.replace(" ", "_")``, then
    the 53-class alphabet (``'_'`` -> 52 + num_tokens = 53); models fed with it are built with ``vocab_size = 54``."""
    return _pad_ids(labels.replace(" ", "_"), LETTER2INDEX_UNDERSCORE, num_tokens, max_len)


STYLE_ID_MAX = 338  # unet.py:1561-1564 / unetPhosc.py:1096-1099 hard-code randint(0, 338), whatever num_classes is


def draw_style_pairs(n: int, rng=random):
    """``n`` writer pairs drawn the way one reference forward draws its pair (unet.py:1561-1564): ``s1 = randint(0, 338)``, then
    ``s2`` likewise, redrawn while equal to ``s1`` - from Python's global ``random`` unless ``rng`` is given.  Drawing the pairs
    of a whole sampling call up front, in loop order, leaves the generator in the state the reference's loop leaves it in."""
    out = []
    for _ in range(n):
        s1 = rng.randint(0, STYLE_ID_MAX)
        s2 = rng.randint(0, STYLE_ID_MAX)
        while s1 == s2:
            s2 = rng.randint(0, STYLE_ID_MAX)
        out.append((s1, s2))
    return out


def _stream_ptr(device):
    return torch.cuda.current_stream(device).cuda_stream


def _dptr(t):
    return None if t is None else t.data_ptr()


class EMA:
    """``train.py:140-170``."""

    def __init__(self, beta):
        self.beta = beta
        self.step = 0

    def update_model_average(self, ma_model, current_model):
        lib = N.lib()
        for cur, ma in zip(current_model.parameters(), ma_model.parameters()):
            if not ma.is_cuda:
                raise N.NativeError("EMA.update_model_average runs on the GPU only (no CPU fallback)")
            assert ma.is_contiguous() and cur.is_contiguous() and ma.dtype == torch.float32
            N.check(lib.wd_ema_update(ma.data_ptr(), cur.data_ptr(), ma.numel(), float(self.beta),
                                      _stream_ptr(ma.device)), "wd_ema_update")
        # the kernel wrote the averaged parameters behind autograd's back: the engine of ``ma_model`` (which keys its packed
        # operands on the parameters' state, engine._signature) must repack before the next forward / sampling
        from .engine import note_native_write
        note_native_write()

    def step_ema(self, ema_model, model, step_start_ema=2000):
        if self.step < step_start_ema:
            self.reset_parameters(ema_model, model)
            self.step += 1
            return
        self.update_model_average(ema_model, model)
        self.step += 1

    def reset_parameters(self, ema_model, model):
        ema_model.load_state_dict(model.state_dict())


class _Sampler(NamedTuple):
    """What one sampler is to the reverse loop of ``Diffusion._denoise`` (built by ``Diffusion._ddpm`` / ``_ddim`` / ``_dpmpp``, no GPU)."""
    # per visited step, in loop order: (film_prepare argument = row of the pairs table, calls the model, index into ``noise`` or None)
    steps: list
    t_first: int  # the timestep of the first step
    tau: Optional[list]  # the visited timesteps when FiLM rows and pairs are indexed by the step index; None: indexed by t
    # update(lib, P, run) -> launch(stream): puts the sampler's tables (and any buffer of its own) on ``run.device`` and returns
    # its one update launch, which keeps them alive; the rest of a step's tail is ``Diffusion._step_tail``
    update: Callable
    stats: dict  # what ``last_stats`` reports of the sampler itself
    walk: Optional["_Walk"] = None  # a resampled call: ``steps`` and ``tau`` are the walk's, row = index into ``noise`` = the walk index k


WALK_MAX = 16384  # the most entries a resampled call may walk: its FiLM table has one time-MLP row per entry


class _Walk(NamedTuple):
    """The walk of a resampled call (``Diffusion.resample_walk``, no GPU): per entry k, in loop order."""
    tau: list  # tau'[k]: the level entry k starts from
    to: list  # the level it reaches: the next visited timestep (0 after the last) of a down entry, the level jumped to of an up entry
    up: list  # bool: an up entry (``wd_forward_jump``), else a step of the sampler
    g1: torch.Tensor  # fp32 [entries]: sqrt(alpha_hat[to] / alpha_hat[from]) at the up entries, 0 elsewhere
    g2: torch.Tensor  # fp32 [entries]: sqrt(1 - alpha_hat[to] / alpha_hat[from]) likewise
    resample: int
    jump: int

    @property
    def down(self):
        """The walk indices of the down entries."""
        return [k for k, u in enumerate(self.up) if not u]


class _Known(NamedTuple):
    """What a known-region / partial-noise call is to the reverse loop (built by ``Diffusion._known_setup``, no GPU)."""
    x0: torch.Tensor  # the known latents, fp32 [n, C*h*w] on the host
    mask: Optional[torch.Tensor]  # fp32 [n, C*h*w] on the host, 1 = keep; None: ``start`` alone, nothing is blended
    start: Optional[int]  # the level the loop starts from (``x0`` noised to it); None: from x_T / noise as ever
    tau: Optional[list]  # the retained visited timesteps of a DDIM / DPM++ call (None: DDPM)
    mode: str  # "fresh": the blend draws its noise per step; "fixed": one eps per sample
    eps: Optional[torch.Tensor]  # the caller's fixed eps, fp32 [n, C*h*w]; None: stream WD_STREAM_KNOWN of the call's seed


WINDOW_MAX = N.DEFINES["WD_WINDOW_MAX"]  # the most windows a line may have (``wd_window_blend``)


def window_profile(w, feather=0):
    """The weight of a window's columns, fp32 [w]: ``min(j + 1, w - j, feather + 1) / (feather + 1)`` - 1 in the middle, a linear
    ramp over ``feather`` columns at each end.  ``feather = 0`` is all ones: the plain average of MultiDiffusion as published."""
    w, feather = int(w), int(feather)
    if w < 1 or feather < 0:
        raise ValueError(f"window_profile needs w >= 1 and feather >= 0, got w = {w}, feather = {feather}")
    j = torch.arange(w, dtype=torch.float64)
    ramp = torch.minimum(torch.minimum(j + 1, w - j), torch.tensor(float(feather + 1), dtype=torch.float64))
    return (ramp / (feather + 1)).float()


class LineWindows(NamedTuple):
    """How the lines of a ``windows=`` sampler call are cut into windows of the model's width (``Diffusion.line_windows``); host
    tensors, not to be written to."""
    offsets: torch.Tensor  # int32 [n, K]: the first line column of window k of line s
    wn: torch.Tensor  # fp32 [n, K, w]: the normalised weights ``wd_window_blend`` reads
    width: int  # the line's latent columns
    K: int
    w: int


class _Call(NamedTuple):
    """What one sampler call is to the reverse loop: everything ``Diffusion._sample`` settles on the host before anything is
    launched, and what follows from it."""
    sampler: _Sampler
    noise_steps: int
    tabulate_film: bool  # ``Diffusion.tabulate_film``
    plain_forwards: int  # ``Diffusion.forwards_per_step``: the forwards of a step that has one prediction
    known: Optional[_Known] = None
    attention: Optional[tuple] = None  # (weights, N) of ``_attention_setup``
    mix: Optional[tuple] = None  # (pairs int32 [nf, rows, n, 2], rates fp32 [n], guidance scale) of ``_mix_setup``
    writer_free: Optional[float] = None  # the scale of ``_guidance_setup``
    x_T: Optional[torch.Tensor] = None
    noise: Optional[Sequence] = None
    seed: Optional[int] = None
    sample_offset: int = 0
    record: Optional[list] = None
    record_pred: Optional[list] = None
    use_graph: bool = True
    windows: Optional[LineWindows] = None  # a line call: ``n`` counts lines, the model runs on n * K windows

    @property
    def mix_forwards(self):
        """The forwards per step of an interpolating call, each reading pairs of its own (0: the call does not interpolate)."""
        return 0 if self.mix is None else int(self.mix[0].shape[0])

    @property
    def two(self):
        """Whether a step has two predictions, which its update lerps (train.py:223-228 with two different forwards)."""
        return self.mix_forwards == 2 or self.writer_free is not None

    @property
    def scale(self):
        """The weight of that lerp; None for a step with one prediction."""
        return None if not self.two else float(self.mix[2]) if self.mix is not None else float(self.writer_free)

    @property
    def forwards(self):
        """``last_stats["forwards_per_step"]``."""
        return self.mix_forwards or (2 if self.writer_free is not None else self.plain_forwards)

    @property
    def model_steps(self):
        return sum(fwd for _, fwd, _ in self.sampler.steps)

    @property
    def model_calls(self):
        return self.model_steps * (2 if self.two else 1)

    @property
    def plan_keywords(self):
        """What ``engine.plan`` takes besides the shapes.  (The interpolation and guidance plans always tabulate the FiLM rows:
        the pairs / rows of every step live in the table's index, not in a per-step upload.)"""
        tau = self.sampler.tau
        film_steps = self.noise_steps if (self.tabulate_film or self.mix is not None or self.writer_free is not None) else 0
        kw = dict(film_steps=film_steps, mix=self.mix_forwards, film_timesteps=tuple(tau) if (film_steps and tau is not None) else None)
        if self.attention is not None:
            kw.update(attn_maps=True, attn_rows=self.attention[0].numel(), attn_by_step=tau is not None)
        if self.writer_free is not None:
            kw.update(guide=2)
        return kw


class _Run:
    """The device side of one ``Diffusion._denoise`` call, filled phase by phase."""
    # guide = (second prediction or None, lerp weight, where the guided prediction is kept or None) and draw = (noise buffer or
    # None, seed, sample_offset) are argument runs of the update launches: device pointers, of buffers this record keeps alive.
    # x, eps, eps1, n, npix are the state a step's tail works on: the plan's ``x_in`` / ``out`` / ``out1`` and the model batch for a
    # plain call; the line latent, the blended line prediction(s) and the lines for a ``windows=`` call, whose model batch is
    # ``nb`` = n * K and whose ``win`` = (offsets, wn) on the device with (lines, K, c, h, w, wl), the argument run of its two launches
    __slots__ = ("call", "lib", "engine", "plan", "inputs", "n", "nb", "npix", "device", "stream", "seed", "blend", "zbuf", "eps_g",
                 "guide", "draw", "graphs", "x", "eps", "eps1", "win")


def latent_mask_from_pixels(mask_px):
    """A keep-mask over pixels [..., H, W] (H, W multiples of 8; nonzero / True = keep) -> the fp32 keep-mask [..., H/8, W/8] over
    the latent cells of the 8x VAE: an 8x8 min-pool, so a latent cell is kept only if every pixel it covers is."""
    m = torch.as_tensor(mask_px)
    if m.dim() < 2 or m.shape[-2] % 8 or m.shape[-1] % 8 or not m.shape[-2] or not m.shape[-1]:
        raise ValueError(f"a pixel mask must be [..., H, W] with H and W multiples of 8, got {tuple(m.shape)}")
    m = (m != 0).to(torch.float32)
    H, W = m.shape[-2:]
    return m.reshape(*m.shape[:-2], H // 8, 8, W // 8, 8).amin(dim=(-3, -1)).contiguous()


class Diffusion:
    """``train.py:174-251`` (T=1000) / ``trainModifyCondition.py:515-622`` (T=600)."""

    def __init__(self, noise_steps=1000, beta_start=1e-4, beta_end=0.02, img_size=(64, 128), args=None):
        self.noise_steps = noise_steps
        self.beta_start = beta_start
        self.beta_end = beta_end
        dev = getattr(args, "device", "cpu") if args is not None else "cpu"
        self.beta = self.prepare_noise_schedule().to(dev)
        self.alpha = 1. - self.beta
        self.alpha_hat = torch.cumprod(self.alpha, dim=0)
        self.img_size = img_size
        self.device = dev
        self._tables = None
        self.forwards_per_step = 1
        self.tabulate_film = os.environ.get("WDIFF_FILM_TABLE", "1") != "0"
        self.last_stats = {}
        self.last_attention = None  # the maps of the last sampler call that asked for them (``attention=``)

    def prepare_noise_schedule(self):
        return torch.linspace(self.beta_start, self.beta_end, self.noise_steps)

    def sample_timesteps(self, n):
        return torch.randint(low=1, high=self.noise_steps, size=(n,))

    # --------------------------------------------------------------------------------------------------
    def noise_images(self, x, t, eps=None, seed=None):
        """``train.py:190-194``; the noise comes from the device Philox stream (or ``eps`` if given)."""
        if not x.is_cuda:
            raise N.NativeError("Diffusion.noise_images runs on the GPU only (no CPU fallback)")
        lib = N.lib()
        st = _stream_ptr(x.device)
        x = x.contiguous().float()
        n = x[0].numel()
        if eps is None:
            eps = torch.empty_like(x)
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else seed
            N.check(lib.wd_randn(eps.data_ptr(), x.shape[0], n, seed, 0, 1, st), "wd_randn")
        sa, sb = self._noise_tables(x.device)
        out = torch.empty_like(x)
        t = t.to(x.device).long().contiguous()
        N.check(lib.wd_noise_images(x.data_ptr(), eps.data_ptr(), t.data_ptr(), sa.data_ptr(), sb.data_ptr(),
                                    x.shape[0], n, out.data_ptr(), st), "wd_noise_images")
        return out, eps

    def min_snr_weights(self, gamma=5.0):
        """Min-SNR-gamma loss weights for eps-prediction (Hang et al. 2023): fp32 [noise_steps] on the host,
        w_t = min(SNR_t, gamma) / SNR_t with SNR_t = alpha_hat_t / (1 - alpha_hat_t).  Evaluated in float64 from the fp32 betas
        (alpha_hat recomputed in float64 as in ``_ddim_tables``) and rounded once; exactly 1 wherever SNR_t <= gamma."""
        gamma = float(gamma)
        if not (math.isfinite(gamma) and gamma > 0.0):
            raise ValueError(f"gamma must be a finite number > 0, got {gamma!r}")
        ah = torch.cumprod(1.0 - self.beta.detach().cpu().double(), dim=0)
        snr = ah / (1.0 - ah)
        return (torch.clamp(snr, max=gamma) / snr).float().contiguous()

    @torch.no_grad()
    def eval_loss(self, model, latents, text_features, labels, t, noise=None, seed=None, loss_mask=None, phoscLabels=None,
                  writer_keep=None):
        """Held-out loss: ``noise_images(latents, t)``, the model's inference forward, then the per-sample masked squared error
        (``optim.weighted_mse_loss`` without a gradient) -> device fp32 [B], sample b's UNWEIGHTED mean over its mask (weights
        are the caller's to apply: ``min_snr_weights()[t]``).  The model runs in ``eval()`` for the call and every module's
        ``training`` flag is put back afterwards; no weight is updated and no generator is drawn from: the noise is ``noise``, or
        the device Philox stream of ``seed`` (0 when neither is given, so a held-out set scores the same from call to call).
        ``t``: an integer tensor [B] in [0, noise_steps); ``loss_mask``: the known-region shapes, values in [0, 1].
        ``writer_keep``: handed to the model's forward - ``False`` scores the writer-free branch a guided sampler runs."""
        from .optim import check_timesteps, expand_loss_mask, weighted_mse_loss
        if latents.dim() != 4:
            raise ValueError(f"latents must be [B, C, h, w], got {tuple(latents.shape)}")
        t = check_timesteps(t, latents.shape[0], self.noise_steps)
        if loss_mask is not None:
            loss_mask = expand_loss_mask(loss_mask, latents.shape).reshape(latents.shape)
        if not latents.is_cuda:
            raise N.NativeError("Diffusion.eval_loss runs on the GPU only (no CPU fallback)")
        dev = latents.device
        if noise is not None:
            noise = noise.to(dev).contiguous().float()
        x_t, eps = self.noise_images(latents, t, eps=noise, seed=0 if seed is None else int(seed))
        flags = [(m, m.training) for m in model.modules()]
        model.eval()
        try:
            kw = dict(timesteps=t.to(dev), context=text_features.to(dev), y=None if labels is None else labels.to(dev))
            if writer_keep is not None:
                kw["writer_keep"] = writer_keep
            if getattr(model, "variant", "base") == "phosc":
                pred = model(x_t, None if phoscLabels is None else phoscLabels.to(dev), **kw)
            else:
                pred = model(x_t, **kw)
        finally:
            for m, flag in flags:
                m.training = flag
        return weighted_mse_loss(pred, eps, mask=loss_mask, want_grad=False)[2]

    def _noise_tables(self, device):
        """sqrt(alpha_hat) and sqrt(1 - alpha_hat), the two per-t scalars of ``train.py:190-194`` in the reference's fp32 op order."""
        ah = self.alpha_hat.cpu()
        return torch.sqrt(ah).to(device), torch.sqrt(1 - ah).to(device)

    def _step_tables(self, device):
        """ca = 1/sqrt(alpha), cb = (1-alpha)/sqrt(1-alpha_hat), cs = sqrt(beta): the three per-t scalars of
        ``train.py:236``, evaluated with the reference's fp32 op order."""
        if self._tables is None or self._tables[0].device != torch.device(device):
            a, ah, b = self.alpha.cpu(), self.alpha_hat.cpu(), self.beta.cpu()
            ca = 1 / torch.sqrt(a)
            cb = (1 - a) / (torch.sqrt(1 - ah))
            cs = torch.sqrt(b)
            self._tables = tuple(t.to(device).contiguous() for t in (ca, cb, cs))
        return self._tables

    def ddim_timesteps(self, steps=None, timesteps=None):
        """The timesteps a DDIM call visits, strictly decreasing: ``steps`` of them spread evenly over [1, T-1] in integer
        arithmetic (first T-1, last 1), or the explicit ``timesteps`` after validation.  The predecessor of an entry is the
        next one; the predecessor of the last is index 0 of the schedule, which is never stepped from (train.py:221)."""
        T = self.noise_steps
        if timesteps is not None:
            tau = [int(t) for t in timesteps]
            if not tau or any(t < 1 or t > T - 1 for t in tau) or any(a <= b for a, b in zip(tau, tau[1:])):
                raise ValueError(f"timesteps must be strictly decreasing with every value in [1, {T - 1}]")
            return tau
        S = int(steps)
        if not 1 <= S <= T - 1:
            raise ValueError(f"steps must be in [1, {T - 1}] for a schedule of {T} noise steps (got {steps})")
        if S == 1:
            return [T - 1]
        return list(reversed([1 + ((T - 2) * k) // (S - 1) for k in range(S)]))

    def _ddim_tables(self, tau, eta, device, to=None):
        """The five per-step coefficients of ``wd_ddim_step`` (fp32 [S] each), with a = alpha_hat[tau[k]], p = alpha_hat of the
        predecessor and sigma = eta sqrt((1-p)/(1-a)) sqrt(1 - a/p):  c1 = sqrt(1-a), c2 = 1/sqrt(a), c3 = sqrt(p),
        c4 = sqrt(max(1 - p - sigma^2, 0)), c5 = sigma.  Evaluated in float64 from the fp32 betas (alpha and its cumprod
        recomputed in float64: the fp32 ``1 - alpha_hat[0]`` has lost half its digits) and rounded to fp32 once.
        ``to``: the level every entry lands on, where that is not the next entry's (the down entries of a resampled walk)."""
        ah = torch.cumprod(1.0 - self.beta.detach().cpu().double(), dim=0)
        tau = [int(t) for t in tau]
        a = ah[tau]
        p = ah[tau[1:] + [0] if to is None else [int(t) for t in to]]
        sigma = float(eta) * torch.sqrt((1 - p) / (1 - a)) * torch.sqrt(1 - a / p)
        c4 = torch.sqrt(torch.clamp(1 - p - sigma * sigma, min=0.0))
        return tuple(c.float().to(device).contiguous() for c in (torch.sqrt(1 - a), 1 / torch.sqrt(a), torch.sqrt(p), c4, sigma))

    def dpmpp_timesteps(self, steps=None, spacing="logsnr", timesteps=None):
        """The timesteps a DPM-Solver++ call visits, strictly decreasing ints in [1, T-1]: the explicit ``timesteps`` after the
        validation of ``ddim_timesteps``; ``spacing="time"``: ``ddim_timesteps(steps)``; ``spacing="logsnr"``: ``steps`` of them
        spread evenly in lambda_t = ln(alpha_hat_t / (1 - alpha_hat_t)) / 2 (float64, alpha_hat recomputed as in ``_ddim_tables``).
        Target k of S is lambda_{T-1} + (lambda_1 - lambda_{T-1}) k / (S-1); its candidate is the index whose lambda is nearest
        (the lowest on a tie), and tau[k] = max(min(candidate, tau[k-1] - 1), S - k) keeps the list strictly decreasing with
        room for the entries still to come: always S entries, the first T-1, the last 1."""
        T = self.noise_steps
        if spacing not in ("logsnr", "time"):
            raise ValueError(f"spacing must be 'logsnr' or 'time', not {spacing!r}")
        if timesteps is not None or spacing == "time":
            return self.ddim_timesteps(steps, timesteps)
        S = int(steps)
        if not 1 <= S <= T - 1:
            raise ValueError(f"steps must be in [1, {T - 1}] for a schedule of {T} noise steps (got {steps})")
        if S == 1:
            return [T - 1]
        ah = torch.cumprod(1.0 - self.beta.detach().cpu().double(), dim=0)
        lam = 0.5 * torch.log(ah / (1 - ah))
        target = lam[T - 1] + (lam[1] - lam[T - 1]) * torch.arange(S, dtype=torch.float64) / (S - 1)
        # (one [S, T-1] argmin rather than S of them: this runs on the host in every call; the first of equal minima is returned)
        cands = (1 + torch.argmin((lam[None, 1:] - target[:, None]).abs(), dim=1)).tolist()
        tau = []
        for k, cand in enumerate(cands):
            if k:
                cand = min(cand, tau[-1] - 1)
            tau.append(max(cand, S - k))
        return tau

    def _dpmpp_tables(self, tau, order, device, to=None, restart=()):
        """The five per-step coefficients of ``wd_dpmpp_step`` (fp32 [S] each), with a = alpha_hat[tau[k]], p = alpha_hat of the
        predecessor (alpha_hat[0] after the last entry, as in ``_ddim_tables``) and h_k = lambda(p) - lambda(a):
        c1 = sqrt(1-a), c2 = 1/sqrt(a), c3 = sqrt((1-p)/(1-a)), c4 = -sqrt(p) expm1(-h_k), c5 = h_k / (2 h_{k-1}).  c5 = 0 makes a
        step first order: k = 0, every k at ``order`` 1, and always the last step (no extrapolation into index 0).  Evaluated
        in float64 from the fp32 betas and rounded to fp32 once.
        ``to`` as in ``_ddim_tables``; ``restart``: entries that are first order as well - the down entries of a resampled walk
        that follow a jump, where the stored data prediction belongs to another level.  h_{k-1} is that of the entry before."""
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, not {order!r}")
        ah = torch.cumprod(1.0 - self.beta.detach().cpu().double(), dim=0)
        tau = [int(t) for t in tau]
        a = ah[tau]
        p = ah[tau[1:] + [0] if to is None else [int(t) for t in to]]
        h = 0.5 * torch.log(p / (1 - p)) - 0.5 * torch.log(a / (1 - a))
        c5 = torch.zeros_like(h)
        if order == 2 and len(tau) > 2:
            c5[1:-1] = h[1:-1] / (2 * h[:-2])
        c5[list(restart)] = 0.0
        tabs = (torch.sqrt(1 - a), 1 / torch.sqrt(a), torch.sqrt((1 - p) / (1 - a)), -torch.sqrt(p) * torch.expm1(-h), c5)
        return tuple(c.float().to(device).contiguous() for c in tabs)

    # --------------------------------------------------------------------------------------------------
    def resample_walk(self, tau, jump=10, resample=1):
        """The walk of a resampled call over the visited timesteps ``tau`` (RePaint, Lugmayr et al. 2022, algorithm 1, on any
        sampler's schedule): a ``_Walk``, settled on the host.  With S = len(tau), down(i) the sampler's step from tau[i] to
        tau[i + 1] (0 after the last) and j, r = jump, resample:

            m = 0
            while m < S:
                down(m); m += 1
                if m % j == 0 and m < S:
                    repeat r - 1 times:  up from tau[m] to tau[m - j];  down(m - j) .. down(m - 1)

        S + (r-1) floor((S-1)/j) j down entries and (r-1) floor((S-1)/j) up entries; every entry starts at the level the one
        before it reached and the last reaches 0; r = 1 or j >= S is the plain schedule.  An up entry from a level with
        A = alpha_hat[from] to one with Q = alpha_hat[to] carries g1 = sqrt(Q/A), g2 = sqrt(1 - Q/A), evaluated in float64
        (alpha_hat recomputed as in ``_ddim_tables``) and rounded to fp32 once.  ValueError: more than WALK_MAX entries."""
        tau, j, r = [int(t) for t in tau], int(jump), int(resample)
        S = len(tau)
        ups = (r - 1) * ((S - 1) // j)
        if S + ups * j + ups > WALK_MAX:
            raise ValueError(f"resample={r}, jump={j} over {S} steps walks {S + ups * j + ups} entries; the limit is {WALK_MAX} "
                             f"(WALK_MAX: one FiLM time row per entry)")
        frm, to, up = [], [], []

        def entry(a, b, is_up):
            frm.append(a), to.append(b), up.append(is_up)
        m = 0
        while m < S:
            entry(tau[m], tau[m + 1] if m + 1 < S else 0, False)
            m += 1
            if m % j == 0 and m < S:
                for _ in range(r - 1):
                    entry(tau[m], tau[m - j], True)
                    for i in range(m - j, m):
                        entry(tau[i], tau[i + 1], False)
        ah = torch.cumprod(1.0 - self.beta.detach().cpu().double(), dim=0)
        ratio = ah[to] / ah[frm]
        is_up = torch.tensor(up)
        zero = torch.zeros((), dtype=torch.float64)
        g1 = torch.where(is_up, torch.sqrt(ratio), zero).float().contiguous()
        g2 = torch.where(is_up, torch.sqrt(torch.clamp(1 - ratio, min=0.0)), zero).float().contiguous()
        return _Walk(frm, to, up, g1, g2, r, j)

    @staticmethod
    def _walk_tables(walk, tabs):
        """The per-step tables of the walk's down entries, spread over all its entries (0 at the up entries, which read none)."""
        down = torch.tensor(walk.down, dtype=torch.int64)
        return tuple(torch.zeros(len(walk.up), dtype=t.dtype).index_copy_(0, down, t).contiguous() for t in tabs)

    @staticmethod
    def _walk_steps(walk, draws):
        """``_Sampler.steps`` of a walk: (k, a down entry, k where entry k makes a draw - an up entry its jump's z, a down entry
        its step's z where ``draws(k)`` - else None)."""
        return [(k, not u, k if (u or draws(k)) else None) for k, u in enumerate(walk.up)]

    def _ddpm(self, calls_model=None, deterministic=False, start=None, walk=None):
        """The DDPM family: t = T-1 .. 1 (train.py:221; ``start`` .. 1 for a call that begins at that level), the model called
        where ``calls_model(t)`` holds (None: everywhere; a step that does not call it reuses the previous predicted noise) and
        one entry of ``noise`` per step while t > 1, counted on skipped steps too.  A step ends with ``wd_ddpm_step`` (the
        guided ``wd_ddpm_step_cfg`` after two forwards), ``wd_known_blend`` at the level t - 1 when a region is kept, and
        ``wd_advance_timestep``.
        ``walk`` (a resampled call, over ``first .. 1``): the loop runs in table form over the walk - ``wd_ddpm_step`` still reads
        t = ``*t_dev``, which ``wd_next_timestep`` sets to tau'[k]; FiLM rows and ``noise`` are indexed by the walk index k."""
        first = self.noise_steps - 1 if start is None else int(start)
        steps = [(i, calls_model is None or bool(calls_model(i)), first - i if i > 1 else None) for i in reversed(range(1, first + 1))]
        if walk is not None:
            steps = self._walk_steps(walk, lambda k: walk.tau[k] > 1)

        def update(lib, P, run):
            ca, cb, cs = self._step_tables(run.device)
            if deterministic:  # regenerateFromtrain2.py:618 drops the sqrt(beta) * noise term
                cs = torch.zeros_like(cs)
            guide, draw = run.guide if run.call.two else (), run.draw
            fn, what = (lib.wd_ddpm_step_cfg, "wd_ddpm_step_cfg") if guide else (lib.wd_ddpm_step, "wd_ddpm_step")

            def launch(stream):
                N.check(fn(run.x.data_ptr(), run.eps.data_ptr(), *guide, run.n, run.npix, ca.data_ptr(), cb.data_ptr(), cs.data_ptr(),
                           P.t_dev.data_ptr(), *draw, stream), what)
            return launch
        # (``steps`` is T - 1 even when steps skip the model: it counts the updates)
        if walk is not None:
            return _Sampler(steps, first, list(walk.tau), update, dict(steps=first), walk)
        return _Sampler(steps, first, None, update, dict(steps=first))

    def _ddim(self, tau, eta, walk=None):
        """DDIM over the visited timesteps ``tau``: step k is timestep tau[k]; FiLM rows, pairs and ``noise`` are indexed by k,
        the model is called at every step and ``noise[k]`` is read only where c5[k] != 0.  A step ends with ``wd_ddim_step``,
        ``wd_known_blend`` at the level tau[k + 1] when a region is kept, and ``wd_next_timestep``.
        ``walk`` (a resampled call, over ``tau``): k is the walk index; a down entry's coefficients are those of its (level from,
        level to), as ``_ddim_tables`` computes them."""
        if walk is None:
            tabs = self._ddim_tables(tau, eta, "cpu")
            steps = [(k, True, k if s != 0.0 else None) for k, s in enumerate(tabs[4].tolist())]  # (host tables: no device sync)
        else:
            down = walk.down
            tabs = self._walk_tables(walk, self._ddim_tables([walk.tau[k] for k in down], eta, "cpu", to=[walk.to[k] for k in down]))
            sigma = tabs[4].tolist()
            steps = self._walk_steps(walk, lambda k: sigma[k] != 0.0)

        def update(lib, P, run):
            c = [t.to(run.device) for t in tabs]
            guide, draw = run.guide, run.draw

            def launch(stream):
                N.check(lib.wd_ddim_step(run.x.data_ptr(), run.eps.data_ptr(), *guide, run.n, run.npix, *(t.data_ptr() for t in c),
                                         P.k_dev.data_ptr(), P.t_dev.data_ptr(), *draw, stream), "wd_ddim_step")
            return launch
        stats = dict(sampler="ddim", steps=len(tau), eta=float(eta), timesteps=list(tau))
        return _Sampler(steps, tau[0], list(tau if walk is None else walk.tau), update, stats, walk)

    def _dpmpp(self, tau, order, spacing=None, walk=None):
        """DPM-Solver++(2M) over the visited timesteps ``tau``: step k is timestep tau[k]; FiLM rows and pairs are indexed by k,
        the model is called at every step and no step draws noise.  The previous data prediction lives in a buffer of the
        update's own, written by every step and read only where c5[k] != 0.  A step ends with ``wd_dpmpp_step``,
        ``wd_known_blend`` as in ``_ddim`` and ``wd_next_timestep``.
        ``walk`` (a resampled call, over ``tau``): k is the walk index; coefficients as in ``_ddim``, h_{k-1} is that of the down
        entry before, and the down entry after a jump is first order - the stored data prediction belongs to another level."""
        if walk is None:
            tabs = self._dpmpp_tables(tau, order, "cpu")
            steps = [(k, True, None) for k in range(len(tau))]
        else:
            down = walk.down
            restart = [i for i, k in enumerate(down) if k and walk.up[k - 1]]
            tabs = self._walk_tables(walk, self._dpmpp_tables([walk.tau[k] for k in down], order, "cpu", to=[walk.to[k] for k in down],
                                                              restart=restart))
            steps = self._walk_steps(walk, lambda k: False)

        def update(lib, P, run):
            c = [t.to(run.device) for t in tabs]
            x0_prev = torch.empty_like(run.x)  # (the first step does not read it: c5[0] == 0; the blend changes x alone)
            guide = run.guide

            def launch(stream):
                N.check(lib.wd_dpmpp_step(run.x.data_ptr(), run.eps.data_ptr(), *guide, x0_prev.data_ptr(), run.n, run.npix,
                                          *(t.data_ptr() for t in c), P.k_dev.data_ptr(), stream), "wd_dpmpp_step")
            return launch
        stats = dict(sampler="dpmpp", steps=len(tau), order=int(order), spacing=spacing, timesteps=list(tau))
        return _Sampler(steps, tau[0], list(tau if walk is None else walk.tau), update, stats, walk)

    def _attention_setup(self, model, sampler, attention):
        """The ``attention`` argument of a sampler call, settled on the host (no device, no library): None, or (weights, N) - the
        fp32 table the steps' ``wd_xattn_maps`` launches read, 1/N at the N model-calling steps whose timestep lies in the window
        and 0 elsewhere, indexed as the sampler's FiLM rows are (by t, [noise_steps], or by the step index of its ``tau``).
        attention: None / False (off), True (every model-calling step) or (t_hi, t_lo), both ends included."""
        if attention is None or attention is False:
            return None
        if attention is True:
            hi, lo = self.noise_steps, 0
        else:
            try:
                hi, lo = attention
                ok = all(not isinstance(v, bool) and int(v) == v for v in (hi, lo))
            except (TypeError, ValueError):
                ok = False
            if not ok or int(lo) > int(hi):
                raise ValueError(f"attention must be True or a timestep window (t_hi, t_lo) with t_hi >= t_lo, not {attention!r}")
            hi, lo = int(hi), int(lo)
        if getattr(model, "variant", "base") == "phosc":
            raise NotImplementedError("attention= with the PHOSC model: it has no per-character attention maps")
        tau = sampler.tau
        rows = [row for row, fwd, _ in sampler.steps if fwd and lo <= (row if tau is None else tau[row]) <= hi]
        if not rows:
            raise ValueError(f"attention window ({hi}, {lo}) selects none of the steps that call the model")
        w = torch.zeros(self.noise_steps if tau is None else len(tau), dtype=torch.float32)
        w[rows] = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(len(rows)), dtype=torch.float32)
        return w, len(rows)

    def _known_setup(self, n, known, known_mask=None, start=None, known_noise="auto", x_T=None, *, draws_noise, tau=None, width=None):
        """The ``known`` / ``known_mask`` / ``start`` / ``known_noise`` arguments of a sampler call, validated and settled on the
        host (no device, no library): a ``_Known``, or None where the call passes none of them.

        known        fp32 [n, C, h, w], latents as the model sees them (what ``LatentCache`` holds).
        known_mask   None, or fp32 with values in [0, 1], 1 = keep, of shape [h, w], [n, 1, h, w] or [n, C, h, w]; expanded here,
                     once, to [n, C*h*w].
        start        an int in [1, T-1]: the loop begins from ``known`` noised to that level.  DDPM (``tau`` None) visits
                     start .. 1; DDIM / DPM++ visit the entries of ``tau`` (their usual schedule) that are <= start, returned as
                     ``_Known.tau``, and the level noised to, ``_Known.start``, is the first of them.
        known_noise  "fresh": the blend draws its noise per step (RePaint); "fixed": one eps per sample, the one that noises to
                     ``start``; a tensor [n, C, h, w]: fixed and given; "auto": "fresh" where the call draws step noise itself
                     (``draws_noise``: DDPM, DDIM with eta > 0), "fixed" otherwise - a deterministic sampler stays one.
        width        the latent columns of a line of a ``windows=`` call, which take the place of w in every shape above."""
        T = self.noise_steps
        if known is None:
            if known_mask is not None or start is not None or not (isinstance(known_noise, str) and known_noise == "auto"):
                raise ValueError("known_mask, start and known_noise need the known latents (known=)")
            return None
        if known_mask is None and start is None:
            raise ValueError("known needs a known_mask (the region to keep), a start level, or both")
        h, w = self.img_size[0] // 8, self.img_size[1] // 8 if width is None else int(width)
        x0 = torch.as_tensor(known)
        if not x0.is_floating_point() or x0.dim() != 4 or x0.shape[0] != n or tuple(x0.shape[2:]) != (h, w):
            raise ValueError(f"known must be a float tensor [{n}, C, {h}, {w}], got {x0.dtype} {tuple(x0.shape)}")
        shape = tuple(x0.shape)
        C = shape[1]
        x0 = x0.detach().to(torch.float32).cpu().reshape(n, -1).contiguous()
        mask = None
        if known_mask is not None:
            mask = torch.as_tensor(known_mask)
            if mask.dtype == torch.bool:
                mask = mask.to(torch.float32)
            if not mask.is_floating_point() or tuple(mask.shape) not in ((h, w), (n, 1, h, w), shape):
                raise ValueError(f"known_mask must be a float tensor [{h}, {w}], [{n}, 1, {h}, {w}] or {list(shape)}, "
                                 f"got {mask.dtype} {tuple(mask.shape)}")
            mask = mask.detach().to(torch.float32).cpu()
            if not bool(((mask >= 0) & (mask <= 1)).all()):
                raise ValueError("known_mask values must lie in [0, 1] (1 = keep)")
            mask = mask.expand(n, C, h, w).reshape(n, -1).contiguous()
        if start is not None:
            if x_T is not None:
                raise ValueError("start begins the loop from the noised known latents: it cannot be combined with x_T")
            if isinstance(start, bool) or int(start) != start or not 1 <= int(start) <= T - 1:
                raise ValueError(f"start must be an int in [1, {T - 1}], not {start!r}")
            start = int(start)
            if tau is not None:
                tau = [t for t in tau if t <= start]
                if not tau:
                    raise ValueError(f"start={start} lies below every visited timestep: no step is left")
                start = tau[0]
        eps = None
        if isinstance(known_noise, str):
            if known_noise not in ("auto", "fresh", "fixed"):
                raise ValueError(f"known_noise must be 'auto', 'fresh', 'fixed' or a tensor {list(shape)}, not {known_noise!r}")
            mode = known_noise if known_noise != "auto" else ("fresh" if draws_noise else "fixed")
        else:
            eps = torch.as_tensor(known_noise)
            if not eps.is_floating_point() or tuple(eps.shape) != shape:
                raise ValueError(f"known_noise must be a float tensor {list(shape)}, got {eps.dtype} {tuple(eps.shape)}")
            eps = eps.detach().to(torch.float32).cpu().reshape(n, -1).contiguous()
            mode = "fixed"
        return _Known(x0, mask, start, None if tau is None else list(tau), mode, eps)

    def _resample_setup(self, model, tau, resample, jump, known, attention=None, mix_rate=None, style_pairs=None, noise=None):
        """The ``resample`` / ``jump`` arguments of a sampler call, validated and settled on the host (no device, no library, no
        draw): None where the call does not resample (``resample`` 1: the plain path, whatever ``jump`` holds), else the ``_Walk``
        over ``tau``, the timesteps the plain call would visit.  ValueError: ``resample`` or ``jump`` not an int >= 1, no
        ``known_mask`` (nothing to harmonise), a walk of more than WALK_MAX entries, a ``noise`` list that does not hold one tensor
        per walk entry.  NotImplementedError: ``attention=`` (the accumulators would count revisits) and writer-style
        interpolation."""
        for name, v in (("resample", resample), ("jump", jump)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{name} must be an int >= 1, not {v!r}")
        if resample == 1:
            return None
        if known is None or known.mask is None:
            raise ValueError("resample > 1 needs a known_mask: without a kept region there is nothing to harmonise")
        if attention is not None and attention is not False:
            raise NotImplementedError("attention= with resample > 1: the accumulators would count the revisited steps")
        if style_pairs is not None or (mix_rate is not None and getattr(model, "interpolation", False)):
            raise NotImplementedError("writer-style interpolation (mix_rate / style_pairs) with resample > 1")
        walk = self.resample_walk(tau, jump, resample)
        if noise is not None and len(noise) != len(walk.up):
            raise ValueError(f"noise of a resampled call must hold one entry per walk entry ({len(walk.up)})")
        return walk

    def line_windows(self, n, K, overlap=0, offsets=None, width=None, weight=None, feather=0):
        """How ``n`` lines of ``K`` words each are cut into windows of the model's latent width w (``img_size[1] // 8``), for the
        ``windows=`` argument of the samplers: a ``LineWindows``, settled on the host - nothing is launched.
        offsets  None: window k begins at column k * (w - overlap), the same in every line; or ints [K] / [n, K] in 0 .. width - w.
        width    the line's latent columns; None: K * w - (K - 1) * overlap.
        weight   what a window's columns weigh in the average, >= 0, [w], [K, w] or [n, K, w]; None: ``window_profile(w, feather)``.
        The normalised table is wn[s, k, j] = weight[s, k, j] / (the sum of the weights of the windows that cover column
        offsets[s, k] + j), evaluated in float64 and rounded to fp32 once, as the sampler tables are.  Every column must be covered
        (some window has wn > 0 there).  ValueError: an offset outside its range, a negative weight, K > WD_WINDOW_MAX, an uncovered
        column (the message names the line and the column)."""
        w = self.img_size[1] // 8
        n, K = int(n), int(K)
        if n < 1 or not 1 <= K <= WINDOW_MAX:
            raise ValueError(f"line_windows needs n >= 1 lines of 1 .. {WINDOW_MAX} (WD_WINDOW_MAX) windows, got n = {n}, K = {K}")
        overlap = int(overlap)
        if not 0 <= overlap < w:
            raise ValueError(f"overlap must be in 0 .. {w - 1} latent columns, got {overlap}")
        if offsets is None:
            off = (torch.arange(K, dtype=torch.int64) * (w - overlap)).expand(n, K)
        else:
            off = torch.as_tensor(offsets)
            if off.is_floating_point() or off.dtype == torch.bool or tuple(off.shape) not in ((K,), (n, K)):
                raise ValueError(f"offsets must be integers [{K}] or [{n}, {K}], got {off.dtype} {tuple(off.shape)}")
            off = off.to(torch.int64).cpu().expand(n, K)
        width = K * w - (K - 1) * overlap if width is None else int(width)
        if width < w:
            raise ValueError(f"a line is at least one window wide: width {width} < w = {w}")
        bad = ((off < 0) | (off > width - w)).nonzero()
        if len(bad):
            s, k = (int(v) for v in bad[0])
            raise ValueError(f"offset {int(off[s, k])} of window {k} of line {s} lies outside 0 .. {width - w} (width {width}, w = {w})")
        wt = window_profile(w, feather) if weight is None else torch.as_tensor(weight)
        if not wt.is_floating_point() or tuple(wt.shape) not in ((w,), (K, w), (n, K, w)):
            raise ValueError(f"weight must be a float tensor [{w}], [{K}, {w}] or [{n}, {K}, {w}], got {wt.dtype} {tuple(wt.shape)}")
        wt = wt.detach().to(torch.float32).cpu().expand(n, K, w)
        if not bool((torch.isfinite(wt) & (wt >= 0)).all()):
            raise ValueError("weight values must be finite and >= 0")
        cols = (off[:, :, None] + torch.arange(w, dtype=torch.int64)).reshape(n, K * w)
        total = torch.zeros(n, width, dtype=torch.float64).scatter_add_(1, cols, wt.double().reshape(n, K * w))
        div = total.gather(1, cols).reshape(n, K, w)
        wn = torch.where(div > 0, wt.double() / div, torch.zeros((), dtype=torch.float64)).float().contiguous()
        covered = torch.zeros(n, width, dtype=torch.float32).scatter_add_(1, cols, (wn > 0).float().reshape(n, K * w)) > 0
        if not bool(covered.all()):
            s, J = (int(v) for v in (~covered).nonzero()[0])
            raise ValueError(f"line {s}: column {J} is covered by no window (every column needs a window with a weight > 0 there)")
        return LineWindows(off.to(torch.int32).contiguous(), wn, width, K, w)

    def _line_setup(self, model, n, windows, x_text, labels, phoscLabels, attention, mix_rate, style_pairs):
        """The ``windows`` argument of a sampler call and what it changes of the call's inputs, settled on the host before anything
        is launched or drawn: (the model batch n * K, the n * K words, writer ids and PHOSC labels in model-batch order
        b = s * K + k).  Refuses what does not compose with lines (NotImplementedError): ``attention=`` and writer-style
        interpolation."""
        K = windows.K
        if attention is not None and attention is not False:
            raise NotImplementedError("attention= with windows=: per-character maps of a line are not built")
        if style_pairs is not None or (mix_rate is not None and getattr(model, "interpolation", False)):
            raise NotImplementedError("writer-style interpolation (mix_rate / style_pairs) with windows=")
        rows = list(x_text) if not isinstance(x_text, str) else None
        if rows is not None and len(rows) == K and all(isinstance(v, str) for v in rows):
            rows = [rows] * n  # one list of K words for every line
        if rows is None or len(rows) != n or any(isinstance(r, str) or len(r) != K or not all(isinstance(v, str) for v in r) for r in rows):
            raise ValueError(f"x_text of a windows= call must be a list of {n} lists of {K} words, or one list of {K} words for all lines")
        words = [v for r in rows for v in r]
        if labels is not None:
            labels = torch.as_tensor(labels)
            if tuple(labels.shape) != (n,):
                raise ValueError(f"labels of a windows= call must hold one writer per line [{n}], got {tuple(labels.shape)}")
            labels = labels.repeat_interleave(K)
        if phoscLabels is not None:
            p = torch.as_tensor(phoscLabels)
            if not ((p.dim() == 3 and tuple(p.shape[:2]) == (n, K)) or (p.dim() == 2 and p.shape[0] == n * K)):
                raise ValueError(f"phoscLabels of a windows= call must be [{n}, {K}, L] or [{n * K}, L], got {tuple(p.shape)}")
            phoscLabels = p.reshape(n * K, p.shape[-1])
        return n * K, words, labels, phoscLabels

    def _line_width(self, windows, n):
        """The latent columns of a line of the call (None without ``windows``), after checking that the layout is this call's."""
        if windows is None:
            return None
        if not isinstance(windows, LineWindows):
            raise TypeError(f"windows must be what Diffusion.line_windows returns, not {type(windows).__name__}")
        if tuple(windows.offsets.shape) != (n, windows.K) or windows.w != self.img_size[1] // 8:
            raise ValueError(f"windows lays out {windows.offsets.shape[0]} lines of windows {windows.w} wide; the call has n = {n} "
                             f"lines and the model's latent is {self.img_size[1] // 8} wide")
        return windows.width

    def _denoise(self, model, n, text_features, labels, phosc, device, call):
        """The one reverse loop of every sampler (``_ddpm`` / ``_ddim`` / ``_dpmpp``); ``call`` is the ``_Call`` of ``_sample``.
        ``_plan_call`` refuses and plans; then, on a side stream, ``_start_latent`` and ``_upload`` fill the plan's buffers,
        ``_step_tail`` builds the step, ``_capture`` turns it into one or two hipGraphs, ``_loop`` visits the sampler's steps and
        ``_results`` leaves ``last_stats`` / ``last_attention`` and returns x.  The graphs are destroyed on every exit path, after
        the stream that may still be running them has drained."""
        run = self._plan_call(model, n, text_features, labels, phosc, device, call)
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        run.stream = side.cuda_stream
        try:
            with torch.cuda.stream(side):
                self._start_latent(run)
                self._upload(run)
                step = self._step_tail(run)  # (kept out of ``run``, which it refers to: no reference cycle holds the buffers)
                self._capture(run, step)
                self._loop(run, step)
                x = self._results(run)
            torch.cuda.current_stream(device).wait_stream(side)
        finally:
            if run.graphs:
                side.synchronize()
                for g in run.graphs:
                    run.lib.wd_graph_destroy(g)
        return x

    def _plan_call(self, model, n, text_features, labels, phosc, device, call):
        """Refuses ids that do not fit their tables (host tensors: nothing is launched for them and no device sync), repacks
        weights that changed (``engine.refresh_weights``), gets the launch plan and settles the call's seed.  Launches nothing else.
        A ``windows=`` call plans the forward at the model batch n * K and the model's own h, w; its ``npix`` is the line's."""
        run = _Run()
        run.call, run.lib, run.engine, run.n, run.device, run.graphs = call, N.lib(), model.engine, n, device, []
        win = call.windows
        run.nb = n if win is None else n * win.K
        if call.mix is not None:
            run.engine.check_pairs(call.mix[0])  # first: nothing is launched for an id that does not fit the table
            labels = None  # unused in this mode (unet.py:1558-1573)
        run.engine.refresh_weights()
        run.engine.check_ids(text_features, labels, phosc, need_y=call.mix is None)
        run.inputs = (text_features, labels, phosc)
        run.plan = run.engine.plan(run.nb, self.img_size[0] // 8, self.img_size[1] // 8, text_features.shape[1],
                                   0 if phosc is None else phosc.shape[1], **call.plan_keywords)
        shape = tuple(run.plan.x_in.shape[1:]) if win is None else tuple(run.plan.x_in.shape[1:3]) + (win.width,)
        run.npix = math.prod(shape)
        if win is not None:  # (a plain call's x_T and noise are checked by the copies that read them, as ever)
            given = [("x_T", call.x_T)] + [(f"noise[{i}]", z) for i, z in enumerate(call.noise or ())]
            for name, t in given:
                if t is not None and tuple(t.shape) != (n,) + shape:
                    raise ValueError(f"{name} of a windows= call must be line-shaped {[n, *shape]}, got {list(t.shape)}")
        run.seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if call.seed is None else int(call.seed)
        if call.known is not None and call.known.x0.shape[1] != run.npix:
            raise ValueError(f"known holds {call.known.x0.shape[1]} values per sample, the model's latent {run.npix} {shape}")
        return run

    def _start_latent(self, run):
        """Fills ``run.x``, the latent the loop starts from: the known latents noised to ``known.start`` (``wd_noise_images`` with
        the call's fixed eps - the caller's, or ``wd_randn`` on stream WD_STREAM_KNOWN of the seed at the global rows), the
        caller's ``x_T``, or ``wd_randn``.  With a mask, ``run.blend`` = (x0, mask, eps or None, sqrt_ah, sqrt_1m_ah) on the device is
        what every step's ``wd_known_blend`` reads (eps None: it draws its noise per step).
        First it settles the state a step's tail works on (``run.x`` / ``eps`` / ``eps1``): the plan's own buffers, or, for a
        ``windows=`` call, the line latent and line prediction(s) with the layout's offsets and weights on the device
        (``run.win``) - the start latent is then the line's: line s depends on (seed, sample_offset + s) only."""
        call, lib, P, n, npix, device, st = run.call, run.lib, run.plan, run.n, run.npix, run.device, run.stream
        if call.windows is None:
            run.x, run.eps, run.eps1, run.win = P.x_in, P.out, P.out1 if call.two else None, None
        else:
            W = call.windows
            c, h, w = P.x_in.shape[1:]
            run.x = torch.empty((n, c, h, W.width), dtype=torch.float32, device=device)
            run.eps = torch.empty_like(run.x)
            run.eps1 = torch.empty_like(run.x) if call.two else None
            run.win = (W.offsets.to(device), W.wn.to(device), (n, W.K, c, h, w, W.width))
        known, run.blend = call.known, None
        if known is not None:
            kx0 = known.x0.to(device)
            sa, sb = self._noise_tables(device)
            keps = None
            if known.start is not None or (known.mask is not None and known.mode == "fixed"):
                if known.eps is not None:
                    keps = known.eps.to(device)
                else:
                    keps = torch.empty_like(kx0)
                    N.check(lib.wd_randn(keps.data_ptr(), n, npix, run.seed, call.sample_offset, N.STREAM_KNOWN, st), "wd_randn")
            if known.mask is not None:
                run.blend = (kx0, known.mask.to(device), keps if known.mode == "fixed" else None, sa, sb)
        if known is not None and known.start is not None:
            level = torch.full((n,), known.start, dtype=torch.int64, device=device)
            N.check(lib.wd_noise_images(kx0.data_ptr(), keps.data_ptr(), level.data_ptr(), sa.data_ptr(), sb.data_ptr(), n, npix,
                                        run.x.data_ptr(), st), "wd_noise_images")
        elif call.x_T is not None:
            run.x.copy_(call.x_T.to(device))
        else:
            N.check(lib.wd_randn(run.x.data_ptr(), n, npix, run.seed, call.sample_offset, 0, st), "wd_randn")

    def _upload(self, run):
        """The call's side inputs into the plan's buffers: word ids, writer ids and PHOSC labels, the pairs and rates of an
        interpolating call, the attention weights with zeroed accumulators, the first timestep; and the two buffers the loop
        itself fills or reads: ``zbuf`` for a step's ``noise`` entry, ``eps_g`` for the guided prediction ``record_pred`` receives."""
        call, P, device = run.call, run.plan, run.device
        text_features, labels, phosc = run.inputs
        run.engine.load_inputs(P, None, None, text_features.to(device), labels.to(device) if labels is not None else None,
                               phosc.to(device) if phosc is not None else None, check=False)
        if call.mix is not None:
            run.engine.load_mix(P, call.mix[0].to(device), call.mix[1].to(device), check=False)
        if call.attention is not None:
            P.map_w.copy_(call.attention[0])
            for acc in P.maps:
                acc.zero_()
        run.eps_g = torch.empty_like(run.eps) if (call.two and call.record_pred is not None) else None
        P.t_dev.fill_(call.sampler.t_first)
        P.t_in.fill_(call.sampler.t_first)
        # (a resampled call that draws its own step noise fills ``zbuf`` on the device, per walk entry: ``_step_tail``)
        fills = call.noise is None and call.sampler.walk is not None and any(fwd and z is not None for _, fwd, z in call.sampler.steps)
        run.zbuf = torch.zeros_like(run.x) if (call.noise is not None or fills) else None
        run.guide = (run.eps1.data_ptr(), call.scale, _dptr(run.eps_g)) if call.two else (None, 0.0, None)
        run.draw = (_dptr(run.zbuf), run.seed, call.sample_offset)

    def _step_tail(self, run):
        """One step as the loop and the capture launch it, ``step(stream, forward)``: the forward(s) (``run_step1`` after
        ``run_step`` when the step has two predictions), the sampler's own update launch, ``wd_known_blend`` when a region is kept
        and the advance.  A sampler indexed by t (``tau`` None) blends at the level t - 1 and advances with
        ``wd_advance_timestep``; one that visits ``tau`` (put on the device here, its step counter ``k_dev`` zeroed) blends at the
        level of tau[k + 1] (index 0 after the last entry) and advances with ``wd_next_timestep``.
        A ``windows=`` call wraps the forward(s) of a step in its two launches: ``wd_window_gather`` cuts the line into the plan's
        ``x_in`` before them, ``wd_window_blend`` averages the plan's ``out`` (and ``out1``) into the line prediction(s) after them;
        update and blend then work on the line, the advance on the model batch.  A step without a forward runs neither.
        A resampled call (``sampler.walk``) visits the walk table tau', so blend and advance are right as they stand, and its draws
        are keyed by the walk index k: a down entry that draws its own step noise fills ``zbuf`` first (``wd_walk_randn``,
        WD_WALK_STEP), which the update reads through its ``noise`` argument, and a blend that draws per step reads a second
        buffer filled likewise (WD_WALK_BLEND).  ``step(stream, up=True)`` is an up entry: ``wd_forward_jump`` on the whole state -
        its z the entry's ``noise`` tensor, or its own draw - and the advance, nothing else."""
        call, lib, P, n, nb, npix = run.call, run.lib, run.plan, run.n, run.nb, run.npix
        update = call.sampler.update(lib, P, run)
        tau, two, walk = call.sampler.tau, call.two, call.sampler.walk
        forwards = 1 if (two or call.mix is not None) else call.plain_forwards
        if tau is not None:
            tau_dev = torch.tensor(tau, dtype=torch.int32, device=run.device)
            P.k_dev.zero_()
        x, win = run.x, run.win
        zfill = kbuf = None
        if walk is not None:
            g1, g2 = walk.g1.to(run.device), walk.g2.to(run.device)
            zfill = run.zbuf if call.noise is None else None
            kbuf = torch.empty_like(x) if (run.blend is not None and run.blend[2] is None) else None
            jump_draw = (_dptr(run.zbuf) if call.noise is not None else None, run.seed, call.sample_offset)

        def fill(buf, which, stream):
            N.check(lib.wd_walk_randn(buf.data_ptr(), n, npix, run.seed, call.sample_offset, which, P.k_dev.data_ptr(), stream),
                    "wd_walk_randn")

        def advance(stream):
            if tau is None:
                N.check(lib.wd_advance_timestep(P.t_dev.data_ptr(), -1, P.t_in.data_ptr(), nb, stream), "wd_advance_timestep")
            else:
                N.check(lib.wd_next_timestep(P.k_dev.data_ptr(), tau_dev.data_ptr(), len(tau), P.t_dev.data_ptr(), P.t_in.data_ptr(), nb,
                                             stream), "wd_next_timestep")

        def step(stream, forward=True, up=False):
            if up:
                N.check(lib.wd_forward_jump(x.data_ptr(), n, npix, g1.data_ptr(), g2.data_ptr(), P.k_dev.data_ptr(), *jump_draw, stream),
                        "wd_forward_jump")
                advance(stream)
                return
            if forward:
                if win is not None:
                    N.check(lib.wd_window_gather(x.data_ptr(), win[0].data_ptr(), *win[2], P.x_in.data_ptr(), stream), "wd_window_gather")
                for _ in range(forwards):
                    P.run_step(stream)
                if two:  # train.py:223-228 with two different forwards: lerp(second, first, cfg_scale) feeds the update
                    P.run_step1(stream)
                if win is not None:
                    N.check(lib.wd_window_blend(P.out.data_ptr(), P.out1.data_ptr() if two else None, win[1].data_ptr(), win[0].data_ptr(),
                                                *win[2], run.eps.data_ptr(), _dptr(run.eps1), stream), "wd_window_blend")
            if zfill is not None:
                fill(zfill, N.WALK_STEP, stream)
            update(stream)
            if run.blend is not None:
                x0, mask, eps, sa, sb = run.blend
                if kbuf is not None:
                    fill(kbuf, N.WALK_BLEND, stream)
                    eps = kbuf
                level = (None, None, 0) if tau is None else (P.k_dev.data_ptr(), tau_dev.data_ptr(), len(tau))
                N.check(lib.wd_known_blend(x.data_ptr(), x0.data_ptr(), mask.data_ptr(), n, npix, sa.data_ptr(), sb.data_ptr(),
                                           P.t_dev.data_ptr(), *level, _dptr(eps), run.seed, call.sample_offset, stream), "wd_known_blend")
            advance(stream)
        return step

    def _capture(self, run, step):
        """What the steps share, before any of them: the word embedding and cross-attention K/V (``run_cond``), the time MLP of
        every timestep (``run_film``) and the FiLM rows of the first step - the captured step only reads the table, whose rows are
        indexed by t or by the step index.  Then, unless the call is eager, one hipGraph of a whole step and, where steps reuse the
        previous predicted noise, one of the tail alone - for a resampled call, one of the up entry; ``run.graphs`` holds each from
        the moment it exists."""
        call, lib, P, st = run.call, run.lib, run.plan, run.stream
        P.run_cond(st)
        P.run_film(st)
        if call.sampler.steps:
            P.film_prepare(call.sampler.steps[0][0], st)
        if not call.use_graph or call.record is not None or call.record_pred is not None:
            return  # eager launches: asked for, or needed to read a step's tensors
        up = call.sampler.walk is not None  # a resampled call's entries without a forward are its up entries
        for forward in (True, False) if call.model_steps < len(call.sampler.steps) else (True,):
            N.check(lib.wd_graph_begin(st), "wd_graph_begin")
            try:
                step(st, forward, up and not forward)
            finally:  # (ends the capture when a launch of the step raised, too)
                g = C.c_void_p()
                rc = lib.wd_graph_end(st, C.byref(g))
            N.check(rc, "wd_graph_end")
            run.graphs.append(g)

    def _loop(self, run, step):
        """Per visited step: x into ``record``, the step's ``noise`` entry into ``zbuf`` if it has one, the FiLM rows of the step
        (``film_prepare``, computed per chunk of rows) when it calls the model, then the step - ``wd_graph_launch`` of the whole
        step or of its tail, or its eager launches - and its predictions into ``record_pred``.  An up entry of a resampled call
        is a step without a forward whose launches are the jump's: x into ``record``, its ``noise`` entry, its graph."""
        call, lib, P, st, device = run.call, run.lib, run.plan, run.stream, run.device
        record, record_pred, noise, zbuf, two = call.record, call.record_pred, call.noise, run.zbuf, call.two
        gexec, gskip = (run.graphs + [None, None])[:2]
        up = call.sampler.walk is not None  # (as in ``_capture``: the second graph of a resampled call is its up entry)
        for row, fwd, z in call.sampler.steps:
            if record is not None:
                record.append(run.x.clone())
            if noise is not None and z is not None:
                zbuf.copy_(noise[z].to(device))
            if fwd:
                P.film_prepare(row, st)
            if gexec is not None:
                N.check(lib.wd_graph_launch(gexec if fwd else gskip, st), "wd_graph_launch")
            else:
                step(st, fwd, up and not fwd)
            if record_pred is not None and fwd:
                pred = (P.out.clone(),) if not two else (P.out.clone(), P.out1.clone())
                if run.win is not None:  # the window predictions, then the line prediction(s) they were blended into
                    pred += (run.eps.clone(),) if not two else (run.eps.clone(), run.eps1.clone())
                record_pred.append(pred + ((run.eps_g.clone(),) if two else ()))

    def _results(self, run):
        """x, cloned out of the plan's buffer; ``last_attention`` (the accumulators, cloned likewise, or None) and ``last_stats``."""
        call, P, known = run.call, run.plan, run.call.known
        x = run.x.clone()
        self.last_attention = None
        if call.attention is not None:
            self.last_attention = {k: acc.clone().reshape(run.n, mh, mw, -1)
                                   for k, acc, (mh, mw) in zip(("input", "middle", "output"), P.maps, P.map_hw)}
        self.last_stats = dict(call.sampler.stats, forwards_per_step=call.forwards, graph=bool(run.graphs), seed=run.seed,
                               sample_offset=call.sample_offset, model_calls=call.model_calls, known=known is not None,
                               start=None if known is None else known.start, known_noise=None if known is None else known.mode)
        walk = call.sampler.walk
        self.last_stats.update(resample=1 if walk is None else walk.resample, jump=None if walk is None else walk.jump,
                               walk=len(call.sampler.steps))
        if call.attention is not None:
            self.last_stats["attention_steps"] = call.attention[1]
        if call.writer_free is not None:
            self.last_stats["guidance"] = "writer_free"
        if call.windows is not None:
            self.last_stats.update(windows=call.windows.K, line_width=call.windows.width, model_batch=run.nb)
        return x

    def _guidance_setup(self, model, guidance, cfg_scale, mix):
        """The ``guidance`` argument of a sampler call, settled on the host: the ``writer_free`` field of the ``_Call`` - None,
        or the scale of the guided update.  ``guidance="writer_free"`` with ``cfg_scale > 0`` runs, per model-calling step, the
        conditional forward, the forward without the writer term and ``torch.lerp(free, cond, cfg_scale)``; with ``cfg_scale == 0``
        one forward runs, as behind the reference's ``if cfg_scale > 0`` (train.py:223), and the call is the plain one."""
        if guidance is None:
            return None
        if guidance != "writer_free":
            raise ValueError(f"guidance must be None or 'writer_free', not {guidance!r}")
        if mix is not None:
            raise ValueError("guidance='writer_free' cannot be combined with writer-style interpolation (args.interpolation "
                             "with a mix_rate, or style_pairs)")
        if getattr(model, "num_classes", None) is None:
            raise ValueError("guidance='writer_free' needs a class-conditional model (num_classes)")
        s = float(cfg_scale)
        if not math.isfinite(s) or s < 0:
            raise ValueError(f"cfg_scale must be a finite number >= 0, got {cfg_scale!r}")
        return s if s > 0 else None

    def _mix_setup(self, model, n, mix_rate, style_pairs, cfg_scale, *, sampler=None):
        """The ``mix`` field of the ``_Call`` of a sampler call, or None where the call does not interpolate (``_mix_check``, which
        refuses a bad ``mix_rate`` / ``style_pairs`` before anything is drawn, then ``_mix_table``).

        Fixed-pair mode (``style_pairs`` given: one ``(s1, s2)`` or an int tensor [n, 2]; ``mix_rate`` a float or fp32 [n]): the
        same pair at every step, so the two guidance forwards of train.py:223-228 are identical and one runs.
        Reference mode (``model.interpolation`` and a ``mix_rate``): every forward of the reference's loop draws a pair of its own
        (unet.py:1561-1564) - they are drawn here, all of them, in loop order, before anything is launched; with
        ``cfg_scale > 0`` a step runs both forwards and the guided update.
        Otherwise ``mix_rate`` is ignored, as the reference's forward ignores it (unet.py:1558), and ``random`` is not touched.
        ``sampler`` (default ``_ddpm()``) says which steps those are: pairs are drawn for its model-calling steps only, in loop
        order, and the table is indexed as its FiLM rows are - by t, [nf, T, n, 2], or by the step index of its ``tau``,
        [nf, S, n, 2]."""
        checked = self._mix_check(model, n, mix_rate, style_pairs)
        return None if checked is None else self._mix_table(checked, n, cfg_scale, sampler or self._ddpm())

    def _mix_check(self, model, n, mix_rate, style_pairs):
        """The deciding and validating half of ``_mix_setup``, which touches neither ``random`` nor the device: None where the
        call does not interpolate, else (the fixed pairs, int32 [n, 2], or None where they are to be drawn; the rates, fp32 [n])."""
        if style_pairs is not None:
            if mix_rate is None:
                raise ValueError("style_pairs needs a mix_rate (a float, or one per sample)")
            sp = torch.as_tensor(style_pairs)
            if sp.is_floating_point() or sp.shape not in ((2,), (n, 2)):
                raise ValueError(f"style_pairs must be (s1, s2) or an integer tensor [{n}, 2]")
            sp = sp.to(torch.int32).cpu().reshape(-1, 2).expand(n, 2)
        elif mix_rate is not None and getattr(model, "interpolation", False):
            sp = None
        else:
            return None
        m = torch.as_tensor(mix_rate, dtype=torch.float32).cpu().reshape(-1)
        if m.numel() not in (1, n):
            raise ValueError(f"mix_rate must be a float or hold one rate per sample ({n})")
        return sp, m.expand(n).contiguous()

    def _mix_table(self, checked, n, cfg_scale, sampler):
        """The other half: the pairs table of a call ``_mix_check`` accepted - here the pairs are drawn - with its rates and scale."""
        sp, m = checked
        T = self.noise_steps if sampler.tau is None else len(sampler.tau)
        if sp is not None:
            tab = sp.reshape(1, 1, n, 2).expand(1, T, n, 2).contiguous()
        else:
            steps = [row for row, fwd, _ in sampler.steps if fwd]
            nf = 2 if cfg_scale > 0 else 1
            drawn = draw_style_pairs(nf * len(steps))
            tab = torch.zeros((nf, T, n, 2), dtype=torch.int32)
            for k, i in enumerate(steps):
                for f in range(nf):
                    tab[f, i] = torch.tensor(drawn[nf * k + f], dtype=torch.int32)
        return tab, m, float(cfg_scale)

    def _text_features(self, x_text, n, underscore=False):
        words = [x_text] * n if isinstance(x_text, str) else list(x_text)
        if len(words) != n:
            raise ValueError("x_text must be one word or a list of n words")
        pad = label_padding_underscore if underscore else label_padding
        return torch.tensor(np.array([pad(w, NUM_TOKENS) for w in words], dtype="int64"))

    def _prepare(self, who, model, n, x_text, args, phoscLabels, underscore=None, check_latent=True):
        """What every sampler entry point settles before its loop: (device, word ids, PHOSC labels or None)."""
        device = torch.device(getattr(args, "device", self.device))
        if device.type != "cuda":
            raise N.NativeError(f"Diffusion.{who} runs on an MI355X only (no CPU fallback)")
        if check_latent and (self.img_size is None or not (getattr(args, "latent", True) == True)):  # noqa: E712
            raise NotImplementedError("latent=False")
        if underscore is None:
            underscore = int(model.word_emb.embedding.weight.shape[0]) == VOCAB_SIZE_UNDERSCORE
        tf = self._text_features(x_text, n, underscore)
        phosc = None
        if getattr(args, "phosc", 0) == 1 or getattr(args, "phos", 0) == 1:
            if phoscLabels is None:
                raise ValueError("args.phosc/phos set but phoscLabels missing")
            phosc = phoscLabels.int()
        return device, tf, phosc

    def _finish(self, x, vae, args):
        """``train.py:238-250``: latents / 0.18215 -> vae.decode -> [0,1] image (vae is duck-typed)."""
        latent = getattr(args, "latent", True)
        if latent == True:  # noqa: E712  (argparse type=bool quirk of the reference)
            if vae is None:
                return x
            latents = 1 / 0.18215 * x
            image = vae.decode(latents).sample
            image = (image / 2 + 0.5).clamp(0, 1)
            image = image.cpu().permute(0, 2, 3, 1).numpy()
            image = torch.from_numpy(image)
            return image.permute(0, 3, 1, 2)
        raise NotImplementedError("latent=False (pixel-space UNet) is dead code in the reference (SURVEY.md 0.5)")

    def _sample(self, who, model, vae, n, x_text, labels, args, build, *, phoscLabels=None, underscore=None, bulk=False,
                attention=None, mix_rate=None, style_pairs=None, cfg_scale=3, guidance=None, **loop):
        """What every public sampler does around its loop, after its own argument handling: ``_prepare``, the ``_Sampler``
        (``build()``), the attention, interpolation and guidance arguments settled on the host - a refused call has launched
        nothing and drawn nothing from ``random``: the pairs are drawn last - then ``_denoise`` on the ``_Call`` (``loop``: its
        remaining fields) with the model in eval mode and in TRAIN mode afterwards, whatever happened (train.py:201,238), and
        ``_finish``.  ``bulk`` (``sampling3``): the caller has put the model in eval mode and it stays there, and ``args.latent``
        is not looked at.  With ``windows`` (``loop``'s, a ``LineWindows``) ``n`` counts lines: ``_line_setup`` refuses what lines do not
        compose with and spreads words, writers and PHOSC labels over the model batch n * K; the loop and the result are the line's."""
        nb = n
        if loop.get("windows") is not None:
            nb, x_text, labels, phoscLabels = self._line_setup(model, n, loop["windows"], x_text, labels, phoscLabels, attention, mix_rate,
                                                               style_pairs)
        device, tf, phosc = self._prepare(who, model, nb, x_text, args, phoscLabels, underscore, check_latent=not bulk)
        sampler = build()
        att = self._attention_setup(model, sampler, attention)
        checked = self._mix_check(model, nb, mix_rate, style_pairs)
        wf = self._guidance_setup(model, guidance, cfg_scale, checked)
        mix = None if checked is None else self._mix_table(checked, n, cfg_scale, sampler)
        call = _Call(sampler, self.noise_steps, self.tabulate_film, self.forwards_per_step, attention=att, mix=mix, writer_free=wf, **loop)
        model.eval()
        try:
            x = self._denoise(model, n, tf, labels, phosc, device, call)
        finally:
            if not bulk:
                model.train()  # train.py:238 (unconditional)
        return x if vae is None else self._finish(x, vae, args)

    @torch.no_grad()
    def sampling(self, model, vae, n, x_text, labels, args, mix_rate=None, cfg_scale=3, phoscLabels=None,
                 noise=None, x_T=None, seed=None, sample_offset=0, record=None, use_graph=True, underscore=None, *,
                 style_pairs=None, record_pred=None, known=None, known_mask=None, start=None, known_noise="auto", attention=None,
                 guidance=None, windows=None, resample=1, jump=10):
        """``train.py:200`` signature; extra keyword-only style arguments (phoscLabels, noise, x_T, seed,
        sample_offset) serve the PHOSC variant (``trainGWModifyCondition.py:249``), the parity tests and
        rank-sharded sampling.  ``vae=None`` returns the denoised latents.  ``underscore``: word ids from the 53-class
        ``'_'`` alphabet of the ModifyCondition scripts (default: when the model's table has the 54 rows that alphabet
        needs).  Like the reference (``train.py:201,238``) the model is put in eval mode for the loop and in TRAIN mode
        afterwards, whatever mode it came in.

        ``mix_rate`` (writer-style interpolation, ``_mix_setup``): ignored unless the model was built with
        ``args.interpolation`` - then every forward blends a freshly drawn pair of writers and, with ``cfg_scale > 0``, a step
        is two forwards and ``torch.lerp(second, first, cfg_scale)`` (``last_stats["forwards_per_step"] == 2``) - or
        ``style_pairs`` is given: the writers to blend, the same at every step (one forward per step).  ``labels`` is unused
        in both modes.  ``record_pred`` receives every step's predictions (eager launches).

        ``known`` / ``known_mask`` / ``start`` / ``known_noise`` (``_known_setup``): keep the masked region of the latents
        ``known`` through the whole trajectory (every step ends by blending it back in at the level the step reached, the last
        one noise-free, so the kept region of the result IS ``known``) and / or begin at the level ``start`` from ``known``
        noised to it instead of from noise at T - 1; ``noise`` then holds one tensor per visited step with t > 1.
        ``last_stats`` reports ``known``, ``start`` (the level noised to) and ``known_noise`` (the resolved mode).

        ``attention=True | (t_hi, t_lo)``: the per-character cross-attention maps of the call (the reference's --attentionMaps 1
        outputs, unet.py:1645-1832), averaged over the model-calling steps (those with t_lo <= t <= t_hi), are left in
        ``last_attention = {"input", "middle", "output"}``, fp32 [n, h, w, L] at latent resolution; ``last_stats`` gains
        ``attention_steps``.  Base model only.

        ``guidance="writer_free"`` (``_guidance_setup``; DESIGN.md "Writer-free guidance"): classifier-free guidance on the writer.
        With ``cfg_scale > 0`` every model-calling step runs the conditional forward, the forward without the writer term and the
        guided update ``torch.lerp(free, cond, cfg_scale)``; ``last_stats`` reports ``forwards_per_step == 2`` and
        ``guidance``, ``record_pred`` receives (cond, free, guided) and ``attention`` reads the conditional forward.  With
        ``cfg_scale == 0`` the call is the plain one.  Without the argument ``cfg_scale`` stays inert outside interpolation mode,
        as in the reference, whose two forwards are identical (train.py:224-228).  Not together with the interpolation modes.

        ``windows=line_windows(n, K, ...)`` (DESIGN.md "Lines"): whole lines in one call, as K overlapping windows of the model's
        width per line (MultiDiffusion).  ``n`` counts lines; ``x_text`` is n lists of K words (or one list for every line),
        ``labels`` one writer per line, ``phoscLabels`` [n, K, L] or [n * K, L]; ``x_T``, ``noise``, ``known``, ``known_mask``,
        ``start`` and ``record`` are line-shaped, [n, C, h, width], and so is the result.  Every model-calling step gathers the
        windows, runs the forward(s) at batch n * K and averages the predictions into one line prediction, on which the ordinary
        update, guidance and known-region blend run; line s depends on (seed, sample_offset + s) only.  ``last_stats`` gains
        ``windows``, ``line_width`` and ``model_batch``; ``record_pred`` receives (window predictions, line prediction), or (window
        cond, window free, line cond, line free, guided line).  ``attention=`` and the interpolation modes are refused
        (NotImplementedError) before anything is launched or drawn.

        ``resample=r, jump=j`` (DESIGN.md "Resampling jumps"; ``resample_walk``): RePaint's resampling on top of ``known_mask`` -
        after every ``jump`` visited steps the state is diffused forward again by those steps (``wd_forward_jump``, kept and free
        cells alike) and they are denoised once more, ``resample - 1`` times per stretch, so that the free region is re-drawn in the
        context of what the kept one has become.  ``resample=1`` (the default) is the call without the argument, launch for
        launch.  In a resampled call every draw is keyed by the walk entry, so a revisited level draws afresh; ``noise`` holds
        one tensor per walk entry (a down entry's step z, an up entry's jump z), ``record`` receives x before every entry and
        ``last_stats`` reports ``resample``, ``jump``, ``walk`` (entries) and ``model_calls`` (down entries, times the forwards
        of a guided step).  Needs a ``known_mask`` (ValueError); ``attention=`` and the interpolation modes are refused
        (NotImplementedError) before anything is launched or drawn."""
        kn = self._known_setup(n, known, known_mask, start, known_noise, x_T, draws_noise=True, width=self._line_width(windows, n))
        first = self.noise_steps - 1 if kn is None or kn.start is None else kn.start
        walk = self._resample_setup(model, range(first, 0, -1), resample, jump, kn, attention, mix_rate, style_pairs, noise)
        return self._sample("sampling", model, vae, n, x_text, labels, args,
                            lambda: self._ddpm(start=None if kn is None else kn.start, walk=walk),
                            phoscLabels=phoscLabels, underscore=underscore, attention=attention, mix_rate=mix_rate,
                            style_pairs=style_pairs, cfg_scale=cfg_scale, guidance=guidance, known=kn, x_T=x_T, noise=noise, seed=seed,
                            sample_offset=sample_offset, record=record, record_pred=record_pred, use_graph=use_graph, windows=windows)

    @torch.no_grad()
    def sampling_ddim(self, model, vae, n, x_text, labels, args, steps=50, eta=0.0, *, timesteps=None, mix_rate=None, cfg_scale=3,
                      phoscLabels=None, noise=None, x_T=None, seed=None, sample_offset=0, record=None, record_pred=None,
                      use_graph=True, underscore=None, style_pairs=None, known=None, known_mask=None, start=None,
                      known_noise="auto", attention=None, guidance=None, windows=None, resample=1, jump=10):
        """DDIM sampling (Song et al. 2020) with the same trained model: ``steps`` UNet evaluations over the subsequence
        ``ddim_timesteps(steps)`` of the schedule (or the explicit ``timesteps``) instead of ``noise_steps - 1``.  ``eta = 0`` is
        deterministic given x_T (``seed`` then only draws x_T); ``eta = 1`` has the DDPM posterior variance; in between the
        noise of a sample at timestep t is the draw ``sampling`` makes there (same Philox key), whatever the batch or sharding.
        The last step lands on index 0 of the schedule (alpha_hat[0], not 1), the index the reference never steps from.
        Everything else follows ``sampling``: eval mode for the loop and TRAIN mode afterwards, ``vae=None`` returns latents,
        ``phoscLabels`` for the PHOSC model, ``mix_rate`` / ``style_pairs`` as there (pairs are drawn for the visited steps
        only).  ``noise``: one tensor per visited step, read only where sigma != 0; ``record`` / ``record_pred`` as in
        ``sampling``.  ``last_stats`` carries ``sampler="ddim"``, ``steps``, ``eta`` and ``timesteps``.
        ``known`` / ``known_mask`` / ``start`` / ``known_noise`` as in ``sampling``; with ``start`` the call visits the entries of
        its usual schedule that are <= start (``steps`` and ``timesteps`` of ``last_stats`` are the retained ones, FiLM rows,
        pairs and ``noise`` are indexed by them) and the first of them is the level noised to.  With ``eta = 0`` the default
        ``known_noise`` is one fixed eps per sample, so the call stays deterministic given ``seed``.  ``attention``,
        ``guidance``, ``windows`` and ``resample`` / ``jump`` as in ``sampling``; the walk is built over the retained schedule
        and ``jump`` counts visited steps."""
        tau = self.ddim_timesteps(steps, timesteps)
        kn = self._known_setup(n, known, known_mask, start, known_noise, x_T, draws_noise=float(eta) > 0, tau=tau,
                               width=self._line_width(windows, n))
        if kn is not None:
            tau = kn.tau
        walk = self._resample_setup(model, tau, resample, jump, kn, attention, mix_rate, style_pairs, noise)
        if walk is None and noise is not None and len(noise) != len(tau):
            raise ValueError(f"noise must hold one tensor per visited step ({len(tau)})")
        return self._sample("sampling_ddim", model, vae, n, x_text, labels, args, lambda: self._ddim(tau, eta, walk),
                            phoscLabels=phoscLabels, underscore=underscore, attention=attention, mix_rate=mix_rate,
                            style_pairs=style_pairs, cfg_scale=cfg_scale, guidance=guidance, known=kn, x_T=x_T, noise=noise, seed=seed,
                            sample_offset=sample_offset, record=record, record_pred=record_pred, use_graph=use_graph, windows=windows)

    @torch.no_grad()
    def sampling_dpmpp(self, model, vae, n, x_text, labels, args, steps=20, order=2, *, spacing="logsnr", timesteps=None,
                       mix_rate=None, cfg_scale=3, phoscLabels=None, x_T=None, seed=None, sample_offset=0, record=None,
                       record_pred=None, use_graph=True, underscore=None, style_pairs=None, known=None, known_mask=None,
                       start=None, known_noise="auto", attention=None, guidance=None, windows=None, resample=1, jump=10):
        """DPM-Solver++(2M) sampling (Lu et al. 2022) with the same trained model: ``steps`` UNet evaluations over
        ``dpmpp_timesteps(steps, spacing)`` (or the explicit ``timesteps``), each step extrapolating the data prediction from
        the previous step's (``order = 2``; ``order = 1`` is DDIM with eta = 0 on the same timesteps).  The first and the last
        step are always first order.  ``spacing="logsnr"`` spreads the timesteps evenly in log-SNR, where the solver's error
        estimate holds on this schedule; ``"time"`` is DDIM's spacing.  Deterministic given x_T: ``seed`` only draws x_T (the
        Philox key of ``sampling``), and there is no ``noise``.  The last step lands on index 0 of the schedule, as in
        ``sampling_ddim``, and everything else follows it too: eval mode for the loop and TRAIN mode afterwards, ``vae=None``
        returns latents, ``phoscLabels``, ``mix_rate`` / ``style_pairs``, ``record`` / ``record_pred``.  ``last_stats`` carries
        ``sampler="dpmpp"``, ``steps``, ``order``, ``spacing`` (None with explicit ``timesteps``) and ``timesteps``.
        ``known`` / ``known_mask`` / ``start`` / ``known_noise`` as in ``sampling_ddim`` (the default noise is the fixed eps: no
        step draws); the first retained step is first order, like the first step of any call.  ``attention``, ``guidance``,
        ``windows`` and ``resample`` / ``jump`` as in ``sampling_ddim``; the step after a jump is first order as well (only the
        jumps draw, and a blend with ``known_noise="fresh"``)."""
        tau = self.dpmpp_timesteps(steps, spacing, timesteps)
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, not {order!r}")
        kn = self._known_setup(n, known, known_mask, start, known_noise, x_T, draws_noise=False, tau=tau, width=self._line_width(windows, n))
        if kn is not None:
            tau = kn.tau
        walk = self._resample_setup(model, tau, resample, jump, kn, attention, mix_rate, style_pairs)
        return self._sample("sampling_dpmpp", model, vae, n, x_text, labels, args,
                            lambda: self._dpmpp(tau, order, None if timesteps is not None else spacing, walk), phoscLabels=phoscLabels,
                            underscore=underscore, attention=attention, mix_rate=mix_rate, style_pairs=style_pairs, cfg_scale=cfg_scale,
                            guidance=guidance, known=kn, x_T=x_T, seed=seed, sample_offset=sample_offset, record=record,
                            record_pred=record_pred, use_graph=use_graph, windows=windows)

    sample = sampling  # sampling.py:119 / full_sampling.py:167 call .sample(...)

    @staticmethod
    def sampling3_calls_model(i, noise_steps, epoch=0):
        """The step-skipping predicate of ``regenerateFromtrain2.py:536`` (literal; its last clause ``epoch>50==0`` is a
        chained comparison that is always False): the UNet runs at ``i == T-1`` and whenever ``i % 5 == 0``."""
        return bool(i % 100 == 0 or i % 5 == 0 or i == noise_steps or i == noise_steps - 1 or (epoch > 3 and i % 25 == 0) or
                    (epoch > 5 and i % 15 == 0) or (epoch > 10 and i % 10 == 0) or (epoch > 50 == 0))

    @torch.no_grad()
    def sampling3(self, epoch, x_t, words, phoscLabels, model, model1, vae, emaOld, noiseInput, n, x_text, labels, args,
                  mix_rate=None, cfg_scale=3, seed=None, sample_offset=0, use_graph=True, x_T=None, noise=None, record=None, *,
                  style_pairs=None, attention=None, windows=None, resample=1, jump=10):
        """Bulk-regeneration sampler of ``regenerateFromtrain2.py:465-648`` (same argument order): the predicted noise is
        refreshed only on the steps of ``sampling3_calls_model`` (1 in 5) and reused in between, and unless
        ``args.fullSampling`` the update is deterministic (no ``sqrt(beta) * noise`` term, ``:618``).  ``noiseInput == 0``
        starts from ``x_t`` instead of fresh noise (``:518-519``).  Returns ``(0, [images], images)`` like the reference when
        a ``vae`` is given, the denoised latents otherwise.  The per-step ``flagGen.txt`` poll (``:523-530``) is not
        reproduced.  ``x_T`` / ``noise`` / ``record`` (as in ``sampling``): the start latent, the per-step draws and a list that
        receives every step's x - how the tests replay the trajectories recorded from the reference's own loop
        (``tests/golden/ddpm_traj_sampling3.npz``, ``oracle/make_golden_sampling3.py``).  ``mix_rate`` / ``style_pairs`` as in
        ``sampling``; this loop calls the model once per model-calling step, so with ``args.interpolation`` one pair is drawn for
        each of those steps and none for the others.  (The reference's own loop accepts ``mix_rate`` and does not hand it to
        the model, ``:587,591``: there the argument has no effect; here it selects the blend, as it does in ``sampling``.)
        ``attention`` as in ``sampling``: the steps that reuse the previous prediction run no forward and add nothing, and
        ``attention_steps`` counts the model-calling steps of the window only.  ``windows`` (line sampling, see ``sampling``) is
        refused: this loop regenerates single words; so is ``resample > 1``: it keeps no region."""
        if windows is not None:
            raise NotImplementedError("sampling3 with windows=: the step-skipping bulk sampler regenerates single words")
        if resample != 1:
            raise NotImplementedError("sampling3 with resample > 1: the step-skipping bulk sampler keeps no region to harmonise")
        if emaOld == 1:
            model = model1
        model.eval()  # and it stays in eval mode: ``#model.train()`` is commented out at regenerateFromtrain2.py:622
        if isinstance(x_text, str) or len(x_text) <= 1:
            word_list = [x_text if isinstance(x_text, str) else x_text[0]] * n
        else:
            word_list = list(words)
        full = bool(getattr(args, "fullSampling", False))
        calls_model = None if full else (lambda i: self.sampling3_calls_model(i, self.noise_steps, epoch))
        # (cfg_scale 0: one forward per step, no guidance here)
        out = self._sample("sampling3", model, vae, n, word_list, labels, args, lambda: self._ddpm(calls_model, deterministic=not full),
                           phoscLabels=phoscLabels, bulk=True, attention=attention, mix_rate=mix_rate, style_pairs=style_pairs,
                           cfg_scale=0, x_T=x_t if noiseInput == 0 else x_T, noise=noise, seed=seed, sample_offset=sample_offset,
                           record=record, use_graph=use_graph)
        return out if vae is None else (0, [out], out)

    def sampling_modify_condition(self, model, vae, latents, x_text, words, n, labels, args, **kw):
        """Argument order of ``trainModifyCondition.py:545``; that variant feeds writer id 1 for every sample
        (``s_id = torch.ones(...)``, ``:565``) whatever ``labels`` holds, reads its word ids from the ``'_'`` alphabet
        (``:166-180``) and never runs the second forward (``if 0:`` at ``:590``).  Its schedule is the caller's:
        ``Diffusion()`` of that script defaults to ``noise_steps = 600`` (``:516``) - pass it to the constructor."""
        s_id = torch.ones(n, dtype=torch.int64)
        kw.setdefault("underscore", True)
        return self.sampling(model, vae, n, x_text, s_id, args, cfg_scale=0, **kw)

    def sampling_phosc(self, model, vae, n, x_text, phoscLabels, labels, args, mix_rate=None, cfg_scale=3, **kw):
        """Argument order of ``trainGWModifyCondition.py:249``."""
        return self.sampling(model, vae, n, x_text, labels, args, mix_rate=mix_rate, cfg_scale=cfg_scale,
                             phoscLabels=phoscLabels, **kw)
