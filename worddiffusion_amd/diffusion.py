"""``Diffusion`` / ``EMA`` / ``label_padding`` with the reference's call surface (``train.py:42-52,140-251``).

Every sampler runs through the one reverse loop of ``Diffusion._denoise``, entirely on the device: the step-invariant
conditioning (word embedding, cross-attention K/V) is computed once, one denoising step (UNet forward(s) + the sampler's
update with on-device Philox noise + its timestep advance) is captured into a hipGraph and replayed once per visited step;
there is no per-step host->device traffic.  What a sampler is to that loop is a ``_Sampler``, fixed on the host before
anything is launched: ``_ddpm`` (``sampling``, ``train.py:221-236``: ``x <- 1/sqrt(a) (x - (1-a)/sqrt(1-ah) eps) + sqrt(b) z``
at t = T-1 .. 1; ``sampling3`` skips the model on most of those steps), ``_ddim`` (``sampling_ddim``: a subsequence) and
``_dpmpp`` (``sampling_dpmpp``: a subsequence spaced in log-SNR, second-order multistep).

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
    # update(lib, P, guide, zbuf, seed, sample_offset, device, known=None) -> end_step(stream), the launches that end a step;
    # known = (x0, mask, eps or None, sqrt_ah, sqrt_1m_ah) on the device: ``wd_known_blend`` between the update and the advance
    update: Callable
    stats: dict  # what ``last_stats`` reports of the sampler itself


class _Known(NamedTuple):
    """What a known-region / partial-noise call is to the reverse loop (built by ``Diffusion._known_setup``, no GPU)."""
    x0: torch.Tensor  # the known latents, fp32 [n, C*h*w] on the host
    mask: Optional[torch.Tensor]  # fp32 [n, C*h*w] on the host, 1 = keep; None: ``start`` alone, nothing is blended
    start: Optional[int]  # the level the loop starts from (``x0`` noised to it); None: from x_T / noise as ever
    tau: Optional[list]  # the retained visited timesteps of a DDIM / DPM++ call (None: DDPM)
    mode: str  # "fresh": the blend draws its noise per step; "fixed": one eps per sample
    eps: Optional[torch.Tensor]  # the caller's fixed eps, fp32 [n, C*h*w]; None: stream WD_STREAM_KNOWN of the call's seed


def latent_mask_from_pixels(mask_px):
    """A keep-mask over pixels [..., H, W] (H, W multiples of 8; nonzero / True = keep) -> the fp32 keep-mask [..., H/8, W/8] over
    the latent cells of the 8x VAE: an 8x8 min-pool, so a latent cell is kept only if every pixel it covers is."""
    m = torch.as_tensor(mask_px)
    if m.dim() < 2 or m.shape[-2] % 8 or m.shape[-1] % 8 or not m.shape[-2] or not m.shape[-1]:
        raise ValueError(f"a pixel mask must be [..., H, W] with H and W multiples of 8, got {tuple(m.shape)}")
    m = (m != 0).to(torch.float32)
    H, W = m.shape[-2:]
    return m.reshape(*m.shape[:-2], H // 8, 8, W // 8, 8).amin(dim=(-3, -1)).contiguous()


def _blend_known(lib, P, known, p_args, seed, sample_offset, stream):
    """The ``wd_known_blend`` launch of a step's tail; p_args = (t_dev, k_dev, tau, S) as the kernel takes them."""
    x0, mask, eps, sa, sb = known
    N.check(lib.wd_known_blend(P.x_in.data_ptr(), x0.data_ptr(), mask.data_ptr(), P.x_in.shape[0], P.x_in[0].numel(), sa.data_ptr(),
                               sb.data_ptr(), *p_args, _dptr(eps), seed, sample_offset, stream), "wd_known_blend")


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

    def _ddim_tables(self, tau, eta, device):
        """The five per-step coefficients of ``wd_ddim_step`` (fp32 [S] each), with a = alpha_hat[tau[k]], p = alpha_hat of the
        predecessor and sigma = eta sqrt((1-p)/(1-a)) sqrt(1 - a/p):  c1 = sqrt(1-a), c2 = 1/sqrt(a), c3 = sqrt(p),
        c4 = sqrt(max(1 - p - sigma^2, 0)), c5 = sigma.  Evaluated in float64 from the fp32 betas (alpha and its cumprod
        recomputed in float64: the fp32 ``1 - alpha_hat[0]`` has lost half its digits) and rounded to fp32 once."""
        ah = torch.cumprod(1.0 - self.beta.detach().cpu().double(), dim=0)
        tau = [int(t) for t in tau]
        a = ah[tau]
        p = ah[tau[1:] + [0]]
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

    def _dpmpp_tables(self, tau, order, device):
        """The five per-step coefficients of ``wd_dpmpp_step`` (fp32 [S] each), with a = alpha_hat[tau[k]], p = alpha_hat of the
        predecessor (alpha_hat[0] after the last entry, as in ``_ddim_tables``) and h_k = lambda(p) - lambda(a):
        c1 = sqrt(1-a), c2 = 1/sqrt(a), c3 = sqrt((1-p)/(1-a)), c4 = -sqrt(p) expm1(-h_k), c5 = h_k / (2 h_{k-1}).  c5 = 0 makes a
        step first order: k = 0, every k at ``order`` 1, and always the last step (no extrapolation into index 0).  Evaluated
        in float64 from the fp32 betas and rounded to fp32 once."""
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, not {order!r}")
        ah = torch.cumprod(1.0 - self.beta.detach().cpu().double(), dim=0)
        tau = [int(t) for t in tau]
        a = ah[tau]
        p = ah[tau[1:] + [0]]
        h = 0.5 * torch.log(p / (1 - p)) - 0.5 * torch.log(a / (1 - a))
        c5 = torch.zeros_like(h)
        if order == 2 and len(tau) > 2:
            c5[1:-1] = h[1:-1] / (2 * h[:-2])
        tabs = (torch.sqrt(1 - a), 1 / torch.sqrt(a), torch.sqrt((1 - p) / (1 - a)), -torch.sqrt(p) * torch.expm1(-h), c5)
        return tuple(c.float().to(device).contiguous() for c in tabs)

    # --------------------------------------------------------------------------------------------------
    def _ddpm(self, calls_model=None, deterministic=False, start=None):
        """The DDPM family: t = T-1 .. 1 (train.py:221; ``start`` .. 1 for a call that begins at that level), the model called
        where ``calls_model(t)`` holds (None: everywhere; a step that does not call it reuses the previous predicted noise) and
        one entry of ``noise`` per step while t > 1, counted on skipped steps too.  A step ends with ``wd_ddpm_step`` (the
        guided ``wd_ddpm_step_cfg`` after two forwards), ``wd_known_blend`` at the level t - 1 when a region is kept, and
        ``wd_advance_timestep``."""
        first = self.noise_steps - 1 if start is None else int(start)
        steps = [(i, calls_model is None or bool(calls_model(i)), first - i if i > 1 else None) for i in reversed(range(1, first + 1))]

        def update(lib, P, guide, zbuf, seed, sample_offset, device, known=None):
            ca, cb, cs = self._step_tables(device)
            if deterministic:  # regenerateFromtrain2.py:618 drops the sqrt(beta) * noise term
                cs = torch.zeros_like(cs)
            n, npix = P.x_in.shape[0], P.x_in[0].numel()

            def end_step(stream):
                if guide is not None:
                    N.check(lib.wd_ddpm_step_cfg(P.x_in.data_ptr(), P.out.data_ptr(), P.out1.data_ptr(), guide[0],
                                                 _dptr(guide[1]), n, npix, ca.data_ptr(), cb.data_ptr(), cs.data_ptr(),
                                                 P.t_dev.data_ptr(), _dptr(zbuf), seed, sample_offset, stream), "wd_ddpm_step_cfg")
                else:
                    N.check(lib.wd_ddpm_step(P.x_in.data_ptr(), P.out.data_ptr(), n, npix, ca.data_ptr(), cb.data_ptr(),
                                             cs.data_ptr(), P.t_dev.data_ptr(), _dptr(zbuf), seed, sample_offset, stream),
                            "wd_ddpm_step")
                if known is not None:
                    _blend_known(lib, P, known, (P.t_dev.data_ptr(), None, None, 0), seed, sample_offset, stream)
                N.check(lib.wd_advance_timestep(P.t_dev.data_ptr(), -1, P.t_in.data_ptr(), n, stream),
                        "wd_advance_timestep")
            return end_step
        # (``steps`` is T - 1 even when steps skip the model: it counts the updates)
        return _Sampler(steps, first, None, update, dict(steps=first))

    def _ddim(self, tau, eta):
        """DDIM over the visited timesteps ``tau``: step k is timestep tau[k]; FiLM rows, pairs and ``noise`` are indexed by k,
        the model is called at every step and ``noise[k]`` is read only where c5[k] != 0.  A step ends with ``wd_ddim_step``,
        ``wd_known_blend`` at the level tau[k + 1] when a region is kept, and ``wd_next_timestep``."""
        tabs = self._ddim_tables(tau, eta, "cpu")
        steps = [(k, True, k if s != 0.0 else None) for k, s in enumerate(tabs[4].tolist())]  # (host tables: no device sync)

        def update(lib, P, guide, zbuf, seed, sample_offset, device, known=None):
            c = [t.to(device) for t in tabs]
            tau_dev = torch.tensor(tau, dtype=torch.int32, device=device)
            P.k_dev.zero_()
            n, npix = P.x_in.shape[0], P.x_in[0].numel()
            scale, eps_g = guide or (0.0, None)

            def end_step(stream):
                N.check(lib.wd_ddim_step(P.x_in.data_ptr(), P.out.data_ptr(), P.out1.data_ptr() if guide is not None else None,
                                         scale, _dptr(eps_g), n, npix, *(t.data_ptr() for t in c), P.k_dev.data_ptr(),
                                         P.t_dev.data_ptr(), _dptr(zbuf), seed, sample_offset, stream), "wd_ddim_step")
                if known is not None:  # at the level of tau[k + 1] (index 0 after the last entry), read from k_dev
                    _blend_known(lib, P, known, (P.t_dev.data_ptr(), P.k_dev.data_ptr(), tau_dev.data_ptr(), len(tau)), seed,
                                 sample_offset, stream)
                N.check(lib.wd_next_timestep(P.k_dev.data_ptr(), tau_dev.data_ptr(), len(tau), P.t_dev.data_ptr(),
                                             P.t_in.data_ptr(), n, stream), "wd_next_timestep")
            return end_step
        stats = dict(sampler="ddim", steps=len(tau), eta=float(eta), timesteps=list(tau))
        return _Sampler(steps, tau[0], list(tau), update, stats)

    def _dpmpp(self, tau, order, spacing=None):
        """DPM-Solver++(2M) over the visited timesteps ``tau``: step k is timestep tau[k]; FiLM rows and pairs are indexed by k,
        the model is called at every step and no step draws noise.  The previous data prediction lives in a buffer of the
        update's own, written by every step and read only where c5[k] != 0.  A step ends with ``wd_dpmpp_step``,
        ``wd_known_blend`` as in ``_ddim`` and ``wd_next_timestep``."""
        tabs = self._dpmpp_tables(tau, order, "cpu")
        steps = [(k, True, None) for k in range(len(tau))]

        def update(lib, P, guide, zbuf, seed, sample_offset, device, known=None):
            c = [t.to(device) for t in tabs]
            tau_dev = torch.tensor(tau, dtype=torch.int32, device=device)
            x0_prev = torch.empty_like(P.x_in)  # (the first step does not read it: c5[0] == 0)
            P.k_dev.zero_()
            n, npix = P.x_in.shape[0], P.x_in[0].numel()
            scale, eps_g = guide or (0.0, None)

            def end_step(stream):
                N.check(lib.wd_dpmpp_step(P.x_in.data_ptr(), P.out.data_ptr(), P.out1.data_ptr() if guide is not None else None,
                                          scale, _dptr(eps_g), x0_prev.data_ptr(), n, npix, *(t.data_ptr() for t in c),
                                          P.k_dev.data_ptr(), stream), "wd_dpmpp_step")
                if known is not None:  # (x0_prev keeps the model's own data prediction: the blend changes x alone)
                    _blend_known(lib, P, known, (P.t_dev.data_ptr(), P.k_dev.data_ptr(), tau_dev.data_ptr(), len(tau)), seed,
                                 sample_offset, stream)
                N.check(lib.wd_next_timestep(P.k_dev.data_ptr(), tau_dev.data_ptr(), len(tau), P.t_dev.data_ptr(),
                                             P.t_in.data_ptr(), n, stream), "wd_next_timestep")
            return end_step
        stats = dict(sampler="dpmpp", steps=len(tau), order=int(order), spacing=spacing, timesteps=list(tau))
        return _Sampler(steps, tau[0], list(tau), update, stats)

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

    def _known_setup(self, n, known, known_mask=None, start=None, known_noise="auto", x_T=None, *, draws_noise, tau=None):
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
                     (``draws_noise``: DDPM, DDIM with eta > 0), "fixed" otherwise - a deterministic sampler stays one."""
        T = self.noise_steps
        if known is None:
            if known_mask is not None or start is not None or not (isinstance(known_noise, str) and known_noise == "auto"):
                raise ValueError("known_mask, start and known_noise need the known latents (known=)")
            return None
        if known_mask is None and start is None:
            raise ValueError("known needs a known_mask (the region to keep), a start level, or both")
        h, w = self.img_size[0] // 8, self.img_size[1] // 8
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

    def _denoise(self, model, n, text_features, labels, phosc, device, sampler, x_T=None, noise=None, seed=None,
                 sample_offset=0, record=None, use_graph=True, mix=None, record_pred=None, known=None, attention=None,
                 writer_free=None):
        """The one reverse loop.  Per visited step of ``sampler`` (``_ddpm`` / ``_ddim``): this step's ``noise`` entry into
        the noise buffer if it has one, ``film_prepare`` and the forward(s) when the step calls the model, the sampler's update.
        mix = (pairs int32 [nf, rows, n, 2], rates fp32 [n], guidance scale): writer-style interpolation with ``nf`` forwards per
        step, forward f of a step reading pairs[f, its film_prepare argument]; nf = 2 ends the step with the guided update.
        record_pred: a list that receives, per model-calling step, the predictions of its forwards (and, for nf = 2, the guided
        one) - eager launches only, like ``record``.
        known: a ``_Known``.  Its fixed eps (the caller's, or stream WD_STREAM_KNOWN of ``seed`` at the global rows) noises the
        known latents to ``known.start``, where the loop then begins, and with a mask every step's tail blends the kept region
        back in at the level the step reached (``wd_known_blend``, inside the captured graph).
        attention: what ``_attention_setup`` returned.  The plan then holds three map accumulators, zeroed here, and every
        model-calling step adds its weight times its maps (``wd_xattn_maps`` inside the captured step, the first forward of a
        step only); the weighted mean lands in ``last_attention``.
        writer_free: None, or the guidance scale of a writer-free guided call (``_guidance_setup``): a step is the conditional
        forward, the forward without the writer term (``engine.plan`` guide = 2) and the guided update
        ``torch.lerp(free, cond, scale)`` - the two-forward step of the interpolation mode with other FiLM rows."""
        lib = N.lib()
        eng = model.engine
        nf = 0 if mix is None else int(mix[0].shape[0])
        two = nf == 2 or writer_free is not None  # forwards per step with predictions of their own, lerped by the update
        if nf:
            eng.check_pairs(mix[0])  # first: nothing is launched for an id that does not fit the table
            labels = None  # unused in this mode (unet.py:1558-1573)
        eng.refresh_weights()
        eng.check_ids(text_features, labels, phosc, need_y=not nf)  # host tensors here: no device sync
        h, w = self.img_size[0] // 8, self.img_size[1] // 8
        ctx_len = text_features.shape[1]
        phosc_len = 0 if phosc is None else phosc.shape[1]
        # (the interpolation plan always tabulates: the pairs of every step live in the table's index, not in a per-step upload)
        film_steps = self.noise_steps if (self.tabulate_film or nf or writer_free is not None) else 0
        P = eng.plan(n, h, w, ctx_len, phosc_len, film_steps=film_steps, mix=nf,
                     film_timesteps=tuple(sampler.tau) if (film_steps and sampler.tau is not None) else None,
                     **(dict(attn_maps=True, attn_rows=attention[0].numel(), attn_by_step=sampler.tau is not None)
                        if attention is not None else {}),
                     **(dict(guide=2) if writer_free is not None else {}))
        fps = nf or (2 if writer_free is not None else self.forwards_per_step)
        ncalls = sum(fwd for _, fwd, _ in sampler.steps)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
        npix = P.x_in[0].numel()
        if known is not None and known.x0.shape[1] != npix:
            raise ValueError(f"known holds {known.x0.shape[1]} values per sample, the model's latent {npix} {tuple(P.x_in.shape[1:])}")

        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            st = side.cuda_stream
            blend = None
            if known is not None:
                kx0 = known.x0.to(device)
                sa, sb = self._noise_tables(device)
                keps = None
                if known.start is not None or (known.mask is not None and known.mode == "fixed"):
                    if known.eps is not None:
                        keps = known.eps.to(device)
                    else:
                        keps = torch.empty_like(kx0)
                        N.check(lib.wd_randn(keps.data_ptr(), n, npix, seed, sample_offset, N.STREAM_KNOWN, st), "wd_randn")
                if known.mask is not None:
                    blend = (kx0, known.mask.to(device), keps if known.mode == "fixed" else None, sa, sb)
            if known is not None and known.start is not None:
                level = torch.full((n,), known.start, dtype=torch.int64, device=device)
                N.check(lib.wd_noise_images(kx0.data_ptr(), keps.data_ptr(), level.data_ptr(), sa.data_ptr(), sb.data_ptr(), n, npix,
                                            P.x_in.data_ptr(), st), "wd_noise_images")
            elif x_T is not None:
                P.x_in.copy_(x_T.to(device))
            else:
                N.check(lib.wd_randn(P.x_in.data_ptr(), n, P.x_in[0].numel(), seed, sample_offset, 0, st), "wd_randn")
            eng.load_inputs(P, None, None, text_features.to(device), labels.to(device) if labels is not None else None,
                            phosc.to(device) if phosc is not None else None, check=False)
            if nf:
                eng.load_mix(P, mix[0].to(device), mix[1].to(device), check=False)
            if attention is not None:
                P.map_w.copy_(attention[0])
                for acc in P.maps:
                    acc.zero_()
            eps_g = torch.empty_like(P.out) if (two and record_pred is not None) else None
            P.t_dev.fill_(sampler.t_first)
            P.t_in.fill_(sampler.t_first)
            zbuf = torch.zeros_like(P.x_in) if noise is not None else None
            scale = None if not two else float(mix[2]) if nf else float(writer_free)
            end_step = sampler.update(lib, P, (scale, eps_g) if two else None, zbuf, seed, sample_offset, device, known=blend)
            P.run_cond(st)
            P.run_film(st)  # time MLP of every timestep; the FiLM rows follow per chunk of timesteps (P.film_prepare)
            # before the capture: the captured step only reads the table (its rows are indexed by t, or by the DDIM step index)
            if sampler.steps:
                P.film_prepare(sampler.steps[0][0], st)

            def one_step(stream, forward=True):
                if forward:
                    for _ in range(1 if two or nf else fps):
                        P.run_step(stream)
                    if two:  # train.py:223-228 with two different forwards: lerp(second, first, cfg_scale) feeds the update
                        P.run_step1(stream)
                end_step(stream)

            def capture(forward):
                N.check(lib.wd_graph_begin(st), "wd_graph_begin")
                try:
                    one_step(st, forward)
                finally:
                    g = C.c_void_p()
                    rc = lib.wd_graph_end(st, C.byref(g))
                N.check(rc, "wd_graph_end")
                return g

            gexec = gskip = None
            if use_graph and record is None and record_pred is None:
                gexec = capture(True)
                if ncalls < len(sampler.steps):
                    gskip = capture(False)  # steps that reuse the previous predicted noise: update only
            for row, fwd, z in sampler.steps:
                if record is not None:
                    record.append(P.x_in.clone())
                if zbuf is not None and z is not None:
                    zbuf.copy_(noise[z].to(device))
                if fwd:
                    P.film_prepare(row, st)  # FiLM rows of this step (computed per chunk of rows, see engine.plan)
                if gexec is not None:
                    N.check(lib.wd_graph_launch(gexec if fwd else gskip, st), "wd_graph_launch")
                else:
                    one_step(st, fwd)
                if record_pred is not None and fwd:
                    record_pred.append((P.out.clone(),) if not two else (P.out.clone(), P.out1.clone(), eps_g.clone()))
            x = P.x_in.clone()
            self.last_attention = None
            if attention is not None:
                self.last_attention = {k: acc.clone().reshape(n, mh, mw, -1)
                                       for k, acc, (mh, mw) in zip(("input", "middle", "output"), P.maps, P.map_hw)}
        torch.cuda.current_stream(device).wait_stream(side)
        if gexec is not None:
            side.synchronize()
            lib.wd_graph_destroy(gexec)
            if gskip is not None:
                lib.wd_graph_destroy(gskip)
        self.last_stats = dict(sampler.stats, forwards_per_step=fps, graph=gexec is not None, seed=seed,
                               sample_offset=sample_offset, model_calls=ncalls * (2 if two else nf or 1), known=known is not None,
                               start=None if known is None else known.start, known_noise=None if known is None else known.mode)
        if attention is not None:
            self.last_stats["attention_steps"] = attention[1]
        if writer_free is not None:
            self.last_stats["guidance"] = "writer_free"
        return x

    def _guidance_setup(self, model, guidance, cfg_scale, mix):
        """The ``guidance`` argument of a sampler call, settled on the host: the ``writer_free`` argument of ``_denoise`` - None,
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
        """The ``mix`` argument of ``_denoise`` for a sampler call, or None where the call does not interpolate.

        Fixed-pair mode (``style_pairs`` given: one ``(s1, s2)`` or an int tensor [n, 2]; ``mix_rate`` a float or fp32 [n]): the
        same pair at every step, so the two guidance forwards of train.py:223-228 are identical and one runs.
        Reference mode (``model.interpolation`` and a ``mix_rate``): every forward of the reference's loop draws a pair of its own
        (unet.py:1561-1564) - they are drawn here, all of them, in loop order, before anything is launched; with
        ``cfg_scale > 0`` a step runs both forwards and the guided update.
        Otherwise ``mix_rate`` is ignored, as the reference's forward ignores it (unet.py:1558), and ``random`` is not touched.
        ``sampler`` (default ``_ddpm()``) says which steps those are: pairs are drawn for its model-calling steps only, in loop
        order, and the table is indexed as its FiLM rows are - by t, [nf, T, n, 2], or by the step index of its ``tau``,
        [nf, S, n, 2]."""
        sampler = sampler or self._ddpm()
        T = self.noise_steps if sampler.tau is None else len(sampler.tau)
        if style_pairs is not None:
            if mix_rate is None:
                raise ValueError("style_pairs needs a mix_rate (a float, or one per sample)")
            sp = torch.as_tensor(style_pairs)
            if sp.is_floating_point() or sp.shape not in ((2,), (n, 2)):
                raise ValueError(f"style_pairs must be (s1, s2) or an integer tensor [{n}, 2]")
            tab = sp.to(torch.int32).cpu().reshape(-1, 2).expand(n, 2).reshape(1, 1, n, 2).expand(1, T, n, 2).contiguous()
        elif mix_rate is not None and getattr(model, "interpolation", False):
            steps = [row for row, fwd, _ in sampler.steps if fwd]
            nf = 2 if cfg_scale > 0 else 1
            drawn = draw_style_pairs(nf * len(steps))
            tab = torch.zeros((nf, T, n, 2), dtype=torch.int32)
            for k, i in enumerate(steps):
                for f in range(nf):
                    tab[f, i] = torch.tensor(drawn[nf * k + f], dtype=torch.int32)
        else:
            return None
        m = torch.as_tensor(mix_rate, dtype=torch.float32).cpu().reshape(-1)
        if m.numel() not in (1, n):
            raise ValueError(f"mix_rate must be a float or hold one rate per sample ({n})")
        return tab, m.expand(n).contiguous(), float(cfg_scale)

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

    @torch.no_grad()
    def sampling(self, model, vae, n, x_text, labels, args, mix_rate=None, cfg_scale=3, phoscLabels=None,
                 noise=None, x_T=None, seed=None, sample_offset=0, record=None, use_graph=True, underscore=None, *,
                 style_pairs=None, record_pred=None, known=None, known_mask=None, start=None, known_noise="auto", attention=None,
                 guidance=None):
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
        as in the reference, whose two forwards are identical (train.py:224-228).  Not together with the interpolation modes."""
        kn = self._known_setup(n, known, known_mask, start, known_noise, x_T, draws_noise=True)
        device, tf, phosc = self._prepare("sampling", model, n, x_text, args, phoscLabels, underscore)
        sampler = self._ddpm(start=None if kn is None else kn.start)
        att = self._attention_setup(model, sampler, attention)
        mix = self._mix_setup(model, n, mix_rate, style_pairs, cfg_scale, sampler=sampler)
        wf = self._guidance_setup(model, guidance, cfg_scale, mix)
        model.eval()
        try:
            x = self._denoise(model, n, tf, labels, phosc, device, sampler, x_T=x_T, noise=noise, seed=seed,
                              sample_offset=sample_offset, record=record, use_graph=use_graph, mix=mix,
                              record_pred=record_pred, known=kn, attention=att, writer_free=wf)
        finally:
            model.train()  # train.py:238 (unconditional)
        return self._finish(x, vae, args)

    @torch.no_grad()
    def sampling_ddim(self, model, vae, n, x_text, labels, args, steps=50, eta=0.0, *, timesteps=None, mix_rate=None, cfg_scale=3,
                      phoscLabels=None, noise=None, x_T=None, seed=None, sample_offset=0, record=None, record_pred=None,
                      use_graph=True, underscore=None, style_pairs=None, known=None, known_mask=None, start=None,
                      known_noise="auto", attention=None, guidance=None):
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
        ``known_noise`` is one fixed eps per sample, so the call stays deterministic given ``seed``.  ``attention`` and
        ``guidance`` as in ``sampling``."""
        tau = self.ddim_timesteps(steps, timesteps)
        kn = self._known_setup(n, known, known_mask, start, known_noise, x_T, draws_noise=float(eta) > 0, tau=tau)
        if kn is not None:
            tau = kn.tau
        if noise is not None and len(noise) != len(tau):
            raise ValueError(f"noise must hold one tensor per visited step ({len(tau)})")
        device, tf, phosc = self._prepare("sampling_ddim", model, n, x_text, args, phoscLabels, underscore)
        sampler = self._ddim(tau, eta)
        att = self._attention_setup(model, sampler, attention)
        mix = self._mix_setup(model, n, mix_rate, style_pairs, cfg_scale, sampler=sampler)
        wf = self._guidance_setup(model, guidance, cfg_scale, mix)
        model.eval()
        try:
            x = self._denoise(model, n, tf, labels, phosc, device, sampler, x_T=x_T, noise=noise, seed=seed,
                              sample_offset=sample_offset, record=record, use_graph=use_graph, mix=mix, record_pred=record_pred,
                              known=kn, attention=att, writer_free=wf)
        finally:
            model.train()  # as ``sampling`` (train.py:238)
        return self._finish(x, vae, args)

    @torch.no_grad()
    def sampling_dpmpp(self, model, vae, n, x_text, labels, args, steps=20, order=2, *, spacing="logsnr", timesteps=None,
                       mix_rate=None, cfg_scale=3, phoscLabels=None, x_T=None, seed=None, sample_offset=0, record=None,
                       record_pred=None, use_graph=True, underscore=None, style_pairs=None, known=None, known_mask=None,
                       start=None, known_noise="auto", attention=None, guidance=None):
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
        step draws); the first retained step is first order, like the first step of any call.  ``attention`` and ``guidance`` as in
        ``sampling``."""
        tau = self.dpmpp_timesteps(steps, spacing, timesteps)
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, not {order!r}")
        kn = self._known_setup(n, known, known_mask, start, known_noise, x_T, draws_noise=False, tau=tau)
        if kn is not None:
            tau = kn.tau
        device, tf, phosc = self._prepare("sampling_dpmpp", model, n, x_text, args, phoscLabels, underscore)
        sampler = self._dpmpp(tau, order, None if timesteps is not None else spacing)
        att = self._attention_setup(model, sampler, attention)
        mix = self._mix_setup(model, n, mix_rate, style_pairs, cfg_scale, sampler=sampler)
        wf = self._guidance_setup(model, guidance, cfg_scale, mix)
        model.eval()
        try:
            x = self._denoise(model, n, tf, labels, phosc, device, sampler, x_T=x_T, seed=seed, sample_offset=sample_offset,
                              record=record, use_graph=use_graph, mix=mix, record_pred=record_pred, known=kn, attention=att,
                              writer_free=wf)
        finally:
            model.train()  # as ``sampling`` (train.py:238)
        return self._finish(x, vae, args)

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
                  style_pairs=None, attention=None):
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
        ``attention_steps`` counts the model-calling steps of the window only."""
        if emaOld == 1:
            model = model1
        model.eval()  # and it stays in eval mode: ``#model.train()`` is commented out at regenerateFromtrain2.py:622
        if isinstance(x_text, str) or len(x_text) <= 1:
            word_list = [x_text if isinstance(x_text, str) else x_text[0]] * n
        else:
            word_list = list(words)
        device, tf, phosc = self._prepare("sampling3", model, n, word_list, args, phoscLabels, check_latent=False)
        full = bool(getattr(args, "fullSampling", False))
        sampler = self._ddpm(None if full else (lambda i: self.sampling3_calls_model(i, self.noise_steps, epoch)),
                             deterministic=not full)
        att = self._attention_setup(model, sampler, attention)
        mix = self._mix_setup(model, n, mix_rate, style_pairs, 0, sampler=sampler)  # (one forward per step: no guidance here)
        x = self._denoise(model, n, tf, labels, phosc, device, sampler, x_T=x_t if noiseInput == 0 else x_T, noise=noise,
                          seed=seed, sample_offset=sample_offset, record=record, use_graph=use_graph, mix=mix, attention=att)
        if vae is None:
            return x
        image = self._finish(x, vae, args)
        return 0, [image], image

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
