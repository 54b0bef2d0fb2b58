"""Bulk sampling driver in the shape of the reference's ``full_sampling.py`` / ``sampling.py``.

The reference walks the ground-truth list one row at a time - one 999-step ``diffusion.sampling`` call with ``n = 1`` per
(writer, word) row (``full_sampling.py:147-170``).  Here the rows are cut into rank shards and batches, every batch is ONE
sampling call (B rows at once), and the on-device noise is keyed by the global row index, so the result of a row does not
depend on the batch size or the number of ranks.  Host-side pieces restated from the reference:

  * ``read_gt``       - ``writer,image word`` lines (``full_sampling.py:132-143``);
  * ``writer_dict``   - writer id -> class index in order of first appearance (``train.py:371-388``,
                        ``writers_dict_train.json``);
  * ``write_png``     - 8-bit RGB / grey PNG without PIL / cv2 (the reference saves through torchvision + PIL,
                        ``train.py:104-137``);
  * ``regenerate``    - the loop; ``vae=None`` writes latents (``.npy``), a duck-typed VAE (``vae.decode(z).sample``) PNGs.
  * ``--encode_images`` - the other direction: the gt rows' images through the VAE encoder into a latent cache
                        (``latents.build_latent_cache``), then exit.
  * ``--init_latents`` - regenerate FROM such a cache: ``--keep_cols A:B`` keeps those latent columns of every row's own latent
                        and re-draws the rest, ``--start T`` begins from the latent noised to level T (``regenerate(known=...)``).
  * ``--lines``       - whole lines instead of gt rows: every ``writer<TAB>word word ...`` row of the file is one sampler call's
                        line of overlapping word windows (``regenerate_lines``, ``Diffusion.sampling(..., windows=)``).
  * ``--verify``      - the OCR filter the reference's ``regenerateFrom*.py`` pipelines end a batch with, on the recogniser that is
                        in its checkout (``phoscnet.PHOSCnet`` / ``WordVerifier``): rejected rows are drawn again, then dropped;
                        ``save_path/verify.csv`` logs every attempt (``regenerate(verifier=...)``).
  * ``interpolate``   - one strip per gt row: the row's word in ``mix_steps`` styles from writer ``s1`` to writer ``s2``
                        (``sampling.py --interpolation --mix_rate`` renders one such blend of two random writers per call).
"""
from __future__ import annotations

import argparse
import json
import os
import struct
import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .dist import env_rank_world, shard_range


def read_gt(path: str) -> List[Tuple[str, str, str]]:
    """[(writer id, image name, transcription)] - ``full_sampling.py:132-143``: ``i.strip().split(' ')``, writer and image
    are the two comma-separated fields of the first token, the transcription is the second token."""
    rows = []
    with open(path, "r") as f:
        for line in f.readlines():
            parts = line.strip().split(" ")
            if len(parts) < 2 or "," not in parts[0]:
                continue
            s_id, image = parts[0].split(",")[0], parts[0].split(",")[1]
            rows.append((s_id, image, parts[1]))
    return rows


def writer_dict(rows: Sequence[Tuple[str, str, str]], path: Optional[str] = None) -> Dict[str, int]:
    """Writer id -> class index.  ``path``: an existing ``writers_dict_train.json`` (``full_sampling.py:152-153``); otherwise
    built like ``train.py:371-388`` (first appearance order)."""
    if path is not None and os.path.exists(path):
        with open(path, "r") as f:
            return {str(k): int(v) for k, v in json.load(f).items()}
    out: Dict[str, int] = {}
    for s_id, _, _ in rows:
        if s_id not in out:
            out[s_id] = len(out)
    return out


def make_phosc_of(alphabet_csv: str, version: str = "eng", phosc: int = 1, phos: int = 0):
    """word -> int64 PHOSC vector (``datasets.py:44-70``) with the reference's shape-count table read from ``alphabet_csv``
    (``ResPhoSCNetZSL/modules/utils/Alphabet.csv``; a data file of the reference, not shipped here).  One vector per
    distinct word is computed and kept (the reference recomputes or unpickles a ``wordPhosc`` dictionary,
    trainModifyCondition.py:268-292)."""
    from .phosc import load_alphabet, phosc_vector
    index, table = load_alphabet(alphabet_csv)
    memo: Dict[str, torch.Tensor] = {}

    def phosc_of(word: str) -> torch.Tensor:
        if word not in memo:
            memo[word] = torch.from_numpy(phosc_vector(word, index, table, version, phosc=phosc, phos=phos))
        return memo[word]

    return phosc_of


def write_png(path: str, img: np.ndarray) -> None:
    """uint8 [H, W] (grey) or [H, W, 3] (RGB) -> PNG (zlib-deflated, filter 0 scanlines)."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
        raise ValueError("write_png expects uint8 [H,W] or [H,W,3]")
    h, w = img.shape[:2]
    color = 0 if img.ndim == 2 else 2
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color, 0, 0, 0)) + \
        chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(png)


def keep_cols_mask(keep_cols, h: int, w: int) -> torch.Tensor:
    """fp32 [h, w] keep-mask of the latent columns ``a <= column < b`` (``keep_cols = (a, b)``, a half-open range within w)."""
    try:
        a, b = (int(v) for v in keep_cols)
    except (TypeError, ValueError):
        raise ValueError(f"keep_cols must be a pair (a, b) of latent columns, not {keep_cols!r}") from None
    if not 0 <= a < b <= w:
        raise ValueError(f"keep_cols must be a non-empty half-open range within the {w} latent columns, not {a}:{b}")
    mask = torch.zeros(h, w, dtype=torch.float32)
    mask[:, a:b] = 1.0
    return mask


def _known_latent(known, image: str) -> torch.Tensor:
    """The cached latent of a gt row: under the image name itself or, as ``build_latent_cache`` writes it, with ``.png``."""
    for key in (image, image + ".png"):
        if key in known:
            return known[key]
    raise KeyError(f"no latent of gt row image {image!r} in the known-latent cache")


def _check_sampler(sampler: str, skip_steps=False) -> None:
    if sampler not in ("ddpm", "ddim", "dpmpp"):
        raise ValueError(f"sampler must be 'ddpm', 'ddim' or 'dpmpp', not {sampler!r}")
    if sampler != "ddpm" and skip_steps:
        raise ValueError(f"sampler={sampler!r} and skip_steps are two ways to run fewer steps: choose one")


@torch.no_grad()
def regenerate(model, diffusion, rows: Sequence[Tuple[str, str, str]], wr_dict: Dict[str, int], args, vae=None,
               batch: int = 64, out_dir: Optional[str] = None, seed: int = 0, rank: Optional[int] = None,
               world: Optional[int] = None, skip_steps: bool = False, phosc_of=None, mix_rate=None, sampler: str = "ddpm",
               ddim_steps: int = 50, eta: float = 0.0, dpmpp_steps: int = 20, dpmpp_order: int = 2, dpmpp_spacing: str = "logsnr",
               known=None, keep_cols: Optional[Tuple[int, int]] = None, start: Optional[int] = None, known_noise="auto",
               attention=None, attn_out: Optional[str] = None, guidance: Optional[str] = None, cfg_scale: float = 3.0,
               resample: int = 1, jump: int = 10, verifier=None, verify_min_score: Optional[float] = None,
               verify_lexicon: Optional[Sequence[str]] = None, verify_tries: int = 1, verify_csv: Optional[str] = None):
    """Samples every gt row once (this rank's shard of them), ``batch`` rows per ``sampling`` call.

    Returns ``(start, latents_or_images)`` for the shard.  With ``out_dir`` the results are written as
    ``<image>.png`` (a VAE was given) or ``<image>.npy`` (latents).  ``skip_steps`` selects the step-skipping sampler of
    ``regenerateFromtrain2.py`` (``Diffusion.sampling3``); ``phosc_of(word) -> int tensor [769]`` supplies PHOSC vectors for
    ``UNetModelPhosc`` (``args.phosc == 1``).  ``mix_rate`` is handed to the sampler as ``full_sampling.py:171`` hands it: it has
    an effect on a model built with ``args.interpolation`` only.  ``sampler="ddim"``: ``Diffusion.sampling_ddim`` over
    ``ddim_steps`` timesteps with ``eta`` instead of the full ``sampling`` loop; ``sampler="dpmpp"``: ``Diffusion.sampling_dpmpp``
    over ``dpmpp_steps`` timesteps at ``dpmpp_order`` with ``dpmpp_spacing``.

    ``known`` (a ``LatentCache``, or any mapping image name -> latent [C, h, w]): every gt row is regenerated from its own cached
    latent - ``keep_cols = (a, b)`` keeps the latent columns a <= column < b and re-draws the rest, ``start`` begins the loop
    from the latent noised to that level, ``known_noise`` as in ``Diffusion.sampling``.  A row whose latent is missing raises
    KeyError naming it, before anything is sampled.  Not with ``skip_steps``.  ``resample`` / ``jump`` (``Diffusion.sampling``):
    RePaint's resampling jumps around the kept columns; ``resample > 1`` needs ``keep_cols``.

    ``attention`` (True or a timestep window ``(t_hi, t_lo)``, as in ``Diffusion.sampling``): every call also leaves its
    per-character cross-attention maps; ``attn_out`` (a ``.npz`` path; a relative one lands in ``out_dir``, beside the images)
    receives them for the shard: ``input`` / ``middle`` / ``output`` fp32 [rows, h, w, 10], row i belonging to ``images[i]`` /
    ``words[i]``.  ``attn_out`` alone means ``attention=True``.

    ``guidance="writer_free"`` with ``cfg_scale`` (``Diffusion.sampling``): classifier-free guidance on the writer, two forwards
    per step.  Not with ``skip_steps``, whose sampler has no guidance.

    ``verifier`` (a ``phoscnet.WordVerifier``; the OCR filter the reference's ``regenerateFrom*.py`` pipelines end a batch with):
    every decoded batch is scored against its own words.  A row is accepted when its score is at least ``verify_min_score``
    (where given) and, where ``verify_lexicon`` is given, its word is the lexicon's best match.  Rejected rows are drawn again, up
    to ``verify_tries`` draws in all: try t (0-based) of global row r is sample ``r + t * len(rows)`` of the noise stream, whatever
    the batch size or the number of ranks, so a rerun repeats every draw (a redraw call spans the chunk's first to last rejected
    row).  Rows still rejected after the last try are not written (the returned tensor keeps their last draw).  ``verify_csv``
    receives one row per attempt: image, word, score, best word (empty without a lexicon), accepted (0 / 1), try.  Needs a VAE
    (a ValueError before anything is launched otherwise); not with ``attention``."""
    if verifier is not None:
        if vae is None:
            raise ValueError("verifier needs decoded images: pass the VAE (latents alone cannot be read)")
        if attention is not None or attn_out is not None:
            raise ValueError("verifier cannot be combined with attention maps (a redraw would replace a row's maps)")
        if int(verify_tries) < 1:
            raise ValueError(f"verify_tries must be at least 1, not {verify_tries}")
    elif verify_min_score is not None or verify_lexicon is not None or verify_tries != 1 or verify_csv is not None:
        raise ValueError("verify_min_score / verify_lexicon / verify_tries / verify_csv need a verifier")
    if guidance is not None and skip_steps:
        raise ValueError("guidance is not supported by the step-skipping sampler (skip_steps)")
    if attn_out is not None and attention is None:
        attention = True
    _check_sampler(sampler, skip_steps)
    if resample != 1 and (skip_steps or keep_cols is None):
        raise ValueError("resample > 1 needs kept columns (known= with keep_cols=) and is not supported by the step-skipping sampler")
    if known is None and (keep_cols is not None or start is not None):
        raise ValueError("keep_cols and start need the known latents (known=)")
    if known is not None:
        if skip_steps:
            raise ValueError("known latents are not supported by the step-skipping sampler (skip_steps)")
        if keep_cols is None and start is None:
            raise ValueError("known needs keep_cols (the latent columns to keep), a start level, or both")
    r0, w0, _ = env_rank_world()
    rank = r0 if rank is None else rank
    world = w0 if world is None else world
    first, count = shard_range(len(rows), rank, world)
    mine = rows[first:first + count]
    outs, maps = [], []
    kmask = None
    if known is not None:
        if keep_cols is not None:
            kmask = keep_cols_mask(keep_cols, diffusion.img_size[0] // 8, diffusion.img_size[1] // 8)
        latents = [_known_latent(known, image) for _, image, _ in mine]  # (all of them first: a missing row fails up front)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)

    def draw(lo: int, hi: int, offset: int):
        """One sampler call for the shard's rows lo .. hi - 1 with sample ``offset + i`` of the noise stream for row lo + i."""
        part = mine[lo:hi]
        words = [t for _, _, t in part]
        labels = torch.tensor([wr_dict[s] for s, _, _ in part], dtype=torch.int64)
        phosc = torch.stack([phosc_of(wd) for wd in words]) if phosc_of is not None else None
        kw = dict(seed=seed, sample_offset=offset, mix_rate=mix_rate)
        if attention is not None:
            kw.update(attention=attention)
        if guidance is not None:
            kw.update(guidance=guidance, cfg_scale=cfg_scale)
        if known is not None:
            kw.update(known=torch.stack(latents[lo:hi]), known_mask=kmask, start=start, known_noise=known_noise)
        if resample != 1:
            kw.update(resample=resample, jump=jump)
        if sampler == "ddim":
            res = diffusion.sampling_ddim(model, vae, len(part), words, labels, args, steps=ddim_steps, eta=eta, phoscLabels=phosc, **kw)
        elif sampler == "dpmpp":
            res = diffusion.sampling_dpmpp(model, vae, len(part), words, labels, args, steps=dpmpp_steps, order=dpmpp_order,
                                           spacing=dpmpp_spacing, phoscLabels=phosc, **kw)
        elif skip_steps:
            res = diffusion.sampling3(0, None, words, phosc, model, model, vae, 0, 1, len(part), words, labels, args, **kw)
            res = res if vae is None else res[2]
        else:
            res = diffusion.sampling(model, vae, len(part), words, labels, args, phoscLabels=phosc, **kw)
        return res.detach()

    log = []  # verify_csv rows
    for b0 in range(0, count, batch):
        chunk = mine[b0:b0 + batch]
        res = draw(b0, b0 + len(chunk), first + b0)
        accepted = [True] * len(chunk)
        if verifier is not None:
            words = [t for _, _, t in chunk]
            res = res.clone()
            pending = list(range(len(chunk)))
            for attempt in range(int(verify_tries)):
                if attempt:
                    lo, hi = pending[0], pending[-1] + 1
                    again = draw(b0 + lo, b0 + hi, first + b0 + lo + attempt * len(rows))
                    for i in pending:
                        res[i] = again[i - lo]
                sc, best, ok = verifier.verify(res[pending], [words[i] for i in pending], verify_min_score, verify_lexicon)
                sc, ok = sc.cpu().tolist(), ok.cpu().tolist()
                for j, i in enumerate(pending):
                    log.append((chunk[i][1], words[i], sc[j], best[j] if best is not None else "", int(ok[j]), attempt))
                pending = [i for j, i in enumerate(pending) if not ok[j]]
                if not pending:
                    break
            for i in pending:
                accepted[i] = False
        res = res.cpu()
        outs.append(res)
        if attention is not None:
            maps.append({k: v.cpu() for k, v in diffusion.last_attention.items()})
        if out_dir is not None:
            for (_, image, _), item, keep in zip(chunk, res, accepted):
                if not keep:
                    continue
                if vae is None:
                    np.save(os.path.join(out_dir, f"{image}.npy"), item.numpy())
                else:
                    arr = (item.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()
                    write_png(os.path.join(out_dir, f"{image}.png"), arr if arr.shape[2] == 3 else arr[:, :, 0])
    if verify_csv is not None:
        os.makedirs(os.path.dirname(os.path.abspath(verify_csv)), exist_ok=True)
        with open(verify_csv, "w") as f:
            f.write("image,word,score,best_word,accepted,try\n")
            for image, word, score, best, ok, attempt in log:
                f.write(f"{image},{word},{score!r},{best},{ok},{attempt}\n")
    if attn_out is not None and maps:
        path = attn_out if (os.path.isabs(attn_out) or out_dir is None) else os.path.join(out_dir, attn_out)
        np.savez_compressed(path, images=np.array([image for _, image, _ in mine]), words=np.array([t for _, _, t in mine]),
                            **{k: torch.cat([m[k] for m in maps]).numpy() for k in maps[0]})
    return first, (torch.cat(outs) if outs else torch.empty(0))


@torch.no_grad()
def interpolate(model, diffusion, rows: Sequence[Tuple[str, str, str]], args, style_pair: Tuple[int, int], mix_steps: int = 8,
                vae=None, out_dir: Optional[str] = None, seed: int = 0, rank: Optional[int] = None, world: Optional[int] = None,
                phosc_of=None, sampler: str = "ddpm", ddim_steps: int = 50, eta: float = 0.0, dpmpp_steps: int = 20,
                dpmpp_order: int = 2, dpmpp_spacing: str = "logsnr"):
    """One interpolation strip per gt row (this rank's shard of them): the row's word sampled ``mix_steps`` times in one call,
    sample j with the writer embedding ``(1 - m_j) * label[s1] + m_j * label[s2]``, ``m = linspace(0, 1, mix_steps)``
    (``Diffusion.sampling(..., style_pairs=)``, one forward per step; ``sampler="ddim"``: ``sampling_ddim`` over ``ddim_steps``
    timesteps with ``eta``; ``sampler="dpmpp"``: ``sampling_dpmpp`` over ``dpmpp_steps`` timesteps at ``dpmpp_order`` with
    ``dpmpp_spacing``).  Sample j of row r is global sample ``r * mix_steps + j``
    of the noise stream, whatever the sharding.

    Returns ``(start, [mix_steps, ...] tensor per row)``.  With ``out_dir``, ``<image>_interp.png`` is written per row: the
    decoded images side by side when a VAE is given; otherwise the latents are kept as ``<image>_interp.npy`` and the PNG is a
    grey preview of them (per sample the 4 channels stacked, min-max scaled over the strip)."""
    if mix_steps < 2:
        raise ValueError("mix_steps must be at least 2 (the two writers themselves)")
    _check_sampler(sampler)
    r0, w0, _ = env_rank_world()
    rank = r0 if rank is None else rank
    world = w0 if world is None else world
    start, count = shard_range(len(rows), rank, world)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    m = torch.linspace(0, 1, mix_steps)
    labels = torch.zeros(mix_steps, dtype=torch.int64)  # unused: the pair replaces the writer id
    outs = []
    for r in range(start, start + count):
        _, image, word = rows[r]
        phosc = torch.stack([phosc_of(word)] * mix_steps) if phosc_of is not None else None
        kw = dict(mix_rate=m, phoscLabels=phosc, seed=seed, sample_offset=r * mix_steps, style_pairs=tuple(int(s) for s in style_pair))
        if sampler == "ddim":
            res = diffusion.sampling_ddim(model, vae, mix_steps, word, labels, args, steps=ddim_steps, eta=eta, **kw).detach().cpu()
        elif sampler == "dpmpp":
            res = diffusion.sampling_dpmpp(model, vae, mix_steps, word, labels, args, steps=dpmpp_steps, order=dpmpp_order,
                                           spacing=dpmpp_spacing, **kw).detach().cpu()
        else:
            res = diffusion.sampling(model, vae, mix_steps, word, labels, args, **kw).detach().cpu()
        outs.append(res)
        if out_dir is None:
            continue
        if vae is None:
            np.save(os.path.join(out_dir, f"{image}_interp.npy"), res.numpy())
            lo, hi = float(res.min()), float(res.max())
            tiles = ((res - lo) / max(hi - lo, 1e-12) * 255).round().to(torch.uint8)  # [N, c, h, w]
            n, c, h, w = tiles.shape
            strip = tiles.reshape(n, c * h, w).permute(1, 0, 2).reshape(c * h, n * w).numpy()
        else:
            arr = (res.clamp(0, 1) * 255).round().to(torch.uint8)  # [N, ch, H, W]
            n, c, h, w = arr.shape
            strip = arr.permute(2, 0, 3, 1).reshape(h, n * w, c).numpy()
            strip = strip if c == 3 else strip[:, :, 0]
        write_png(os.path.join(out_dir, f"{image}_interp.png"), strip)
    return start, outs


def read_lines(path: str) -> List[Tuple[str, Tuple[str, ...]]]:
    """[(writer id, the words of the line)] of a ``--lines`` file: one row per line, ``writer<TAB>word word ...``.  Empty rows are
    skipped; a row without a tab or without a word is an error that names it."""
    rows = []
    with open(path, "r") as f:
        for i, line in enumerate(f.read().splitlines()):
            if not line.strip():
                continue
            writer, tab, text = line.partition("\t")
            if not tab or not writer.strip() or not text.split():
                raise ValueError(f"{path}, row {i + 1}: expected 'writer<TAB>word word ...', got {line!r}")
            rows.append((writer.strip(), tuple(text.split())))
    return rows


@torch.no_grad()
def regenerate_lines(model, diffusion, lines: Sequence[Tuple[str, Sequence[str]]], wr_dict: Dict[str, int], args, vae=None,
                     batch: int = 64, out_dir: Optional[str] = None, seed: int = 0, rank: Optional[int] = None,
                     world: Optional[int] = None, overlap: int = 2, feather: int = 0, phosc_of=None, sampler: str = "ddpm",
                     ddim_steps: int = 50, eta: float = 0.0, dpmpp_steps: int = 20, dpmpp_order: int = 2, dpmpp_spacing: str = "logsnr",
                     guidance: Optional[str] = None, cfg_scale: float = 3.0):
    """Samples every line once (this rank's shard of them) through the ``windows=`` argument of the chosen sampler: a line of K
    words is K windows of the model's width that overlap by ``overlap`` latent columns, weighted by ``window_profile(w, feather)``.
    One call takes lines of one K, so the lines are ordered by (K, row index) - a line's place in that order is its global sample
    index in the noise stream, whatever the batch size or the number of ranks - and every group runs in chunks of ``batch // K``
    lines (at least 1).  Returns {row index: latent or image}.  With ``out_dir`` row i is written as ``line_<i>.png`` (a VAE was
    given) or ``line_<i>.npy`` (latents)."""
    _check_sampler(sampler)
    r0, w0, _ = env_rank_world()
    rank = r0 if rank is None else rank
    world = w0 if world is None else world
    order = sorted(range(len(lines)), key=lambda i: (len(lines[i][1]), i))
    first, count = shard_range(len(order), rank, world)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    outs = {}
    pos = first
    while pos < first + count:
        K = len(lines[order[pos]][1])
        per_call = max(1, batch // K)
        chunk = [i for i in order[pos:min(pos + per_call, first + count)] if len(lines[i][1]) == K]  # (a chunk ends with its group)
        n = len(chunk)
        words = [list(lines[i][1]) for i in chunk]
        labels = torch.tensor([wr_dict[lines[i][0]] for i in chunk], dtype=torch.int64)
        kw = dict(seed=seed, sample_offset=pos, windows=diffusion.line_windows(n, K, overlap=overlap, feather=feather))
        if phosc_of is not None:
            kw.update(phoscLabels=torch.stack([torch.stack([phosc_of(wd) for wd in row]) for row in words]))
        if guidance is not None:
            kw.update(guidance=guidance, cfg_scale=cfg_scale)
        if sampler == "ddim":
            res = diffusion.sampling_ddim(model, vae, n, words, labels, args, steps=ddim_steps, eta=eta, **kw)
        elif sampler == "dpmpp":
            res = diffusion.sampling_dpmpp(model, vae, n, words, labels, args, steps=dpmpp_steps, order=dpmpp_order, spacing=dpmpp_spacing,
                                           **kw)
        else:
            res = diffusion.sampling(model, vae, n, words, labels, args, **kw)
        for i, item in zip(chunk, res.detach().cpu()):
            outs[i] = item
            if out_dir is None:
                continue
            if vae is None:
                np.save(os.path.join(out_dir, f"line_{i}.npy"), item.numpy())
            else:
                arr = (item.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()
                write_png(os.path.join(out_dir, f"line_{i}.png"), arr if arr.shape[2] == 3 else arr[:, :, 0])
        pos += n
    return outs


def build_parser() -> argparse.ArgumentParser:
    """The command line of ``main`` (flags follow ``full_sampling.py:40-66`` where they exist); needs no device."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gt_train", default=None, help="the ground-truth list: 'writer,image word' rows (required unless --lines)")
    ap.add_argument("--models_path", default=None, help="directory holding models/ema_ckpt.pt (reference layout)")
    ap.add_argument("--save_path", required=True)
    ap.add_argument("--writer_dict", default="./writers_dict_train.json")
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--emb_dim", type=int, default=320)
    ap.add_argument("--num_heads", type=int, default=4)
    ap.add_argument("--num_res_blocks", type=int, default=1)
    ap.add_argument("--noise_steps", type=int, default=1000)
    ap.add_argument("--phosc", type=int, default=0)
    ap.add_argument("--alphabet_csv", default=None,
                    help="--phosc 1: the reference's shape-count table (ResPhoSCNetZSL/modules/utils/Alphabet.csv)")
    ap.add_argument("--vocab_size", type=int, default=53, choices=[53, 54],
                    help="53: the 52-letter alphabet of train.py; 54: the '_' alphabet of trainModifyCondition.py:68")
    ap.add_argument("--skip_steps", type=int, default=0, help="1: regenerateFromtrain2.py's step-skipping sampler")
    ap.add_argument("--sampler", default="ddpm", choices=["ddpm", "ddim", "dpmpp"],
                    help="ddpm: every one of the noise_steps - 1 steps (train.py:221); ddim: --ddim_steps of them (Song et al. 2020); "
                         "dpmpp: --dpmpp_steps of them with DPM-Solver++(2M) (Lu et al. 2022)")
    ap.add_argument("--ddim_steps", type=int, default=50, help="--sampler ddim: UNet evaluations per image")
    ap.add_argument("--eta", type=float, default=0.0, help="--sampler ddim: 0 deterministic .. 1 the DDPM posterior variance")
    ap.add_argument("--dpmpp_steps", type=int, default=20, help="--sampler dpmpp: UNet evaluations per image")
    ap.add_argument("--dpmpp_order", type=int, default=2, choices=[1, 2], help="--sampler dpmpp: 2 multistep; 1 is DDIM with eta 0")
    ap.add_argument("--dpmpp_spacing", default="logsnr", choices=["logsnr", "time"],
                    help="--sampler dpmpp: timesteps evenly spaced in log-SNR, or in t as --sampler ddim spaces them")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--interpolation", type=bool, nargs="?", const=True, default=False,
                    help="args.interpolation of the reference (sampling.py:64; any value is true, as there): with --mix_rate "
                         "every forward blends two random writers")
    ap.add_argument("--mix_rate", type=float, default=None, help="weight of the second writer, 0..1 (sampling.py:65)")
    ap.add_argument("--style_pair", type=int, nargs=2, default=None, metavar=("S1", "S2"),
                    help="two writer class indices: one strip per gt row from S1 to S2 in --mix_steps samples is written "
                         "instead of the rows themselves")
    ap.add_argument("--mix_steps", type=int, default=8)
    ap.add_argument("--guidance", default=None, choices=["writer_free"],
                    help="writer_free: classifier-free guidance on the writer - every step also runs the model without the writer "
                         "embedding and extrapolates by --cfg_scale (for a model trained with label dropout)")
    ap.add_argument("--cfg_scale", type=float, default=3.0, help="--guidance: the guidance scale (train.py:200); 0 turns it off")
    ap.add_argument("--stable_dif_path", default=None,
                    help="local Stable-Diffusion checkout in diffusers layout (its vae/ subfolder is read; train.py:415): with it "
                         "the rows are decoded and written as PNGs, without it as latents (.npy)")
    ap.add_argument("--encode_images", default=None, metavar="DIR",
                    help="build a latent cache instead of sampling: encode DIR/<image>.png of every gt row with the VAE encoder of "
                         "--stable_dif_path, write --latents_out and exit (the --vaeFromDict 1 input of the training scripts)")
    ap.add_argument("--latents_out", default=None, metavar="FILE", help="--encode_images: the container to write (.safetensors / .npz)")
    ap.add_argument("--latent_mode", default="sample", choices=["sample", "mode"],
                    help="--encode_images: a posterior draw per image (keyed by --seed and the row index) or the posterior mean")
    ap.add_argument("--init_latents", default=None, metavar="FILE",
                    help="a latent cache (--latents_out of an --encode_images run): every gt row is regenerated from its own latent, "
                         "as --keep_cols and / or --start say")
    ap.add_argument("--keep_cols", default=None, metavar="A:B",
                    help="--init_latents: keep the latent columns A <= column < B of the 32 and re-draw the rest")
    ap.add_argument("--start", type=int, default=None, metavar="T",
                    help="--init_latents: begin from the latent noised to level T (1 .. noise_steps - 1) instead of from noise")
    ap.add_argument("--resample", type=int, default=1, metavar="R",
                    help="--keep_cols: RePaint's resampling - every stretch of --jump steps is diffused forward again and denoised "
                         "once more, R - 1 times (1: off)")
    ap.add_argument("--jump", type=int, default=10, metavar="J", help="--resample: the length of a stretch, in visited steps")
    ap.add_argument("--attn_maps", default=None, metavar="FILE",
                    help="also save the per-character cross-attention maps of every generated row (.npz beside the images: input / "
                         "middle / output [rows, h, w, 10], images, words); base model only")
    ap.add_argument("--attn_window", default=None, metavar="HI:LO",
                    help="--attn_maps: average over the model-calling steps with LO <= t <= HI only (default: all of them)")
    ap.add_argument("--lines", default=None, metavar="FILE",
                    help="sample whole lines instead of the gt rows: every row of FILE is 'writer<TAB>word word ...' and becomes one "
                         "image (or latent), line_<row index>, of overlapping word windows denoised together")
    ap.add_argument("--verify", default=None, metavar="CKPT",
                    help="a PHOSCnet checkpoint (ResPhoSCNetZSL state_dict): every decoded batch is read back by the recogniser, rejected "
                         "rows are drawn again and, if still rejected, not written; save_path/verify.csv logs every attempt "
                         "(needs --alphabet_csv and --stable_dif_path)")
    ap.add_argument("--verify_min_score", type=float, default=None, metavar="S",
                    help="--verify: accept a row when the cosine of its predicted PHOSC vector against its word's is at least S")
    ap.add_argument("--verify_lexicon", default=None, metavar="FILE",
                    help="--verify: one word per line; accept a row when its word is the best match among them")
    ap.add_argument("--verify_tries", type=int, default=1, metavar="N", help="--verify: draws per row in all (N - 1 redraws)")
    ap.add_argument("--line_overlap", type=int, default=2, metavar="V", help="--lines: latent columns two neighbouring words share")
    ap.add_argument("--line_feather", type=int, default=0, metavar="F",
                    help="--lines: latent columns over which a window's weight ramps up at its ends (0: the plain average)")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.gt_train is None and a.lines is None:
        ap.error("the following arguments are required: --gt_train")
    if a.lines is not None:
        for flag, on in (("--gt_train", a.gt_train), ("--skip_steps 1", a.skip_steps), ("--style_pair", a.style_pair),
                         ("--mix_rate", a.mix_rate), ("--init_latents", a.init_latents), ("--attn_maps", a.attn_maps),
                         ("--encode_images", a.encode_images)):
            if on:
                ap.error(f"--lines does not take {flag}")
        if not 0 <= a.line_overlap < 32:
            ap.error(f"--line_overlap must be in [0, 31] latent columns, not {a.line_overlap}")
        if a.line_feather < 0:
            ap.error(f"--line_feather must be >= 0, not {a.line_feather}")
    if a.verify is None:
        if a.verify_min_score is not None or a.verify_lexicon is not None or a.verify_tries != 1:
            ap.error("--verify_min_score, --verify_lexicon and --verify_tries need --verify (the recogniser's checkpoint)")
    else:
        for flag, on in (("--lines", a.lines), ("--style_pair", a.style_pair), ("--encode_images", a.encode_images),
                         ("--attn_maps", a.attn_maps)):
            if on:
                ap.error(f"--verify does not take {flag}")
        if not a.alphabet_csv:
            ap.error("--verify needs --alphabet_csv (the PHOS shape-count table)")
        if a.verify_tries < 1:
            ap.error(f"--verify_tries must be at least 1, not {a.verify_tries}")
    if a.sampler != "ddpm" and a.skip_steps:
        ap.error(f"--sampler {a.sampler} and --skip_steps 1 are two ways to run fewer steps: choose one")
    if a.sampler == "ddim" and not 1 <= a.ddim_steps <= a.noise_steps - 1:
        ap.error(f"--ddim_steps must be in [1, {a.noise_steps - 1}] (--noise_steps {a.noise_steps})")
    if a.sampler == "dpmpp" and not 1 <= a.dpmpp_steps <= a.noise_steps - 1:
        ap.error(f"--dpmpp_steps must be in [1, {a.noise_steps - 1}] (--noise_steps {a.noise_steps})")
    if a.guidance is not None and (a.skip_steps or a.style_pair is not None or (a.interpolation and a.mix_rate is not None)):
        ap.error("--guidance cannot be combined with --skip_steps 1, --style_pair or --interpolation with a --mix_rate")
    if a.init_latents is None and (a.keep_cols is not None or a.start is not None):
        ap.error("--keep_cols and --start need --init_latents (the latents to start from)")
    if a.init_latents is not None:
        if a.skip_steps:
            ap.error("--skip_steps 1 does not take --init_latents / --keep_cols / --start")
        if a.style_pair is not None:
            ap.error("--style_pair strips do not take --init_latents / --keep_cols / --start")
        if a.keep_cols is None and a.start is None:
            ap.error("--init_latents needs --keep_cols A:B, --start T, or both")
        if a.start is not None and not 1 <= a.start <= a.noise_steps - 1:
            ap.error(f"--start must be in [1, {a.noise_steps - 1}] (--noise_steps {a.noise_steps})")
    if a.resample < 1 or a.jump < 1:
        ap.error("--resample and --jump must be >= 1")
    if a.resample > 1:
        if a.skip_steps:
            ap.error("--skip_steps 1 does not take --resample")
        if a.keep_cols is None:  # (--lines keeps no region yet: it does not take --init_latents)
            ap.error("--resample needs a kept region (--init_latents with --keep_cols): without one there is nothing to harmonise")
        if a.attn_maps is not None:
            ap.error("--resample does not take --attn_maps: the maps would count the revisited steps")
        if a.interpolation and a.mix_rate is not None:
            ap.error("--resample cannot be combined with --interpolation with a --mix_rate")
    if a.attn_window is not None:
        if a.attn_maps is None:
            ap.error("--attn_window needs --attn_maps (the file to write)")
        parts = a.attn_window.split(":")
        if len(parts) != 2 or not all(p.strip().isdigit() for p in parts) or int(parts[0]) < int(parts[1]):
            ap.error(f"--attn_window takes HI:LO, two timesteps with HI >= LO, not {a.attn_window!r}")
        a.attn_window = (int(parts[0]), int(parts[1]))
    if a.attn_maps is not None:
        if a.phosc:
            ap.error("--attn_maps: the PHOSC model has no per-character attention maps")
        if a.style_pair is not None:
            ap.error("--style_pair strips do not take --attn_maps")
        if not a.attn_maps.endswith(".npz"):
            a.attn_maps += ".npz"
    if a.keep_cols is not None:
        parts = a.keep_cols.split(":")
        if len(parts) != 2 or not all(p.strip().isdigit() for p in parts):
            ap.error(f"--keep_cols takes A:B, two latent column indices, not {a.keep_cols!r}")
        a.keep_cols = (int(parts[0]), int(parts[1]))
        if not 0 <= a.keep_cols[0] < a.keep_cols[1] <= 32:
            ap.error(f"--keep_cols must be a non-empty half-open range within the 32 latent columns, not {parts[0]}:{parts[1]}")
    return ap, a


def main(argv=None):
    """``python -m worddiffusion_amd.driver --gt_train gt.txt --models_path run/ --save_path out/`` (one process per GPU under
    torchrun)."""
    import copy
    import types
    from . import Diffusion, UNetModel, UNetModelPhosc
    ap, a = parse_args(argv)
    rank, world, local = env_rank_world()
    if a.verify is not None and not a.stable_dif_path:
        raise ValueError("--verify reads decoded images: it needs --stable_dif_path (the VAE); latents alone cannot be verified")
    dev = f"cuda:{local}"
    torch.cuda.set_device(local)
    if a.encode_images:
        if not a.stable_dif_path or not a.latents_out:
            ap.error("--encode_images needs --stable_dif_path (the VAE) and --latents_out (the file to write)")
        from .latents import build_latent_cache
        from .vae import AutoencoderKL
        vae = AutoencoderKL.from_pretrained(a.stable_dif_path, subfolder="vae").to(dev)
        rows = read_gt(a.gt_train)
        build_latent_cache(vae, rows, a.encode_images, a.latents_out, mode=a.latent_mode == "mode", seed=a.seed, batch=a.batch_size)
        print(f"latents of {len({r[1] for r in rows})} images ({a.latent_mode}) written to {a.latents_out}")
        return
    args = types.SimpleNamespace(device=dev, interpolation=bool(a.interpolation), charLevelEmb=0, charImages=0, attentionMaps=0, ocrTraining=0,
                                 imgConditioned=0, wrdChrWrStyl=0, phosc=a.phosc, phos=0, latent=True, fullSampling=False)
    lines = read_lines(a.lines) if a.lines is not None else None
    rows = read_gt(a.gt_train) if lines is None else [(writer, f"line_{i}", " ".join(words)) for i, (writer, words) in enumerate(lines)]
    wr = writer_dict(rows, a.writer_dict)
    cls = UNetModelPhosc if a.phosc else UNetModel
    unet = cls(image_size=(64, 256), in_channels=4, model_channels=a.emb_dim, out_channels=4, num_res_blocks=a.num_res_blocks,
               attention_resolutions=(1, 1), channel_mult=(1, 1), num_heads=a.num_heads, num_classes=max(339, len(wr)),
               context_dim=a.emb_dim, vocab_size=a.vocab_size, args=args, max_seq_len=10).to(dev)
    if a.models_path:
        unet.load_state_dict(torch.load(os.path.join(a.models_path, "models", "ema_ckpt.pt"), map_location=dev,
                                        weights_only=True))
    ema_model = copy.deepcopy(unet).eval().requires_grad_(False)
    diffusion = Diffusion(noise_steps=a.noise_steps, img_size=(64, 256), args=args)
    vae = None
    if a.stable_dif_path:
        from .vae import AutoencoderKL
        vae = AutoencoderKL.from_pretrained(a.stable_dif_path, subfolder="vae").to(dev)
    phosc_of = None
    if a.phosc:
        if not a.alphabet_csv:
            ap.error("--phosc 1 needs --alphabet_csv (the PHOS shape-count table)")
        phosc_of = make_phosc_of(a.alphabet_csv)
    if lines is not None:
        res = regenerate_lines(ema_model, diffusion, lines, wr, args, vae=vae, batch=a.batch_size, out_dir=os.path.join(a.save_path, "images"),
                               seed=a.seed, overlap=a.line_overlap, feather=a.line_feather, phosc_of=phosc_of, sampler=a.sampler,
                               ddim_steps=a.ddim_steps, eta=a.eta, dpmpp_steps=a.dpmpp_steps, dpmpp_order=a.dpmpp_order,
                               dpmpp_spacing=a.dpmpp_spacing, guidance=a.guidance, cfg_scale=a.cfg_scale)
        print(f"[rank {rank}/{world}] {len(res)} of {len(lines)} lines written to {a.save_path}/images")
        return
    if a.style_pair is not None:
        start, res = interpolate(ema_model, diffusion, rows, args, tuple(a.style_pair), a.mix_steps, vae=vae,
                                 out_dir=os.path.join(a.save_path, "images"), seed=a.seed, phosc_of=phosc_of, sampler=a.sampler,
                                 ddim_steps=a.ddim_steps, eta=a.eta, dpmpp_steps=a.dpmpp_steps, dpmpp_order=a.dpmpp_order,
                                 dpmpp_spacing=a.dpmpp_spacing)
        print(f"[rank {rank}/{world}] strips of rows {start}..{start + len(res)} of {len(rows)} written to {a.save_path}/images")
        return
    known = None
    if a.init_latents:
        from .latents import LatentCache
        known = LatentCache(a.init_latents)
    verify_kw = {}
    if a.verify is not None:
        from .phoscnet import PHOSCnet, WordVerifier
        net = PHOSCnet()
        net.load_state_dict(torch.load(a.verify, map_location="cpu", weights_only=True), strict=True)
        lexicon = None
        if a.verify_lexicon:
            with open(a.verify_lexicon) as f:
                lexicon = [ln.strip() for ln in f if ln.strip()]
        verify_kw = dict(verifier=WordVerifier(net.to(dev), a.alphabet_csv), verify_min_score=a.verify_min_score, verify_lexicon=lexicon,
                         verify_tries=a.verify_tries,
                         verify_csv=os.path.join(a.save_path, "verify.csv" if world == 1 else f"verify.rank{rank}.csv"))
    start, res = regenerate(ema_model, diffusion, rows, wr, args, vae=vae, batch=a.batch_size,
                            out_dir=os.path.join(a.save_path, "images"), seed=a.seed, skip_steps=bool(a.skip_steps),
                            phosc_of=phosc_of, mix_rate=a.mix_rate, sampler=a.sampler, ddim_steps=a.ddim_steps, eta=a.eta,
                            dpmpp_steps=a.dpmpp_steps, dpmpp_order=a.dpmpp_order, dpmpp_spacing=a.dpmpp_spacing, known=known,
                            keep_cols=a.keep_cols, start=a.start, resample=a.resample, jump=a.jump,
                            guidance=a.guidance, cfg_scale=a.cfg_scale, **verify_kw,
                            attention=None if a.attn_maps is None else (a.attn_window or True),
                            attn_out=None if a.attn_maps is None else
                            (a.attn_maps if world == 1 else a.attn_maps[:-4] + f".rank{rank}.npz"))
    print(f"[rank {rank}/{world}] rows {start}..{start + len(res)} of {len(rows)} written to {a.save_path}/images")


if __name__ == "__main__":
    main()
